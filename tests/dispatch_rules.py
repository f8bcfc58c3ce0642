"""The host-side dispatch rules of the GP, popgen, kinship and MLE paths restated in plain Python, each next to the source line it
restates.  tests/test_gpu_dispatch_edges_gp.py, tests/test_gpu_dispatch_edges_popgen.py and the kinship parameter lists assert these
predicates for every shape they run: when a rule moves in the C++ and not here (or a point slides off its edge), the point fails
before anything is launched.  Nothing here needs a GPU (tests/test_dispatch_rules.py exercises it on the CPU)."""

# ---- pg_sweep.hip ------------------------------------------------------------------------------------------------------------
SW_CH, SW_WAVES = 32, 4                   # :34-42
SW_TILE = 64 * (SW_CH + 2)                # :43-47
MB_TILE = 64 * (SW_CH + 4)                # :773-774
MS_MAX_COLS = 48                          # :933
PG_MAX_SWEEP_COLS = 34                    # pg_common.h:12
COL_SIZES = (2, 3, 4, 6, 8, 12, 16, 24, PG_MAX_SWEEP_COLS)


def ms_pick_u(nc):
    """chunks per load group (pg_sweep.hip:958-965): the U of 8 .. 5 that pads least, the larger on a tie"""
    U, best = 8, 1 << 30
    for u in (8, 7, 6, 5):
        padded = (nc + u - 1) // u * u
        if padded < best:
            best, U = padded, u
    return U


def ms_threads(ncg):
    return 256 if ncg == 3 else 512       # :411


def ms_pitch(cu, mode):
    return ((cu + 2) | 1) if mode == 2 else ((cu + 1) | 1)   # :967


def ms_fits(n, cu, mode):
    """pg_sweep.hip:969-972: the B table plus the closing stage of a MODE launch within 160 KiB of LDS, from 5 chunks (33 pools) up"""
    nc = (n + 7) // 8
    U = ms_pick_u(nc)
    ncp = (nc + U - 1) // U * U
    ncg = (cu + 15) // 16
    return nc >= 5 and cu <= MS_MAX_COLS and (ncg * ncp * 128 + (ms_threads(ncg) // 64) * 64 * ms_pitch(cu, mode)) * 8 <= 160 * 1024


def last_ms_count(cu, mode):
    """the largest pool count with ms_fits (the predicate is not monotonic in n inside a chunk group, so: the last True)"""
    return max(n for n in range(33, 4097) if ms_fits(n, cu, mode))


def round_cols(c):
    """pg_sweep.hip:1005-1010: the template width that carries c columns, -1 beyond 34"""
    for s in COL_SIZES:
        if c <= s:
            return s
    return -1


def beta_route(n, ncol, colmajor=True, ss=False, env=()):
    """pg_gp_beta_cols (pg_sweep.hip:1484-1544) for an even ld and an aligned G: (route, template width).  env: the set of
    POOLGEN_GP_BETA_* suffixes that are set ("OLD", "VALU", "SCALAR")."""
    cols = round_cols(ncol)
    assert cols > 0
    n_even = (n + 1) & ~1
    zrows = (n + SW_CH - 1) // SW_CH * SW_CH
    mfma_lds = (zrows * 16 + SW_WAVES * MB_TILE) * 8
    wdoubles = n_even * cols
    lds_need = (wdoubles + SW_WAVES * SW_TILE) * 8
    if ms_fits(n, ncol, 1) and "OLD" not in env:                                                       # :1520
        return "matrix-core", cols
    if not ss and colmajor and 5 <= ncol <= 16 and mfma_lds <= 150 * 1024 and "VALU" not in env:      # :1523
        return "beta_mfma", 16
    if (not ss and cols >= 6 and cols % 2 == 0 and cols <= 24 and wdoubles * 8 > 12288 and lds_need <= 150 * 1024
            and "SCALAR" not in env):                                                                  # :1530-1531
        return "beta_lds", cols
    return "beta_scalar", cols                                                                         # :1537


# ---- pg_gp.hip ---------------------------------------------------------------------------------------------------------------
GP_LMAX, GP_CP = 16, 16                   # :38, :859


def path_len(lambda_step):
    """penalised_path (pg_gp.hip:1030-1033): L = llround(1 / step) + 1 lambdas (llround: halves away from zero)"""
    x = 1.0 / lambda_step
    return int(x + 0.5) + 1


def path_lp(L):
    """with_path_len (pg_gp.hip:502-506): the even template length that carries L lambdas"""
    return (L + 1) & ~1


def cv_route(n, p, C, n_reps, env=()):
    """penalised_path :1045 and cv_fused :874: "per_fold" (tall design or more than 34 fold x trait columns), else "batched"
    (n_reps > 1) or "per_rep".  (The memory test of :877 is not restated: the shapes here are megabytes.)"""
    if not (C <= PG_MAX_SWEEP_COLS and n < p + 1) or "POOLGEN_RIDGE_PER_FOLD" in env:
        return "per_fold"
    return "batched" if n_reps > 1 and "POOLGEN_RIDGE_PER_REP" not in env else "per_rep"


def batched_passes(C, k, n_reps):
    """form_upto (pg_gp.hip:894-916): the column counts of the coefficient passes of a batched call, and whether the first one is
    the short one (repetition 0 alone, :898-899)"""
    total = n_reps * C + k
    short_first = C < GP_CP and 1 + (total - C + GP_CP - 1) // GP_CP == (total + GP_CP - 1) // GP_CP
    out, formed = [], 0
    while formed < total:
        c1 = C if (short_first and formed == 0) else min(formed + GP_CP, total)
        out.append(c1 - formed)
        formed = c1
    return out, short_first


def predict_geometry(n, n_folds, L):
    """PredictPipeline::launch (pg_gp.hip:820-836)"""
    LPr = (L + 1) & ~1
    masses_b = 8 * n_folds * (2 * GP_LMAX + 1)
    chunk = max(4, min(64, (49152 - masses_b) // (8 * n_folds * (LPr + 2))))
    threads = 512 if n > 128 else 256
    groups = threads // (((n + 63) // 64) * 64) if n <= 256 else 1
    grid_y = 1 if groups > 1 else (n + threads - 1) // threads
    lds = 8 * chunk * n_folds * (LPr + 2) + masses_b
    return dict(LPr=LPr, chunk=chunk, threads=threads, groups=groups, grid_y=grid_y, lds=lds,
                variant=(LPr, groups > 1, bool(L & 1)))


def mass_nb(p):
    """ridge_path_params_cols (pg_gp.hip:631): blocks per column of the mass step"""
    return min(1024, max(32, p // 2048))


# ---- pg_popgen.hip -----------------------------------------------------------------------------------------------------------
FTILE = 32                                # :169-171


def fst_tiles(n):
    """:492-493: tiles per edge, upper-triangular tiles"""
    t = (n + FTILE - 1) // FTILE
    return t, t * (t + 1) // 2


def fst_chunk(L):
    """:464-465: loci per chunk of the genome-wide mean, number of chunks, loci in the last one"""
    chunk = max(64, (L + 2047) // 2048)
    nchunks = (L + chunk - 1) // chunk
    return chunk, nchunks, L - (nchunks - 1) * chunk


def fst_slab(n, n_windows):
    """:506: windows per trip of the per-window loop"""
    return max(1, min(n_windows, (1 << 30) // (8 * n * n)))


def blocks_256(items):
    """the (window, pool) and (locus, pool) kernels: one thread per item, 256 per block (:331, :439-441)"""
    return (items + 255) // 256


# ---- pg_kinship.hip ----------------------------------------------------------------------------------------------------------
KIN_WAVES, KIN_PAIR_FLOOR, KIN_FUSE_MAXK = 16, 2.7, 2     # :28, :646, :33


def kin_layout(n):
    """pg_launch_kinship (pg_kinship.hip:685, :698-725, :811, :833): w8 (the 8-wave build up to 64 pools), T tile columns, nb pool
    blocks of Tb tile columns, merged pairs, split, the 13-tile kernel and its narrow-tile bits"""
    T = (n + 15) // 16
    if T <= 13:
        Tb, nb = T, 1
    else:
        Tb, nb = 8, (T + 7) // 8
    merged = nb >= 4 or (nb == 2 and T >= 15)
    if not merged and 2 <= nb <= 3:
        best, best_tb = 1e30, Tb
        for tb in range((T + nb - 1) // nb, 9):
            units = 0.0
            for bi in range(nb):
                for bj in range(bi, nb):
                    Ta, Tbb = min(tb, T - bi * tb), min(tb, T - bj * tb)
                    if Ta <= 0 or Tbb <= 0:
                        units += 1e6
                        continue
                    tiles = Ta * (Ta + 1) // 2 if bi == bj else Ta * Tbb
                    units += max(KIN_PAIR_FLOOR, float((tiles + KIN_WAVES - 1) // KIN_WAVES))
            if units <= best:
                best, best_tb = units, tb
        Tb = best_tb
    spec13 = nb == 1 and T == 13
    return dict(w8=n <= 64, T=T, nb=nb, Tb=Tb, merged=merged, weighted=(not merged and 2 <= nb <= 3),
                split=2 if (merged and nb == 2) else 1, spec13=spec13,
                small=(0 if not spec13 else ((2 if n <= 200 else 0) | 1)))


def kin_fuses(n, k):
    """the fused intercept-only sums: one pool block (:798), phenotypes kept by pg_set_phenotypes (:874: k <= 4 and n <= 256) and
    at most KIN_FUSE_MAXK traits (:798)"""
    return kin_layout(n)["nb"] == 1 and n <= 256 and k <= min(4, KIN_FUSE_MAXK)


# ---- pg_mle.hip --------------------------------------------------------------------------------------------------------------
MLE_MAXP, MLE_MAXP_LDS = 4, 10            # :26-27


def mle_sums_route(n, m, k):
    """pg_mle_kinship_dev :464: the sums Z'g of the m + 1 + k columns [1 | C | Y] and g'g (ss_out_dev) through pg_gp_beta_cols,
    row-major"""
    return beta_route(n, m + 1 + k, colmajor=False, ss=True)
