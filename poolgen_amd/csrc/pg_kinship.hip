// pg_kinship.hip -- S = sum_l g_l g_l^T over a slab of loci, fp64 MFMA (v_mfma_f64_16x16x4_f64).
//
// Reference: `kinship = g.dot(&g.t()) / p` (gwas/ols.rs:291-295) and the X X^T contraction of
// gp::ols (gp/ols.rs:56, base/helpers.rs:222-255).  G is locus-major (p x n, ld), so both MFMA
// operands of a 16x16 output tile are "4 loci x 16 pools" fragments of the SAME rows:
//     A[i][k] = G[l0+k][a0+i]   (lane l: i = l&15, k = l>>4)
//     B[k][j] = G[l0+k][b0+j]   (lane l: j = l&15, k = l>>4)
// i.e. 16 consecutive lanes read 128 contiguous bytes of one locus row -- no transposition.
//
// Decomposition.  One 1024-thread workgroup (16 waves, 4 per SIMD) owns a contiguous slab of
// loci and a pair (bi <= bj) of pool blocks (a block = up to `Tb` 16-pool tiles).  For
// n <= 208 pools there is a single block: the workgroup holds the WHOLE upper triangle of S
// (<= 91 tiles, <= 6 per wave, 4 fp64 accumulators per lane per tile) in registers while it
// streams its loci once from HBM through a double-buffered LDS stage (16 loci per stage; 32 in the 13-tile kernels).
// The contraction is MFMA-bound (intensity n/4 flop per byte); HBM traffic is the single read
// of G.  Each workgroup finally writes its partial tiles to a slab; a second tiny kernel sums
// the slabs in a fixed order (deterministic, no atomics) and mirrors the lower triangle.
#include "pg_common.h"
#include <cstdlib>
#include <cstring>
#include <utility>

namespace {

#ifndef KIN_WAVES_DEF
#define KIN_WAVES_DEF 16
#endif
constexpr int KIN_WAVES = KIN_WAVES_DEF; // 16 (6 tile slots per wave) or 8 (12 slots)
constexpr int KIN_THREADS = 64 * KIN_WAVES;
#ifndef KIN_RING_D
#define KIN_RING_D 3
#endif
constexpr int KIN_FUSE_MAXK = 2; // traits the fused intercept-only pass carries
constexpr int KIN_TPW = 96 / KIN_WAVES;  // max tiles per wave (>= ceil(91 / waves), ceil(81 / waves))
#ifndef KIN_KC_DEF
#define KIN_KC_DEF 16
#endif
constexpr int KIN_KC = KIN_KC_DEF;  // loci per LDS stage (4 loci = one MFMA k-step)
constexpr int KIN_PPT = (KIN_KC * 128 + KIN_THREADS - 1) / KIN_THREADS;  // 16-byte staging pieces per thread per stage (13-tile kernels: per staging half)
// The 13-tile kernels (193..208 pools, 16 waves) run stages of 32 loci: one barrier and one hand-over per 32 loci, and 8 tasks of
// 4 loci for the fused sums.  They are STAGED in halves of KIN_KC loci (same registers, same pieces per thread), and the
// launcher's slab rule stays in units of KIN_KC, so a slab may end in a half stage, which the kernel peels.
constexpr int KC13 = 32;
constexpr bool KIN_HAS13 = (KIN_WAVES == 16); // (the 8-wave build never runs the 13-tile shape and does not build its kernels)

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef unsigned int uint4_t __attribute__((ext_vector_type(4)));
typedef unsigned int uint2_t __attribute__((ext_vector_type(2)));

// v + (v shifted by a DPP control) on the VALU only: the generic __shfl_xor goes through ds_bpermute,
// whose latency would stall the issuing wave in the middle of the MFMA stream.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, true);
    return v + __hiloint2double(hi, lo);
}
// value of lane ((l & 15) + N) % 16 of the same 16-lane row (row_ror:(16 - N) moves data towards higher lanes by 16 - N)
template <int N>
__device__ __forceinline__ double row_from_plus(double v) {
    static_assert(N >= 1 && N <= 15, "row rotation");
    constexpr int CTRL = 0x120 + (16 - N); // row_ror:(16 - N)
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// ---- compile-time helpers ------------------------------------------------------------------------
template <int... I, typename F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F &&f) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F &&f) {
    static_for_impl(std::make_integer_sequence<int, N>{}, f);
}
// row-major enumeration of the upper triangle of a T x T tile grid
constexpr int kin_tri_ti(int t, int T) { int ti = 0; while (ti < T && t >= T - ti) { t -= T - ti; ++ti; } return ti < T ? ti : 0; }
constexpr int kin_tri_tj(int t, int T) { int ti = 0; while (ti < T && t >= T - ti) { t -= T - ti; ++ti; } return ti < T ? ti + t : 0; }
// tile of slot u of wave w (slots past the end of the list recompute tile 0 and are never stored)
constexpr int kin_slot_tile(int w, int u, int T) { return (w + KIN_WAVES_DEF * u) < T * (T + 1) / 2 ? (w + KIN_WAVES_DEF * u) : 0; }

// ---- 13-tile shape: which tiles a wave owns, chosen so that they SHARE fragments ------------------------------
// A fragment "4 loci x 16 pools of tile column c" serves as the A operand of every tile in tile row c and as the B
// operand of every tile in tile column c.  Waves 0..3 own the 3 x 3 triangles on the diagonal (6 tiles from 3
// fragments), waves 4..9 the 2 x 3 blocks (6 tiles from 5 fragments), the rest what is left, grouped for shared
// columns: 69 fragment reads per k-step for the 91 tiles instead of 182, and 23/23/23/22 tiles on the four SIMDs.
constexpr int KIN13_T[16][6][2] = {
    {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}},
    {{3, 3}, {3, 4}, {3, 5}, {4, 4}, {4, 5}, {5, 5}},
    {{6, 6}, {6, 7}, {6, 8}, {7, 7}, {7, 8}, {8, 8}},
    {{9, 9}, {9, 10}, {9, 11}, {10, 10}, {10, 11}, {11, 11}},
    {{0, 3}, {0, 4}, {0, 5}, {1, 3}, {1, 4}, {1, 5}},
    {{0, 6}, {0, 7}, {0, 8}, {1, 6}, {1, 7}, {1, 8}},
    {{0, 9}, {0, 10}, {0, 11}, {1, 9}, {1, 10}, {1, 11}},
    {{3, 6}, {3, 7}, {3, 8}, {4, 6}, {4, 7}, {4, 8}},
    {{3, 9}, {3, 10}, {3, 11}, {4, 9}, {4, 10}, {4, 11}},
    {{6, 9}, {6, 10}, {6, 11}, {7, 9}, {7, 10}, {7, 11}},
    {{2, 4}, {2, 11}, {2, 12}, {4, 12}, {11, 12}, {12, 12}},
    {{2, 5}, {2, 6}, {2, 7}, {5, 6}, {5, 7}, {-1, -1}},
    // (rows 12, 13, 15 in this order so that the four waves of a SIMD -- w, w + 4, w + 8, w + 12 -- carry nearly equal matrix time
    //  once the narrow tiles run on 4 x 4 x 4 blocks: 1339 / 1369 / 1357 / 1334 cycles per 4 loci)
    {{0, 12}, {2, 3}, {3, 12}, {6, 12}, {7, 12}, {-1, -1}},
    {{5, 9}, {5, 10}, {5, 12}, {9, 12}, {10, 12}, {-1, -1}},
    {{2, 8}, {2, 9}, {2, 10}, {8, 9}, {8, 10}, {-1, -1}},
    {{1, 12}, {5, 8}, {5, 11}, {8, 11}, {8, 12}, {-1, -1}},
};
constexpr int kin13_ntiles(int w) { int c = 0; for (int u = 0; u < 6; ++u) c += KIN13_T[w][u][0] >= 0; return c; }
// distinct tile columns of wave w, in order of first use; kin13_col(w, i) = -1 past the end
constexpr int kin13_col(int w, int idx) {
    int seen[12] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, ns = 0;
    for (int u = 0; u < 6; ++u)
        for (int h = 0; h < 2; ++h) {
            const int c = KIN13_T[w][u][h];
            if (c < 0) continue;
            bool dup = false;
            for (int i = 0; i < ns; ++i) dup = dup || seen[i] == c;
            if (!dup) seen[ns++] = c;
        }
    return idx < ns ? seen[idx] : -1;
}
constexpr int kin13_ncols(int w) { int c = 0; while (c < 12 && kin13_col(w, c) >= 0) ++c; return c; }
constexpr int kin13_slot(int w, int col) { int i = 0; while (kin13_col(w, i) != col) ++i; return i; } // fragment register of a column
constexpr int KIN13_MAXC = 6;
constexpr int kin13_ndiag(int w) { int c = 0; for (int u = 0; u < 6; ++u) c += (KIN13_T[w][u][0] >= 0 && KIN13_T[w][u][0] == KIN13_T[w][u][1]); return c; }
constexpr int kin13_diag_index(int w, int u) { int c = 0; for (int v = 0; v < u; ++v) c += (KIN13_T[w][v][0] >= 0 && KIN13_T[w][v][0] == KIN13_T[w][v][1]); return c; }

struct KinParams {
    const double *G;
    int64_t p;
    int64_t ld;
    int64_t loci_per_wg;
    double *slabs; // [gridDim.x][npad * npad]
    int n, T, npad, Tb, nb;
    int split;  // nb == 2: the one pair's tile list (A x B, A x A, B x B: 136 tiles at T = 16) is dealt to `split` = 2
                // workgroups per slab of loci instead of three workgroups of which two are a third full
    int merged; // nb >= 4: no workgroups for the diagonal blocks -- every off-diagonal pair (A, B) also takes 1/(nb-1) of
                // the tiles of A x A and of B x B (64 + 12 + 12 of its 96 tile slots at Tb = 8 instead of 64, or 36 on a
                // diagonal workgroup), and every pool column is staged nb - 1 times instead of nb
    // fused speculative intercept-only sums (FUSE kernels only)
    const double *ytil; // k x 256 centred phenotypes, zero padded
    double *spec;       // p x (2 + k)
    int k;
    // More than one pool-block pair (n > 208): the workgroups that stream the SAME slab of loci are placed on ONE XCD, so that
    // a slab's lines reach HBM once and the other pairs that stage them hit that XCD's L2 (workgroups go to the XCDs round-robin
    // by linear id; with (slab, pair) = blockIdx.(x, y) the pairs of a slab landed on different XCDs and each pool column came
    // from HBM nb - 1 times: 54 GB for the 20 GB of config 4).  xcd_spx = slabs per XCD in that placement, 0 = plain 2-D grid.
    int xcd_spx, npairs, nslab;
    // run-time tile tables: a wave skips the slots it has no tile for (28 tiles on 16 waves: 4 of 32 slots; 10 tiles on 8 waves: 6 of
    // 16) -- their LDS reads and matrix cycles.  4 M loci, ms, without -> with: 32 pools 0.89 -> 0.77, 64: 1.02 -> 0.95, 100: 1.54 ->
    // 1.43, 150: 2.57 -> 2.36, 250 (merged pair lists): 6.83 -> 5.53.  Off for the weighted pairs (wq_n), whose slab lengths are
    // balanced on the slot counts (224 and 300 pools: 10-15 % slower with it), and from four blocks on.
    int skip_dead; // (host side only: selects the kernel instance)
    // Two or three pool blocks without the merged tile lists (n = 209..224, 257..384): the pairs differ in work (a diagonal pair
    // of 8 tile columns has 36 tiles, an off-diagonal one 64, the pairs of a short last block fewer still), so each pair gets its
    // own number of workgroups -- and with it its own slab length -- in proportion to the tile slots its waves run.  With one
    // slab length for all, the diagonal workgroups finished early and a third of the CUs idled (n = 300: 47 of 79 TFLOP/s).
    // wq_n[q] > 0 switches this on: pair q = workgroups wq_first[q] .. + wq_n[q] of a 1-D grid, wq_len[q] loci each.
    int wq_n[6], wq_first[6];
    int64_t wq_len[6];
};

// SMALL (13-tile shape only): the tiles that are not full 16 x 16 blocks of useful products run on v_mfma_f64_4x4x4_4b_f64
// (four independent 4 x 4 x 4 blocks per instruction, a quarter of the matrix-pipe time of a 16 x 16 x 4):
//   * the 13 diagonal tiles need their upper triangle only: 3 instructions (the block diagonals d = 0, 1, 2 of the 4 x 4 grid of
//     4 x 4 blocks; the wrapped block of d = 1 is the transpose of the one block d = 3 would add) instead of 4 instructions' worth;
//   * with n <= 200 pools tile column 12 holds at most 8 pools: 2 instructions (4 row blocks x one 4-pool column block each)
//     per tile instead of 4.
// Lane layout of the instruction (probed on the device, tools/probe_mfma4.hip): A[blk][i][k] in lane 16 k + 4 blk + i,
// B[blk][k][j] in lane 16 k + 4 blk + j, D[blk][i][j] in lane 16 i + 4 blk + j -- so the 16 x 16 fragment of tile column c
// (lane: pool = lane & 15, locus = lane >> 4) IS the A operand whose four blocks are the four 4-pool groups of that column,
// a B operand "column group (blk + d) % 4" is the same register rotated by 4 d lanes inside its 16-lane row (DPP, no LDS), and
// only the 8-pool strip needs reads of its own.  200 pools: 5 200 instead of 5 824 matrix cycles per 4 loci.
// SKIP (run-time tile tables only): see KinParams::skip_dead -- a template parameter because even a never-taken branch around an
// item keeps the compiler from running the fragment reads ahead of the MFMAs (measured: +8..10 % at 224 and 500 pools).
// ODDN (13-tile shape only): the pool count may be odd, so the staging zeroes the second half of a row's last piece; the instance
// for even pool counts carries no such select in its stage loop.
template <bool FUSE, bool SPEC13, int SMALL = 0, bool SKIP = false, bool ODDN = true> // SMALL bits: 1 = diagonal tiles on 4 x 4 blocks, 2 = 8-pool last column (n <= 200) on 4 x 4 blocks
__global__ __launch_bounds__(KIN_THREADS, 1) void k_kinship_syrk(KinParams P) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int fi = lane & 15; // pool within fragment / output column
    const int kq = lane >> 4; // locus within k-step / output row group

    // ---- which slab of loci, which pair of pool blocks ------------------------------------
    int bx = blockIdx.x, by = blockIdx.y;
    if (P.xcd_spx) { // 1-D grid: linear id -> (XCD, position on it) -> (slab, pair); see KinParams::xcd_spx
        const int xcd = blockIdx.x & 7, s = blockIdx.x >> 3, main = P.xcd_spx * P.npairs;
        if (s < main) { bx = xcd * P.xcd_spx + s / P.npairs; by = s % P.npairs; }
        else { const int e = (s - main) * 8 + xcd; bx = 8 * P.xcd_spx + e / P.npairs; by = e % P.npairs; } // the slabs left over
        if (bx >= P.nslab) return;
    }
    int64_t loci_per_wg = P.loci_per_wg;
    if (P.wq_n[0] > 0) { // weighted pairs: see KinParams::wq_n
        int q = 0;
        while (q + 1 < P.npairs && (int)blockIdx.x >= P.wq_first[q + 1]) ++q;
        by = q;
        bx = (int)blockIdx.x - P.wq_first[q];
        loci_per_wg = P.wq_len[q];
    }
    int bi = 0, bj = 0;
    {
        int q = by / P.split;
        const int first = P.merged ? 1 : 0; // merged: pairs with bi < bj only
        for (bi = 0; bi < P.nb; ++bi) {
            const int cnt = P.nb - bi - first;
            if (q < cnt) { bj = bi + first + q; break; }
            q -= cnt;
        }
    }
    const bool diag = (bi == bj);
    const int Ta = min(P.Tb, P.T - bi * P.Tb);
    const int Tbb = min(P.Tb, P.T - bj * P.Tb);
    const int colsA = Ta * 16;
    const int colsB = diag ? 0 : Tbb * 16;
    int ldsld = colsA + colsB;
    if ((ldsld & 31) != 16) ldsld += 16; // rows 2 apart hit disjoint bank halves (ds_read_b64)
    const int a0 = bi * P.Tb * 16;
    const int b0 = bj * P.Tb * 16;
    const int wa = min(colsA, P.n - a0);
    const int wb = diag ? 0 : min(colsB, P.n - b0);
    const int npa = (wa + 1) >> 1, npb = (wb + 1) >> 1;
    const int npr = npa + npb; // 16-byte pieces per staged locus row

    // ---- this wave's tiles ---------------------------------------------------------------
    const int nrect = diag ? 0 : Ta * Tbb;
    const int NA = Ta * (Ta + 1) / 2, NB = Tbb * (Tbb + 1) / 2, part = P.nb - 1;
    const int rankA = bj - 1, rankB = bi; // position of the partner among the other blocks, in block order
    const int cntA = P.merged ? (NA > rankA ? (NA - rankA + part - 1) / part : 0) : 0;
    const int cntB = P.merged ? (NB > rankB ? (NB - rankB + part - 1) / part : 0) : 0;
    const int ntiles = diag ? NA : nrect + cntA + cntB;
    const int split_id = by % P.split;
    // Every wave runs exactly KIN_TPW tile slots so that the k-loop is straight-line code; a slot
    // beyond the tile list recomputes tile 0 into an accumulator that is never stored.
    int acol[KIN_TPW], bcol[KIN_TPW], orow[KIN_TPW], ocol[KIN_TPW];
    bool live[KIN_TPW];
#pragma unroll
    for (int u = 0; u < KIN_TPW; ++u) {
        const int t = split_id + P.split * (wave + KIN_WAVES * u);
        int ti = 0, tj = 0;
        live[u] = t < ntiles;
        int kind = diag ? 1 : 0; // 0: A x B, 1: inside A, 2: inside B
        if (t < ntiles) {
            int q = t, Td = Ta;
            if (!diag && t >= nrect) {
                const bool inA = t - nrect < cntA;
                kind = inA ? 1 : 2;
                q = inA ? rankA + part * (t - nrect) : rankB + part * (t - nrect - cntA);
                Td = inA ? Ta : Tbb;
            }
            if (kind) {
                for (ti = 0; ti < Td; ++ti) {
                    const int cnt = Td - ti;
                    if (q < cnt) { tj = ti + q; break; }
                    q -= cnt;
                }
            } else {
                ti = t / Tbb;
                tj = t - ti * Tbb;
            }
        }
        acol[u] = (kind == 2 ? colsA : 0) + 16 * ti;
        bcol[u] = (kind == 1 ? 0 : colsA) + 16 * tj;
        orow[u] = (kind == 2 ? b0 : a0) + 16 * ti;
        ocol[u] = (kind == 1 ? a0 : b0) + 16 * tj;
    }

    // ---- staging assignment (constant over the stages) -------------------------------------
    int st_loc[KIN_PPT], st_lcol[KIN_PPT];
    int st_gcol[KIN_PPT];
    bool st_on[KIN_PPT], st_two[KIN_PPT];
#pragma unroll
    for (int r = 0; r < KIN_PPT; ++r) {
        const int t = tid + r * KIN_THREADS;
        const int loc = t / npr;
        const int q = t - loc * npr;
        st_on[r] = loc < KIN_KC;
        st_loc[r] = loc;
        int gcol, lcol;
        bool two;
        if (q < npa) {
            gcol = a0 + 2 * q; lcol = 2 * q; two = (2 * q + 1) < wa;
        } else {
            const int q2 = q - npa;
            gcol = b0 + 2 * q2; lcol = colsA + 2 * q2; two = (2 * q2 + 1) < wb;
        }
        st_lcol[r] = lcol;
        st_two[r] = two;
        st_gcol[r] = st_on[r] ? gcol : a0;
        if (!st_on[r]) st_loc[r] = 0;
    }

    const int64_t l_begin = (int64_t)bx * loci_per_wg;
    const int64_t l_end = min(P.p, l_begin + loci_per_wg);
    const int nstages = (l_end > l_begin) ? (int)((l_end - l_begin + KIN_KC - 1) / KIN_KC) : 0; // (SPEC13: half stages)
    const int bufsz = (SPEC13 ? KC13 : KIN_KC) * ldsld;

    // zero both buffers once: the padding columns must stay zero for the edge tiles
    for (int i = tid; i < 2 * bufsz; i += KIN_THREADS) lds[i] = 0.0;
    double *ylds = lds + 2 * bufsz; // FUSE: KIN_FUSE_MAXK x 256 centred phenotypes, then the partial-sum scratch
    if (FUSE)
        for (int i = tid; i < P.k * 256; i += KIN_THREADS) ylds[i] = P.ytil[i];
    __syncthreads();

    // Staging uses raw buffer loads over a descriptor that covers exactly this workgroup's slab:
    // pieces of loci past the slab end are out of range and come back as zeros in hardware, so
    // the loop carries no tail branches and the loads stay in flight across the MFMA block.
    const uint64_t slab_bytes64 = (uint64_t)(l_end > l_begin ? l_end - l_begin : 0) * P.ld * 8;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<double *>(P.G + l_begin * P.ld), 0, (int)(uint32_t)slab_bytes64, 0x00020000);
    uint4_t stage_reg[KIN_PPT];
    uint32_t st_voff[KIN_PPT];
#pragma unroll
    for (int r = 0; r < KIN_PPT; ++r)
        st_voff[r] = st_on[r] ? (uint32_t)(((int64_t)st_loc[r] * P.ld + st_gcol[r]) * 8) : 0xFFFFFFF0u;
    const uint32_t stage_stride = (uint32_t)(KIN_KC * P.ld * 8);
    auto stage_load = [&](int c) {
#pragma unroll
        for (int r = 0; r < KIN_PPT; ++r)
            // the whole offset goes through VGPR: the scalar offset is not range-checked on gfx9
            stage_reg[r] = __builtin_amdgcn_raw_buffer_load_b128(
                rsrc, st_on[r] ? st_voff[r] + (uint32_t)c * stage_stride : 0xFFFFFFF0u, 0, 0);
    };
    auto stage_store = [&](int buf) {
#pragma unroll
        for (int r = 0; r < KIN_PPT; ++r) {
            if (st_on[r]) {
                uint4_t v = stage_reg[r];
                if (!st_two[r]) { v.z = 0u; v.w = 0u; }
                *reinterpret_cast<uint4_t *>(&lds[buf * bufsz + st_loc[r] * ldsld + st_lcol[r]]) = v;
            }
        }
    };

    if (nstages > 0) {
        stage_load(0);
        stage_store(0);
    }
    if constexpr (SPEC13) { // the second half of the first 32-locus stage: rows KIN_KC .. of buffer 0
        if (nstages > 1) {
            stage_load(1);
#pragma unroll
            for (int r = 0; r < KIN_PPT; ++r) {
                if (st_on[r]) {
                    uint4_t v = stage_reg[r];
                    if (!st_two[r]) { v.z = 0u; v.w = 0u; }
                    *reinterpret_cast<uint4_t *>(&lds[(KIN_KC + st_loc[r]) * ldsld + st_lcol[r]]) = v;
                }
            }
        }
    }
    __syncthreads();

    // FUSE: from the stage that is in LDS anyway, wave w also forms the sums an intercept-only fit of
    // locus w of the stage needs (g' = g - g[0]):  sum g', sum g'^2, sum g' ytil_t.  Its 64 lanes cover
    // the pools 4 apiece; the 64 partials per value are transposed through a wave-private LDS scratch
    // so that row v of the wave (16 lanes) holds value v, 4 partials per lane, and a 4-step intra-row
    // DPP shift-add finishes the sum in lanes 15/31/47/63 -- no ds_bpermute, no cross-row step, no
    // extra barrier (a wave's own LDS writes and reads are ordered).  (The 13-tile kernels form the same sums by DPP rows, without
    // the scratch and the phenotype registers: spec_rows below.)
    const int NV = 2 + P.k;
    double *scratch = ylds + KIN_FUSE_MAXK * 256 + wave * (4 * 64); // [4 values][64 lanes]
    // this lane's four pools' centred phenotypes: registers, not one more LDS read per use
    double yreg[KIN_FUSE_MAXK][4];
#pragma unroll
    for (int t = 0; t < KIN_FUSE_MAXK; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) yreg[t][j] = (FUSE && t < P.k) ? ylds[t * 256 + lane + 64 * j] : 0.0;
    auto spec_pass = [&](const double *buf, int64_t lbase) {
#pragma unroll
        for (int jl = 0; jl < KIN_KC / KIN_WAVES; ++jl) {
            const int loc = wave + KIN_WAVES * jl;
            const double *row = buf + loc * ldsld;
            const double shift = row[0]; // same address in every lane: an LDS broadcast
            double s1 = 0.0, s2 = 0.0, sy[KIN_FUSE_MAXK], d[4];
#pragma unroll
            for (int t = 0; t < KIN_FUSE_MAXK; ++t) sy[t] = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int pool = lane + 64 * j;
                // 13-tile shape: 193..208 pools, pitch 208 -- the first three 64-pool groups are always whole
                if (SPEC13 && j < 3) d[j] = row[pool] - shift;
                else {
                    const double gv = row[pool < ldsld ? pool : ldsld - 1];
                    d[j] = (pool < P.n) ? gv - shift : 0.0;
                }
                s1 += d[j];
                s2 = fma(d[j], d[j], s2);
                sy[0] = fma(d[j], yreg[0][j], sy[0]);
            }
            const bool two = P.k > 1; // wave-uniform
            if (two) {
#pragma unroll
                for (int j = 0; j < 4; ++j) sy[1] = fma(d[j], yreg[1][j], sy[1]);
            }
            scratch[lane] = s1;
            scratch[64 + lane] = s2;
            scratch[2 * 64 + lane] = sy[0];
            if (two) scratch[3 * 64 + lane] = sy[1];
            __builtin_amdgcn_wave_barrier();
            const int v = lane >> 4, r = lane & 15;
            const double *sc = scratch + v * 64 + r;
            double tot = (sc[0] + sc[16]) + (sc[32] + sc[48]);
            tot = dpp_add<0x111, 0xf>(tot); // row_shr:1
            tot = dpp_add<0x112, 0xf>(tot); // row_shr:2
            tot = dpp_add<0x114, 0xf>(tot); // row_shr:4
            tot = dpp_add<0x118, 0xf>(tot); // row_shr:8 -> lane 15 of row v holds value v
            const int64_t l = lbase + loc;
            if (r == 15 && v < NV && l < l_end) P.spec[l * NV + v] = tot;
            __builtin_amdgcn_wave_barrier();
        }
    };

    // ---- main loop ------------------------------------------------------------------------------
    // Rolling software pipeline over the (k-step, tile-slot) sequence of a stage: the fragment pair
    // of item q + D is requested before the MFMA of item q is issued (ring of D + 1 pairs in
    // registers).  The stage barrier sits D items before the end of the stage, so every wave still
    // holds D MFMAs' worth of operands when it arrives: the barrier's arrival skew and the first LDS
    // round trip of the next stage hide behind them.
    // W >= 0 (SPEC13 kernels: one block of 13 tiles, 193..208 pools, LDS pitch 208): the body is
    // instantiated once per wave with COMPILE-TIME tile coordinates, so every fragment address is
    // "lane base + immediate" (no per-item address arithmetic; the buffer parity is compile-time as well, see below).
    // W = -1: run-time tile tables, any shape.
    // TPW = tile slots per wave actually run (2..6): a work-group with few tiles (small n, or a
    // diagonal block pair) would otherwise spend most of its matrix-core time on dead slots.
    auto run = [&](auto wc, auto tc) {
        constexpr int W = decltype(wc)::value;
        constexpr int TPW = decltype(tc)::value;
        constexpr int KS = KIN_KC / 4;
        constexpr int NQ = KS * TPW; // items per stage
        constexpr int D = KIN_RING_D, R = KIN_RING_D + 1;
        static_assert(NQ % R == 0 && NQ > 2 * D, "ring indexing assumes the stage length is a multiple of the ring");
        double4_t acc[TPW];
#pragma unroll
        for (int u = 0; u < TPW; ++u) acc[u] = (double4_t){0.0, 0.0, 0.0, 0.0};
#ifndef KIN_SHARED_FRAGS
#define KIN_SHARED_FRAGS 1
#endif
        if constexpr (W >= 0 && KIN_SHARED_FRAGS) {
            // ---- 13-tile shape with shared fragments: per k-step the wave reads its <= 6 distinct fragments once
            // (two register sets: the set of step s + 1 is requested before the MFMAs of step s are issued) and
            // feeds its <= 6 tiles from them.  The stage barrier sits in front of the LAST k-step's MFMAs: their
            // operands are already in registers, and the first reads of the next stage hide behind them.
            constexpr int NC = kin13_ncols(W), NT = kin13_ntiles(W);
            static_assert(KIN_WAVES == 16 && KC13 == 2 * KIN_KC && KC13 == 2 * KIN_WAVES, "a 32-locus stage: two staging halves, 8 four-locus tasks for 8 of the waves");
            static_assert(NC <= KIN13_MAXC, "fragment registers");
            // A stage is KC13 = 32 loci (8 k-steps, one barrier).  Within ONE stage buffer every k-step, tile column, staging row and
            // fused-sum row is a COMPILE-TIME offset from a per-lane base, so a fragment, strip, rotated-diagonal, staging-store or
            // fused-sum row address is "base register + immediate" (32 x 208 x 8 = 53 248 bytes per buffer: inside the 16-bit offset
            // field of the LDS instructions).  The two buffers together (106 496 bytes) are not, so every base is FLIPPED to the other
            // buffer once per stage with one v_add_u32 (at the barrier; the loop runs two stages per trip, so the sign of the flip is
            // compile-time: + in the stage that computes from buffer 0, - in the other).  The flipped value goes through an empty asm
            // statement: without it the compiler sees that "base + BUF - BUF" is loop-invariant and keeps BOTH values of every base
            // in registers, which the fused kernel does not have.
            constexpr int LD13 = 208, HALF13 = KIN_KC * LD13, BUF13 = KC13 * LD13; // row pitch, doubles per staging half and per stage buffer
            constexpr int KSW = KC13 / 4, KSH = KIN_KC / 4;                        // k-steps of a whole stage and of a half stage
            static_assert(KSW % 2 == 0 && KSH % 2 == 0, "fragment sets alternate with the k-step parity");
            static_assert(BUF13 * 8 < 65536, "a stage buffer must lie inside the 16-bit offset field of the LDS instructions");
            typedef __attribute__((address_space(3))) double lds_f64;
            typedef __attribute__((address_space(3))) uint4_t lds_u128;
            // One ds_read_b64 per operand, its whole offset in the instruction: left to itself the compiler pairs the reads into
            // ds_read2_b64, whose two 8-bit offsets reach 2 040 bytes -- a k-step is 6 656 bytes from the next -- and pays for every
            // pair with a v_add_u32 that builds its base.  `base` is a byte address in LDS, `d` an offset in doubles.
            auto ldv = [](uint32_t base, int d) __attribute__((always_inline)) { return *(const volatile lds_f64 *)(base + (uint32_t)(d * 8)); };
            auto flip = [](uint32_t &base, auto up) __attribute__((always_inline)) {
                if constexpr (decltype(up)::value) base += (uint32_t)(BUF13 * 8);
                else base -= (uint32_t)(BUF13 * 8);
                asm("" : "+v"(base));
            };
            const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_f64 *)lds;
            double fr[2][KIN13_MAXC];
            uint32_t lb = lds0 + (uint32_t)((kq * LD13 + fi) * 8);
            // which of this wave's tiles are strip tiles (r, 12), r < 12
            constexpr bool has_strip = [] { bool h = false; for (int u = 0; u < 6; ++u) h = h || (KIN13_T[W][u][0] >= 0 && KIN13_T[W][u][0] < 12 && KIN13_T[W][u][1] == 12); return h; }();
            double bs[2][2];                          // strip B operands: pools 192 + 4 c + (lane & 3), c = 0, 1
            uint32_t lbs = lds0 + (uint32_t)((kq * LD13 + 192 + (lane & 3)) * 8);
            // diagonal tiles: the B operands of the block diagonals d = 1, 2 = the tile's fragment rotated by 4 d lanes inside its
            // 16-lane row.  Read from LDS at the rotated address (a DPP rotation is VALU work on the port the MFMAs issue from:
            // measured, it ate the saving)
            constexpr int ND = (SMALL & 1) ? kin13_ndiag(W) : 0;
            double bd[2][ND > 0 ? ND : 1][2];
            uint32_t lbr1 = lds0 + (uint32_t)((kq * LD13 + ((fi + 4) & 15)) * 8), lbr2 = lds0 + (uint32_t)((kq * LD13 + ((fi + 8) & 15)) * 8);
            auto load_set = [&](auto sc, auto pc) __attribute__((always_inline)) { // k-step sc of the buffer the bases point at
                constexpr int s2 = decltype(sc)::value, par = decltype(pc)::value;
                constexpr int o = 4 * s2 * LD13;
                static_for<NC>([&](auto cc) __attribute__((always_inline)) {
                    constexpr int ci = decltype(cc)::value;
                    fr[par][ci] = ldv(lb, o + 16 * kin13_col(W, ci));
                });
                if constexpr ((SMALL & 2) != 0 && has_strip) {
                    bs[par][0] = ldv(lbs, o);
                    bs[par][1] = ldv(lbs, o + 4);
                }
                if constexpr (ND > 0) {
                    static_for<NT>([&](auto uc) __attribute__((always_inline)) {
                        constexpr int u = decltype(uc)::value;
                        if constexpr (KIN13_T[W][u][0] == KIN13_T[W][u][1]) {
                            constexpr int di = kin13_diag_index(W, u);
                            bd[par][di][0] = ldv(lbr1, o + 16 * KIN13_T[W][u][0]);
                            bd[par][di][1] = ldv(lbr2, o + 16 * KIN13_T[W][u][0]);
                        }
                    });
                }
            };
            auto mfma_set = [&](auto pc) __attribute__((always_inline)) {
                constexpr int par = decltype(pc)::value;
                static_for<NT>([&](auto uc) __attribute__((always_inline)) {
                    constexpr int u = decltype(uc)::value;
                    constexpr int ti = KIN13_T[W][u][0], tj = KIN13_T[W][u][1];
                    const double fa = fr[par][kin13_slot(W, ti)];
                    if constexpr ((SMALL & 1) != 0 && ti == tj) {
                        // diagonal tile: block diagonals d = 0, 1, 2 of its 4 x 4 grid of 4 x 4 blocks
                        acc[u][0] = __builtin_amdgcn_mfma_f64_4x4x4f64(fa, fa, acc[u][0], 0, 0, 0);
                        acc[u][1] = __builtin_amdgcn_mfma_f64_4x4x4f64(fa, bd[par][kin13_diag_index(W, u)][0], acc[u][1], 0, 0, 0);
                        acc[u][2] = __builtin_amdgcn_mfma_f64_4x4x4f64(fa, bd[par][kin13_diag_index(W, u)][1], acc[u][2], 0, 0, 0);
                    } else if constexpr ((SMALL & 2) != 0 && tj == 12 && ti != tj) {
                        acc[u][0] = __builtin_amdgcn_mfma_f64_4x4x4f64(fa, bs[par][0], acc[u][0], 0, 0, 0);
                        acc[u][1] = __builtin_amdgcn_mfma_f64_4x4x4f64(fa, bs[par][1], acc[u][1], 0, 0, 0);
                    } else {
                        acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, fr[par][kin13_slot(W, tj)], acc[u], 0, 0, 0);
                    }
                });
            };
            // ---- staging of this wave's pieces.  193..208 pools are 97..104 pieces per locus row, 1552..1664 per staging half (KIN_KC loci), so with the
            // wave known at compile time piece r of its lanes is on in every lane (kind 2: no predicate at all), in no lane (kind 0: the
            // piece does not exist for this wave -- no load, no store, no registers) or decided per lane (kind 1: under the exec mask).
            // The byte offset of a piece is a kept register that advances by one staging half (KIN_KC loci) per load: a stage is
            // staged as two halves one after the other through the SAME registers, pieces and kinds.
            constexpr auto st_kind = [](int r) { const int t0 = W * 64 + r * KIN_THREADS; return t0 + 63 < KIN_KC * 97 ? 2 : (t0 >= KIN_KC * 104 ? 0 : 1); };
            uint4_t sreg[KIN_PPT];
            uint32_t voff[KIN_PPT];
            uint32_t sdst[KIN_PPT]; // byte address of the piece in the buffer that is NOT computed from (flipped with the other bases)
#pragma unroll
            for (int r = 0; r < KIN_PPT; ++r) {
                sreg[r] = (uint4_t){0u, 0u, 0u, 0u};
                voff[r] = st_voff[r] + stage_stride; // (both halves of the first stage were staged by the prologue)
                sdst[r] = lds0 + (uint32_t)((BUF13 + st_loc[r] * LD13 + st_lcol[r]) * 8); // 16-byte aligned: even column, pitch 208
            }
            auto st_load = [&]() __attribute__((always_inline)) { // the pieces of the next half of the NEXT stage
                static_for<KIN_PPT>([&](auto rc) __attribute__((always_inline)) {
                    constexpr int r = decltype(rc)::value;
                    if constexpr (st_kind(r) == 2) {
                        voff[r] += stage_stride;
                        sreg[r] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff[r], 0, 0);
                    } else if constexpr (st_kind(r) == 1) {
                        if (st_on[r]) {
                            voff[r] += stage_stride;
                            sreg[r] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff[r], 0, 0);
                        }
                    }
                });
            };
            auto st_store = [&](auto hc) __attribute__((always_inline)) { // into half hc of the other buffer
                constexpr int H = decltype(hc)::value;
                static_for<KIN_PPT>([&](auto rc) __attribute__((always_inline)) {
                    constexpr int r = decltype(rc)::value;
                    if constexpr (st_kind(r) != 0) {
                        uint4_t v = sreg[r];
                        if constexpr (ODDN) { // the last piece of a row of an odd pool count carries one pool
                            if (!st_two[r]) { v.z = 0u; v.w = 0u; }
                        }
                        if (st_kind(r) == 2 || st_on[r]) *(lds_u128 *)(sdst[r] + (uint32_t)(H * HALF13 * 8)) = v;
                    }
                });
            };
            // ---- FUSE: the per-locus sums by DPP rows.  A TASK is 4 consecutive loci of the stage: row r = lane >> 4 of the wave is
            // locus r of the task, and lane i = lane & 15 of the row sums the 13 pools i, i + 16, .., i + 192 of that locus -- slot j
            // of the chain is tile column j, so its address is the fragment base `lb` plus an immediate (k-step = task, column j).
            // Within a 32-lane half the rows r, r + 1 and i = 0..15 read 32 consecutive doubles (pitch 208 = 16 mod 32): no bank
            // conflict; the centred phenotype of the slot is the same address in all four rows (a broadcast over 16 banks).
            // Only slot 12 (pools 192 + i) can lie past the last pool: such a lane reads column 0 of its row, the shift itself, so
            // its d is +0.0 exactly -- no select, no correction after the sum (which would cancel on near-fixed loci) -- and its
            // phenotype is the zero padding.  The four intra-row DPP shift-adds per value leave each locus's total in lane 15 of
            // its row: no transpose, no scratch, no wave barrier.  13 x (sub, add, fma, fma) + 3 x 4 DPP adds = 64 f64
            // instructions per 4 loci and one trait, 13 x 5 + 16 = 81 for two.  The order of the operations of a row does not
            // depend on the task or the stage kind, so a locus has the same sums wherever it sits in a slab.
            // The sums leave through a buffer descriptor that ends with this workgroup's loci (a locus past the end is out of range
            // and dropped by the hardware), offset and lane predicate kept.
            uint32_t srow0 = lds0 + (uint32_t)(kq * LD13 * 8), srow12 = lds0 + (uint32_t)((kq * LD13 + (fi + 192 < P.n ? fi + 192 : 0)) * 8);
            // (behind the two stage buffers: not flipped, and past the 16-bit offset field -- hidden from the compiler like the flipped
            //  bases, or it keeps the small part and pays every read with a v_add_u32 of the large one)
            uint32_t ybase = lds0 + (uint32_t)((2 * BUF13 + fi) * 8);
            if constexpr (FUSE) asm("" : "+v"(ybase));
            const bool sp_on = fi == 15;
            // a wave's task is (W & 7) wherever it has one (see below), so the row's offset in the sums is kept whole and advances by one stage
            uint32_t sp_voff = (uint32_t)((4 * (W & 7) + kq) * 8) * (uint32_t)NV;
            const __amdgpu_buffer_rsrc_t srsrc = __builtin_amdgcn_make_buffer_rsrc(
                FUSE ? P.spec + l_begin * NV : nullptr, 0, FUSE ? (int)(uint32_t)((uint64_t)(l_end > l_begin ? l_end - l_begin : 0) * NV * 8) : 0, 0x00020000);
            auto spec_rows = [&](auto nyc) __attribute__((always_inline)) { // task W & 7 of the buffer the bases point at, NY traits
                constexpr int NY = decltype(nyc)::value, ro = 4 * (W & 7) * LD13;
                const double shift = ldv(srow0, ro); // the same address in the 16 lanes of a row: a broadcast
                double s1 = 0.0, s2 = 0.0, sy[NY];
#pragma unroll
                for (int t = 0; t < NY; ++t) sy[t] = 0.0;
                static_for<13>([&](auto jc) __attribute__((always_inline)) {
                    constexpr int j = decltype(jc)::value;
                    const double d = (j < 12 ? ldv(lb, ro + 16 * j) : ldv(srow12, ro)) - shift;
                    s1 += d;
                    s2 = fma(d, d, s2);
#pragma unroll
                    for (int t = 0; t < NY; ++t) sy[t] = fma(d, ldv(ybase, t * 256 + 16 * j), sy[t]);
                });
                double tot[2 + NY];
                tot[0] = s1; tot[1] = s2;
#pragma unroll
                for (int t = 0; t < NY; ++t) tot[2 + t] = sy[t];
#pragma unroll
                for (int v = 0; v < 2 + NY; ++v) tot[v] = dpp_add<0x111, 0xf>(tot[v]); // row_shr:1
#pragma unroll
                for (int v = 0; v < 2 + NY; ++v) tot[v] = dpp_add<0x112, 0xf>(tot[v]); // row_shr:2
#pragma unroll
                for (int v = 0; v < 2 + NY; ++v) tot[v] = dpp_add<0x114, 0xf>(tot[v]); // row_shr:4
#pragma unroll
                for (int v = 0; v < 2 + NY; ++v) tot[v] = dpp_add<0x118, 0xf>(tot[v]); // row_shr:8 -> lane 15 of row r holds the totals of locus r
                if (sp_on) {
#pragma unroll
                    for (int v = 0; v < 2 + NY; ++v)
                        __builtin_amdgcn_raw_buffer_store_b64((uint2_t){(uint32_t)__double2loint(tot[v]), (uint32_t)__double2hiint(tot[v])}, srsrc,
                                                              sp_voff + (uint32_t)(v * 8), 0, 0);
                }
            };
            auto spec13 = [&]() __attribute__((always_inline)) {
                if (P.k > 1) spec_rows(std::integral_constant<int, 2>{}); // wave-uniform
                else spec_rows(std::integral_constant<int, 1>{});
            };
            // FUSE: the 8 tasks of a stage go to the waves 0 .. 7 when the stage computes from buffer 0 and to the waves 8 .. 15 when it
            // computes from buffer 1 (the parity is compile-time, and a SIMD holds the waves W, W + 4, W + 8, W + 12): two tasks per
            // SIMD and stage, one task per wave and 64 loci.  The two waves of a SIMD that have a task do it in different k-steps
            // of the 8; none in the barrier's (the last), and none in the first, where every wave's first reads of the new stage
            // are in the LDS queue.  A half stage has 4 tasks: one wave per SIMD (0 .. 3), in its second k-step.
            // (measured, fused kernel at 200 pools x 10 M loci, three runs each, interleaved on one box, profiles/kin_rowsums_ab.txt:
            //  k-steps 1, 4: 6.83-6.88 ms; 1, 5: 6.82-6.90; 1, 3: 6.90-6.97; 1, 2: 6.98-7.04; the parent's chain: 7.06-7.09;
            //  and on another box 1, 4: 6.68-6.70; 2, 5: 6.77-6.80; the parent: 6.83-6.87)
            constexpr int spec_step = ((W / 4) & 1) == 0 ? 1 : 4, spec_step_half = 1;
            // One whole stage, computed from the buffer the read bases point at (buffer B).  Staging of the next stage into the
            // OTHER buffer: its first half is requested at the top and written in the middle, its second half is requested there
            // and written in front of the barrier.  Both writes are safe without a further barrier: the other buffer was last read
            // in the previous stage, whose fragment reads (the last set is requested in front of that stage's barrier) and fused-sum
            // reads (spec_step < KSW - 1) all precede that stage's barrier in program order and have returned there (__syncthreads
            // waits for the wave's LDS operations), so no wave still reads it once any wave is past that barrier; and its next
            // reader starts behind THIS stage's barrier, which both writes precede.  `more`: a stage or a half stage follows (if
            // only a half follows, the second half's pieces lie past the slab's end: the descriptor returns zeros, which nobody
            // reads; the launcher's cap on a slab leaves the room of one half for these offsets).
            auto stage = [&](auto bc, const auto more) __attribute__((always_inline)) {
                constexpr bool up = decltype(bc)::value == 0;
                if (more) st_load();
                static_for<KSW>([&](auto sc) __attribute__((always_inline)) {
                    constexpr int s2 = decltype(sc)::value;
                    if constexpr (FUSE && (W < 8) == up && s2 == spec_step) spec13();
                    if constexpr (s2 == KSW / 2 - 1) {
                        if (more) { st_store(std::integral_constant<int, 0>{}); st_load(); }
                    }
                    if constexpr (s2 + 1 < KSW) {
                        load_set(std::integral_constant<int, s2 + 1>{}, std::integral_constant<int, (s2 + 1) & 1>{});
                    } else {
                        if (more) st_store(std::integral_constant<int, 1>{});
                        __syncthreads();
                        flip(lb, std::bool_constant<up>{});
                        if constexpr ((SMALL & 2) != 0 && has_strip) flip(lbs, std::bool_constant<up>{});
                        if constexpr (ND > 0) { flip(lbr1, std::bool_constant<up>{}); flip(lbr2, std::bool_constant<up>{}); }
                        if constexpr (FUSE) {
                            flip(srow0, std::bool_constant<up>{}); flip(srow12, std::bool_constant<up>{});
                            sp_voff += (uint32_t)(KC13 * 8) * (uint32_t)NV;
                        }
                        static_for<KIN_PPT>([&](auto rc) __attribute__((always_inline)) {
                            if constexpr (st_kind(decltype(rc)::value) != 0) flip(sdst[decltype(rc)::value], std::bool_constant<!up>{});
                        });
                        if (more) load_set(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
                    }
                    mfma_set(std::integral_constant<int, s2 & 1>{});
                });
            };
            // the half stage a slab may end in: the first KIN_KC rows of the buffer the bases point at, its 4 tasks on the waves 0 .. 3, nothing follows
            auto half_stage = [&]() __attribute__((always_inline)) {
                static_for<KSH>([&](auto sc) __attribute__((always_inline)) {
                    constexpr int s2 = decltype(sc)::value;
                    if constexpr (FUSE && W < 4 && s2 == spec_step_half) spec13();
                    if constexpr (s2 + 1 < KSH) load_set(std::integral_constant<int, s2 + 1>{}, std::integral_constant<int, (s2 + 1) & 1>{});
                    mfma_set(std::integral_constant<int, s2 & 1>{});
                });
            };
            const int nwhole = nstages >> 1;
            const bool half = (nstages & 1) != 0;
            if (nstages > 0) load_set(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
            // two stages per trip (inside the loop the first always has a successor); an odd count of whole stages ends with a peeled
            // stage, and a slab of an odd number of halves with the half stage
            int c = 0;
            for (; c + 1 < nwhole; c += 2) {
                stage(std::integral_constant<int, 0>{}, std::true_type{});
                stage(std::integral_constant<int, 1>{}, c + 2 < nwhole || half);
            }
            if (c < nwhole) stage(std::integral_constant<int, 0>{}, half);
            if (half) half_stage();
            double *slab = P.slabs + (size_t)bx * P.npad * P.npad;
            static_for<NT>([&](auto uc) __attribute__((always_inline)) {
                constexpr int u = decltype(uc)::value;
                constexpr int ti = KIN13_T[W][u][0], tj = KIN13_T[W][u][1];
                constexpr int r0 = 16 * ti, c0 = 16 * tj;
                // 4 x 4 blocks: this lane holds D[blk][i][j] with i = lane >> 4, blk = (lane >> 2) & 3, j = lane & 3
                const int bi = lane >> 4, bb = (lane >> 2) & 3, bj = lane & 3;
                if constexpr ((SMALL & 1) != 0 && ti == tj) {
                    // d = 0: block (bb, bb); d = 1: (bb, bb + 1), the wrapped (3, 0) stored as its transpose (0, 3); d = 2: (0, 2), (1, 3)
                    slab[(size_t)(r0 + 4 * bb + bi) * P.npad + c0 + 4 * bb + bj] = acc[u][0];
                    if (bb < 3) slab[(size_t)(r0 + 4 * bb + bi) * P.npad + c0 + 4 * (bb + 1) + bj] = acc[u][1];
                    else slab[(size_t)(r0 + bj) * P.npad + c0 + 12 + bi] = acc[u][1];
                    if (bb < 2) slab[(size_t)(r0 + 4 * bb + bi) * P.npad + c0 + 4 * (bb + 2) + bj] = acc[u][2];
                } else if constexpr ((SMALL & 2) != 0 && tj == 12 && ti != tj) {
                    slab[(size_t)(r0 + 4 * bb + bi) * P.npad + c0 + bj] = acc[u][0];
                    slab[(size_t)(r0 + 4 * bb + bi) * P.npad + c0 + 4 + bj] = acc[u][1];
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) slab[(size_t)(r0 + kq + 4 * r) * P.npad + c0 + fi] = acc[u][r];
                }
            });
            return;
        }
        double fa[R], fb[R];
        const double *lanebase = lds + kq * ldsld + fi; // + buffer + 4 s ldsld + tile column
        auto frag_load = [&](const double *bufbase, auto qc) {
            constexpr int q = decltype(qc)::value;
            constexpr int s = q / TPW, u = q % TPW;
            if constexpr (W >= 0) {
                if constexpr (W + KIN_WAVES * u >= 91) return; // no such tile: the slot is simply skipped
                constexpr int t = kin_slot_tile(W, u, 13);
                constexpr int ao = 4 * s * 208 + 16 * kin_tri_ti(t, 13);
                constexpr int bo = 4 * s * 208 + 16 * kin_tri_tj(t, 13);
                fa[q % R] = bufbase[ao];
                fb[q % R] = bufbase[bo];
            } else {
                if constexpr (SKIP) { if (!live[u]) return; } // (wave-uniform) a slot beyond this wave's tiles: neither its reads nor its matrix cycles
                const double *row = bufbase + 4 * s * ldsld;
                fa[q % R] = row[acol[u]];
                fb[q % R] = row[bcol[u]];
            }
        };
        auto mfma_item = [&](auto qc) {
            constexpr int q = decltype(qc)::value;
            constexpr int u = q % TPW;
            if constexpr (W >= 0 && W + KIN_WAVES * u >= 91) return;
            if constexpr (W < 0 && SKIP) { if (!live[u]) return; }
            acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[q % R], fb[q % R], acc[u], 0, 0, 0);
        };
        if (nstages > 0)
            static_for<D>([&](auto qc) { frag_load(lanebase, qc); });
        for (int c = 0; c < nstages; ++c) {
            const bool more = (c + 1) < nstages;
            if (more) stage_load(c + 1);
            const double *buf = lds + (c & 1) * bufsz;
            const double *fb0 = lanebase + (c & 1) * bufsz;
            const double *fb1 = lanebase + ((c + 1) & 1) * bufsz;
            // FUSE: the per-locus sums are VALU/LDS work that only overlaps the matrix cores if the waves of a
            // SIMD do it at DIFFERENT times: with compile-time wave ids (W >= 0) wave w of SIMD w % 4 runs its
            // spec_pass after item (w / 4) * NQ / 4 of the MFMA block instead of all four at its end.
#ifndef KIN_SPEC_STAGGER
#define KIN_SPEC_STAGGER 1
#endif
            constexpr int spec_at = (FUSE && W >= 0 && KIN_SPEC_STAGGER) ? ((W / 4) % 4) * ((NQ - D) / 4) : -1;
            static_for<NQ - D>([&](auto qc) {
                if constexpr (decltype(qc)::value == spec_at) spec_pass(buf, l_begin + (int64_t)c * KIN_KC);
                frag_load(fb0, std::integral_constant<int, decltype(qc)::value + D>{});
                mfma_item(qc);
            });
            if (more) stage_store((c + 1) & 1);
            if (FUSE && spec_at < 0) spec_pass(buf, l_begin + (int64_t)c * KIN_KC); // staging registers are free again here
            __syncthreads();
            static_for<D>([&](auto dc) {
                constexpr int q = NQ - D + decltype(dc)::value;
                if (more) frag_load(fb1, std::integral_constant<int, q + D - NQ>{});
                mfma_item(std::integral_constant<int, q>{});
            });
        }
        // ---- write this workgroup's partial tiles -----------------------------------------------
        // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg.
        double *slab = P.slabs + (size_t)bx * P.npad * P.npad;
        static_for<TPW>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            bool on;
            int r0, c0;
            if constexpr (W >= 0) {
                constexpr int t = W + KIN_WAVES * u;
                on = t < 91;
                r0 = 16 * kin_tri_ti(kin_slot_tile(W, u, 13), 13);
                c0 = 16 * kin_tri_tj(kin_slot_tile(W, u, 13), 13);
            } else {
                on = live[u]; r0 = orow[u]; c0 = ocol[u];
            }
            if (on) {
#pragma unroll
                for (int r = 0; r < 4; ++r) slab[(size_t)(r0 + kq + 4 * r) * P.npad + c0 + fi] = acc[u][r];
            }
        });
    };
    if constexpr (SPEC13) {
        switch (wave) {
        case 0: run(std::integral_constant<int, 0>{}, std::integral_constant<int, KIN_TPW>{}); break;
        case 1: run(std::integral_constant<int, 1>{}, std::integral_constant<int, KIN_TPW>{}); break;
        case 2: run(std::integral_constant<int, 2>{}, std::integral_constant<int, KIN_TPW>{}); break;
        case 3: run(std::integral_constant<int, 3>{}, std::integral_constant<int, KIN_TPW>{}); break;
        case 4: run(std::integral_constant<int, 4>{}, std::integral_constant<int, KIN_TPW>{}); break;
        case 5: run(std::integral_constant<int, 5>{}, std::integral_constant<int, KIN_TPW>{}); break;
        case 6: run(std::integral_constant<int, 6>{}, std::integral_constant<int, KIN_TPW>{}); break;
#if KIN_WAVES_DEF == 8
        default: run(std::integral_constant<int, 7>{}, std::integral_constant<int, KIN_TPW>{}); break;
#else
        case 7: run(std::integral_constant<int, 7>{}, std::integral_constant<int, KIN_TPW>{}); break;
        case 8: run(std::integral_constant<int, 8>{}, std::integral_constant<int, KIN_TPW>{}); break;
        case 9: run(std::integral_constant<int, 9>{}, std::integral_constant<int, KIN_TPW>{}); break;
        case 10: run(std::integral_constant<int, 10>{}, std::integral_constant<int, KIN_TPW>{}); break;
        case 11: run(std::integral_constant<int, 11>{}, std::integral_constant<int, KIN_TPW>{}); break;
        case 12: run(std::integral_constant<int, 12>{}, std::integral_constant<int, KIN_TPW>{}); break;
        case 13: run(std::integral_constant<int, 13>{}, std::integral_constant<int, KIN_TPW>{}); break;
        case 14: run(std::integral_constant<int, 14>{}, std::integral_constant<int, KIN_TPW>{}); break;
        default: run(std::integral_constant<int, 15>{}, std::integral_constant<int, KIN_TPW>{}); break;
#endif
        }
    } else {
        constexpr std::integral_constant<int, -1> any{};
        switch ((ntiles + KIN_WAVES - 1) / KIN_WAVES) {
        case 0: case 1: case 2: run(any, std::integral_constant<int, 2>{}); break;
        case 3: run(any, std::integral_constant<int, 3>{}); break;
        case 4: run(any, std::integral_constant<int, 4>{}); break;
        case 5: run(any, std::integral_constant<int, 5>{}); break;
        default: run(any, std::integral_constant<int, KIN_TPW>{}); break;
        }
    }
}

// Sum the per-workgroup slabs in a FIXED order and mirror: S[i][j] = S[j][i] = sum_w slab_w[i][j] for
// i <= j (only upper-triangular tiles were written).  256 threads = 64 columns x 4 slab groups: group g
// adds slabs g, g+4, ... in order, then (g0 + g1) + (g2 + g3) -- deterministic, no atomics, and four
// times the loads in flight of a one-thread-per-entry loop (the slabs are 88 MB at n = 200).
constexpr double KIN_PAIR_FLOOR = 2.7; // slots' worth of time a block pair costs at least (stage hand-over)
struct KinCounts { int blk, nb, n[6]; }; // weighted pairs: slabs that hold the tiles of block pair q (row-major upper triangle); blk = 0: all
__global__ __launch_bounds__(256) void k_kinship_reduce(const double *__restrict__ slabs, int nslabs, int npad, int n,
                                                        double add_const, double *__restrict__ S, const KinCounts C) {
    __shared__ double part[4][64];
    const int jj = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + jj;
    const int i = blockIdx.y;
    const bool on = i < n && j < n && i <= j;
    double s = 0.0;
    if (on && C.blk) {
        const int bi = i / C.blk, bj = j / C.blk;
        nslabs = C.n[bi * C.nb - bi * (bi - 1) / 2 + (bj - bi)];
    }
    if (on) {
        const size_t off = (size_t)i * npad + j;
        const size_t stride = (size_t)npad * npad;
        for (int w = grp; w < nslabs; w += 4) s += slabs[w * stride + off];
    }
    part[grp][jj] = s;
    __syncthreads();
    if (on && grp == 0) {
        const double t = ((part[0][jj] + part[1][jj]) + (part[2][jj] + part[3][jj])) + add_const;
        S[(size_t)i * n + j] = t;
        S[(size_t)j * n + i] = t;
    }
}

} // namespace

#ifndef KIN_LAUNCH_NAME
#define KIN_LAUNCH_NAME pg_launch_kinship
#endif
int KIN_LAUNCH_NAME(pg_ctx *ctx, const double *G, int64_t p, int n, int64_t ld, double *S,
                      bool add_intercept, int kid, bool allow_fuse) {
#if KIN_WAVES_DEF == 16
    // Up to 64 pools (<= 10 tiles) a 16-wave workgroup leaves most of its waves without a tile: the same kernel built for 8-wave
    // workgroups (pg_kinship_w8.hip) takes over -- 1.36 -> 1.01 ms per 4 M loci at 48 and 64 pools; from 100 pools on it is no
    // faster, at 150 slower (profiles/r03_kinship_small_n.log).
    if (n <= 64) return pg_launch_kinship_w8(ctx, G, p, n, ld, S, add_intercept, kid, allow_fuse);
#endif

    PG_CHECK(ctx, G && S, "kinship: null pointer");
    PG_CHECK(ctx, p > 0 && n > 0, "kinship: need p > 0 and n > 0 (p=%lld n=%d)", (long long)p, n);
    PG_CHECK(ctx, ld >= n && (ld % 2) == 0, "kinship: ld (%lld) must be even and >= n (%d)",
             (long long)ld, n);
    PG_CHECK(ctx, (reinterpret_cast<uintptr_t>(G) & 15) == 0, "kinship: G must be 16-byte aligned");
    PG_HIP(ctx, hipSetDevice(ctx->device));
    const int cus = ctx->cus;

    KinParams P;
    P.G = G; P.p = p; P.ld = ld; P.n = n;
    P.T = (n + 15) / 16;
    P.npad = P.T * 16;
    if (P.T <= 13) { P.Tb = P.T; P.nb = 1; }
    else { P.Tb = 8; P.nb = (P.T + 7) / 8; }
    // nb >= 4: 64 + 2 * ceil(36 / (nb - 1)) <= 96 slots; nb == 2: measured -- a win at T = 15, 16 (7.6 -> 6.9 ms at n = 240..256,
    // 4 M loci), a loss at T = 14 where the diagonal workgroups stage few columns
    P.merged = (P.nb >= 4 || (P.nb == 2 && P.T >= 15)) ? 1 : 0;
    if (!P.merged && P.nb >= 2 && P.nb <= 3) {
        // the block size that runs the fewest tile slots over all pairs (T = 17: blocks of 6, 6, 5 tile columns = 13 slot units
        // where 8, 8, 1 ran 16)
        // (a pair with two slots is bound by its stage hand-over, not by its MFMAs: it costs about 2.7 slots' worth -- measured
        //  at T = 14, where blocks of 7 + 7 (2, 2 and 4 slots) ran 5.98 ms against 5.46 ms for 8 + 6 (3, 2 and 3))
        double best = 1e30;
        int best_tb = P.Tb;
        for (int tb = (P.T + P.nb - 1) / P.nb; tb <= 8; ++tb) {
            double units = 0.0;
            for (int bi = 0; bi < P.nb; ++bi)
                for (int bj = bi; bj < P.nb; ++bj) {
                    const int Ta = std::min(tb, P.T - bi * tb), Tbb = std::min(tb, P.T - bj * tb);
                    if (Ta <= 0 || Tbb <= 0) { units += 1e6; continue; }
                    const int tiles = bi == bj ? Ta * (Ta + 1) / 2 : Ta * Tbb;
                    units += std::max(KIN_PAIR_FLOOR, (double)((tiles + KIN_WAVES - 1) / KIN_WAVES));
                }
            if (units <= best) { best = units; best_tb = tb; }
        }
        P.Tb = best_tb;
    }
    P.split = (P.merged && P.nb == 2) ? 2 : 1;                                               // nb == 2: all 136 tiles, 68 + 68
    const int npairs = (P.merged ? P.nb * (P.nb - 1) / 2 : P.nb * (P.nb + 1) / 2) * P.split;
    int nslab = cus / npairs;
    if (nslab < 1) nslab = 1;
    const int64_t max_slabs = (p + KIN_KC - 1) / KIN_KC;
    if (nslab > max_slabs) nslab = (int)max_slabs;
    P.loci_per_wg = (p + nslab - 1) / nslab;
    P.loci_per_wg = (P.loci_per_wg + KIN_KC - 1) / KIN_KC * KIN_KC;
    // a slab must be addressable with the 32-bit offsets of its buffer descriptor
    const int64_t max_loci_per_wg = ((int64_t)0xFFFFFFF0 / (ld * 8)) / KIN_KC * KIN_KC - KIN_KC;
    if (P.loci_per_wg > max_loci_per_wg) P.loci_per_wg = max_loci_per_wg;
    nslab = (int)((p + P.loci_per_wg - 1) / P.loci_per_wg);

    P.npairs = npairs; P.nslab = nslab;
    P.skip_dead = P.nb <= 2 ? 1 : 0; // (from 4 blocks on the lists are full: 500 pools 10.17 -> 10.36 ms with it)
    P.xcd_spx = 0;
    if (npairs > 1 && cus % 8 == 0) {
        const int spx = (cus / 8) / npairs;        // whole slabs (all their pairs) that fit one XCD's CUs
        if (spx >= 1 && 8 * spx <= nslab) P.xcd_spx = spx;
    }
    for (int q = 0; q < 6; ++q) { P.wq_n[q] = 0; P.wq_first[q] = 0; P.wq_len[q] = 0; }
    KinCounts KC;
    KC.blk = 0; KC.nb = P.nb;
    for (int q = 0; q < 6; ++q) KC.n[q] = 0;
    int grid1d = 0;
    if (P.nb >= 2 && P.nb <= 3 && !P.merged) {
        // tile slots a wave of pair (bi, bj) runs per k-step (the kernel's TPW) + a constant for its share of the staging
        double wgt[6], wsum = 0.0;
        int q = 0;
        for (int bi = 0; bi < P.nb; ++bi)
            for (int bj = bi; bj < P.nb; ++bj, ++q) {
                const int Ta = std::min(P.Tb, P.T - bi * P.Tb), Tbb = std::min(P.Tb, P.T - bj * P.Tb);
                const int tiles = bi == bj ? Ta * (Ta + 1) / 2 : Ta * Tbb;
                wgt[q] = std::max(KIN_PAIR_FLOOR, (double)((tiles + KIN_WAVES - 1) / KIN_WAVES)) + 0.35;
                wsum += wgt[q];
            }
        int used = 0;
        for (q = 0; q < npairs; ++q) { P.wq_n[q] = std::max(1, (int)(cus * wgt[q] / wsum)); used += P.wq_n[q]; }
        for (int left = cus - used; left > 0; --left) { // the CUs left over go where the slabs are longest
            int best = 0;
            for (q = 1; q < npairs; ++q)
                if (wgt[q] / P.wq_n[q] > wgt[best] / P.wq_n[best]) best = q;
            ++P.wq_n[best];
        }
        int first = 0, maxn = 0;
        for (q = 0; q < npairs; ++q) {
            int64_t len = (p + P.wq_n[q] - 1) / P.wq_n[q];
            len = (len + KIN_KC - 1) / KIN_KC * KIN_KC;
            if (len > max_loci_per_wg) len = max_loci_per_wg;
            P.wq_len[q] = len;
            P.wq_n[q] = (int)((p + len - 1) / len);
            P.wq_first[q] = first;
            first += P.wq_n[q];
            maxn = std::max(maxn, P.wq_n[q]);
            KC.n[q] = P.wq_n[q];
        }
        grid1d = first;
        nslab = maxn;
        P.nslab = nslab;
        P.xcd_spx = 0;
        P.skip_dead = 0;
        KC.blk = P.Tb * 16;
    }
    const size_t slab_bytes = (size_t)nslab * P.npad * P.npad * sizeof(double);
    int rc = pg_ws_reserve(ctx, slab_bytes);
    if (rc) return rc;
    P.slabs = static_cast<double *>(ctx->ws.get());

    // worst-case LDS row: two blocks of Tb tiles (+16 pad)
    int ldsld = (P.nb == 1) ? P.Tb * 16 : 2 * P.Tb * 16;
    if ((ldsld & 31) != 16) ldsld += 16;
    // fused speculative intercept-only sums: only in the single-block path and with phenotypes announced
    const bool spec13 = KIN_HAS13 && P.nb == 1 && P.T == 13;
    // LDS of a launch, in ONE place for the guard and the launch: two stage buffers of the kernel family's stage length (13-tile
    // kernels: KC13 loci; the rest: KIN_KC), and for the fused sums the phenotypes and, outside the 13-tile kernels (whose sums stay
    // in DPP rows), the waves' scratch ([4][64] doubles each).  13-tile, fused: 2 x 32 x 208 x 8 + 4 096 = 110 592 bytes.
    auto lds_bytes = [&](bool fused) -> size_t {
        return (size_t)2 * (spec13 ? KC13 : KIN_KC) * ldsld * sizeof(double) +
               (fused ? ((size_t)KIN_FUSE_MAXK * 256 + (spec13 ? 0 : (size_t)KIN_WAVES * 4 * 64)) * sizeof(double) : 0);
    };
    const bool fuse = allow_fuse && ctx->ph_armed && lds_bytes(true) <= 160 * 1024 && P.nb == 1 && ctx->ph_n == n && ctx->ph_k >= 1 && ctx->ph_k <= KIN_FUSE_MAXK &&
                      ctx->ph_ytil_dev != nullptr;
    P.ytil = nullptr; P.spec = nullptr; P.k = 0;
    ctx->spec_valid = false;
    if (fuse) {
        const size_t need = (size_t)p * (2 + ctx->ph_k) * sizeof(double);
        const int rrc = ctx->spec_dev.reserve(ctx, need, "kinship");
        if (rrc) return rrc;
        P.ytil = ctx->ph_ytil_dev; P.spec = ctx->spec_dev; P.k = ctx->ph_k;
    }
    const size_t shmem = lds_bytes(fuse);
    const int max_cols = (P.nb == 1) ? P.Tb * 16 : 2 * P.Tb * 16; // staged pools per locus row
    PG_CHECK(ctx, KIN_KC * (max_cols / 2) <= KIN_PPT * KIN_THREADS, "kinship: staging overflow");
    auto launch = [&](auto kern) -> hipError_t {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        if (e != hipSuccess) return e;
        if (grid1d) hipLaunchKernelGGL(kern, dim3(grid1d), dim3(KIN_THREADS), shmem, ctx->stream, P);
        else if (P.xcd_spx) hipLaunchKernelGGL(kern, dim3(8 * ((P.xcd_spx * npairs) + ((nslab - 8 * P.xcd_spx) * npairs + 7) / 8)), dim3(KIN_THREADS), shmem,
                                          ctx->stream, P);
        else hipLaunchKernelGGL(kern, dim3(nslab, npairs), dim3(KIN_THREADS), shmem, ctx->stream, P);
        return hipSuccess;
    };
    pg_prof_begin(ctx, kid);
    hipError_t le;
    // 4 x 4 x 4 blocks for the narrow tiles of the 13-tile shape (see k_kinship_syrk): the diagonal tiles (bit 1) and the last
    // column when it holds <= 8 pools (bit 2).  Measured at 200 pools x 10 M loci (tools/bench_kin_ab.py, one box, ms):
    //   bits          0      1      2      3
    //   fused sums   7.62   7.59   7.31   7.23     (bit 1 costs the fused kernel 19 spilled registers and still pays)
    //   plain        6.84   6.80   6.41   6.30
    // So the 13-tile shape runs bits 3 up to 200 pools and bits 1 for 201 .. 208 (the last column holds more than 8 pools).
    auto pick = [&](auto fz) -> hipError_t {
        constexpr bool FZ = decltype(fz)::value;
        if (!spec13) return P.skip_dead ? launch(k_kinship_syrk<FZ, false, 0, true>) : launch(k_kinship_syrk<FZ, false, 0, false>);
        if constexpr (KIN_HAS13) {
            // (an even pool count, the headline among them, runs the instance without the odd-tail zeroing in its stage loop)
            if (n & 1) return n <= 200 ? launch(k_kinship_syrk<FZ, true, 3>) : launch(k_kinship_syrk<FZ, true, 1>);
            return n <= 200 ? launch(k_kinship_syrk<FZ, true, 3, false, false>) : launch(k_kinship_syrk<FZ, true, 1, false, false>);
        }
        return hipErrorInvalidDeviceFunction; // (not reached: spec13 implies KIN_HAS13)
    };
    le = fuse ? pick(std::true_type{}) : pick(std::false_type{});
    PG_HIP(ctx, le);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    if (fuse) { // (behind the check: a launch the device refused leaves no sums)
        ctx->spec_G = G; ctx->spec_p = p; ctx->spec_ld = ld; ctx->spec_n = n; ctx->spec_k = ctx->ph_k;
        ctx->spec_valid = true;
    }
    pg_prof_begin(ctx, PG_K_KINSHIP_REDUCE);
    hipLaunchKernelGGL(k_kinship_reduce, dim3((n + 63) / 64, n), dim3(256), 0, ctx->stream,
                       P.slabs, nslab, P.npad, n, add_intercept ? 1.0 : 0.0, S, KC);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    return PG_OK;
}

#ifndef KIN_NO_EXPORTS // (pg_kinship_w8.hip includes this file for its launcher only)
extern "C" int pg_kinship_partial_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n,
                                      int64_t ld, double *S_dev) {
    if (!ctx) return PG_ERR_INVALID;
    return pg_launch_kinship(ctx, G_dev, p, n, ld, S_dev, false, PG_K_KINSHIP, true);
}

extern "C" int pg_gp_xxt_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld,
                             double *XXt_dev) {
    if (!ctx) return PG_ERR_INVALID;
    // X = [1 | G^T]  =>  X X^T = 1 1^T + sum_l g_l g_l^T
    return pg_launch_kinship(ctx, G_dev, p, n, ld, XXt_dev, true, PG_K_GP_XXT);
}

extern "C" int pg_set_phenotypes(pg_ctx *ctx, int n, const double *Y, int k) {
    if (!ctx) return PG_ERR_INVALID;
    const int rc = pg_phenotypes_upload(ctx, n, Y, k);
    ctx->ph_armed = rc == PG_OK && ctx->ph_n > 0; // the caller's own opt-in (or its end)
    return rc;
}

int pg_phenotypes_upload(pg_ctx *ctx, int n, const double *Y, int k) {
    ctx->spec_valid = false;
    if (n > 0 && Y && ctx->ph_n == n && ctx->ph_k == k && ctx->ph_ytil_dev && ctx->ph_Y.size() == (size_t)n * k &&
        std::memcmp(ctx->ph_Y.data(), Y, sizeof(double) * n * k) == 0)
        return PG_OK; // same phenotypes as last time: the centred copy is already on the device
    if (ctx->ph_n > 0) ++ctx->ph_serial; // an announcement goes
    ctx->ph_n = 0; ctx->ph_k = 0; ctx->ph_Y.clear();
    if (n == 0 || !Y) return PG_OK; // switched off
    PG_CHECK(ctx, n >= 2 && k >= 1, "set_phenotypes: bad shape n=%d k=%d", n, k);
    if (k > 4 || n > 256) return PG_OK; // not an error: the regular two-pass path is used
    for (int i = 0; i < n * k; ++i)
        PG_CHECK(ctx, Y[i] == Y[i], "set_phenotypes: phenotype matrix contains NaN; remove pools with "
                                    "missing phenotypes first (gwas/ols.rs:287)");
    PG_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<double> yt((size_t)k * 256, 0.0);
    for (int t = 0; t < k; ++t) {
        double mu = 0.0;
        for (int i = 0; i < n; ++i) mu += Y[(size_t)i * k + t];
        mu /= n;
        double syy = 0.0;
        for (int i = 0; i < n; ++i) {
            const double y = Y[(size_t)i * k + t] - mu;
            yt[(size_t)t * 256 + i] = y;
            syy += y * y;
        }
        ctx->ph_syy[t] = syy;
    }
    const int rc = ctx->ph_ytil_dev.reserve(ctx, sizeof(double) * 4 * 256, "set_phenotypes");
    if (rc) return rc;
    PG_HIP(ctx, hipMemcpyAsync(ctx->ph_ytil_dev, yt.data(), sizeof(double) * k * 256, hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->ph_Y.assign(Y, Y + (size_t)n * k);
    ctx->ph_n = n; ctx->ph_k = k;
    return PG_OK;
}
#endif // KIN_NO_EXPORTS
