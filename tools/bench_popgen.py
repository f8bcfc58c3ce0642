"""Throughput of fst / theta_pi / tajima_d / theta_watterson / gudmc on a resident synthetic matrix:
    python tools/bench_popgen.py [pools] [loci] [--rounds R] [--baseline-lib other/libpoolgen_hip.so]
Every leg is warmed up once, then the legs alternate for R rounds in this one process and the median wall time of each is
printed (one JSON line per leg).  --baseline-lib adds two legs that call pg_pi_dev the same way, on the same matrix and windows
with locus_col already an array (the Engine's `theta_pi` leg also converts it from a list on every call, which costs more
than the kernels): `theta_pi_raw` of this build and `theta_pi_baseline` of another build of the library (e.g. the previous
commit's), loaded beside this one.
The gudmc legs: `gudmc_stage` = pg_gudmc_dev alone on the two tables already on the device, `gudmc` = tajima_d + fst + the stage
(Engine.gudmc); one more line gives the histogram of the iterations the D and Fst fits took (10000 = the cap)."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from poolgen_amd import Engine, Filter, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("pools", nargs="?", type=int, default=200)
ap.add_argument("loci", nargs="?", type=int, default=500_000)
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--baseline-lib", default=None)
args = ap.parse_args()
n, L = args.pools, args.loci
eng = Engine(0)
counts = synth.sync_counts(L, n, "cuda", seed=3)
ps = np.full(n, 20.0)
G, col_locus, col_allele, cov = eng.load_frequencies(counts, ps, Filter(), coverages=True)
del counts
cl = col_locus.cpu().numpy()
starts = np.flatnonzero(np.r_[True, cl[1:] != cl[:-1]]).tolist() + [len(cl)]
nl = len(starts) - 1
pos = np.arange(nl, dtype=np.uint64) * 37 + 100
chrom = (np.arange(nl) // (nl // 4 + 1)).astype(np.int32)
wh, wt = eng.sliding_windows(chrom, pos, 37 * 400, 37 * 200, 10)      # ~400 loci per window, half-overlapping
legs = [("theta_pi", lambda: eng.theta_pi(G, cov, starts, wh, wt, n=n)),
        ("tajima_d", lambda: eng.tajima_d(G, cov, starts, wh, wt, ps, n=n)),          # counted mode
        ("theta_watterson", lambda: eng.theta_watterson(G, starts, wh, wt, ps, n=n)),
        ("fst", lambda: eng.fst(G, cov, starts, wh, wt, n=n))]
wchr, wini, wfin = chrom[wh], pos[wh], pos[wt]
d_tab = torch.from_numpy(eng.tajima_d(G, cov, starts, wh, wt, ps, n=n)[0]).cuda()
f_tab = torch.from_numpy(eng.fst(G, cov, starts, wh, wt, n=n)[1]).cuda()
legs += [("gudmc_stage", lambda: eng.gudmc_from_tables(d_tab, f_tab, wchr, wini, wfin)),
         ("gudmc", lambda: eng.gudmc(G, cov, starts, wh, wt, wchr, wini, wfin, ps, n=n))]
if args.baseline_lib:
    base = C.CDLL(args.baseline_lib)
    base.pg_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p]
    base.pg_pi_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                               C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    bctx = C.c_void_p()
    assert base.pg_create(C.byref(bctx), 0, C.c_void_p(torch.cuda.current_stream(0).cuda_stream)) == 0
    lc = np.ascontiguousarray(starts, dtype=np.int64)
    bwin, bmean = np.empty((len(wh), n)), np.empty(n)

    def raw(lib, ctx):
        def call():
            assert lib.pg_pi_dev(ctx, G.data_ptr(), cov.data_ptr(), G.shape[0], n, G.shape[1], lc.ctypes.data, nl, wh.ctypes.data,
                                 wt.ctypes.data, len(wh), bwin.ctypes.data, bmean.ctypes.data) == 0
            return bwin, bmean
        return call
    baseline = raw(base, bctx)
    legs[1:1] = [("theta_pi_raw", raw(eng._lib, eng._ctx)), ("theta_pi_baseline", baseline)]
    assert np.array_equal(baseline()[0], eng.theta_pi(G, cov, starts, wh, wt, n=n)[0])
times = {name: [] for name, _ in legs}
for name, fn in legs:
    fn()
torch.cuda.synchronize()
for _ in range(args.rounds):
    for name, fn in legs:
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times[name].append(time.perf_counter() - t0)
pairs = n * (n + 1) // 2
iters = torch.cat([eng.normal_fit(torch.round(d_tab * 1e8) / 1e8)[3], eng.normal_fit(f_tab)[3]]).cpu().numpy()
edges = [0, 1, 50, 100, 150, 200, 300, 500, 1000, 5000, 10000, 10001]
print(json.dumps({"op": "gudmc_fit_iterations", "pools": n, "windows": int(len(wh)), "fits": int(iters.size),
                  "median": float(np.median(iters)), "at_cap": int((iters == 10000).sum()), "edges": edges,
                  "histogram": np.histogram(iters, bins=edges)[0].tolist()}))
for name, _ in legs:
    dt = statistics.median(times[name])
    print(json.dumps({"op": name, "pools": n, "loci": nl, "columns": int(G.shape[0]), "windows": int(len(wh)), "rounds": args.rounds,
                      "wall_s": dt, "wall_s_min": min(times[name]), "wall_s_max": max(times[name]), "loci_per_s": nl / dt,
                      "pair_locus_evals_per_s": (3 * nl * pairs / dt) if name == "fst" else None}))
