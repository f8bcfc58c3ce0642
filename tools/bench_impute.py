"""Throughput of the imputation steps on a resident synthetic matrix:
    python tools/bench_impute.py [pools] [loci] [--rounds R] [--aldknn-loci M] [--window-loci W] [--leg-seconds S]\n        [--out profiles/impute_ops.jsonl]
The depth below which a pool counts as missing is set to the quantile of the synthetic coverages that puts --missing (0.2) of
the cells below it.  Legs, warmed up once and then alternating for R rounds in this one process (median wall time, one JSON
line per leg):
    missing_filter   set_missing_by_depth + the NaN counts + the keep rule + the compaction, pools then loci
    impute_mean      pg_impute_mean_dev on the filtered table (wall time of the call, and the kernels by HIP events); useful bytes =
                     one read of G plus the cells written
    impute_aldknn    Engine.impute_aldknn on the first M loci of the filtered table, windows of W loci, half overlapping
    aldknn_links / aldknn_walk   the two stages inside that call, from the library's HIP-event timers (kernel time)
    impute_composed  Engine.impute(method="aLD-kNNi") from the loaded matrix of those M loci to the table the writer prints
In-place steps run on a fresh copy made outside the timed region."""
import argparse
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
ap.add_argument("loci", nargs="?", type=int, default=300_000)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--missing", type=float, default=0.2)
ap.add_argument("--aldknn-loci", type=int, default=30_000)
ap.add_argument("--window-loci", type=int, default=40)
ap.add_argument("--leg-seconds", type=float, default=60.0)
ap.add_argument("--out", default=None)
args = ap.parse_args()
n, L = args.pools, args.loci
eng = Engine(0)
counts = synth.sync_counts(L, n, "cuda", seed=3)
ps = np.full(n, 20.0)
G0, col_locus, col_allele, cov0 = eng.load_frequencies(counts, ps, Filter(), coverages=True)
del counts
cl = col_locus.cpu().numpy()
lc0 = np.r_[np.flatnonzero(np.r_[True, cl[1:] != cl[:-1]]), len(cl)].astype(np.int64)
nl = len(lc0) - 1
sample = cov0[torch.as_tensor(lc0[:-1][:: max(1, nl // 20000)]).cuda(), :n].flatten()
min_depth = float(torch.quantile(sample, args.missing).item()) + 0.5
pos = np.arange(nl, dtype=np.uint64) * 37 + 100
chrom = (np.arange(nl) // (nl // 4 + 1)).astype(np.int32)


def filtered(G, cov, lc):
    """the steps 2 - 4 of impute_mean / impute_aLDkNN on copies -> the filtered table"""
    eng.set_missing_by_depth(G, cov, lc, min_depth, n=n)
    pool_nan, _ = eng.missingness(G, cov, lc, n=n)
    pools = eng.top_missing_keep(pool_nan, 0.1, "pools")
    G, cov, lc, _, _ = eng.impute_compact(G, cov, lc, pools, np.arange(len(lc) - 1), n=n)
    locus_nan = eng.missingness(G, cov, lc, n=len(pools))[1]
    loci = eng.top_missing_keep(locus_nan, 0.1, "loci")
    G, cov, lc, _, _ = eng.impute_compact(G, cov, lc, np.arange(len(pools)), loci, n=len(pools))
    return G, cov, lc, pools, loci


Gf, covf, lcf, pools, loci = filtered(G0.clone(), cov0.clone(), lc0)
n2 = len(pools)
missing_cells = int(torch.isnan(Gf[:, :n2]).sum())
M = min(args.aldknn_loci, len(lcf) - 1)
Ga = Gf[: lcf[M]].contiguous()
lca = lcf[: M + 1]
wh, wt = eng.sliding_windows(chrom[loci][:M], pos[loci][:M], 37 * args.window_loci, 37 * args.window_loci // 2, 2)
M0 = int(loci[M - 1]) + 1            # the loci of the loaded matrix that the composed leg starts from
state = {}


def leg_filter():
    filtered(state["G"], state["cov"], lc0)


def leg_mean():
    eng.impute_mean(state["Gf"], lcf, n=n2)


def leg_aldknn():
    eng.impute_aldknn(Ga, lca, wh, wt, 10, 5, n=n2)


def leg_composed():
    eng.impute(G0[: lc0[M0]], cov0[: lc0[M0]], lc0[: M0 + 1], chrom[:M0], pos[:M0], "aLD-kNNi", min_depth, 0.1, 0.1, 37 * args.window_loci,
               37 * args.window_loci // 2, 2, 10, 5, n=n)


def prepare(name):
    if name == "missing_filter":
        state["G"], state["cov"] = G0.clone(), cov0.clone()
    if name == "impute_mean":
        state["Gf"] = Gf.clone()
    torch.cuda.synchronize()


legs = [("missing_filter", leg_filter), ("impute_mean", leg_mean), ("impute_aldknn", leg_aldknn), ("impute_composed", leg_composed)]
times = {name: [] for name, _ in legs}
kernel_ms = {"impute_links": [], "impute_walk": [], "impute": []}
eng.profile(True)
rounds = {}
for name, fn in legs:      # warm-up; a leg whose R rounds would take longer than --leg-seconds runs fewer (at least 3)
    prepare(name)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    warm = time.perf_counter() - t0
    rounds[name] = max(3, min(args.rounds, int(args.leg_seconds / max(warm, 1e-9))))
    print(f"# warm-up {name}: {warm:.3f} s, {rounds[name]} rounds", flush=True)
for r in range(args.rounds):
    for name, fn in legs:
        if r >= rounds[name]:
            continue
        prepare(name)
        if name in ("impute_aldknn", "impute_mean"):
            eng.profile_reset()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times[name].append(time.perf_counter() - t0)
        if name == "impute_aldknn":
            for k in ("impute_links", "impute_walk"):
                kernel_ms[k].append(eng.profile_get(k)[0])
        if name == "impute_mean":
            kernel_ms["impute"].append(eng.profile_get("impute")[0])
rows = []
for name, _ in legs:
    dt = statistics.median(times[name])
    row = {"op": name, "pools": n, "loci": nl if name in ("missing_filter",) else (len(lcf) - 1 if name == "impute_mean" else M),
           "columns": int(G0.shape[0]) if name == "missing_filter" else int(Gf.shape[0]) if name == "impute_mean" else int(Ga.shape[0]),
           "pools_kept": n2, "min_depth": min_depth, "missing_cells_share": missing_cells / float(Gf.shape[0] * n2), "rounds": rounds[name],
           "wall_s": dt, "wall_s_min": min(times[name]), "wall_s_max": max(times[name])}
    if name == "impute_mean":
        useful = 8.0 * (Gf.shape[0] * n2 + missing_cells)
        kms = statistics.median(kernel_ms["impute"])
        row.update(useful_bytes=useful, useful_gb_per_s=useful / dt / 1e9, share_of_8_tb_per_s=useful / dt / 8e12, kernel_ms=kms,
                   kernel_share_of_8_tb_per_s=useful / (kms * 1e-3) / 8e12)
    if name in ("impute_aldknn", "impute_composed"):
        row.update(windows=int(len(wh)), window_loci=args.window_loci, n_loci_to_estimate_distance=10, k_neighbours=5)
    rows.append(row)
links, walk = statistics.median(kernel_ms["impute_links"]), statistics.median(kernel_ms["impute_walk"])
for op, ms in (("aldknn_links", links), ("aldknn_walk", walk)):
    rows.append({"op": op, "pools": n2, "loci": M, "columns": int(Ga.shape[0]), "windows": int(len(wh)), "rounds": rounds["impute_aldknn"],
                 "kernel_ms": ms, "share_of_both": ms / (links + walk) if links + walk > 0 else None})
for row in rows:
    print(json.dumps(row))
if args.out:
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
