#!/usr/bin/env python3
"""gwalpha on synthetic batches (device-resident counts): 1 M loci x 5 and 10 pools, least squares and maximum likelihood.  Per
case one JSON line, appended to profiles/gwalpha_ops.jsonl: the call's time (host clock around calls that end in a device
synchronise, median and spread of the repetitions), fits per second, the mean number of Nelder-Mead iterations per fit and the
share of fits that ran into the 1000-iteration cap, and -- so that the fit's own time is known -- the time of the loader's
filter pass alone on the same counts (pg_load_plan_dev with keep_p_minus_1: the header pass gwalpha starts with, plus its
column count).  The operator is bound by arithmetic (continued fractions of fp64 divisions), not by the 24 n bytes per locus.

    python tools/bench_gwalpha.py [--loci 1000000] [--reps 5] [--warmup 1] [--pools 5 10]

(The lines with "lanes_per_fit": 16 in profiles/gwalpha_ops.jsonl are from the build that still carried a 16-lane instance of
the fit kernel, measured through a knob that went with it.)
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from poolgen_amd import Engine, Filter, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pools", type=int, nargs="*", default=[5, 10])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gwalpha_ops.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gwalpha: no GPU (a time from a CPU would say nothing)")
    eng = Engine(0)
    f = Filter()
    fc = f.to_c()
    with open(a.out, "a") as log:
        for n in a.pools:
            counts = synth.sync_counts(a.loci, n, "cuda")
            bins = np.full(n, 1.0 / n)
            q = np.concatenate([[0.0], (np.arange(1, n) - 0.5) / (n - 1)])
            p_out = C.c_int64()

            def filter_only():
                eng._check(eng._lib.pg_load_plan_dev(eng._ctx, counts.data_ptr(), a.loci, n, bins.ctypes.data, C.byref(fc), 1, None,
                                                     C.byref(p_out)), "pg_load_plan_dev")

            for method in ("LS", "ML"):
                def fit():
                    return eng.gwalpha(counts, bins, q, 0.25, 0.0, 1.0, f, method, raw=True)

                for _ in range(a.warmup):
                    fit(); filter_only()
                torch.cuda.synchronize()
                t = {"fit": [], "filter": []}
                for _ in range(a.reps):
                    for k, fn in (("fit", fit), ("filter", filter_only)):
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        t[k].append(time.perf_counter() - t0)
                n_out, _, _, alpha, _, _, iters = fit()
                rows = int(n_out.sum())
                live = torch.arange(5, device=n_out.device)[:, None] < n_out[None, :]
                it = iters[live].double()
                med = {k: statistics.median(v) for k, v in t.items()}
                rec = {"op": "gwalpha", "method": method, "pools": n, "loci": a.loci, "reps": a.reps, "rows": rows,
                       "lanes_per_fit": 8,
                       "ms": med["fit"] * 1e3, "ms_min": min(t["fit"]) * 1e3, "ms_max": max(t["fit"]) * 1e3,
                       "filter_pass_ms": med["filter"] * 1e3, "fit_only_ms": (med["fit"] - med["filter"]) * 1e3,
                       "fits_per_s": rows / med["fit"], "mean_iterations": float(it.mean()),
                       "share_at_cap": float((it == 1000).double().mean()),
                       "alpha_nan": int(torch.isnan(alpha[live]).sum())}
                line = json.dumps(rec)
                print(line, flush=True)
                log.write(line + "\n")
                log.flush()
            del counts
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
