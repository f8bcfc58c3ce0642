#!/usr/bin/env python3
"""fisher_exact_test on synthetic batches (device-resident counts): 100 and 200 pools x 1 M loci, clean and with 0.5 % of the
reads misread.  Per case one JSON line: the call's time (host clock around calls that end in a device synchronise, median and
spread of the repetitions, alternating with the yardstick), loci/s, the algorithmic bytes L * n * 24 over that time as a
fraction of the 8 TB/s HBM peak, and -- the yardstick -- Engine.chisq on the SAME counts in the same process, an operator that
reads the same bytes.  Fisher reads the counts three times (the filter pass, then total and cells; the third read hits the
cache), so its fraction is a rate of useful bytes, not of traffic.

    python tools/bench_fisher.py [--loci 1000000] [--reps 30] [--warmup 3] > profiles/fisher_ops.jsonl
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from poolgen_amd import Engine, Filter, synth

HBM_PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fisher: no GPU (a time from a CPU would say nothing)")
    eng = Engine(0)
    f = Filter()
    for n in (100, 200):
        for err in (0.0, 0.005):
            counts = synth.sync_counts(a.loci, n, "cuda", error_rate=err)
            ps = np.full(n, 20.0)
            ops = {"fisher": lambda: eng.fisher(counts, ps, f, raw=True), "chisq": lambda: eng.chisq(counts, ps, f, raw=True)}
            for fn in ops.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in ops}
            for _ in range(a.reps):                          # alternating: both see the same neighbours on the machine
                for k, fn in ops.items():
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    t[k].append(time.perf_counter() - t0)
            n_out = eng.fisher(counts, ps, f, raw=True)[0]
            emitted = int((n_out > 0).sum())
            multi = int((n_out >= 3).sum())
            med = {k: statistics.median(v) for k, v in t.items()}
            nbytes = 24.0 * n * a.loci
            print(json.dumps({
                "op": "fisher_exact_test", "pools": n, "loci": a.loci, "error_rate": err, "reps": a.reps,
                "rows_emitted": emitted, "loci_with_3_or_more_alleles": multi,
                "ms": med["fisher"] * 1e3, "ms_min": min(t["fisher"]) * 1e3, "ms_max": max(t["fisher"]) * 1e3,
                "loci_per_s": a.loci / med["fisher"], "frac_of_hbm_peak": nbytes / med["fisher"] / HBM_PEAK,
                "chisq_ms": med["chisq"] * 1e3, "chisq_ms_min": min(t["chisq"]) * 1e3, "chisq_ms_max": max(t["chisq"]) * 1e3,
                "chisq_frac_of_hbm_peak": nbytes / med["chisq"] / HBM_PEAK, "fisher_over_chisq": med["fisher"] / med["chisq"]}), flush=True)
            del counts
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
