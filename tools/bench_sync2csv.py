#!/usr/bin/env python3
"""sync2csv's writer on a synthetic table (200 pools x 1 M biallelic loci = 2 M rows, 4e8 cells, device-resident): the text
formatted on the GPU (pg_csv_freq_rows_dev) against the same text formatted on the host (pg_host_csv_freq_rows, 16 threads).
One JSON line, appended to profiles/sync2csv_ops.jsonl: per leg the median of the rounds (the legs alternate inside a round,
after a warm-up of each):
  format_dev      the three kernels (measure, scan, emit), by device events (Engine.profile, kernel id "csv")
  format_dev_d2h  the call + the copy of the text into pinned host memory, host clock around a device synchronise
  format_host     the copy of G into pinned host memory + the host formatter
and the text's size, the speed-up format_host / format_dev_d2h, and for format_dev the useful bytes (8 * ld * rows read once +
the text written) over the kernel time as a share of the 8 TB/s HBM peak -- a rate of useful bytes, not of traffic: measure
and emit both read G.

    python tools/bench_sync2csv.py [--loci 1000000] [--pools 200] [--rounds 7] [--threads 16]
"""
import argparse
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
from poolgen_amd.engine import freq_csv_host

HBM_PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=1_000_000)
    ap.add_argument("--pools", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sync2csv_ops.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sync2csv: no GPU (a time from a CPU would say nothing)")
    eng = Engine(0)
    n, L = a.pools, a.loci
    counts = synth.sync_counts(L, n, "cuda")
    G, col_locus, col_allele = eng.load_frequencies(counts, np.full(n, 20.0), Filter())
    del counts
    torch.cuda.empty_cache()
    rows, ld = G.shape
    chrom_names = ["chr%d" % (i + 1) for i in range(5)]
    chrom_ids = (np.arange(L, dtype=np.int64) * 5 // L).astype(np.int32)
    pos = np.arange(1, L + 1, dtype=np.uint64)
    ch_dev = torch.from_numpy(chrom_ids).cuda()
    pos_dev = torch.from_numpy(pos.view(np.int64)).cuda()
    size = eng.freq_csv(G, col_locus, col_allele, ch_dev, pos_dev, chrom_names, n=n).numel()
    text_dev = torch.empty(size, dtype=torch.uint8, device="cuda")
    text_pin = torch.empty(size, dtype=torch.uint8).pin_memory()
    G_pin = torch.empty(G.shape, dtype=torch.float64).pin_memory()
    text_host = np.empty(size, dtype=np.uint8)
    cl_host, ca_host = col_locus.cpu().numpy(), col_allele.cpu().numpy()

    def format_dev():
        eng.profile_reset()
        eng.freq_csv(G, col_locus, col_allele, ch_dev, pos_dev, chrom_names, n=n, out=text_dev, validate=False)
        return eng.profile_get("csv")[0] * 1e-3

    def format_dev_d2h():
        t0 = time.perf_counter()
        out = eng.freq_csv(G, col_locus, col_allele, ch_dev, pos_dev, chrom_names, n=n, out=text_dev, validate=False)
        text_pin[:out.numel()].copy_(out)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def format_host():
        t0 = time.perf_counter()
        G_pin.copy_(G)
        torch.cuda.synchronize()
        freq_csv_host(G_pin.numpy(), cl_host, ca_host, chrom_ids, pos, chrom_names, n=n, n_threads=a.threads, out=text_host)
        return time.perf_counter() - t0

    legs = {"format_dev": format_dev, "format_dev_d2h": format_dev_d2h, "format_host": format_host}
    eng.profile(True)
    for fn in legs.values():
        fn()
    if not np.array_equal(text_pin.numpy(), text_host):
        sys.exit("bench_sync2csv: the device's text and the host's differ")
    t = {k: [] for k in legs}
    for _ in range(a.rounds):                                # alternating: the legs see the same neighbours on the machine
        for k, fn in legs.items():
            t[k].append(fn())
    eng.profile(False)
    med = {k: statistics.median(v) for k, v in t.items()}
    useful = 8.0 * ld * rows + size
    rec = {"op": "sync2csv_format", "pools": n, "loci": L, "rows": rows, "cells": rows * n, "rounds": a.rounds,
           "host_threads": a.threads, "text_bytes": size,
           **{f"{k}_ms": med[k] * 1e3 for k in legs},
           **{f"{k}_ms_min": min(t[k]) * 1e3 for k in legs}, **{f"{k}_ms_max": max(t[k]) * 1e3 for k in legs},
           "speedup_host_over_dev_d2h": med["format_host"] / med["format_dev_d2h"],
           "format_dev_useful_bytes": useful, "format_dev_frac_of_hbm_peak": useful / med["format_dev"] / HBM_PEAK}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
