#!/usr/bin/env python3
"""The VCF parser on a synthetic GT:PL:DP:AD text (200 pools x 500 k loci, biallelic, two-digit depths): the text parsed on the
GPU (pg_vcf_parse_dev) against the same text parsed on the host (pg_host_vcf_parse, 16 threads), and the CLI from the file.
One JSON line per leg, appended to profiles/vcf_ops.jsonl: the median of the rounds (the library's legs alternate inside a
round, after a warm-up of each):
  parse_dev       the kernels of one call (index, parse + scan, emit: kernel id "vcf" sums the three stages), by device events
  parse_dev_h2d   the copy of the text from pinned host memory + the call (capacities known: one call), host clock around a
                  device synchronise; the rows stay on the device
  parse_host      the host twin on the text in host memory
  cli_vcf2sync    `poolgen vcf2sync` on the file, wall clock of the process (the sync file is written)
  cli_ols_iter    `poolgen ols_iter` on the *.vcf, wall clock of the process
with the text's size, bytes of text per second and, for parse_dev, that rate as a share of the 8 TB/s HBM peak.

    python tools/bench_vcf.py [--loci 500000] [--pools 200] [--rounds 7] [--cli-rounds 3] [--threads 16] [--dir /tmp]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from poolgen_amd import Engine, vcf_parse_host
from poolgen_amd._native import PgVcfInfo

HBM_PEAK = 8e12
CLI = ROOT / "poolgen_amd" / "csrc" / "poolgen"


def synthetic_vcf(loci, pools, seed=1):
    """fixed-width lines, so that the text is made by array operations: 'chrC <9-digit pos> . A T 50.0 . DP=100 GT:PL:DP:AD' and
    per pool '0/1:42,0,61:DD:AA,BB' with AA, BB two digits each (a leading zero is a valid u64) and DD their sum"""
    rng = np.random.default_rng(seed)
    head = b"chr0\t000000000\t.\tA\tT\t50.0\t.\tDP=100\tGT:PL:DP:AD\t"
    field = b"0/1:42,0,61:000:00,00\t"
    line = np.frombuffer(head + field * pools, dtype=np.uint8)
    text = np.tile(line, (loci, 1))
    text[:, -1] = ord("\n")
    text[:, 3] = ord("1") + (np.arange(loci) * 5 // loci).astype(np.uint8)
    pos = np.arange(1, loci + 1)
    for d in range(9):
        text[:, 5 + 8 - d] = ord("0") + (pos // 10 ** d % 10).astype(np.uint8)
    f = text[:, len(head):].reshape(loci, pools, len(field))
    a = rng.integers(0, 100, size=(loci, pools), dtype=np.int32)
    b = rng.integers(0, 100, size=(loci, pools), dtype=np.int32)
    b[rng.random(loci) < 0.3] = 0                                  # loci that the frequency rule drops
    s = a + b
    for k, v in ((12, s // 100), (13, s // 10 % 10), (14, s % 10), (16, a // 10), (17, a % 10), (19, b // 10), (20, b % 10)):
        f[:, :, k] = (v + ord("0")).astype(np.uint8)
    names = "".join(f"\tPool{i}" for i in range(pools))
    header = ("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT" + names + "\n").encode()
    return np.concatenate([np.frombuffer(header, dtype=np.uint8), text.reshape(-1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=500_000)
    ap.add_argument("--pools", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cli-rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vcf_ops.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_vcf: no GPU (a time from a CPU would say nothing)")
    eng = Engine(0)
    n, L = a.pools, a.loci
    text = synthetic_vcf(L, n)
    size = text.size
    sizes = np.full(n, 1.0 / n)
    text_pin = torch.from_numpy(text).pin_memory()
    text_dev = torch.empty(size, dtype=torch.uint8, device="cuda")
    host = vcf_parse_host(text, sizes, n_threads=a.threads)                 # also the warm-up of the host leg
    kept = len(host["pos"])
    counts = torch.empty(kept * n * 6, dtype=torch.int32, device="cuda")
    pos = torch.empty(kept, dtype=torch.int64, device="cuda"); off = torch.empty(kept, dtype=torch.int64, device="cuda")
    ref = torch.empty(kept, dtype=torch.uint8, device="cuda"); clen = torch.empty(kept, dtype=torch.int32, device="cuda")
    info = PgVcfInfo()

    def call():
        rc = eng._lib.pg_vcf_parse_dev(eng._ctx, text_dev.data_ptr(), size, sizes.ctypes.data, n, 1, 1.0, 0.001, counts.data_ptr(), pos.data_ptr(),
                                       ref.data_ptr(), off.data_ptr(), clen.data_ptr(), kept, counts.numel(), C.byref(info))
        if rc != 0:
            sys.exit(f"bench_vcf: pg_vcf_parse_dev failed ({rc})")

    def parse_dev():
        eng.profile_reset()
        call()
        return eng.profile_get("vcf")[0] * 1e-3

    def parse_dev_h2d():
        t0 = time.perf_counter()
        text_dev.copy_(text_pin, non_blocking=True)
        call()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    h_counts = np.empty(kept * n * 6, dtype=np.uint32); h_pos = np.empty(kept, dtype=np.uint64); h_ref = np.empty(kept, dtype=np.uint8)
    h_off = np.empty(kept, dtype=np.int64); h_clen = np.empty(kept, dtype=np.int32)
    h_info = PgVcfInfo()

    def parse_host():                                        # capacities known, as for the device: one call
        t0 = time.perf_counter()
        rc = eng._lib.pg_host_vcf_parse(text.ctypes.data, size, sizes.ctypes.data, n, 1, 1.0, 0.001, h_counts.ctypes.data, h_pos.ctypes.data,
                                        h_ref.ctypes.data, h_off.ctypes.data, h_clen.ctypes.data, kept, h_counts.size, C.byref(h_info), a.threads)
        if rc != 0:
            sys.exit(f"bench_vcf: pg_host_vcf_parse failed ({rc})")
        return time.perf_counter() - t0

    text_dev.copy_(text_pin)
    legs = {"parse_dev": parse_dev, "parse_dev_h2d": parse_dev_h2d, "parse_host": parse_host}
    eng.profile(True)
    for k in ("parse_dev", "parse_dev_h2d"):
        legs[k]()
    if info.kept != kept or not np.array_equal(counts.cpu().numpy().view(np.uint32).reshape(kept, n, 6), host["counts"]) \
            or not np.array_equal(pos.cpu().numpy().view(np.uint64), host["pos"]):
        sys.exit("bench_vcf: the device's rows and the host's differ")
    t = {k: [] for k in legs}
    for _ in range(a.rounds):                                # alternating: the legs see the same neighbours on the machine
        for k, fn in legs.items():
            t[k].append(fn())
    eng.profile(False)
    # ---- the CLI, from the file ----------------------------------------------------------------------------------------------
    work = Path(tempfile.mkdtemp(prefix="bench_vcf_", dir=a.dir))
    vcf, phen = work / "synthetic.vcf", work / "phen.csv"
    text.tofile(vcf)
    rng = np.random.default_rng(2)
    phen.write_text("#pop,size,trait\n" + "".join(f"Pool{i},20.0,{rng.random():.6f}\n" for i in range(n)))
    cli = {"cli_vcf2sync": ["vcf2sync"], "cli_ols_iter": ["ols_iter"]}
    for k, args in cli.items():
        t[k] = []
        for r in range(a.cli_rounds):
            out = work / f"{k}_{r}.out"
            t0 = time.perf_counter()
            p = subprocess.run([str(CLI), *args, "-f", str(vcf), "-p", str(phen), "-o", str(out), "--n-threads", str(a.threads)], capture_output=True, text=True)
            t[k].append(time.perf_counter() - t0)
            if p.returncode != 0:
                sys.exit(f"bench_vcf: {k} failed: {p.stderr}")
            out_bytes = out.stat().st_size
            out.unlink()
        cli[k] = out_bytes
    vcf.unlink(); phen.unlink(); os.rmdir(work)
    common = {"pools": n, "loci": L, "kept": kept, "text_bytes": int(size), "host_threads": a.threads}
    with open(a.out, "a") as f:
        for k, v in t.items():
            med = statistics.median(v)
            rec = {"op": "vcf_" + k, **common, "rounds": len(v), "ms": med * 1e3, "ms_min": min(v) * 1e3, "ms_max": max(v) * 1e3,
                   "text_bytes_per_s": size / med}
            if k == "parse_dev":
                rec["frac_of_hbm_peak"] = size / med / HBM_PEAK
            if k == "parse_dev_h2d":
                rec["speedup_over_parse_host"] = statistics.median(t["parse_host"]) / med
            if k in cli:
                rec["output_bytes"] = cli[k]
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
