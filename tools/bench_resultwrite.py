#!/usr/bin/env python3
"""Measures the result writer (pg_result_rows_dev, pg_kinship_rows_dev) against today's route at the sizes a user runs, in one
process: the median of 7 alternating rounds after a warm-up, one JSON line per case appended to profiles/resultwrite_ops.jsonl.

Legs, per case:
  (a) the three kernels of one call, by device events (the library's own PG_K_RESULTFMT profile);
  (b) the call plus the copy of the text into pinned host memory, wall clock;
  (c) today's route: the result arrays copied to (pinned) host memory plus the host twin on 16 threads, wall clock;
  (d) a device-to-device copy of the same number of bytes, by device events: the yardstick of a memory-bound kernel.
Reported: bytes of text per second for (a) and (b), the share of the 8 TB/s peak that (a)'s useful bytes (inputs read + text
written) reach, and the ratios (c)/(b) and (a)/(d).

    python tools/bench_resultwrite.py [--out profiles/resultwrite_ops.jsonl] [--scale 1.0]
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
from poolgen_amd import Engine  # noqa: E402
from poolgen_amd.engine import RESULT_OPS, name_table  # noqa: E402

PEAK = 8e12
ROUNDS = 7
NAMES = ["chr%d" % i for i in range(1, 21)]


def realistic(rng, size, kind):
    if kind == "freq":
        return rng.integers(1, 400, size=size) / rng.integers(400, 900, size=size)
    if kind == "stat":
        return rng.normal(size=size) * rng.choice([1e-3, 1.0, 50.0], size=size)
    if kind == "fisher":                       # hypergeometric ratios: tiny, long cells
        return np.exp(-rng.random(size) * 60.0)
    return rng.random(size) ** rng.choice([1, 4, 30], size=size)


def locus_case(op, L, k, rng):
    per_locus = op in ("fisher_exact_test", "chisq_test")
    n_out = np.ones(L, dtype=np.int32)
    n_out[rng.random(L) < 0.1] = 0             # a tenth of the loci dropped by the filter
    ids = rng.integers(0, 4, size=5 * L).astype(np.int32)
    size = L if per_locus else 5 * L * k
    a = dict(n_out=n_out, ids=ids, freq=None if per_locus else realistic(rng, 5 * L, "freq"),
             stat=realistic(rng, size, "fisher" if per_locus else "stat"), pval=realistic(rng, size, "fisher" if per_locus else "pval"),
             chrom=np.sort(rng.integers(0, len(NAMES), size=L)).astype(np.int32), pos=np.sort(rng.integers(1, 250_000_000, size=L)).astype(np.uint64))
    used = 1                                   # biallelic: the operators fill slot 0 only, and only that much crosses the link today
    host_bytes = 4 * L + 4 * L * used + (0 if per_locus else 8 * L * used) + 2 * 8 * (L if per_locus else L * used * k)
    return a, host_bytes


def run_case(eng, name, make_dev_call, make_host_call, in_bytes, host_copy):
    lib = eng._lib
    need = C.c_int64()
    make_dev_call(None, 0, need)
    nbytes = need.value
    text = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    other = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    pin = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    host_text = np.empty(nbytes, dtype=np.uint8)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def leg_a():
        eng.profile(True); eng.profile_reset()
        assert make_dev_call(text.data_ptr(), nbytes, need) == 0
        ms, _ = eng.profile_get("resultfmt")
        eng.profile(False)
        return ms / 1e3

    def leg_b():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        assert make_dev_call(text.data_ptr(), nbytes, need) == 0
        pin.copy_(text); torch.cuda.synchronize()
        return time.perf_counter() - t0

    def leg_c():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        arrays = host_copy()
        torch.cuda.synchronize()
        assert make_host_call(arrays, host_text.ctypes.data, nbytes, need) == 0
        return time.perf_counter() - t0

    def leg_d():
        ev0.record(); other.copy_(text); ev1.record(); torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / 1e3

    legs = dict(a=leg_a, b=leg_b, c=leg_c, d=leg_d)
    for f in legs.values():
        f()                                    # warm-up
    times = {k: [] for k in legs}
    for _ in range(ROUNDS):                    # alternating rounds
        for k, f in legs.items():
            times[k].append(f())
    assert bytes(pin[:4096].numpy()) == bytes(host_text[:4096])          # the two routes wrote the same text
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (min(v), max(v)) for k, v in times.items()}
    rec = dict(case=name, text_bytes=nbytes, input_bytes=in_bytes, rounds=ROUNDS,
               kernels_ms=med["a"] * 1e3, call_plus_d2h_ms=med["b"] * 1e3, host_route_ms=med["c"] * 1e3, d2d_copy_ms=med["d"] * 1e3,
               min_max_ms={k: [round(lo * 1e3, 3), round(hi * 1e3, 3)] for k, (lo, hi) in spread.items()},
               kernels_text_GBps=nbytes / med["a"] / 1e9, call_plus_d2h_text_GBps=nbytes / med["b"] / 1e9,
               share_of_peak_useful_bytes=(nbytes + in_bytes) / med["a"] / PEAK, host_route_over_call=med["c"] / med["b"],
               kernels_over_d2d_copy=med["a"] / med["d"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "resultwrite_ops.jsonl"))
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every size (for a quick look)")
    args = ap.parse_args()
    eng = Engine(0)
    lib, ctx = eng._lib, eng._ctx
    rng = np.random.default_rng(1)
    names_text, names_off = name_table(NAMES)
    names_dev, off_dev = torch.from_numpy(names_text).cuda(), torch.from_numpy(names_off).cuda()
    records = []
    to_dev = lambda a: None if a is None else torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
    ptr = lambda t: None if t is None else t.data_ptr()
    for op, L, k in (("ols_iter", 1_000_000, 1), ("ols_iter", 1_000_000, 3), ("fisher_exact_test", 1_000_000, 1)):
        L = max(1000, int(L * args.scale))
        a, host_bytes = locus_case(op, L, k, rng)
        d = {key: to_dev(v) for key, v in a.items()}
        opi = RESULT_OPS[op]
        per_locus = op == "fisher_exact_test"

        def dev_call(text, cap, need, d=d, opi=opi, L=L, k=k):
            return lib.pg_result_rows_dev(ctx, opi, L, k, ptr(d["n_out"]), ptr(d["ids"]), ptr(d["freq"]), ptr(d["stat"]), ptr(d["pval"]), ptr(d["chrom"]),
                                          ptr(d["pos"]), names_dev.data_ptr(), off_dev.data_ptr(), len(NAMES), text, cap, C.byref(need))

        pins = {key: (None if v is None else torch.empty(v.shape, dtype=v.dtype, pin_memory=True)) for key, v in d.items()}

        def host_copy(d=d, pins=pins, L=L, k=k, per_locus=per_locus):
            # what crosses the link today: n_out, then slot 0 of the slot-major arrays (biallelic data)
            pins["n_out"].copy_(d["n_out"], non_blocking=True)
            pins["ids"][:L].copy_(d["ids"][:L], non_blocking=True)
            if not per_locus:
                pins["freq"][:L].copy_(d["freq"][:L], non_blocking=True)
            m = L if per_locus else L * k
            pins["stat"][:m].copy_(d["stat"][:m], non_blocking=True)
            pins["pval"][:m].copy_(d["pval"][:m], non_blocking=True)
            return pins

        chrom_h, pos_h = a["chrom"], a["pos"]

        def host_call(p, text, cap, need, opi=opi, L=L, k=k, chrom_h=chrom_h, pos_h=pos_h):
            return lib.pg_host_result_rows(opi, L, k, ptr(p["n_out"]), ptr(p["ids"]), ptr(p["freq"]), ptr(p["stat"]), ptr(p["pval"]), chrom_h.ctypes.data,
                                           pos_h.ctypes.data, names_text.ctypes.data, names_off.ctypes.data, len(NAMES), text, cap, C.byref(need), 16)

        in_bytes = host_bytes + 12 * L
        records.append(run_case(eng, f"{op} L={L} k={k}", dev_call, host_call, in_bytes, host_copy))
        print(json.dumps(records[-1]), flush=True)
        del d, pins
        torch.cuda.empty_cache()
    p = max(1000, int(10_000_000 * args.scale))
    beta, pval = realistic(rng, p, "stat"), realistic(rng, p, "pval")
    cc = np.sort(rng.integers(0, len(NAMES), size=p)).astype(np.int32)
    cp = np.sort(rng.integers(1, 250_000_000, size=p)).astype(np.uint64)
    ca = rng.integers(0, 4, size=p).astype(np.int32)
    bd, pd, ccd, cpd, cad = (to_dev(x) for x in (beta, pval, cc, cp, ca))

    def kin_dev(text, cap, need):
        return lib.pg_kinship_rows_dev(ctx, p, 1, 0, p, bd.data_ptr(), pd.data_ptr(), ccd.data_ptr(), cpd.data_ptr(), cad.data_ptr(), names_dev.data_ptr(),
                                       off_dev.data_ptr(), len(NAMES), text, cap, C.byref(need))

    bp, pp = torch.empty(p, dtype=torch.float64, pin_memory=True), torch.empty(p, dtype=torch.float64, pin_memory=True)

    def kin_copy():
        bp.copy_(bd, non_blocking=True); pp.copy_(pd, non_blocking=True)
        return None

    def kin_host(_, text, cap, need):
        return lib.pg_host_kinship_rows(p, 1, 0, p, bp.data_ptr(), pp.data_ptr(), cc.ctypes.data, cp.ctypes.data, ca.ctypes.data, names_text.ctypes.data,
                                        names_off.ctypes.data, len(NAMES), text, cap, C.byref(need), 16)

    records.append(run_case(eng, f"kinship rows p={p} k=1", kin_dev, kin_host, 32 * p, kin_copy))
    print(json.dumps(records[-1]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
