#!/usr/bin/env python3
"""Measures the popgen writer (pg_f64_table_dev, pg_gudmc_rows_dev) against today's route at the sizes of profiles/popgen_ops.jsonl
(200 pools x 1 496 windows) and at a 5-pool shape, in one process: the median of 7 alternating rounds after a warm-up, one JSON
line per case appended to profiles/popgenwrite_ops.jsonl.

Legs, per case:
  (a) the kernels of one call, by device events (the library's own PG_K_RESULTFMT profile);
  (b) the call plus the copy of the text into pinned host memory, wall clock;
  (c) today's route: the arrays copied to pinned host memory plus the host twin on 16 threads, wall clock;
  (d) a device-to-device copy of the same number of bytes, by device events: the yardstick of a memory-bound kernel.
The fst window table is formatted whole (60 M cells).  gudmc's file at that shape is 59.8 M rows, some 9 GB of text, which the CLI
writes in slabs; the case here is one run of `--gudmc-rows` rows (default 4 M) out of the full layout, and both routes scale with
the rows.

    python tools/bench_popgenwrite.py [--out profiles/popgenwrite_ops.jsonl] [--scale 1.0] [--gudmc-rows 4000000]
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
from poolgen_amd.engine import label_table, name_table  # noqa: E402

ROUNDS = 7
THREADS = 16


def run_case(eng, name, dev_call, host_call, host_copy, in_bytes, extra):
    need = C.c_int64()
    dev_call(None, 0, need)
    nbytes = need.value
    text = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    other = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    pin = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    host_text = np.empty(nbytes, dtype=np.uint8)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def leg_a():
        eng.profile(True); eng.profile_reset()
        assert dev_call(text.data_ptr(), nbytes, need) == 0
        ms, _ = eng.profile_get("resultfmt")
        eng.profile(False)
        return ms / 1e3

    def leg_b():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        assert dev_call(text.data_ptr(), nbytes, need) == 0
        pin.copy_(text); torch.cuda.synchronize()
        return time.perf_counter() - t0

    def leg_c():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        arrays = host_copy()
        torch.cuda.synchronize()
        assert host_call(arrays, host_text.ctypes.data, nbytes, need) == 0
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
    step = max(1, nbytes // 64)
    assert all(bytes(pin[o:o + 4096].numpy()) == bytes(host_text[o:o + 4096]) for o in range(0, nbytes, step))   # the two routes wrote the same text
    med = {k: statistics.median(v) for k, v in times.items()}
    rec = dict(case=name, text_bytes=nbytes, input_bytes=in_bytes, rounds=ROUNDS, host_threads=THREADS,
               kernels_ms=med["a"] * 1e3, call_plus_d2h_ms=med["b"] * 1e3, host_route_ms=med["c"] * 1e3, d2d_copy_ms=med["d"] * 1e3,
               min_max_ms={k: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in times.items()},
               kernels_text_GBps=nbytes / med["a"] / 1e9, call_plus_d2h_text_GBps=nbytes / med["b"] / 1e9,
               host_route_over_call=med["c"] / med["b"], kernels_over_d2d_copy=med["a"] / med["d"], **extra)
    del text, other, pin
    torch.cuda.empty_cache()
    return rec


def fst_case(eng, n, nw, rng):
    """the window table of fst: nw rows of n*n cells (Fst in [0, 1], the diagonal zero), labels chr,ini,fin,"""
    lib, ctx = eng._lib, eng._ctx
    nn = n * n
    x = torch.rand((nw, nn), dtype=torch.float64, device="cuda") * 0.4
    x[:, ::n + 1] = 0.0
    ltext, loff = label_table([f"chr{1 + w // 400},{1 + 50 * w},{101 + 50 * w}," for w in range(nw)])
    ltext_dev, loff_dev = torch.from_numpy(ltext).cuda(), torch.from_numpy(loff).cuda()
    xpin = torch.empty((nw, nn), dtype=torch.float64, pin_memory=True)

    def dev_call(text, cap, need):
        return lib.pg_f64_table_dev(ctx, x.data_ptr(), nw, nn, nn, 1, 0, nw, -1, -1, ltext_dev.data_ptr(), loff_dev.data_ptr(), text, cap, C.byref(need))

    def host_copy():
        xpin.copy_(x, non_blocking=True)
        return xpin

    def host_call(p, text, cap, need):
        return lib.pg_host_f64_table(p.data_ptr(), nw, nn, nn, 1, 0, nw, -1, -1, ltext.ctypes.data, loff.ctypes.data, text, cap, C.byref(need), THREADS)

    return run_case(eng, f"fst window table n={n} windows={nw}", dev_call, host_call, host_copy, 8 * nw * nn, dict(cells=nw * nn))


def gudmc_case(eng, n, w, rows, rng):
    """`rows` rows out of gudmc's n*n*w (every population with a row per window), values as pg_gudmc_dev leaves them"""
    lib, ctx = eng._lib, eng._ctx
    nn = n * n
    rows = min(rows, nn * w)
    pairs = (rows + w - 1) // w                                                 # the pairs those rows touch: what today's route copies down
    f64 = lambda *s: torch.rand(s, dtype=torch.float64, device="cuda")
    pop_rows = torch.full((n,), w, dtype=torch.int64, device="cuda")
    per = [f64(n) - 0.5, f64(n) + 0.5, f64(nn) * 0.3, f64(nn) * 0.1]            # d_mean, d_sd, fst_mean, fst_sd
    win = torch.arange(w, dtype=torch.int64, device="cuda").repeat(nn, 1)
    r_d = (torch.randn((nn, w), dtype=torch.float64, device="cuda") * 1e8).round() / 1e8
    r_width = torch.randint(0, 5, (nn, w), device="cuda").double() * 87.0
    row = [r_d, r_width, r_width - 7300.0, f64(nn, w), f64(nn, w) - 0.5, f64(nn, w)]
    chr_h = (np.arange(w) // 400).astype(np.int32); ini_h = (1 + 50 * np.arange(w)).astype(np.uint64); fin_h = ini_h + 100
    wchr, wini, wfin = torch.from_numpy(chr_h).cuda(), torch.from_numpy(ini_h.view(np.int64)).cuda(), torch.from_numpy(fin_h.view(np.int64)).cuda()
    pools, chroms = [f"Pool_{i:03d}" for i in range(n)], [f"chr{i}" for i in range(1, 2 + w // 400)]
    pt, po = name_table(pools); ct, co = name_table(chroms)
    ptd, pod, ctd, cod = (torch.from_numpy(a).cuda() for a in (pt, po, ct, co))
    pins = [torch.empty((pairs, w), dtype=t.dtype, pin_memory=True) for t in [win] + row]
    small = [t.cpu().numpy() for t in [pop_rows] + per]

    def dev_call(text, cap, need):
        return lib.pg_gudmc_rows_dev(ctx, n, w, 0, rows, pop_rows.data_ptr(), *[t.data_ptr() for t in per], win.data_ptr(), *[t.data_ptr() for t in row],
                                     wchr.data_ptr(), wini.data_ptr(), wfin.data_ptr(), ptd.data_ptr(), pod.data_ptr(), ctd.data_ptr(), cod.data_ptr(),
                                     len(chroms), text, cap, C.byref(need))

    def host_copy():
        for p, t in zip(pins, [win] + row):
            p.copy_(t[:pairs], non_blocking=True)
        return pins

    def host_call(p, text, cap, need):
        return lib.pg_host_gudmc_rows(n, w, 0, rows, *[a.ctypes.data for a in small], *[t.data_ptr() for t in p], chr_h.ctypes.data, ini_h.ctypes.data,
                                      fin_h.ctypes.data, pt.ctypes.data, po.ctypes.data, ct.ctypes.data, co.ctypes.data, len(chroms), text, cap,
                                      C.byref(need), THREADS)

    return run_case(eng, f"gudmc rows n={n} windows={w} rows={rows} of {nn * w}", dev_call, host_call, host_copy, 7 * 8 * rows, dict(rows=rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "popgenwrite_ops.jsonl"))
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the number of windows (for a quick look)")
    ap.add_argument("--gudmc-rows", type=int, default=4_000_000)
    args = ap.parse_args()
    eng = Engine(0)
    rng = np.random.default_rng(1)
    records = []
    for n, nw in ((200, 1496), (5, 1496)):
        nw = max(8, int(nw * args.scale))
        for rec in (fst_case(eng, n, nw, rng), gudmc_case(eng, n, nw, max(1000, int(args.gudmc_rows * args.scale)), rng)):
            records.append(rec)
            print(json.dumps(rec), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
