#!/usr/bin/env python3
"""The CLI with --result-writer host and gpu, and another build's binary beside them (--parent-cli: the parent commit's), on the
200-pool x 1 M-locus synthetic sync file of tools/bench_sync.py: `ols_iter` and `ols_iter_with_kinship` with both sync parsers,
`fisher_exact_test` with the host parser.  --n-threads 16, PGH_TIMING=1, the legs in turn inside each of the rounds; the wall clock
of every run, the medians and the laps of the last run of each leg go to profiles/resultwrite_e2e.txt.

    python tools/bench_resultwrite_e2e.py [--parent-cli path/to/poolgen] [--rounds 7] [--shape 200x1000000] [--dir /tmp]
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from bench_sync import synthetic_sync  # noqa: E402

CLI = ROOT / "poolgen_amd" / "csrc" / "poolgen"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-cli", default="")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--shape", default="200x1000000")
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--only", default="", help="one analysis instead of the three")
    ap.add_argument("--reverse", action="store_true", help="the writers in the order parent, gpu, host inside a round (the order is part of what a run sees)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "resultwrite_e2e.txt"))
    a = ap.parse_args()
    n, L = (int(x) for x in a.shape.split("x"))
    work = Path(tempfile.mkdtemp(prefix="bench_resultwrite_", dir=a.dir))
    sync, phen = work / "synthetic.sync", work / "phen.csv"
    text, _ = synthetic_sync(L, n)
    text.tofile(sync)
    size = int(text.size)
    del text
    rng = np.random.default_rng(2)
    phen.write_text("#pop,size,trait\n" + "".join(f"Pool{i},20.0,{rng.random():.6f}\n" for i in range(n)))
    env = dict(os.environ, PGH_TIMING="1")
    writers = ["host", "gpu"] + (["parent"] if a.parent_cli else [])
    if a.reverse:
        writers.reverse()
    legs = [(an, ps, w) for an, parsers in (("ols_iter", ("host", "gpu")), ("ols_iter_with_kinship", ("host", "gpu")), ("fisher_exact_test", ("host",)))
            if not a.only or an == a.only for ps in parsers for w in writers]
    t = {leg: [] for leg in legs}
    laps, sizes = {}, {}
    for r in range(a.rounds):
        print(f"bench_resultwrite_e2e: round {r + 1} of {a.rounds}", file=sys.stderr, flush=True)
        for an, ps, w in legs:
            o = work / f"{an}_{ps}_{w}_{r}.csv"
            cmd = [a.parent_cli if w == "parent" else str(CLI), an, "-f", str(sync), "-p", str(phen), "-o", str(o), "--n-threads", str(a.threads),
                   "--sync-parser", ps] + ([] if w == "parent" else ["--result-writer", w])
            t0 = time.perf_counter()
            p = subprocess.run(cmd, capture_output=True, text=True, env=env)
            t[(an, ps, w)].append(time.perf_counter() - t0)
            if p.returncode != 0:
                sys.exit(f"bench_resultwrite_e2e: {' '.join(cmd)} failed: {p.stderr}")
            laps[(an, ps, w)] = p.stderr
            sizes[(an, ps, w)] = o.stat().st_size
            o.unlink()
    sync.unlink(); phen.unlink(); os.rmdir(work)
    with open(a.out, "w") as f:
        f.write(f"poolgen <analysis> --n-threads {a.threads} --sync-parser <host|gpu> --result-writer <host|gpu> (and the parent commit's binary, which has no\n"
                f"such flag) on {n} pools x {L} loci of synthetic sync text ({size} bytes), PGH_TIMING=1; wall clock of the process, {a.rounds} runs each,\n"
                f"the legs in turn inside every round (--reverse: the writers in the order parent, gpu, host).\n\n")
        for an, ps, w in legs:
            v = t[(an, ps, w)]
            f.write(f"{an} --sync-parser {ps} writer {w}: median {statistics.median(v):.3f} s  (" + " ".join(f"{x:.3f}" for x in v) +
                    f")  min {min(v):.3f} max {max(v):.3f}  output {sizes[(an, ps, w)]} bytes\n")
            if w == writers[-1]:
                med = {x: statistics.median(t[(an, ps, x)]) for x in writers}
                f.write(f"{an} --sync-parser {ps}: host / gpu = {med['host'] / med['gpu']:.3f}" +
                        (f", host / parent = {med['host'] / med['parent']:.3f}" if "parent" in med else "") + "\n\n")
        for leg in legs:
            f.write(f"---- laps of the last run: {leg[0]} --sync-parser {leg[1]} writer {leg[2]}\n{laps[leg]}\n")
    print(Path(a.out).read_text()[:6000], flush=True)


if __name__ == "__main__":
    main()
