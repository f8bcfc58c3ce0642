#!/usr/bin/env python3
"""The CLI's `fst` and `gudmc --popgen-as-documented` with --popgen-writer host and gpu, and another build's binary beside them
(--parent-cli: the parent commit's, which has no such flag), on a synthetic sync file of tools/bench_sync.py (consecutive
positions on five chromosomes: windows of 100 bp every 50 bp give loci / 50 windows).  --n-threads 16, PGH_TIMING=1, the legs in
turn inside each of the rounds; the wall clock of every run, the medians and the laps of the last run of each leg go to
profiles/popgenwrite_e2e.txt.

    python tools/bench_popgenwrite_e2e.py [--parent-cli path/to/poolgen] [--rounds 7] [--shape 200x74800] [--dir /tmp]
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
ANALYSES = {"fst": [], "gudmc": ["--popgen-as-documented"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-cli", default="")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--shape", default="200x74800", help="pools x loci; 74 800 loci are 1 496 windows")
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--out", default=str(ROOT / "profiles" / "popgenwrite_e2e.txt"))
    a = ap.parse_args()
    n, L = (int(x) for x in a.shape.split("x"))
    work = Path(tempfile.mkdtemp(prefix="bench_popgenwrite_", dir=a.dir))
    sync, phen = work / "synthetic.sync", work / "phen.csv"
    text, _ = synthetic_sync(L, n)
    text.tofile(sync)
    size = int(text.size)
    del text
    rng = np.random.default_rng(2)
    phen.write_text("#pop,size,trait\n" + "".join(f"Pool{i},20.0,{rng.random():.6f}\n" for i in range(n)))
    env = dict(os.environ, PGH_TIMING="1")
    writers = ["host", "gpu"] + (["parent"] if a.parent_cli else [])
    legs = [(an, w) for an in ANALYSES for w in writers]
    t = {leg: [] for leg in legs}
    laps, sizes = {}, {}
    for r in range(a.rounds):
        print(f"bench_popgenwrite_e2e: round {r + 1} of {a.rounds}", file=sys.stderr, flush=True)
        for an, w in legs:
            o = work / f"{an}_{w}_{r}.csv"
            cmd = [a.parent_cli if w == "parent" else str(CLI), an, "-f", str(sync), "-p", str(phen), "-o", str(o), "--n-threads", str(a.threads),
                   "--window-size-bp", "100", "--window-slide-size-bp", "50", "--min-loci-per-window", "10", *ANALYSES[an]] + \
                  ([] if w == "parent" else ["--popgen-writer", w])
            t0 = time.perf_counter()
            p = subprocess.run(cmd, capture_output=True, text=True, env=env)
            t[(an, w)].append(time.perf_counter() - t0)
            if p.returncode != 0:
                sys.exit(f"bench_popgenwrite_e2e: {' '.join(cmd)} failed: {p.stderr}")
            laps[(an, w)] = p.stderr
            written = sorted(work.glob(f"{an}_{w}_{r}*.csv"))
            sizes[(an, w)] = sum(f.stat().st_size for f in written)
            for f in written:
                f.unlink()
    sync.unlink(); phen.unlink(); os.rmdir(work)
    with open(a.out, "w") as f:
        f.write(f"poolgen <analysis> --n-threads {a.threads} --popgen-writer <host|gpu> (and the parent commit's binary, which has no such flag) on {n} pools x\n"
                f"{L} loci of synthetic sync text ({size} bytes), windows of 100 bp every 50 bp, PGH_TIMING=1; wall clock of the process, {a.rounds} runs\n"
                f"each, the legs in turn inside every round.\n\n")
        for an, w in legs:
            v = t[(an, w)]
            f.write(f"{an} writer {w}: median {statistics.median(v):.3f} s  (" + " ".join(f"{x:.3f}" for x in v) +
                    f")  min {min(v):.3f} max {max(v):.3f}  output {sizes[(an, w)]} bytes\n")
            if w == writers[-1]:
                med = {x: statistics.median(t[(an, x)]) for x in writers}
                f.write(f"{an}: host / gpu = {med['host'] / med['gpu']:.3f}" + (f", host / parent = {med['host'] / med['parent']:.3f}" if "parent" in med else "") + "\n\n")
        for leg in legs:
            f.write(f"---- laps of the last run: {leg[0]} writer {leg[1]}\n{laps[leg]}\n")
    print(Path(a.out).read_text()[:6000], flush=True)


if __name__ == "__main__":
    main()
