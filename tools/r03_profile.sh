#!/bin/bash
# Round-3 evidence for the bench line, all from ONE command line (python3 bench.py --full [flags]) on one MI355X box:
#   1. the bench JSON itself                                   -> $OUT/${TAG}_bench.json
#   2. rocprofv3 --kernel-trace --stats of the same command    -> $OUT/${TAG}_kernel_stats.csv (our kernels' rows)
#   3. rocprofv3 --pmc passes (FETCH_SIZE | WRITE_SIZE | MFMA busy), one counter group per pass, --kernel-trace only
#                                                             -> $OUT/${TAG}_pmc_summary.txt, $OUT/${TAG}_pmc_traffic.json
# Copy the four files into profiles/ afterwards (profiles/pmc_traffic.json is what bench.py reads for `traffic`; it carries the
# hash of the kernel sources it was measured on, and bench.py says "stale" when the sources have changed since).
# New against r02_profile.sh: the two sweep legs (m = 0 two-pass, forced m = 8) are told apart by dispatch order instead of
# sharing one per-kernel mean, and the secondary legs (count operators, ridge passes) are in the same passes.
# The bench JSON is taken LAST, with the fresh counter file already in place, so that its `traffic` fields are this box's own.
# usage: tools/r03_profile.sh [tag]   (files $OUT/<tag>_*; default r03_b)
TAG=${1:-r03_b}; export TAG
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-profile_out}; export OUT
mkdir -p "$OUT"
# ... and once FIRST, on the box as it comes: after six minutes of profiling passes the memory-bound kernels of the same box run
# 8-10 % slower (sweep 2.97 against 2.71 ms under rocprof minutes earlier: r03_d / r03_e of round 3).  The early line is the one
# kept when the committed counter file already belongs to these sources (its `traffic` is then fresh as well).
python3 bench.py --full > $OUT/${TAG}_bench_first.json 2> $OUT/${TAG}_bench_first.err; echo "first bench rc=$?"
rm -rf $OUT/${TAG}_prof && mkdir -p $OUT/${TAG}_prof
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -- python3 bench.py --full --no-cpu-baseline > $OUT/${TAG}_prof.log 2>&1; echo "rocprof rc=$?"
f=$(find $OUT/${TAG}_prof -name "*kernel_stats.csv" | head -1)
python3 - "$f" > $OUT/${TAG}_kernel_stats.csv <<'PY'
import csv, sys
rows = list(csv.reader(open(sys.argv[1])))
w = csv.writer(sys.stdout)
w.writerow(rows[0])
for r in rows[1:]:
    if "k_" in r[0] and "at::" not in r[0]:
        r[0] = r[0].replace("(anonymous namespace)::", "")
        w.writerow(r)
PY
cut -c1-150 $OUT/${TAG}_kernel_stats.csv
rm -rf $OUT/${TAG}_prof
: > $OUT/${TAG}_pmc_summary.txt
i=0
for ctrs in "FETCH_SIZE" "WRITE_SIZE" "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE"; do
  i=$((i+1))
  rm -rf $OUT/${TAG}_pmc_$i && mkdir -p $OUT/${TAG}_pmc_$i
  timeout -k 10 500 rocprofv3 --pmc $ctrs --kernel-trace --output-format csv -d $OUT/${TAG}_pmc_$i -- python3 bench.py --full --steps 3 --warmup 1 --sweep-steps 2 --no-cpu-baseline > $OUT/${TAG}_pmc_$i.log 2>&1
  echo "pmc pass $i ($ctrs) rc=$?"
  f=$(find $OUT/${TAG}_pmc_$i -name "*counter_collection.csv" | head -1)
  python3 - "$f" >> $OUT/${TAG}_pmc_summary.txt <<'PY'
import csv, sys, collections
rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r.get("Dispatch_Id", 0)))
acc = collections.defaultdict(lambda: collections.defaultdict(list))
for r in rows:
    name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:44]
    if not name.startswith("k_"): continue
    acc[name][r["Counter_Name"]].append(float(r["Counter_Value"]))
for k, d in sorted(acc.items()):
    for c, v in d.items():
        print(f"{k:44s} {c:28s} n={len(v):3d} mean={sum(v)/len(v):.6g}")
        if k.startswith("k_ols_sweep_mfma") and len(v) >= 2 and len(v) % 2 == 0:
            # bench.py launches the m = 0 two-pass leg first, the forced m = 8 leg second, the same number of times each
            h = len(v) // 2
            print(f"{(k + ' [leg two_pass]')[:44]:44s} {c:28s} n={h:3d} mean={sum(v[:h])/h:.6g}")
            print(f"{(k + ' [leg m8]')[:44]:44s} {c:28s} n={h:3d} mean={sum(v[h:])/h:.6g}")
PY
  rm -rf $OUT/${TAG}_pmc_$i
done
python3 - <<'PY'
import hashlib, json, re
import os; OUT = os.environ["OUT"]
from pathlib import Path
vals = {}
import os
TAG = os.environ["TAG"]
for line in open(f"{OUT}/{TAG}_pmc_summary.txt"):
    m = re.match(r"(.{44})\s(\S+)\s+n=\s*(\d+)\s+mean=(\S+)", line)
    if m: vals[(m.group(1).strip(), m.group(2))] = float(m.group(4))
def find(prefix, ctr):
    for (k, c), v in vals.items():
        if c == ctr and k.startswith(prefix): return v
    return None
def hbm(prefix):  # gfx950: FETCH_SIZE (KiB) counts half of a wide streaming read (MI355X_MICROARCH.md, HBM); WRITE_SIZE is exact
    f, w = find(prefix, "FETCH_SIZE"), find(prefix, "WRITE_SIZE")
    return None if f is None or w is None else int((2 * f + w) * 1024)
src = hashlib.sha256()
for p in sorted(list(Path("poolgen_amd/csrc").glob("*.hip")) + list(Path("poolgen_amd/csrc").glob("*.h"))):
    src.update(p.read_bytes())
out = {"_comment": "HBM bytes per launch from rocprofv3 --pmc passes of `python3 bench.py --full --steps 3 --warmup 1 --sweep-steps 2 --no-cpu-baseline` "
                   "(tools/r03_profile.sh; per-kernel means in the `source` file): (2 * FETCH_SIZE + WRITE_SIZE) * 1024, the factor 2 being the "
                   "gfx950 wide-read correction of MI355X_MICROARCH.md.  The sweep legs are separated by dispatch order.",
       "source": f"profiles/{TAG}_pmc_summary.txt", "workload": "200x10000000", "kernel_sources_sha256": src.hexdigest(),
       "kinship_hbm_bytes_per_launch": hbm("k_kinship_syrk<true, true, 3"),
       "kinship_two_pass_hbm_bytes_per_launch": hbm("k_kinship_syrk<false, true, 3"),
       "sweep_two_pass_hbm_bytes_per_launch": hbm("k_ols_sweep_mfma<5, 3, 1, 0> [leg two_pass]"),
       "sweep_m8_hbm_bytes_per_launch": hbm("k_ols_sweep_mfma<5, 3, 1, 0> [leg m8]"),
       "ols_iter_stream_hbm_bytes_per_launch": hbm("k_locus_stream<0, true, 1>"),
       "pearson_stream_hbm_bytes_per_launch": hbm("k_locus_stream<1, true, 1>"),
       "chisq_stream_hbm_bytes_per_launch": hbm("k_locus_stream<2, true, 1>"),
       "ridge_predict_hbm_bytes_per_launch": hbm("k_gp_predict_folds")}
mf, ga = find("k_kinship_syrk<true, true, 3", "SQ_VALU_MFMA_BUSY_CYCLES"), find("k_kinship_syrk<true, true, 3", "GRBM_GUI_ACTIVE")
if mf and ga: out["kinship_mfma_busy_frac"] = mf / 1024.0 / (ga / 8.0)
json.dump(out, open(f"{OUT}/{TAG}_pmc_traffic.json", "w"), indent=1)
print(json.dumps(out, indent=1))
PY
cp $OUT/${TAG}_pmc_traffic.json profiles/pmc_traffic.json
python3 bench.py --full > $OUT/${TAG}_bench_last.json 2> $OUT/${TAG}_bench.err; echo "bench rc=$?"
python3 - <<'PY'
import json, os, shutil
OUT = os.environ["OUT"]
tag = os.environ["TAG"]
first, last = f"{OUT}/{tag}_bench_first.json", f"{OUT}/{tag}_bench_last.json"
try:
    fresh_first = not json.load(open(first))["roofline"].get("traffic_stale", True)
except Exception:
    fresh_first = False
shutil.copy(first if fresh_first else last, f"{OUT}/{tag}_bench.json")
print("bench line kept:", "the first (counter file already matched the sources)" if fresh_first else "the last (taken with the new counter file)")
for f in (first, last):
    try:
        d = json.load(open(f)); print(f, "step %.3f ms" % d["ms_per_step"], "sweep %.3f ms" % d["roofline_sweep"]["two_pass"]["avg_ms"])
    except Exception as e:
        print(f, "unreadable:", e)
PY
python3 -c "
import json; d = json.load(open('$OUT/${TAG}_bench.json'))
print('step %.3f ms' % d['ms_per_step'], 'roofline', d['roofline']['frac'], 'traffic', d['roofline']['traffic'], 'stale' if d['roofline'].get('traffic_stale') else 'fresh')
for leg in ('two_pass', 'm8'): print(leg, d['roofline_sweep'][leg]['avg_ms'], d['roofline_sweep'][leg]['frac'], d['roofline_sweep'][leg]['ms_per_step'])
s = d['secondary']
for op in ('ols_iter', 'pearson_corr', 'chisq_test'): print(op, s['count_operators'][op]['kernel_ms'], s['count_operators'][op]['frac'])
for op in ('coefficient_pass', 'prediction_pass'): print(op, s['ridge'][op]['kernel_ms'], s['ridge'][op]['frac'])
print('ridge wall', s['ridge']['wall_s'])
"
