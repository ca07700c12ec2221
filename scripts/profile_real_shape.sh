cd /tmp && export TMPDIR=/tmp
OUT=$(mkdir -p "${1:?usage: bash scripts/profile_real_shape.sh <output directory>}" && cd "$1" && pwd)
cd "$(dirname "$0")/.."
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/prof_real -- python3 bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-host-inclusive --no-batched --no-train --no-scaling-model > "$OUT"/prof_real.log 2>&1
python3 - "$OUT" <<'PY'
import csv, glob, sys
f = sorted(glob.glob(sys.argv[1] + "/prof_real/**/*kernel_trace.csv", recursive=True))[-1]
rows = [r for r in csv.DictReader(open(f)) if "k_step_fused" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
import collections
by = collections.defaultdict(list)
for r in rows:
    by[(r["Kernel_Name"].split("(")[0][-28:], r.get("Grid_Size_X", r.get("Grid_Size", "?")))].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
for k, v in sorted(by.items(), key=lambda kv: -len(kv[1])):
    v.sort()
    print(k, "n", len(v), "median_us %.2f" % v[len(v) // 2], "min %.2f" % v[0])
# gaps between consecutive launches of the most common small-grid kernel
PY
rm -rf "$OUT"/prof_real
