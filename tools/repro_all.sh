#!/bin/bash
# Reproduces every number quoted in DESIGN.md section 5 on one MI355X (takes ~4 minutes):
#   bash tools/repro_all.sh [output directory, default repro_out]
# The --full bench run covers every single-GPU BASELINE config: the headline in the JSON line, the other legs (g1_2p24, g2_2p20, pairing_2p16,
# normalize / deserialize for both groups, call shapes, in-process multi-device) in the sidecar file; the size sweeps follow.
set -e
export OUT=${1:-repro_out}
mkdir -p "$OUT"
python -m pytest tests -m gpu -x -q 2>&1 | tail -1
python -c "import __graft_entry__ as g; g.smoke()"
python bench.py --full --secondary-out "$OUT/bench_secondary.json" > "$OUT/bench_default.json"
python tools/sweep_sizes.py g1 14 24 --validated > "$OUT/sweep_g1.jsonl" 2>/dev/null
python tools/sweep_sizes.py g2 14 21 --validated > "$OUT/sweep_g2.jsonl" 2>/dev/null
python tools/bench_normalize.py > "$OUT/normalize.txt" 2>&1 || true
python tools/bench_deserialize.py 20 > "$OUT/deserialize.txt" 2>&1 || true
python - <<'PY'
import json, os
out = os.environ["OUT"]
d = json.loads([l for l in open(f"{out}/bench_default.json") if l.startswith("{")][-1])
print("g1_2p20", "%.3g points/s" % d["value"], "%.2f ms" % d["ms_per_step"], "bit_exact", d["bit_exact"], "valu frac %.2f" % d["roofline"]["frac"],
      "cpu_baseline %.3g" % d["cpu_baseline"]["value"])
for k, v in json.load(open(f"{out}/bench_secondary.json"))["secondary"].items():
    if "error" in v:
        print(k, v["error"]); continue
    if "ms_per_step" in v and "value" in v:
        print(k, "%.3g %s" % (v["value"], v.get("unit", "")), "%.2f ms" % v["ms_per_step"], "bit_exact", v.get("bit_exact", v.get("same_result")))
    elif k == "pairing_2p16":
        print(k, "%.3g pairs/s" % v["value"], "%.2f ms" % v["ms"], "cancels", v["product_cancels_to_one"], "exact", v["bit_exact"],
              "cpu_baseline %.3g" % v["cpu_baseline"]["value"])
    else:
        print(k, {a: b for a, b in v.items() if not isinstance(b, (dict, str))})
for f in ("sweep_g1", "sweep_g2"):
    for l in open(f"{out}/{f}.jsonl"):
        r = json.loads(l)
        print(r["group"], "2^%d" % r["log_n"], "c", r["c"], "%.3f ms" % r["ms"], "%.3g points/s" % r["points_per_s"], "ok", r["ok"])
PY
tail -2 "$OUT/normalize.txt"; tail -3 "$OUT/deserialize.txt"
