"""Ranges per host-bound figure, parent vs result, from tools/ab_host.sh's raw
lines: tools/vec_env_bench.py, tools/single_env_bench.py and the vec_env /
single_env variants of bench.py --full.  Prints the ranges (and whether the
result's lies wholly above the parent's), then the raw lines (a bench line
cut down to those two variants)."""
import collections
import json
import sys

vals = collections.defaultdict(lambda: collections.defaultdict(list))
raw = []
label = None
for line in open(sys.argv[1]):
    line = line.strip()
    if line.startswith("## "):
        label = line[3:].split(" ")[0]
        raw.append(line)
        continue
    if not line.startswith("{"):
        continue
    d = json.loads(line)
    if "vec_env_step" in d:
        for k, v in d["vec_env_step"].items():
            vals["vec_env_bench " + k][label].append(v["us_per_step"])
    elif "single_env_step" in d:
        for k, v in d["single_env_step"].items():
            vals["single_env_bench " + k][label].append(v["us_per_step"])
    elif "variants" in d:
        d = {"variants": {s: {k: v for k, v in d["variants"].get(s, {}).items() if isinstance(v, dict) and "us_per_step" in v}
                          for s in ("vec_env", "single_env")}}
        for sect, fig in d["variants"].items():
            for k, v in fig.items():
                vals[f"bench --full {sect} {k}"][label].append(v["us_per_step"])
    raw.append(json.dumps(d))
print("%-62s %-20s %-20s %s" % ("figure (us per step)", "parent min - max", "result min - max", "result wholly above"))
for k, v in vals.items():
    p, r = v.get("parent", []), v.get("result", [])
    if p and r:
        print("%-62s %7.3f - %-10.3f %7.3f - %-10.3f %s" % (k, min(p), max(p), min(r), max(r),
                                                          "YES" if min(r) > max(p) else "no"))
        print("    parent %s\n    result %s" % (" ".join("%.3f" % x for x in p), " ".join("%.3f" % x for x in r)))
print("\nraw lines")
print("\n".join(raw))
