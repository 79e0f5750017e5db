"""tools/slim_suite_profile.py <dir> — the two tables tests/test_kernel_coverage.py reads (gpu_suite_kernel_stats.csv, kernels_by_test.json, as
tools/final_profiles.sh leaves them) cut down to what is committed: the stats rows of this library's kernels only (torch's and hipBLASLt's are
dropped), one witness test per instantiation instead of three, one instantiation per line.  Nothing is added or renamed."""
import json
import os
import sys

d = sys.argv[1]
p = os.path.join(d, "gpu_suite_kernel_stats.csv")
lines = open(p).read().splitlines()
open(p, "w").write("\n".join([lines[0]] + [l for l in lines[1:] if "mpcvr" in l]) + "\n")
p = os.path.join(d, "kernels_by_test.json")
w = json.load(open(p))
kernels = w.pop("kernels")
rows = ",\n".join("%s: %s" % (json.dumps(k), json.dumps({"launches": v["launches"], "tests": v["tests"][:1]})) for k, v in kernels.items())
open(p, "w").write(json.dumps(w)[:-1] + ', "kernels": {\n' + rows + "\n}}\n")
