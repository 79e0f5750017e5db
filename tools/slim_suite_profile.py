"""tools/slim_suite_profile.py <dir> — the two tables tests/test_kernel_coverage.py reads (gpu_suite_kernel_stats.csv, kernels_by_test.json, as
tools/final_profiles.sh leaves them) cut down to what is committed: the stats rows of this library's kernels only (torch's and hipBLASLt's are
dropped), one witness test per instantiation instead of three, one instantiation per line.  From round 14 on the stats rows keep the
instantiation's name with its argument list emptied and its number of calls: the durations of the suite's launches are those of toy shapes under
a tracer and say nothing about the kernels (the timed tables are the tools/bench_*.py files of a round).  Nothing is added or renamed."""
import csv
import json
import os
import sys


def without_arguments(name):
    """'ns::k_x<1>(ns::Params, int)' -> 'ns::k_x<1>()': the last parenthesised group emptied, if the name ends in one (the '(' stays:
    tests/test_kernel_coverage.py finds the end of the template arguments by it)"""
    if not name.endswith(")"):
        return name
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        depth += (name[i] == ")") - (name[i] == "(")
        if depth == 0:
            return name[:i] + "()"
    return name


d = sys.argv[1]
p = os.path.join(d, "gpu_suite_kernel_stats.csv")
rows = [r for r in csv.DictReader(open(p)) if "mpcvr" in r["Name"]]
with open(p, "w", newline="") as f:
    out = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC, lineterminator="\n")
    out.writerow(["Name", "Calls"])
    for r in rows:
        out.writerow([without_arguments(r["Name"]), int(r["Calls"])])
p = os.path.join(d, "kernels_by_test.json")
w = json.load(open(p))
kernels = w.pop("kernels")
rows = ",\n".join("%s: %s" % (json.dumps(k), json.dumps({"launches": v["launches"], "tests": v["tests"][:1]})) for k, v in kernels.items())
open(p, "w").write(json.dumps(w)[:-1] + ', "kernels": {\n' + rows + "\n}}\n")
