"""tools/prof_deint.py — the deinterlacing pass under rocprofv3: what the kernel itself takes, and how busy the vector ALU is.

    rocprofv3 --kernel-trace --output-format csv -d DIR/kt -o p -- python tools/prof_deint.py run
    rocprofv3 --pmc SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY --kernel-trace --output-format csv -d DIR/pmc -o p -- python tools/prof_deint.py run
    python tools/prof_deint.py summarise DIR > deint_counters.txt

`run` launches mpcvr_deint_pass 12 times per case (1920x1080 and 3840x2160, NV12 and P010, both modes) on resident samples with a
synchronize between the cases; the cases are told apart by their order and by the grid of the launch.  `summarise` prints, per
instantiation and grid, the median duration of the kernel trace (no counters) and, from the counter run, the VALU pipe's busy share of
the launch — (SQ_ACTIVE_INST_VALU x 4 / 1024 SIMDs) / (SQ_BUSY_CYCLES / 32 SQs), the reading of tools/pmc_traffic.sh — and the share of
wave cycles spent waiting (SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES).  Needs a GPU."""
import csv
import ctypes as C
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(w, h, f, m) for (w, h) in ((1920, 1080), (3840, 2160)) for f in ("nv12", "p010") for m in (0, 1)]
CALLS = 12


def run():
    import torch
    from videorenderer_amd import api
    L = api.load_library()
    for w, h, f, mode in CASES:
        cformat, by = (api.CF_NV12, 1) if f == "nv12" else (api.CF_P010, 2)
        frame = w * by * h * 3 // 2
        src = [torch.randint(0, 256, (frame,), dtype=torch.uint8, device="cuda") for _ in range(3)]
        dst = torch.empty(frame, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for i in range(CALLS):
            hr = L.mpcvr_deint_pass(C.c_void_p(src[0].data_ptr()), C.c_void_p(src[1].data_ptr()), C.c_void_p(src[2].data_ptr()), cformat, w, h, w * by,
                                    i & 1, 1 - (i & 1), mode, C.c_void_p(dst.data_ptr()), w * by, None)
            assert hr == 0, hr
        torch.cuda.synchronize()


def short(name):
    m = re.search(r"k_deint<[^>]*>", name)
    return m.group(0).replace("(int)", "").replace(" ", "") if m else None


def grid(r):
    """workgroups in x and y of a trace / counter row, as far as the file tells (0: it does not)"""
    gx = r.get("Grid_Size_X") or r.get("Grid_Size") or 0
    return int(float(gx)) // 64, int(float(r.get("Grid_Size_Y") or 0)) // max(1, int(float(r.get("Workgroup_Size_Y") or 1)))


def summarise(d):
    import numpy as np
    dur = {}
    for f in glob.glob(os.path.join(d, "kt", "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            k = short(r.get("Kernel_Name", ""))
            if k:
                key = (k,) + grid(r)
                dur.setdefault(key, []).append((float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) * 1e-3)
    sq = {}
    for f in glob.glob(os.path.join(d, "pmc", "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            k = short(r.get("Kernel_Name", ""))
            if k:
                key = (k, grid(r)[0], 0)
                c = sq.setdefault(key, {})
                c[r["Counter_Name"]] = c.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    print("# kernel trace, no counters: median microseconds of %d launches per case (min .. max); grid = workgroups in x (256 steps each) x workgroups in y (16 rows each); in the counter rows grid-x is the launch's work-items / 64" % CALLS)
    for key in sorted(dur):
        t = dur[key]
        print("%-18s grid %3d x %4d  launches %3d  %8.1f us (%.1f .. %.1f)" % (key[0], key[1], key[2], len(t), float(np.median(t)), min(t), max(t)))
    print("# counter run: VALU busy share of the launch = (SQ_ACTIVE_INST_VALU * 4 / 1024) / (SQ_BUSY_CYCLES / 32); waiting = SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES; summed over the launches of a key")
    for key in sorted(sq):
        c = sq[key]
        if c.get("SQ_BUSY_CYCLES") and c.get("SQ_WAVE_CYCLES"):
            print("%-18s grid-x %5d  valu_busy %.3f  waiting %.3f" % (key[0], key[1], (c["SQ_ACTIVE_INST_VALU"] * 4 / 1024) / (c["SQ_BUSY_CYCLES"] / 32),
                                                                     c["SQ_WAIT_INST_ANY"] / c["SQ_WAVE_CYCLES"]))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) >= 3 and sys.argv[1] == "summarise":
        summarise(sys.argv[2])
    else:
        raise SystemExit(__doc__)
