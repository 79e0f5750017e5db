"""The hot loop of k_fused_up2x_bp — the bi-planar twin of the exact-2x fused kernel (csrc/vp_fused_up2x_bp.h) — read off the compiled
code, and the row identity its carried chroma row stands on (no GPU needed).

The twin's headline instantiation <5, PQ table, P01x, integer dither> is compiled alone (-DMPCVR_UP2X_BP_HEADLINE_ONLY on
vp_fused_up2x_bp_nt5.hip, the way tools/isa_headline.sh compiles the generic one), disassembled, and its hot loop checked with the
checks tests/test_up2x_wait_counts.py applies to the generic loop, plus what the twin is for:

  * one chroma and two luma global_load_dword per unrolled iteration (the generic loop: four and two);
  * `s_waitcnt vmcnt(11)` = 3 loads + 8 row stores in front of each of the four convert stages, lower counts only behind the ladder's
    scalar branches; every load waited for before its first use;
  * occupancy 3, no scratch, no VGPR spills;
  * the loop's VALU classes no higher than the generic loop's (1,120 packed, 829 plain, 96 transcendental: the figures
    tests/test_up2x_wait_counts.py records for it), and no higher than the twin's own baseline + 1 %:
    1,088 packed + 829 plain + 96 transcendental = 3,389 issue units against the generic loop's 3,453 (per four iterations: 32 packed
    instructions fewer — the neighbour column's vertical lerp and the two zero-coefficient matrix FMAs; among the plain ones 24
    conversions fewer, 16 DPP moves and 8 register moves more).

The row identity: every convert stage but a segment's first takes chroma row n from the stage before it, where it was row n + 1.
mpcvr_plan_up2x_row_carry (what LaunchFusedUp2xNT asks before it takes the twin) must say yes only where a replay of the kernel's
iterations — every segment, the clamped rows above and below the rect included — finds the carried row equal to the row the generic
kernel loads, for each (vk1, vk2, vk3) FillFusedArgs emits; and it must say yes for the plan the twin is built for.
"""
import os
import re
import subprocess

import pytest

from tests import test_up2x_wait_counts as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "videorenderer_amd", "csrc", "vp_fused_up2x_bp_nt5.hip")
GENERIC_VALU = {"packed": 1120, "plain": 829, "trans": 96}      # the generic loop today (tests/test_up2x_wait_counts.py's docstring)
TWIN_VALU = {"packed": 1088, "plain": 829, "trans": 96}         # the twin's own baseline
needs_tools = pytest.mark.skipif(WC.HIPCC is None or WC.OBJDUMP is None, reason="hipcc / llvm-objdump not installed")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa_twin")
    cmd = [WC.HIPCC, "-x", "hip", "-c", SRC, "-DMPCVR_UP2X_BP_HEADLINE_ONLY", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
           "-Wno-unused-function", "-Wno-unused-variable", "-save-temps=obj", "-o", str(out / "bp.o"), "-Rpass-analysis=kernel-resource-usage"]
    cc = subprocess.run(cmd, cwd=out, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, cc.stdout[-4000:]
    res = {}
    for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
                     ("vgpr_spill", r"VGPRs Spill: (\d+)")):
        found = re.findall(pat, cc.stdout)
        assert len(found) == 1, (key, found)           # the unit holds one kernel
        res[key] = int(found[0])
    lst = subprocess.run([WC.OBJDUMP, "-d", str(out / "vp_fused_up2x_bp_nt5-hip-amdgcn-amd-amdhsa-gfx950.out")], stdout=subprocess.PIPE, text=True, check=True).stdout
    lines = lst.split("\n")
    start = end = None
    for i, l in enumerate(lines):
        if re.match(r"^[0-9a-f]+ <.*>:$", l):
            if start is not None:
                end = i
                break
            if "k_fused_up2x_bp" in l:
                start = i
    assert start is not None
    body = []
    for l in lines[start + 1:end]:
        m = re.match(r"^\s+(\S+)\s+(.*?)//\s*([0-9A-Fa-f]+):", l)
        if m:
            body.append(WC.Inst(int(m.group(3), 16), m.group(1), m.group(2).strip()))
    index = {ins.addr: i for i, ins in enumerate(body)}
    best = None
    for i, ins in enumerate(body):            # the hot loop: the longest backward branch
        if ins.is_branch() and ins.target() in index and index[ins.target()] < i:
            span = i - index[ins.target()]
            if best is None or span > best[0]:
                best = (span, index[ins.target()], i)
    assert best is not None
    return {"res": res, "body": body, "index": index, "lo": best[1], "hi": best[2]}


@needs_tools
def test_one_chroma_and_two_luma_loads_per_iteration(twin):
    body, lo, hi = twin["body"], twin["lo"], twin["hi"]
    loads = [body[i] for i in range(lo, hi + 1) if body[i].op.startswith("global_load")]
    print("loads of the loop:", [(l.op, l.args) for l in loads])
    assert len(loads) == 12 and all(l.op == "global_load_dword" for l in loads), [(l.op, l.args) for l in loads]
    for g in range(4):                              # a group = one statement: luma, luma, chroma
        offs = [l.args.split(",")[1].strip() for l in loads[3 * g:3 * g + 3]]
        assert offs[0] == offs[1] != offs[2], (g, offs)         # two loads at the lane's luma offset, one at its chroma offset
    # in front of the loop: the segment's first group loads both chroma rows, the second one only the new row
    before = [body[i] for i in range(lo) if body[i].op == "global_load_dword" and re.search(r", s\[\d+:\d+\]$", body[i].args)]
    assert len(before) >= 7, [(l.op, l.args) for l in before]


@needs_tools
def test_counted_wait_of_three_loads_and_eight_stores(twin):
    body, lo, hi = twin["body"], twin["lo"], twin["hi"]
    high = [body[i].vmcnt() for i in range(lo, hi + 1) if body[i].vmcnt() is not None and body[i].vmcnt() >= WC.HIGH]
    assert high == [11, 11, 11, 11], high
    WC.test_counted_wait_in_front_of_each_convert_stage(twin)       # one in front of each store group; lower counts are ladder rungs only
    WC.test_every_load_is_waited_for_before_its_first_use(twin)


@needs_tools
def test_resources_and_valu_classes(twin):
    res, body, lo, hi = twin["res"], twin["body"], twin["lo"], twin["hi"]
    print("resources:", res)
    assert res["vgprs"] <= 168
    assert res["occupancy"] == 3
    assert res["scratch"] == 0 and res["vgpr_spill"] == 0
    cnt = {"packed": 0, "plain": 0, "trans": 0}
    dpp = 0
    for ins in body[lo:hi + 1]:
        if ins.op.startswith("v_pk_") and ins.op.endswith("_f32"):
            cnt["packed"] += 1
        elif ins.op.startswith(("v_exp", "v_log", "v_rcp", "v_rsq", "v_sqrt", "v_sin", "v_cos")):
            cnt["trans"] += 1
        elif ins.op.startswith("v_") and not ins.op.startswith("v_mfma"):
            cnt["plain"] += 1
            dpp += "wave_shl:1" in ins.args
    print("VALU instructions of the twin's loop:", cnt, "generic loop:", GENERIC_VALU, "twin's baseline:", TWIN_VALU)
    assert dpp == 16, dpp                            # four cross-lane moves per iteration, DPP: no LDS round trip
    assert not any(ins.op.startswith("ds_bpermute") for ins in body[lo:hi + 1])
    units = lambda c: c["plain"] + 2 * c["packed"] + 4 * c["trans"]
    for k in cnt:
        assert cnt[k] <= GENERIC_VALU[k], (k, cnt[k], GENERIC_VALU[k])
        assert cnt[k] <= TWIN_VALU[k] * 1.01, (k, cnt[k], TWIN_VALU[k])
    assert units(cnt) <= units(TWIN_VALU) * 1.01 and units(cnt) < units(GENERIC_VALU), (units(cnt), units(TWIN_VALU), units(GENERIC_VALU))


# ---- the row identity ----
SITINGS = {"4:2:2 / 4:4:4": (4, 0, 0), "4:2:0 nearest": (0, 2, 0), "4:2:0 MPEG-2": (2, 0, -1), "4:2:0 co-sited": (2, 0, 0)}      # FillFusedArgs


def chroma_rows(vk, rect_t, H, ch, a):
    """load_raw_unseen's chroma rows (n, n + 1), clamped, for the iteration that converts virtual rows a, a + 1"""
    sy0 = rect_t + min(max(a, 0), H - 1)
    n = (vk[0] * sy0 + vk[1] * (sy0 & ~1) + vk[2]) >> 2
    return min(max(n, 0), ch - 1), min(max(n + 1, 0), ch - 1)


def replay_carries(vk, rect_t, H, ch, seg):
    """the kernel's iterations, segment by segment: does the row carried out of every convert stage equal the row the next one needs?"""
    for s0 in range(0, H, seg):
        s1 = min(s0 + seg, H)
        n_iter = (s1 - s0 + 1) // 2 + 3
        kept = None
        for t in range(n_iter):
            top, bot = chroma_rows(vk, rect_t, H, ch, s0 - 3 + 2 * t)
            if kept is not None and kept != top:
                return False
            kept = bot
    return True


def test_row_carry_is_granted_only_where_every_iteration_finds_its_row(mpcvr):
    from videorenderer_amd import api
    granted = 0
    for name, vk in SITINGS.items():
        for H in (8, 9, 10, 24, 40, 46, 72):
            for rect_t in (0, 1, 2, 6):
                sub = 1 if vk[0] == 4 else 2
                for extra in (0, 1, 4):                    # chroma rows below the rect: none (the frame ends with it), some
                    ch = (rect_t + H + sub - 1) // sub + extra
                    yes = api.plan_up2x_row_carry(*vk, rect_t, H, ch)
                    granted += yes
                    if yes:
                        for seg in (2, 24, 36, 72, 180):     # segment heights are even (LaunchFusedUp2x)
                            assert replay_carries(vk, rect_t, H, ch, min(seg, H + (H & 1))), (name, H, rect_t, ch, seg)
    assert granted > 0
    # the plan the twin is built for: MPEG-2 sited 4:2:0, the whole frame, an even number of rows — and its neighbours that must not
    assert api.plan_up2x_row_carry(2, 0, -1, 0, 2160, 1080) and api.plan_up2x_row_carry(2, 0, -1, 0, 40, 20) and api.plan_up2x_row_carry(2, 0, -1, 0, 8, 4)
    assert not api.plan_up2x_row_carry(2, 0, -1, 2, 40, 21)        # a rect below the frame's top: the rows clamped above it repeat a pair
    assert not api.plan_up2x_row_carry(2, 0, -1, 0, 40, 24)        # a rect that ends above the frame's bottom: the same below it
    assert not api.plan_up2x_row_carry(2, 0, 0, 0, 40, 20)         # co-sited: the clamped rows above the rect repeat rows (0, 1)
    assert not api.plan_up2x_row_carry(4, 0, 0, 0, 40, 40)         # 4:2:2: two chroma rows per iteration
    assert not api.plan_up2x_row_carry(2, 0, -1, 0, 0, 0)
