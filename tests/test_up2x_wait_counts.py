"""What the headline kernel's hot loop waits for, read off the compiled code (no GPU needed).

k_fused_up2x<5, PQ table, P01x, integer dither> prefetches the raw codes of a row pair two iterations ahead so that the row
stores of the iterations in between can stay in flight.  On the gfx9 family loads and stores share one in-order counter, so this
only holds if the wait in front of each convert stage names the exact count; left to the compiler the loop carried
`s_waitcnt vmcnt(3..0)` there — every iteration waited for its own stores.  The headline-only translation unit is compiled the way
tools/isa_headline.sh does it, disassembled, and its hot loop (found as tools/isa_mix.py finds it: the longest backward branch) is
checked:

  * a counted wait (vmcnt >= 8) stands in front of each of the four unrolled convert stages, and every lower count in the loop is
    a fall-back rung: it sits in a block entered only through the ladder's scalar conditional branches;
  * every global load is followed by a vmcnt wait before the first instruction that touches its destination register, and the
    counted wait in front of that instruction leaves no more in flight than was issued behind the load;
  * registers, occupancy, scratch and the VALU work of the loop did not grow.

The VALU figures of the loop before the counted wait were 1,120 packed + 852 plain + 96 transcendental = 3,476 issue units
(plain 1, packed 2, transcendental 4: tools/isa_mix.py).  No class may exceed its figure by more than 1 %, and the issue units stay
within 1 % either way.  (With the counted wait the plain class is 829: the 24 v_mov_b32 that copied prefetched codes between
registers are gone, one v_readlane_b32 came; packed and transcendental are unchanged, 3,453 units.)
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "videorenderer_amd", "csrc", "vp_fused_up2x_nt5.hip")
PARENT_VALU = {"packed": 1120, "plain": 852, "trans": 96}
HIGH = 8            # the row stores of the two preceding iterations may all still be in flight


def _tool(name, *more):
    for cand in (os.environ.get(name.upper()), shutil.which(name)) + more:
        if cand and os.path.exists(cand):
            return cand
    return None


HIPCC = _tool("hipcc", "/opt/rocm/bin/hipcc")
OBJDUMP = _tool("llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/llvm/bin/llvm-objdump")
pytestmark = pytest.mark.skipif(HIPCC is None or OBJDUMP is None, reason="hipcc / llvm-objdump not installed")


class Inst:
    def __init__(self, addr, op, args):
        self.addr, self.op, self.args = addr, op, args

    def vmcnt(self):
        m = re.search(r"vmcnt\((\d+)\)", self.args) if self.op == "s_waitcnt" else None
        return int(m.group(1)) if m else None

    def is_branch(self):
        return self.op == "s_branch" or self.op.startswith("s_cbranch")

    def target(self):
        off = int(self.args.split()[0])
        return self.addr + 4 + (off - 65536 if off >= 32768 else off) * 4

    def is_vmem(self):
        return self.op.startswith(("global_", "buffer_", "flat_", "scratch_"))

    def vgprs(self):
        regs = set()
        for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", self.args):
            regs.update(range(int(a), int(b) + 1))
        regs.update(int(r) for r in re.findall(r"\bv(\d+)\b", self.args))
        return regs

    def load_dest(self):
        first = self.args.split(",")[0].strip()
        m = re.fullmatch(r"v\[(\d+):(\d+)\]", first)
        if m:
            return set(range(int(m.group(1)), int(m.group(2)) + 1))
        return {int(re.fullmatch(r"v(\d+)", first).group(1))}


@pytest.fixture(scope="module")
def headline(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa_headline")
    cmd = [HIPCC, "-x", "hip", "-c", SRC, "-DMPCVR_UP2X_HEADLINE_ONLY", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
           "-Wno-unused-function", "-Wno-unused-variable", "-save-temps=obj", "-o", str(out / "nt5.o"), "-Rpass-analysis=kernel-resource-usage"]
    cc = subprocess.run(cmd, cwd=out, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, cc.stdout[-4000:]
    res = {}
    for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
                     ("vgpr_spill", r"VGPRs Spill: (\d+)")):
        found = re.findall(pat, cc.stdout)
        assert len(found) == 1, (key, found)           # the headline-only unit holds one kernel
        res[key] = int(found[0])
    lst = subprocess.run([OBJDUMP, "-d", str(out / "vp_fused_up2x_nt5-hip-amdgcn-amd-amdhsa-gfx950.out")], stdout=subprocess.PIPE, text=True, check=True).stdout
    lines = lst.split("\n")
    start = end = None
    for i, l in enumerate(lines):
        if re.match(r"^[0-9a-f]+ <.*>:$", l):
            if start is not None:
                end = i
                break
            if "k_fused_up2x" in l:
                start = i
    assert start is not None
    body = []
    for l in lines[start + 1:end]:
        m = re.match(r"^\s+(\S+)\s+(.*?)//\s*([0-9A-Fa-f]+):", l)
        if m:
            body.append(Inst(int(m.group(3), 16), m.group(1), m.group(2).strip()))
    index = {ins.addr: i for i, ins in enumerate(body)}
    best = None
    for i, ins in enumerate(body):            # the hot loop: the longest backward branch (tools/isa_mix.py)
        if ins.is_branch() and ins.target() in index and index[ins.target()] < i:
            span = i - index[ins.target()]
            if best is None or span > best[0]:
                best = (span, index[ins.target()], i)
    assert best is not None
    return {"res": res, "body": body, "index": index, "lo": best[1], "hi": best[2]}


def test_counted_wait_in_front_of_each_convert_stage(headline):
    body, index, lo, hi = headline["body"], headline["index"], headline["lo"], headline["hi"]
    waits = [(i, body[i].vmcnt()) for i in range(lo, hi + 1) if body[i].vmcnt() is not None]
    print("vmcnt waits of the loop (instruction, count):", [(i - lo, n) for i, n in waits])
    high = [i for i, n in waits if n >= HIGH]
    assert len(high) >= 4, f"counted waits (vmcnt >= {HIGH}) in the loop: {len(high)}"
    # one per unrolled iteration: the loop's stores come in four groups, and a counted wait stands in front of each
    stores = [i for i in range(lo, hi + 1) if body[i].op.startswith("global_store")]
    assert stores
    per_iter = len(stores) // 4
    for g in range(4):
        first = stores[g * per_iter]
        before = stores[g * per_iter - 1] if g else lo - 1
        assert any(before < i < first for i in high), f"no counted wait in front of store group {g}"

    targets = {}
    for i, ins in enumerate(body):
        if ins.is_branch() and ins.target() in index:
            targets.setdefault(index[ins.target()], []).append(i)
    leaders = set(targets) | {i + 1 for i, ins in enumerate(body) if ins.is_branch()}

    def scalar_ladder_branch(i):
        return body[i].op in ("s_cbranch_scc0", "s_cbranch_scc1") and body[i - 1].op.startswith("s_cmp_")

    for w, n in waits:
        if n >= HIGH:
            continue
        b = max(l for l in leaders if l <= w)
        prev = body[b - 1]
        into = targets.get(b, [])
        # no way in but the ladder's conditional branches: taken (a target of them alone), or not taken (the block behind one)
        assert prev.op == "s_branch" or scalar_ladder_branch(b - 1), f"vmcnt({n}) at loop instruction {w - lo}: reached by falling through from `{prev.op} {prev.args}`"
        assert all(scalar_ladder_branch(j) for j in into), f"vmcnt({n}) at loop instruction {w - lo}: a target of {[body[j].op for j in into]}"
        assert into or scalar_ladder_branch(b - 1), f"vmcnt({n}) at loop instruction {w - lo}: not behind a conditional branch"


def test_every_load_is_waited_for_before_its_first_use(headline):
    body, lo, hi = headline["body"], headline["lo"], headline["hi"]
    loads = [i for i, ins in enumerate(body) if ins.op.startswith("global_load") and i <= hi]
    assert sum(lo <= i <= hi for i in loads) >= 4
    for i in loads:
        dest = body[i].load_dest()
        # forward from the load; inside the loop with wrap-around, in front of it straight on into the loop
        walk = list(range(i + 1, hi + 1)) + (list(range(lo, i)) if i >= lo else [])
        waited, younger, last_counted = False, 0, None
        for j in walk:
            ins = body[j]
            if ins.vmcnt() is not None:
                waited = True
                if ins.vmcnt() >= HIGH:
                    last_counted = (ins.vmcnt(), younger)
            elif ins.is_vmem() and not ins.vgprs() & dest:
                younger += 1
            elif ins.vgprs() & dest:
                assert waited, f"{ins.op} {ins.args} touches the destination of `{body[i].op} {body[i].args}` with no vmcnt wait in between"
                if i >= lo and last_counted is not None:
                    n, issued = last_counted
                    assert n <= issued, f"vmcnt({n}) in front of the first use of `{body[i].args}`, but only {issued} vector memory operations were issued behind the load"
                break
        else:
            pytest.fail(f"`{body[i].op} {body[i].args}`: destination never used")


def test_resources_do_not_regress(headline):
    res, body, lo, hi = headline["res"], headline["body"], headline["lo"], headline["hi"]
    print("resources:", res)
    assert res["vgprs"] <= 168
    assert res["occupancy"] == 3
    assert res["scratch"] == 0 and res["vgpr_spill"] == 0
    cnt = {"packed": 0, "plain": 0, "trans": 0}
    for ins in body[lo:hi + 1]:
        if ins.op.startswith("v_pk_") and ins.op.endswith("_f32"):
            cnt["packed"] += 1
        elif ins.op.startswith(("v_exp", "v_log", "v_rcp", "v_rsq", "v_sqrt", "v_sin", "v_cos")):
            cnt["trans"] += 1
        elif ins.op.startswith("v_") and not ins.op.startswith("v_mfma"):
            cnt["plain"] += 1
    print("VALU instructions of the loop:", cnt, "before the counted wait:", PARENT_VALU)
    for k, v in PARENT_VALU.items():
        assert cnt[k] <= v * 1.01, (k, cnt[k], v)
    units = lambda c: c["plain"] + 2 * c["packed"] + 4 * c["trans"]
    assert abs(units(cnt) - units(PARENT_VALU)) <= 0.01 * units(PARENT_VALU), (units(cnt), units(PARENT_VALU))
