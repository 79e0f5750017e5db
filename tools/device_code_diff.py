"""Compare the gfx950 device code of two builds of the library, translation unit by translation unit (no GPU needed).

    python tools/device_code_diff.py <parent>/videorenderer_amd/_build <this>/videorenderer_amd/_build

For every object file of python -m videorenderer_amd.build: the .hip_fatbin section is dumped (llvm-objcopy), the gfx950 code object is
unbundled from it (clang-offload-bundler) and compared byte for byte.  Where whole code objects differ, every kernel is compared by the
bytes of its code (the symbol's range of .text), by its descriptor and by the registers, LDS and scratch its metadata note states.
Prints one line per translation unit and a total; exit status 1 when a kernel differs or the sets of kernels of a translation unit both
builds hold are not equal.  A translation unit only one build holds is listed with its number of kernels and not compared.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """The gfx950 code object inside a host object file, or None (a translation unit without kernels)."""
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "gfx950.co")
    for f in (fat, co):
        if os.path.exists(f):
            os.remove(f)
    try:
        run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(tmp, "copy.o"))
    except subprocess.CalledProcessError:       # (no such section: a host-only file)
        return None
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co)
    return open(co, "rb").read() if os.path.exists(co) and os.path.getsize(co) else None


def kernels(blob, tmp):
    """{kernel: (code bytes, descriptor bytes, metadata fields)} of a code object."""
    path = os.path.join(tmp, "k.co")
    open(path, "wb").write(blob)
    readelf = os.path.join(LLVM, "llvm-readelf")
    sections = {}   # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+(\S*)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", run(readelf, "-S", "-W", path), flags=re.M):
        sections[int(m.group(1))] = (int(m.group(3), 16), int(m.group(4), 16))
    syms = {}
    for line in run(readelf, "-s", "-W", path).splitlines():
        p = line.split()
        if len(p) == 8 and p[3] in ("FUNC", "OBJECT") and p[6].isdigit():
            addr, off = sections[int(p[6])]
            start = int(p[1], 16) - addr + off
            syms[p[7]] = blob[start:start + int(p[2])]
    # the metadata note: one "  - .key: value" entry per kernel under amdhsa.kernels, its own keys at four spaces
    out, cur = {}, None
    for line in run(readelf, "--notes", "-W", path).splitlines() + ["  - .end: 0"]:
        m = re.match(r"^  (- | {2})(\.\w+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) == "- ":
            if cur and ".symbol" in cur:
                kd = cur.pop(".symbol").strip("'\"")
                out[kd[:-3]] = (syms.get(kd[:-3]), syms.get(kd), cur)
            cur = {}
        if cur is not None and (m.group(2) in FIELDS or m.group(2) == ".symbol"):
            cur[m.group(2)] = m.group(3).strip()
    return out


def main(a_dir, b_dir):
    in_a, in_b = (set(f for f in os.listdir(d) if f.endswith(".o")) for d in (a_dir, b_dir))
    names = sorted(in_a & in_b)
    total = same_units = differing = 0
    with tempfile.TemporaryDirectory() as tmp:
        # a translation unit only one build has (a new kernel family, a removed one) is listed, not compared: it cannot change an existing kernel
        for n in sorted(in_a ^ in_b):
            blob = code_object(os.path.join(a_dir if n in in_a else b_dir, n), tmp)
            print(f"{n}: only in the {'first' if n in in_a else 'second'} build ({len(kernels(blob, tmp)) if blob else 0} kernels)")
        for n in names:
            a, b = code_object(os.path.join(a_dir, n), tmp), code_object(os.path.join(b_dir, n), tmp)
            if a is None and b is None:
                print(f"{n}: no device code")
                continue
            ka, kb = (kernels(a, tmp) if a else {}), (kernels(b, tmp) if b else {})     # (device code on one side only: every kernel of it differs)
            total += len(set(ka) | set(kb))
            if a == b:
                same_units += 1
                print(f"{n}: code object identical ({len(a)} bytes, {len(ka)} kernels)")
                continue
            bad = sorted(set(ka) ^ set(kb)) + [k for k in sorted(set(ka) & set(kb)) if ka[k] != kb[k] or ka[k][0] is None]
            differing += len(bad)
            print(f"{n}: code objects differ ({len(a or b'')} / {len(b or b'')} bytes); {len(ka)} / {len(kb)} kernels, {len(bad)} differ in code, descriptor or metadata"
                  + "".join("\n    " + k for k in bad[:20]))
    print(f"total: {total} kernels, {same_units} translation units with identical code objects, {differing} kernels differ")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
