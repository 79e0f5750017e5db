"""The 3D LUT extension on the CPU (include/mpcvr.h: mpcvr_plan_lut3d_entries, mpcvr_plan_lut3d_value, mpcvr_plan_batch_lut3d, api.read_cube,
and every refusal of mpcvr_lut3d_pass that is answered before a launch), against the model (tests/lut3d_model.py).  Everything is bits: no
tolerance anywhere.  The kernel itself: tests/test_lut3d_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests import lut3d_model as LM

BGRA8, RGB10A2 = LM.BGRA8, LM.RGB10A2
PAIRS = [(s, d) for s in (BGRA8, RGB10A2) for d in (BGRA8, RGB10A2)]
PAIR_IDS = ["%s-to-%s" % ("rgb10" if s else "bgra8", "rgb10" if d else "bgra8") for s, d in PAIRS]
SIZES = (2, 3, 4, 9, 17, 27, 28, 33, 64, 65)


def random_table(n, seed):
    """n^3 entries of random 16-bit words, the pad word included; every 16-bit value occurs wherever the table has room for it (n >= 28:
    4 n^3 >= 65536 words), and 0 and 65535 always"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 65536, size=(n ** 3, 4), dtype=np.uint16)
    flat = t.reshape(-1)
    if flat.size >= 65536:
        flat[rng.permutation(flat.size)[:65536]] = np.arange(65536, dtype=np.uint16)
        assert np.unique(flat).size == 65536
    else:
        flat[:2] = (0, 65535)
    return t


def texels_with_every_code(fmt, seed, extra=3000):
    """32-bit texels, all bits random, in which every code of every channel occurs (a permutation per channel), plus `extra` random ones"""
    rng = np.random.default_rng(seed)
    m = LM.MAXCODE[fmt] + 1
    s = rng.integers(0, 2 ** 32, size=m + extra, dtype=np.uint64).astype(np.uint32)
    r, g, b = (rng.permutation(m).astype(np.uint32) for _ in range(3))
    keep = np.uint32(0xc0000000 if fmt == RGB10A2 else 0xff000000)
    s[:m] = (s[:m] & keep) | ((r | g << 10 | b << 20) if fmt == RGB10A2 else (b | g << 8 | r << 16))
    return s


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("src_fmt,dst_fmt", PAIRS, ids=PAIR_IDS)
def test_plan_lut3d_value_equals_the_model(mpcvr, src_fmt, dst_fmt, n):
    from videorenderer_amd import api
    table = random_table(n, 100 + n)
    tex = texels_with_every_code(src_fmt, 7 * n + src_fmt, extra=1200)
    got = api.plan_lut3d_value(src_fmt, dst_fmt, table, n, tex)
    want = LM.apply(tex, table, n, src_fmt, dst_fmt)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} texels differ, first {tex[bad[0]]:#x}: got {got[bad[0]]:#x}, model {want[bad[0]]:#x}"
    # the pad word and the A / X bits cannot show
    other = table.copy()
    other[:, 3] ^= 0xffff
    keep = np.uint32(0x3fffffff if src_fmt == RGB10A2 else 0x00ffffff)
    assert np.array_equal(api.plan_lut3d_value(src_fmt, dst_fmt, other, n, tex[:300] & keep), got[:300])


@pytest.mark.parametrize("src_fmt,dst_fmt", PAIRS, ids=PAIR_IDS)
def test_the_identity_table_returns_the_code_for_every_code_and_size(mpcvr, src_fmt, dst_fmt):
    """out == c where the depths agree, (2 c maxout + maxin) / (2 maxin) across depths: the model over every code of every channel beside
    random codes in the other two, for every n; the host function on the gray ramp for every n"""
    from videorenderer_amd import api
    maxin, maxout = LM.MAXCODE[src_fmt], LM.MAXCODE[dst_fmt]
    tex = texels_with_every_code(src_fmt, 900 + src_fmt, extra=0)
    c = np.arange(maxin + 1, dtype=np.uint32)
    gray = LM.pack(c.astype(np.int64), c.astype(np.int64), c.astype(np.int64), src_fmt)
    want_of = lambda x: (2 * x * maxout + maxin) // (2 * maxin)
    for n in range(2, 66):
        table = LM.identity_entries(n, pad=0xbeef)
        got = LM.codes(LM.apply(tex, table, n, src_fmt, dst_fmt), dst_fmt)
        for k, cin in enumerate(LM.codes(tex, src_fmt)):
            assert np.array_equal(got[k], want_of(cin)), (n, k)
            if maxin == maxout:
                assert np.array_equal(got[k], cin), (n, k)
        host = api.plan_lut3d_value(src_fmt, dst_fmt, table, n, gray)
        w = want_of(c.astype(np.int64))
        assert np.array_equal(host, LM.pack(w, w, w, dst_fmt)), n


@pytest.mark.parametrize("n", (2, 3, 17, 33, 65))
@pytest.mark.parametrize("src_fmt", (BGRA8, RGB10A2), ids=["bgra8", "rgb10"])
def test_tied_fractions_give_one_answer_under_every_admissible_order(mpcvr, src_fmt, n):
    """texels with two or three equal fractions, a random table: every vertex order the definition admits gives the same texel, and it is
    the host function's"""
    from videorenderer_amd import api
    maxin = LM.MAXCODE[src_fmt]
    rng = np.random.default_rng(40 + n)
    table = random_table(n, 300 + n)
    c = rng.integers(0, maxin + 1, size=(3, 600)).astype(np.int64)
    for a, b in ((0, 1), (0, 2), (1, 2)):                  # pairs of equal codes have equal fractions; so have all three
        sel = slice(100 * (a + b), 100 * (a + b) + 100)
        c[b, sel] = c[a, sel]
    c[:, 400:500] = c[0, 400:500]
    tex = LM.pack(c[0], c[1], c[2], src_fmt)
    f = np.stack([LM.split(x, n, maxin)[1] for x in c])
    tied = (f[0] == f[1]) | (f[0] == f[2]) | (f[1] == f[2])
    assert tied.sum() >= 400
    for dst_fmt in (BGRA8, RGB10A2):
        ref = LM.apply(tex, table, n, src_fmt, dst_fmt)
        seen = np.zeros(tex.size, dtype=np.int64)
        for perm in LM.PERMS:
            ok = (f[perm[0]] >= f[perm[1]]) & (f[perm[1]] >= f[perm[2]])
            assert np.array_equal(LM.apply(tex[ok], table, n, src_fmt, dst_fmt, perm=perm), ref[ok]), perm
            seen += ok
        all3 = (f[0] == f[1]) & (f[1] == f[2])
        assert (seen[tied] >= 2).all() and all3.sum() >= 100 and (seen[all3] == 6).all()
        assert np.array_equal(api.plan_lut3d_value(src_fmt, dst_fmt, table, n, tex), ref)


@pytest.mark.parametrize("n", (2, 5, 17, 52, 65))
@pytest.mark.parametrize("src_fmt,dst_fmt", PAIRS, ids=PAIR_IDS)
def test_texels_on_nodes_return_the_nodes_entry(mpcvr, src_fmt, dst_fmt, n):
    """a code c with c (n - 1) a multiple of maxin sits on a node: the output is that entry converted to maxout, (E maxout + 32767) / 65535"""
    from videorenderer_amd import api
    maxin, maxout = LM.MAXCODE[src_fmt], LM.MAXCODE[dst_fmt]
    on = np.array([c for c in range(maxin + 1) if (c * (n - 1)) % maxin == 0], dtype=np.int64)
    assert on[0] == 0 and on[-1] == maxin
    node = on * (n - 1) // maxin
    r, g, b = (x.ravel() for x in np.meshgrid(np.arange(on.size), np.arange(on.size), np.arange(on.size), indexing="ij"))
    table = random_table(n, 500 + n)
    tex = LM.pack(on[r], on[g], on[b], src_fmt)
    e = table[(node[b] * n + node[g]) * n + node[r]].astype(np.int64)
    want = LM.pack(*[(e[:, k] * maxout + 32767) // 65535 for k in range(3)], dst_fmt)
    assert np.array_equal(LM.apply(tex, table, n, src_fmt, dst_fmt), want)
    assert np.array_equal(api.plan_lut3d_value(src_fmt, dst_fmt, table, n, tex), want)


def test_the_accumulator_bound_is_reached_and_never_passed(mpcvr):
    """an all-65535 table: acc = maxin * 65535 for every texel, 67,042,305 for 10-bit sources — the header's figure, inside 32 bits — and
    the output is maxout"""
    from videorenderer_amd import api
    assert LM.ACC_BOUND == 67042305 < 2 ** 32
    for n in (2, 33, 65):
        table = np.full((n ** 3, 4), 65535, dtype=np.uint16)
        for src_fmt, dst_fmt in PAIRS:
            tex = texels_with_every_code(src_fmt, 5, extra=200)
            m = LM.MAXCODE[dst_fmt]
            want = LM.pack(*[np.full(tex.size, m, dtype=np.int64)] * 3, dst_fmt)
            assert np.array_equal(LM.apply(tex, table, n, src_fmt, dst_fmt), want)      # (apply asserts acc <= ACC_BOUND)
            assert np.array_equal(api.plan_lut3d_value(src_fmt, dst_fmt, table, n, tex), want)
    # v * maxout stays inside 32 bits too: v <= 65535
    assert 65535 * 1023 + 32767 < 2 ** 32


def test_plan_lut3d_entries(mpcvr):
    from videorenderer_amd import api
    n = 3
    rng = np.random.default_rng(3)
    rgb = rng.random((n ** 3, 3)).astype(np.float32)
    special = [np.nan, -np.nan, -1.0, -0.0, 0.0, -1e-30, 1e-30, 1.0, np.nextafter(np.float32(1), np.float32(2)), 2.0, 1e30, np.inf, -np.inf,
               0.5, 1.0 / 65535, 0.5 / 65535, 1.5 / 65535, 2.5 / 65535, 65534.5 / 65535, np.float32(0.5 / 65535), np.nextafter(np.float32(0.5 / 65535), np.float32(1))]
    rgb.reshape(-1)[:len(special)] = np.array(special, dtype=np.float32)
    got = api.plan_lut3d_entries(rgb, n)
    want = LM.entries_from_float(rgb)
    assert got.shape == (27, 4) and got.dtype == np.uint16 and np.array_equal(got, want)
    assert (got[:, 3] == 0).all()
    flat = got[:, :3].reshape(-1)
    assert list(flat[:13]) == [0, 0, 0, 0, 0, 0, 0, 65535, 65535, 65535, 65535, 65535, 0] and flat[13] == 32768      # rint(32767.5) = 32768 (even)
    # the float nearest k + 1/2 sixty-five-thousandths is not a tie in double: it rounds by its own value
    x = np.float32(2.5 / 65535)
    assert flat[17] == int(np.rint(float(x) * 65535.0))
    # every representable entry comes back from its own quotient
    e = np.arange(65536, dtype=np.float64) / 65535.0
    m = 41                                                 # 41^3 = 68921 >= 65536 / 3 triplets
    pad = np.zeros(3 * m ** 3)
    pad[:65536] = e
    back = api.plan_lut3d_entries(pad.astype(np.float32).reshape(-1, 3), m)[:, :3].reshape(-1)[:65536]
    assert np.array_equal(back, np.arange(65536, dtype=np.uint16))
    L = api.load_library()
    buf = np.zeros(8, dtype=np.float32)
    out = np.zeros(8, dtype=np.uint16)
    assert L.mpcvr_plan_lut3d_entries(None, 2, C.c_void_p(out.ctypes.data)) == api.E_POINTER
    assert L.mpcvr_plan_lut3d_entries(C.c_void_p(buf.ctypes.data), 2, None) == api.E_POINTER
    for bad in (1, 0, -1, 66):
        assert L.mpcvr_plan_lut3d_entries(C.c_void_p(buf.ctypes.data), bad, C.c_void_p(out.ctypes.data)) == api.E_INVALIDARG
    with pytest.raises(ValueError):
        api.plan_lut3d_entries(rgb[:5], 3)


def test_plan_lut3d_value_refusals(mpcvr):
    from videorenderer_amd import api
    L = api.load_library()
    t = LM.identity_entries(2)
    p, out = C.c_void_p(t.ctypes.data), C.c_uint32(0x12345678)
    assert L.mpcvr_plan_lut3d_value(0, 0, None, 2, 0, C.byref(out)) == api.E_POINTER
    assert L.mpcvr_plan_lut3d_value(0, 0, p, 2, 0, None) == api.E_POINTER
    for args in ((2, 0, 2), (0, 2, 2), (-1, 0, 2), (0, 0, 1), (0, 0, 66), (1, 1, 0)):
        assert L.mpcvr_plan_lut3d_value(args[0], args[1], p, args[2], 0, C.byref(out)) == api.E_INVALIDARG
    assert out.value == 0x12345678


def plan_chunks(frame_bytes, n, budget):
    """PlanChunks of csrc/vp_plan.h, by hand"""
    stride = (frame_bytes + 255) // 256 * 256
    fit = (budget or (4 << 30)) // stride
    fpc = max(1, min(n, fit))
    return stride, fpc, (n + fpc - 1) // fpc


@pytest.mark.parametrize("w,h,n,budget", [(1, 1, 1, 0), (5, 3, 7, 0), (64, 32, 7, 3 * 8192), (64, 32, 7, 1), (1921, 1081, 32, 64 << 20),
                                          (7680, 4320, 40, 0), (32768, 32768, 3, 0), (3, 1, 5, 2 * 256)])
def test_plan_batch_lut3d_is_plan_chunks_arithmetic(mpcvr, w, h, n, budget):
    from videorenderer_amd import api
    got = api.plan_batch_lut3d(w, h, n, budget)
    pitch = (4 * w + 15) // 16 * 16
    stride, fpc, chunks = plan_chunks(pitch * h, n, budget)
    assert got == dict(surface_pitch=pitch, frame_stride=stride, frames_per_chunk=fpc, chunks=chunks)
    assert got == api.plan_batch_tensor(w, h, n, budget)


def test_plan_batch_lut3d_refusals(mpcvr):
    from videorenderer_amd import api
    L = api.load_library()
    for w, h, n in ((0, 4, 1), (4, 0, 1), (32769, 4, 1), (4, 32769, 1), (4, 4, 0), (4, 4, -3)):
        assert L.mpcvr_plan_batch_lut3d(w, h, n, 0, None, None, None, None) == api.E_INVALIDARG
    assert L.mpcvr_plan_batch_lut3d(5, 3, 2, 0, None, None, None, None) == 0      # any out pointer may be NULL


# ---- read_cube ----------------------------------------------------------------------------------------------------------------------------
def write_cube(path, n, rows, head=""):
    with open(path, "w") as f:
        f.write(head)
        f.write("LUT_3D_SIZE %d\n" % n)
        for r in rows:
            f.write("%.9g %.9g %.9g\n" % tuple(r))


def test_read_cube(mpcvr, tmp_path):
    from videorenderer_amd import api
    rng = np.random.default_rng(9)
    n = 3
    rows = rng.random((27, 3)).astype(np.float32)
    p = tmp_path / "a.cube"
    write_cube(p, n, rows, head='# a comment\nTITLE "a look # not a comment either way"\n\n')
    got_n, got = api.read_cube(str(p))
    assert got_n == 3 and got.dtype == np.float32 and got.shape == (27, 3) and np.array_equal(got, rows)
    # comments behind values, blank lines, keywords in any order, a domain
    q = tmp_path / "b.cube"
    with open(q, "w") as f:
        f.write("TITLE \"x\"\nDOMAIN_MAX 2 4 1023\n# between\nLUT_3D_SIZE 2\nDOMAIN_MIN 0 -4 0\n\n")
        for i in range(8):
            f.write("%d %d %d   # row %d\n" % (i % 3, i - 4, 128 * i, i))
    got_n, got = api.read_cube(str(q))
    want = np.array([[(i % 3) / 2, (i - 4 + 4) / 8, 128 * i / 1023] for i in range(8)], dtype=np.float64).astype(np.float32)
    assert got_n == 2 and np.array_equal(got, want)
    # the order of the file is the order of the table: R fastest
    ident = [[r, g, b] for b in (0, 1) for g in (0, 1) for r in (0, 1)]
    write_cube(p, 2, ident)
    e = api.plan_lut3d_entries(api.read_cube(str(p))[1], 2)
    assert np.array_equal(e, LM.identity_entries(2))
    assert api.plan_lut3d_value(BGRA8, BGRA8, e, 2, 0x00123456) == 0xff123456


@pytest.mark.parametrize("text,what", [
    ("LUT_1D_SIZE 2\n0 0 0\n1 1 1\n", "1D"),
    ("LUT_3D_SIZE 2\n" + "0 0 0\n" * 7, "entries"),
    ("LUT_3D_SIZE 2\n" + "0 0 0\n" * 9, "entries"),
    ("0 0 0\n" * 8, "LUT_3D_SIZE"),
    ("LUT_3D_SIZE 2\n" + "0 0 0\n" * 7 + "0 0\n", "three"),
    ("LUT_3D_SIZE 1\n0 0 0\n", "outside"),
    ("LUT_3D_SIZE 66\n", "outside"),
    ("LUT_3D_SIZE 2\nLUT_3D_INPUT_RANGE 0 1\n" + "0 0 0\n" * 8, "keyword"),
    ("LUT_3D_SIZE 2\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 1 0 1\n" + "0 0 0\n" * 8, "DOMAIN"),
])
def test_read_cube_raises(mpcvr, tmp_path, text, what):
    from videorenderer_amd import api
    p = tmp_path / "bad.cube"
    p.write_text(text)
    with pytest.raises(ValueError, match=what):
        api.read_cube(str(p))


# ---- the refusals of the pass that need no GPU (nothing is launched: the addresses are never touched) -----------------------------------
A = 0x7f0000000000                                             # an address nobody dereferences


def lut3d_pass_hr(src=A, src_pitch=256, src_fmt=0, w=64, h=4, lut=A + (1 << 30), n=17, dst=A + (1 << 20), dst_pitch=256, dst_fmt=0):
    from videorenderer_amd import api
    return api.load_library().mpcvr_lut3d_pass(C.c_void_p(src), src_pitch, src_fmt, w, h, C.c_void_p(lut), n, C.c_void_p(dst), dst_pitch, dst_fmt, None)


REFUSALS = {
    "null_src": (dict(src=0), "E_POINTER"),
    "null_lut": (dict(lut=0), "E_POINTER"),
    "null_dst": (dict(dst=0), "E_POINTER"),
    "src_fmt": (dict(src_fmt=2), "E_INVALIDARG"),
    "dst_fmt": (dict(dst_fmt=-1), "E_INVALIDARG"),
    "w_0": (dict(w=0), "E_INVALIDARG"),
    "w_big": (dict(w=32769, src_pitch=4 * 32769 + 4, dst_pitch=4 * 32769 + 4), "E_INVALIDARG"),
    "h_0": (dict(h=0), "E_INVALIDARG"),
    "h_big": (dict(h=32769), "E_INVALIDARG"),
    "n_1": (dict(n=1), "E_INVALIDARG"),
    "n_66": (dict(n=66), "E_INVALIDARG"),
    "src_pitch_short": (dict(src_pitch=252), "E_INVALIDARG"),
    "dst_pitch_short": (dict(dst_pitch=252), "E_INVALIDARG"),
    "src_odd": (dict(src=A + 2), "E_INVALIDARG"),
    "dst_odd": (dict(dst=A + (1 << 20) + 1), "E_INVALIDARG"),
    "src_pitch_odd": (dict(src_pitch=258), "E_INVALIDARG"),
    "dst_pitch_odd": (dict(dst_pitch=257), "E_INVALIDARG"),
    "lut_on_4": (dict(lut=A + (1 << 30) + 4), "E_INVALIDARG"),
    "dst_one_texel_into_src": (dict(dst=A + 4), "E_INVALIDARG"),
    "dst_one_row_into_src": (dict(dst=A + 256), "E_INVALIDARG"),
    "in_place_with_another_pitch": (dict(dst=A, dst_pitch=512), "E_INVALIDARG"),
    "dst_ends_inside_src": (dict(dst=A - 3 * 256 - 4), "E_INVALIDARG"),
    "lut_inside_dst": (dict(lut=A + (1 << 20) + 256), "E_INVALIDARG"),
    "lut_ends_inside_dst": (dict(lut=A + (1 << 20) - 8), "E_INVALIDARG"),
    "dst_ends_inside_lut": (dict(dst=A + (1 << 30) + 17 ** 3 * 8 - 8 - 3 * 256 - 248), "E_INVALIDARG"),
}


@pytest.mark.parametrize("label", list(REFUSALS))
def test_lut3d_pass_refuses_before_any_launch(mpcvr, label):
    from videorenderer_amd import api
    kw, want = REFUSALS[label]
    assert lut3d_pass_hr(**kw) == getattr(api, want), label
