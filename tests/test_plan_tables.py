"""The tables of a plan as the processor builds and uploads them (videorenderer_amd/csrc/vp_plan_tables.cpp), read back through
mpcvr_plan_draw_tables — no GPU involved.  Every draw, reversed or not, is held to the structure the kernels rely on (alignment of the
sub-tables, block tables, tap-major transposes, the identity flag of the unfiltered axis' map); an unreversed draw also to
mpcvr_plan_axis_taps, and an unrotated, unflipped plan's strip / periodic tables to mpcvr_plan_strip / mpcvr_plan_period.  No test
claims that a flipped table is the mirrored one: TexCenter rounds differently from the far edge."""
import numpy as np
import pytest

SRC_W, SRC_H = 96, 72
RECTS = {"origin": None, "inner": (8, 4, 88, 68)}
TARGETS = [(144, 108), (128, 96), (64, 48), (96, 100), (192, 144)]


def _settings(api):
    # Lanczos3 up (periodic 3:2 / 4:3 rows at these sizes), Hamming down; no upscale shader for small downscales, so 64x48 normalises
    return api.default_settings(iUpscaling=api.UPSCALE_Lanczos3, bInterpolateAt50pct=0)


def _tables(api, cformat, rect, target, rotation, flip):
    return api.plan_draw_tables(_settings(api), cformat, SRC_W, SRC_H, rect, (0, 0) + target, target[0], target[1], rotation, flip)


def _axis_tables(p):
    """The sub-tables of one axis pack, cut out of its words by the header's offsets."""
    wds, off, n, nt = p["words"], p["off"], p["n_out"], p["ntaps"]
    t = dict(idx=wds[off["idx"]:off["idx"] + n * nt].reshape(n, nt), w=wds[off["w"]:off["w"] + n * nt].reshape(n, nt),
             other=wds[off["other"]:off["other"] + p["n_other"]])
    if off["wsum"] is not None:
        t["wsum"] = wds[off["wsum"]:off["wsum"] + n]
    b = off["blk"]
    n64, n8, n32 = (n + 63) // 64, (n + 7) // 8, (n + 31) // 32
    t["blk_lo"] = wds[b:b + n64]
    b += (n64 + 63) // 64 * 64
    t["idx_t"] = wds[b:b + n * nt].reshape(nt, n)
    t["w_t"] = wds[b + n * nt:b + 2 * n * nt].reshape(nt, n)
    b += 2 * n * nt
    t["blk8_lo"] = wds[b:b + n8]
    t["blk32_lo"] = wds[b + n8:b + n8 + n32]
    assert b + n8 + n32 == len(wds)            # the block pack ends the pack
    return t


def _check_structure(p):
    t = _axis_tables(p)
    for name, o in p["off"].items():
        assert o is None or o % 64 == 0, (name, o)
    assert (p["off"]["wsum"] is not None) == bool(p["normalise"])
    idx = t["idx"]
    for block, lo_name, span_name in ((64, "blk_lo", "blk_span"), (8, "blk8_lo", "blk8_span"), (32, "blk32_lo", "blk32_span")):
        chunks = [idx[b:b + block] for b in range(0, p["n_out"], block)]
        assert np.array_equal(t[lo_name], [c.min() for c in chunks]), lo_name
        assert p[span_name] == max(int(c.max()) - int(c.min()) + 1 for c in chunks), span_name
    assert np.array_equal(t["idx_t"], idx.T)
    assert np.array_equal(t["w_t"], t["w"].T)          # (weights compared as the int32 words they travel as)
    assert bool(p["other_identity"]) == np.array_equal(t["other"], np.arange(p["n_other"]))
    return t


def _resizer(api, src_len, n_out):
    s = _settings(api)
    return (1, s.iUpscaling) if n_out > src_len else (2, s.iDownscaling)


def _check_against_axis_taps(api, p, t, src_l, src_len, n_out, tex_len):
    kind, method = _resizer(api, src_len, n_out)
    idx, w, wsum = api.plan_axis_taps(kind, method, src_l, src_len, n_out, tex_len)
    assert p["n_out"] == n_out and p["ntaps"] == len(idx[0])
    assert np.array_equal(t["idx"], np.array(idx, np.int32))
    assert np.array_equal(t["w"], np.array(w, np.float32).view(np.int32))
    assert (wsum is not None) == bool(p["normalise"])
    if wsum is not None:
        assert np.array_equal(t["wsum"], np.array(wsum, np.float32).view(np.int32))


@pytest.mark.parametrize("target", TARGETS, ids=lambda t: "%dx%d" % t)
@pytest.mark.parametrize("rect", sorted(RECTS))
@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("rotation", [0, 180])
@pytest.mark.parametrize("fmt", ["P010", "XRGB32"])
def test_draw_tables(mpcvr, fmt, rotation, flip, rect, target):
    from videorenderer_amd import api
    cformat = getattr(api, "CF_" + fmt)
    r = RECTS[rect] or (0, 0, SRC_W, SRC_H)
    w1, h1, (w2, h2) = r[2] - r[0], r[3] - r[1], target
    d = _tables(api, cformat, RECTS[rect], target, rotation, flip)
    assert not d["first_swap"] and not d["first_jinc"] and not d["second_jinc"]
    two_pass = w1 != w2 and h1 != h2
    assert d["x"] is not None and (d["y"] is not None) == two_pass
    tx = _check_structure(d["x"])
    ty = _check_structure(d["y"]) if two_pass else None

    # the draw reads the convert output (the rect at its origin) or, for interleaved RGB, the source texture in place
    in_place = fmt == "XRGB32"
    ol, ot, tw, th = (r[0], r[1], SRC_W, SRC_H) if in_place else (0, 0, w1, h1)
    rev_u, rev_v = (rotation == 180) != flip, rotation == 180
    if d["first_axis"] == 0:
        assert w1 != w2
        if not rev_u:
            _check_against_axis_taps(api, d["x"], tx, ol, w1, w2, tw)
    else:                       # one draw that filters the rows
        assert w1 == w2 and not two_pass
        if not rev_v:
            _check_against_axis_taps(api, d["x"], tx, ot, h1, h2, th)
    if two_pass:                # the second draw is never reversed: m_TexResize (h1 rows) onto the target's rows, columns 1:1
        _check_against_axis_taps(api, d["y"], ty, 0, h1, h2, h1)
        assert d["y"]["other_identity"] and d["y"]["n_other"] == w2

    # strip / periodic tables: the context-free entry points describe an unreversed draw from a surface with the rect at its origin
    if rotation == 0 and not flip and two_pass and (not in_place or rect == "origin"):
        (kx, mx), (ky, my) = _resizer(api, w1, w2), _resizer(api, h1, h2)
        sp = api.plan_strip(kx, mx, ky, my, w1, h1, w2, h2)
        assert (sp is not None) == bool(d["strip_planned"])
        if sp is not None:
            s = d["strip"]
            assert (s["taps"], s["px_per_lane"], s["strip_w"], s["ring"], s["acols"]) == (sp["taps"], sp["px_per_lane"], sp["strip_w"], sp["ring"], sp["acols"])
            for o, name in zip(s["off"], ("yrange", "xstrip", "xi_t", "xw_t", "yi", "yw")):
                want = sp[name].reshape(-1).view(np.int32)
                assert np.array_equal(s["words"][o:o + want.size], want), name
        pp = api.plan_period(mx, w1, h1, w2, h2) if kx == ky == 1 else None
        assert (pp["P"], pp["Q"]) == (d["P"], d["Q"]) if pp is not None else d["P"] == 0
        if pp is not None:
            s = d["strip"]
            # (the strip width follows the weight of the convert stage, which mpcvr_plan_period takes as heavy; frames this narrow are one
            # strip of the full width either way)
            assert (s["period_taps"], s["period_acols"], s["period_strip_w"]) == (pp["taps"], pp["acols"], pp["strip_w"])
            assert s["period_off"][2] % 8 == 0          # the weight rows are read 32 bytes at a time
            for o, name in zip(s["period_off"], ("xi_t", "xw_t", "yw", "xstrip")):
                want = pp[name].reshape(-1).view(np.int32)
                assert np.array_equal(s["words"][o:o + want.size], want), name


def test_periodic_ratios_are_planned(mpcvr):
    """The geometries the GPU walk counts on: 3:2 and 4:3 rows are periodic, exact 2x and a downscale are strip plans without one."""
    from videorenderer_amd import api
    got = {t: _tables(api, api.CF_P010, None, t, 0, False) for t in TARGETS}
    assert [(got[t]["strip_planned"], got[t]["P"], got[t]["Q"]) for t in TARGETS] == [(1, 3, 2), (1, 4, 3), (1, 0, 0), (0, 0, 0), (1, 0, 0)]
    assert got[(64, 48)]["x"]["normalise"] and got[(64, 48)]["y"]["normalise"]
    assert got[(96, 100)]["first_axis"] == 1 and got[(96, 100)]["y"] is None and got[(96, 100)]["strip"] is None


def test_a_plan_without_tap_tables_has_empty_packs(mpcvr):
    """Jinc2m draws read no tap tables: both packs are empty, whatever a previous plan built."""
    from videorenderer_amd import api
    s = api.default_settings(iUpscaling=api.UPSCALE_Jinc2)
    d = api.plan_draw_tables(s, api.CF_P010, SRC_W, SRC_H, None, (0, 0, 144, 108), 144, 108)
    assert d["first_jinc"] and d["x"] is None and d["y"] is None and d["strip"] is None and not d["strip_planned"]
