"""The arguments of the tone curves on the GPU (tests/tone_params.py holds the table and the frame, tests/test_tone_params.py the CPU half:
what every row enters, and the oracle bit-identical to the reference's shader text on every case drawn here).

Every frame is the designed 256 x 32 P010 frame (or noise of that size), at most 512 x 64 out.  Every test asserts the route it meant to take.

HDR10 tone-mapping step (k_hdr10_tonemap), every row of HDR10_ROWS x six operators:
  * plain tier (MPCVR_FLAG_NO_FUSED), same size (the step reads the convert output) and 384 x 48 (the post-scale surface): BIT-EXACT with the
    oracle, the 8-bit internal format on two rows too;
  * default tier, 384 x 48 (k_fused_period writes the post-scale surface) and 320 x 40 (k_fused_strip): within two ten-bit codes, a channel
    beyond that only inside the oracle's own interval for the operator's input and the convert output one code off
    (compare_behind_tail(ten_bit=True, lim=2, operator_input=True, convert_output=True)); how MANY such channels a (row, operator) may have
    is HDR_CAPS, 1.5 x the largest count measured for the operator (profiles/r20/tone_params.txt), zero where none was seen;
  * batches of five frames equal five single frames; metadata and display peak changed between two frames of one context (own stream with
    its frame lanes, and a caller's stream) leave each target as a fresh context draws it; the two Dolby Vision rows on both tiers.
SDR tails (PQ -> SDR, HLG -> SDR) over SDR_NITS, every convert route: plain tier bit-exact; the default tier's routes (direct:convert,
fused_up2x with 5 and 4 taps, k_fused_period, k_fused_strip, the fused Jinc2m kernel), MPCVR_FLAG_NO_LUT (the same kernels on the literal chain
instead of the 4096-entry table) and MPCVR_FLAG_NO_FAST_CONVERT (the folded kernels) within one 8-bit code / two ten-bit codes, outliers only
inside the oracle's +-4-ulp pow() interval and capped by SDR_CAPS the same way; Configure from 125 nits to each end of the range and back.
Correction passes 3, 4, 5 over SDR_NITS against the oracle, with the bars of test_correction_passes_vs_oracle.

MPCVR_TONE_PARAMS_LOG=<file>: one line per comparison (what, route, identical share, channels beyond the limit) — profiles/r20/tone_params.txt.
"""
import os

import numpy as np
import pytest

from tests import tone_params as T
from tests.golden.cases import case_frame, oracle_params
from tests.test_parity_gpu import BG, _codes10, compare, compare_behind_tail, compare_rgb10, make_vp, path_ok

pytestmark = pytest.mark.gpu

FRAME = np.array(T.frame()[0])           # (a writable copy: torch.from_numpy wants one)
PITCH = T.PITCH
FUSED_NAMES = ("fused_up2x", "fused_jinc2x", "kernel=fused_strip", "kernel=fused_period")
NO_CAP = 1 << 30            # compare_behind_tail still holds every outlier to its witness; the count is asserted here, after all rows were measured

# Channels beyond the limit (each inside the oracle's own interval), per operator: 1.5 x the largest count of any (row, geometry) measured on an
# MI355X when the file was written — profiles/r20/tone_params.txt holds the counts per (row, operator, geometry).  Zero: none was seen, on any of
# the thirteen rows at either geometry (worst difference 2 ten-bit codes).
HDR_CAPS = {1: 0, 2: 0, 3: 0, 4: 0, 5: 0, 6: 0}
# The Dolby Vision rows at 384 x 48: none on any operator, except row dovi_l2 (level-2 trims inside the step) through operator 5: 6 channels, up to 4 codes
# off, each inside the oracle's own interval -> 1.5 x 6 = 9
DOVI_CAPS = {1: 0, 2: 0, 3: 0, 4: 0, 5: 9, 6: 0}
# ... and per route of the SDR tails (the largest count over SDR_NITS x {PQ, HLG} x both render-target formats): none was seen on any route at any
# nits value — the worst difference is one code, 8-bit and ten-bit alike, the table against the literal chain within two ten-bit codes
SDR_CAPS = {"direct": 0, "up2x_lanczos3": 0, "up2x_catmull": 0, "period": 0, "strip": 0, "jinc2x": 0, "direct_no_lut": 0, "up2x_no_lut": 0, "folded_same": 0,
            "folded_2x": 0}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def log(line):
    print("TONE " + line)
    if os.environ.get("MPCVR_TONE_PARAMS_LOG"):
        with open(os.environ["MPCVR_TONE_PARAMS_LOG"], "a") as f:
            f.write(line + "\n")


_WANT = {}


def want_of(oracle, c):
    """(oracle params, the oracle's frame of a case over the designed frame): computed once, read-only"""
    key = repr(sorted((k, repr(v)) for k, v in c.items() if k != "name"))
    if key not in _WANT:
        p = oracle_params(oracle, c)
        w = oracle.process(p, FRAME, PITCH, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
        w.setflags(write=False)
        _WANT[key] = (p, w)
    return _WANT[key]


def draw(mpcvr, torch, c, extra_flags=0, frame=FRAME):
    """run_product of tests/test_parity_gpu.py over a frame given by the caller (the designed frame is no synth kind) -> (pixels, GetVPInfo)"""
    vp, (ww, wh) = make_vp(mpcvr, c, extra_flags)
    assert vp.GetFrameBytes() == (frame.size, PITCH)
    dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
    vp.CopySample(torch.from_numpy(frame).cuda(), PITCH)
    vp.Process(dst, ww * 4)
    vp.Synchronize()
    info = vp.GetVPInfo()
    out = dst.cpu().numpy()
    vp.close()
    return out, info


def exact(got, want, c, what):
    if c.get("output_format", 0) == 1:
        compare_rgb10(got, want, what, exact=True)
    else:
        compare(got, want, what, exact=True)


# ---- the HDR10 tone-mapping step --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", ["same", "1p5x"])
@pytest.mark.parametrize("op", T.OPERATORS)
def test_hdr10_step_plain_tier_is_exact_on_every_row(mpcvr, oracle, torch_cuda, op, geo):
    from videorenderer_amd import api
    for i, row in enumerate(T.HDR10_ROWS):
        for over in ({}, dict(iTexFormat=8)) if i in (0, 4) else ({},):        # (the 8-bit internal format on two rows: typical_400, knee_free_600)
            c = T.hdr_case(row, op, geo, **over)
            _, want = want_of(oracle, c)
            got, info = draw(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FUSED)
            assert info.startswith("passes:") and "hdr10tonemap" in info and "kernel=" not in info, (c["name"], info)
            exact(got, want, c, f"{c['name']} {over} plain [{info}]")


@pytest.mark.parametrize("geo,kernel", [("1p5x", "kernel=fused_period("), ("1p25x", "kernel=fused_strip(")])
@pytest.mark.parametrize("op", T.OPERATORS)
def test_hdr10_step_behind_the_fused_resize_kernels(mpcvr, oracle, torch_cuda, op, geo, kernel):
    counts = {}
    for row in T.HDR10_ROWS:
        c = T.hdr_case(row, op, geo)
        p, want = want_of(oracle, c)
        got, info = draw(mpcvr, torch_cuda, c)
        assert kernel in info and "hdr10tonemap" in info, (c["name"], info)
        same, n = compare_behind_tail(oracle, p, FRAME, PITCH, got, want, f"{c['name']} [{info}]", ten_bit=True, lim=2, operator_input=True, convert_output=True,
                                      cap=NO_CAP)
        worst = int(np.abs(_codes10(got) - _codes10(want)).max())
        log(f"hdr10 row={row['name']} op={op} geo={geo} route={info} identical={same:.5f} worst={worst} beyond_2_codes={n}")
        counts[row["name"]] = n
    assert max(counts.values()) <= HDR_CAPS[op], (op, geo, HDR_CAPS[op], counts)


@pytest.mark.parametrize("name", ["typical_400", "knee_free_600"])
@pytest.mark.parametrize("op", [5, 6])
def test_hdr10_step_batches_equal_single_frames(mpcvr, torch_cuda, op, name):
    """ProcessBatch of five frames (the designed frame and four noise frames) equals five single frames bit for bit: one k_hdr10_tonemap launch
    per chunk behind batched post-scale textures."""
    torch = torch_cuda
    c = T.hdr_case(T.ROWS_BY_NAME[name], op, "1p5x")
    vp, (ww, wh) = make_vp(mpcvr, c)
    frames = [torch.from_numpy(FRAME).cuda()] + [torch.from_numpy(case_frame(dict(c, kind="noise", seed=9100 + i))[0]).cuda() for i in range(4)]
    singles = []
    for f in frames:
        d = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
        vp.CopySample(f, PITCH)
        vp.Process(d, ww * 4)
        singles.append(d)
    vp.Synchronize()
    info = vp.GetVPInfo()
    assert "kernel=fused_period(" in info and "hdr10tonemap" in info, info
    outs = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in frames]
    vp.ProcessBatch(frames, outs, ww * 4)
    vp.Synchronize()
    route = vp.GetLastBatchInfo()
    info_b = vp.GetVPInfo()
    vp.close()
    assert route["frames"] == 5 and "hdr10tonemap" in info_b, (route, info_b)
    for i, (a, b) in enumerate(zip(singles, outs)):
        assert torch.equal(a, b), (name, op, i, info, route, int((a != b).sum()))
    assert all(not torch.equal(outs[0], o) for o in outs[1:])


@pytest.mark.parametrize("own_stream", [True, False], ids=["own_stream", "callers_stream"])
@pytest.mark.parametrize("op", [4, 5, 6])
def test_metadata_and_display_peak_change_between_two_frames(mpcvr, torch_cuda, op, own_stream):
    """SetHdrMetadata(row A), draw, SetHdrMetadata(row B), SetHdrOutput(another display peak), draw into a second target, and only then
    Synchronize: each target equals a fresh context's frame for its row (the constants travel with their launch, also on the frame lanes of a
    context that owns its stream)."""
    torch = torch_cuda
    a, b = T.ROWS_BY_NAME["typical_400"], T.ROWS_BY_NAME["knee_free_600"]
    fresh = {}
    for row in (a, b):
        fresh[row["name"]], info = draw(mpcvr, torch, T.hdr_case(row, op, "1p5x"))
        assert "kernel=fused_period(" in info and "hdr10tonemap" in info, info
    assert not np.array_equal(fresh[a["name"]], fresh[b["name"]])
    import contextlib
    with (contextlib.nullcontext() if own_stream else torch.cuda.stream(torch.cuda.Stream())):      # (torch's default stream is NULL = the context's own)
        vp, (ww, wh) = make_vp(mpcvr, T.hdr_case(a, op, "1p5x"))
        dev = torch.from_numpy(FRAME).cuda()
        d1 = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
        d2 = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
        vp.CopySample(dev, PITCH)
        vp.Process(d1, ww * 4)
        vp.SetHdrMetadata(*b["meta"])
        vp.SetHdrOutput(True, op, b["display"])
        vp.CopySample(dev, PITCH)
        vp.Process(d2, ww * 4)
        vp.Synchronize()
        info = vp.GetVPInfo()
        o1, o2 = d1.cpu().numpy(), d2.cpu().numpy()
        vp.close()
    assert "kernel=fused_period(" in info and "hdr10tonemap" in info, info
    assert np.array_equal(o1, fresh[a["name"]]), (op, own_stream, int((o1 != fresh[a["name"]]).sum()))
    assert np.array_equal(o2, fresh[b["name"]]), (op, own_stream, int((o2 != fresh[b["name"]]).sum()))


@pytest.mark.parametrize("name", [r["name"] for r in T.DOVI_ROWS])
def test_hdr10_step_on_the_dolby_vision_rows(mpcvr, oracle, torch_cuda, name):
    """Level 1 in place of the HDR10 metadata (operator 5 drawn as 6) and a selected level-2 block (the trims inside the step): the plain tier
    bit-exact, same size and 384 x 48; the default tier (block convert, the surface variant of a fused resize kernel, the step) with the
    suite's Dolby Vision bar for a ten-bit target — two codes, a channel beyond only behind its witness, capped by DOVI_CAPS."""
    from videorenderer_amd import api
    row = next(r for r in T.DOVI_ROWS if r["name"] == name)
    counts = {}
    for op in T.OPERATORS:
        for geo in ("same", "1p5x"):
            c = T.hdr_case(row, op, geo)
            p, want = want_of(oracle, c)
            got, info = draw(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FUSED)
            assert info.startswith("passes:") and "hdr10tonemap" in info and "kernel=" not in info, (c["name"], info)
            exact(got, want, c, f"{c['name']} plain [{info}]")
        got, info = draw(mpcvr, torch_cuda, c)
        assert path_ok(info, "passes:convert,resizeX,resizeY,hdr10tonemap;kernel=fused_strip:surface("), info      # (at 3:2 the periodic kernel's surface variant)
        same, n = compare_behind_tail(oracle, p, FRAME, PITCH, got, want, f"{c['name']} [{info}]", ten_bit=True, lim=2, dovi=True, operator_input=True,
                                      convert_output=True, cap=NO_CAP)
        worst = int(np.abs(_codes10(got) - _codes10(want)).max())
        log(f"dovi row={name} op={op} geo=1p5x route={info} identical={same:.5f} worst={worst} beyond_2_codes={n}")
        counts[op] = n
    over = {op: n for op, n in counts.items() if n > DOVI_CAPS[op]}
    assert not over, (name, over, DOVI_CAPS)
    if row["l1"]:                   # operator 5 IS operator 6 on this row
        a, _ = draw(mpcvr, torch_cuda, T.hdr_case(row, 5, "1p5x"))
        b, _ = draw(mpcvr, torch_cuda, T.hdr_case(row, 6, "1p5x"))
        assert np.array_equal(a, b)


# ---- the SDR tails over iSDRDisplayNits ------------------------------------------------------------------------------------------------
BGRA8, RGB10A2 = 0, 1
# label -> (geometry, settings, flags by name, the GetVPInfo fragment the route must show (None: no fused name), render-target formats)
SDR_ROUTES = {
    "direct": ("same", {}, (), "direct:convert", (BGRA8, RGB10A2)),
    "up2x_lanczos3": ("2x", dict(iUpscaling=4), (), "fused_up2x", (BGRA8, RGB10A2)),
    "up2x_catmull": ("2x", dict(iUpscaling=2), (), "fused_up2x", (BGRA8, RGB10A2)),
    "period": ("1p5x", {}, (), "kernel=fused_period(", (BGRA8,)),
    "strip": ("1p25x", {}, (), "kernel=fused_strip(", (BGRA8,)),
    "jinc2x": ("2x", dict(iUpscaling=5), (), "fused_jinc2x", (BGRA8,)),
    "direct_no_lut": ("same", {}, ("FLAG_NO_LUT",), "direct:convert", (BGRA8, RGB10A2)),
    "up2x_no_lut": ("2x", dict(iUpscaling=4), ("FLAG_NO_LUT",), "fused_up2x", (BGRA8, RGB10A2)),
    "folded_same": ("same", {}, ("FLAG_NO_FAST_CONVERT",), None, (BGRA8,)),
    "folded_2x": ("2x", dict(iUpscaling=4), ("FLAG_NO_FAST_CONVERT",), None, (BGRA8,)),
}
assert set(SDR_ROUTES) == set(SDR_CAPS)


@pytest.mark.parametrize("geo", ["same", "2x"])
@pytest.mark.parametrize("tail", sorted(T.SDR_TAILS))
def test_sdr_tails_plain_tier_is_exact_at_every_nits_value(mpcvr, oracle, torch_cuda, tail, geo):
    from videorenderer_amd import api
    for nits in T.SDR_NITS:
        for fmt in (BGRA8, RGB10A2):
            c = T.sdr_case(tail, nits, geo, output_format=fmt)
            _, want = want_of(oracle, c)
            got, info = draw(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FUSED)
            assert info.startswith("passes:") and "kernel=" not in info, (c["name"], info)
            exact(got, want, c, f"{c['name']} fmt {fmt} plain [{info}]")


_LUT_TWIN = {}           # (route without "_no_lut", tail, nits, fmt) -> (pixels, outliers): what the table draws, for its literal twin


@pytest.mark.parametrize("route", sorted(SDR_ROUTES))
@pytest.mark.parametrize("tail", sorted(T.SDR_TAILS))
def test_sdr_tails_on_every_convert_route_over_the_nits(mpcvr, oracle, torch_cuda, tail, route):
    from videorenderer_amd import api
    geo, over, flag_names, fragment, fmts = SDR_ROUTES[route]
    flags = 0
    for n in flag_names:
        flags |= getattr(api, n)
    counts = {}
    for nits in T.SDR_NITS:
        for fmt in fmts:
            c = T.sdr_case(tail, nits, geo, output_format=fmt, **over)
            p, want = want_of(oracle, c)
            got, info = draw(mpcvr, torch_cuda, c, extra_flags=flags)
            if fragment is None:
                assert not any(k in info for k in FUSED_NAMES), (c["name"], info)
            elif fragment == "fused_jinc2x" and os.environ.get("MPCVR_LDS_LIMIT"):
                assert info == fragment or info.startswith("passes:convert,resizeX"), (c["name"], info)      # (a device that grants less LDS)
            else:
                assert fragment in info, (c["name"], info)
            ten = fmt == RGB10A2
            same, n = compare_behind_tail(oracle, p, FRAME, PITCH, got, want, f"{c['name']} {route} fmt {fmt} [{info}]", ten_bit=ten, lim=2 if ten else 1,
                                          cap=NO_CAP)
            codes = _codes10 if ten else (lambda a: a[..., :3].astype(np.int16))
            worst = int(np.abs(codes(got) - codes(want)).max())
            log(f"sdr tail={tail} nits={nits} route={route} fmt={'rgb10a2' if ten else 'bgra8'} info={info} identical={same:.5f} worst={worst} beyond_limit={n}")
            counts[(nits, fmt)] = n
            # the table against the literal chain: the same kernel either way, so a table-only error is a difference between the two
            twin = ({"direct_no_lut": "direct", "up2x_no_lut": "up2x_lanczos3"}.get(route, route), tail, nits, fmt)
            if route in ("direct", "up2x_lanczos3"):
                _LUT_TWIN[twin] = (got, n)
            elif route.endswith("_no_lut") and twin in _LUT_TWIN:
                lut, n_lut = _LUT_TWIN[twin]
                d = np.abs(codes(got) - codes(lut))
                log(f"sdr tail={tail} nits={nits} route={route} fmt={'rgb10a2' if ten else 'bgra8'} table_vs_literal identical={float((d == 0).mean()):.5f} worst={int(d.max())}")
                if n == 0 and n_lut == 0:           # both within lim of the oracle on every channel
                    assert d.max() <= 2 * (2 if ten else 1), (c["name"], int(d.max()))
    assert max(counts.values()) <= SDR_CAPS[route], (route, tail, SDR_CAPS[route], {k: v for k, v in counts.items() if v})


@pytest.mark.parametrize("geo,fragment", [("same", "direct:convert"), ("2x", "fused_up2x"), ("1p5x", "kernel=fused_period(")])
def test_configure_from_125_nits_to_each_end_and_back(mpcvr, torch_cuda, geo, fragment):
    """One context walks 125 -> 25 -> 125 -> 400 -> 125 through Configure (the table is rebuilt and uploaded again each time): every frame
    equals a fresh context's.  Configure refuses 24 and 401 and leaves the context as it was."""
    torch = torch_cuda
    from videorenderer_amd import api
    fresh = {}
    for nits in (25, 125, 400):
        fresh[nits], info = draw(mpcvr, torch, T.sdr_case("pq", nits, geo))
        assert fragment in info, info
    assert not np.array_equal(fresh[25], fresh[125]) and not np.array_equal(fresh[125], fresh[400])
    vp, (ww, wh) = make_vp(mpcvr, T.sdr_case("pq", 125, geo))
    dev = torch.from_numpy(FRAME).cuda()
    for step, nits in enumerate((125, 25, 125, 400, 125)):
        if step:
            assert vp.Configure(vp.settings.copy(iSDRDisplayNits=nits)) == api.S_OK
        for bad in (24, 401):
            with pytest.raises(api.MpcvrError) as e:
                vp.Configure(vp.settings.copy(iSDRDisplayNits=bad))
            assert e.value.hr == api.E_INVALIDARG
        dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
        vp.CopySample(dev, PITCH)
        vp.Process(dst, ww * 4)
        vp.Synchronize()
        assert fragment in vp.GetVPInfo(), vp.GetVPInfo()
        out = dst.cpu().numpy()
        assert np.array_equal(out, fresh[nits]), (geo, step, nits, int((out != fresh[nits]).sum()))
    vp.close()


# ---- the correction passes over iSDRDisplayNits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [3, 4, 5])
@pytest.mark.parametrize("src_fmt,dst_fmt", [(0, 0), (1, 1), (1, 0)])
def test_correction_passes_over_the_nits(mpcvr, oracle, torch_cuda, kind, src_fmt, dst_fmt):
    """Kinds 3, 4, 5 of mpcvr_correction_pass read LuminanceScale = 10000 / nits: a 200 x 64 surface (random texels and the corners of the cube)
    at every SDR_NITS value against the oracle, with the bars of test_correction_passes_vs_oracle."""
    torch = torch_cuda
    from videorenderer_amd import api
    rng = np.random.default_rng(2000 + kind * 10 + src_fmt * 3 + dst_fmt)
    w, h = 200, 64
    src = rng.integers(0, 1 << 32, size=(h, w), dtype=np.uint64).astype(np.uint32)
    src[0, :8] = [0, 0xffffffff, 0x3ff, 0x3ff << 10, 0x3ff << 20, 0x00ff0000, 0x0000ff00, 0x000000ff]
    d_src = torch.from_numpy(src.view(np.int32)).cuda()
    seen = set()
    for nits in T.SDR_NITS:
        want = oracle.correction_pass(kind, src, 10 if src_fmt else 8, 10 if dst_fmt else 8, sdr_nits=nits)
        dst = torch.full((h, w, 4), BG, dtype=torch.uint8, device="cuda")
        api.correction_pass(kind, d_src, w * 4, src_fmt, dst, w * 4, dst_fmt, w, h, sdr_nits=nits)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        what = f"correction pass {kind} ({src_fmt} -> {dst_fmt}) at {nits} nits [route: mpcvr_correction_pass]"
        if dst_fmt:
            compare_rgb10(got, want.reshape(h, w, 1).view(np.uint8).reshape(h, w, 4), what)
        else:
            compare(got, want.view(np.uint8).reshape(h, w, 4), what, min_same=0.99)
        seen.add(got.tobytes())
    assert len(seen) == len(T.SDR_NITS), "the nits do not reach the pass"
