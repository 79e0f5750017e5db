"""The largest ratios and frame extents the resize routes accept, on the GPU (tests/large_geometry.py holds the table,
tests/test_large_geometry.py its CPU half).

Every case is drawn on three tiers and held to the project's bars:
  * the plain tier (MPCVR_FLAG_NO_FUSED) equals the oracle bit for bit;
  * the folded tier (MPCVR_FLAG_NO_FAST_CONVERT) equals the plain tier byte for byte (behind a PQ / HLG tail its convert kernel is built with
    the fused tiers' transcendentals and is held to the oracle under the fused tiers' bar, as test_folded_kernels_vs_oracle does; the
    Jinc2m phase table is within one code of the per-pixel kernel with >= 0.999 identical, as test_full_size_general_ratio_tiers_agree holds it);
  * the default tier is within one code of the oracle with >= 0.99 of the channels identical (R10G10B10A2 targets: compare_rgb10 as
    test_default_path_vs_oracle calls it — two codes for a PQ- / HLG-tagged source, five behind 8-bit intermediates); GetVPInfo shows the fused kernel the table names, or no fused name where it must have stepped aside.
A group's cases are all drawn before the group fails, and every default-tier frame prints `LARGE <case> [<route>] max |delta| <n>, off by one
<share>` so that a run leaves the measured figures behind.
"""
import numpy as np
import pytest

from tests import large_geometry as G
from tests.golden.cases import case_frame, oracle_params
from tests.test_parity_gpu import BG, CarvedTargets, _codes10, compare, compare_rgb10, has_tail, internal_is_8bit, make_vp, run_product

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


_WANT = {}


def oracle_frame(oracle, c):
    """the oracle's window for a case, untouched pixels = BG: computed once, read-only"""
    if c["name"] not in _WANT:
        frame, pitch = case_frame(c)
        p = oracle_params(oracle, c)
        want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
        want.setflags(write=False)
        _WANT[c["name"]] = want
    return _WANT[c["name"]]


def tail_of(c):
    """a transcendental tail in the convert draw (an HDR10 display takes PQ as it is: no tail)"""
    return bool(has_tail(c)) and not c.get("hdr_output")


def codes(c, a):
    return _codes10(a) if c.get("output_format", 0) == 1 else a[..., :3].astype(np.int16)


def measured(c, got, want):
    d = np.abs(codes(c, got).astype(np.int32) - codes(c, want).astype(np.int32))
    return int(d.max()), float((d != 0).mean())


def hold(c, got, want, what, exact=False):
    if c.get("output_format", 0) == 1:
        compare_rgb10(got, want, what, exact=exact, tail=has_tail(c), internal8=internal_is_8bit(c))      # (as test_default_path_vs_oracle calls it)
    else:
        compare(got, want, what, exact=exact, min_same=0.99)


def check_case(mpcvr, oracle, torch, c):
    from videorenderer_amd import api
    name = c["name"]
    want = oracle_frame(oracle, c)
    plain, info_p = run_product(mpcvr, torch, c, extra_flags=api.FLAG_NO_FUSED)
    assert info_p.startswith("passes:") and "kernel=" not in info_p and "fused" not in info_p, (name, info_p)
    hold(c, plain, want, f"{name} plain [{info_p}]", exact=True)
    folded, info_f = run_product(mpcvr, torch, c, extra_flags=api.FLAG_NO_FAST_CONVERT)
    assert not any(k in info_f for k in G.FUSED_NAMES), (name, info_f)
    if tail_of(c):
        hold(c, folded, want, f"{name} folded [{info_f}]")
    elif c.get("iUpscaling") == G.JINC2 and not c.get("aside"):
        # Jinc2m at a dyadic ratio: k_jinc2_phases holds the weights of the nominal phases, the per-pixel kernel evaluates them at the
        # interpolated texture coordinate — the bar test_full_size_general_ratio_tiers_agree holds this pair to.  (`aside`: the planner
        # refuses the phase table, both tiers run the per-pixel kernel: byte for byte)
        if c.get("output_format", 0) == 1:
            compare_rgb10(folded, plain, f"{name} folded: phase table vs per-pixel weights [{info_f}]", min_same=0.999)
        else:
            compare(folded, plain, f"{name} folded: phase table vs per-pixel weights [{info_f}]", min_same=0.999)
    else:
        assert np.array_equal(folded, plain), f"{name} folded [{info_f}]: {int((folded != plain).sum())} bytes differ from the plain tier"
    default, info = run_product(mpcvr, torch, c)
    worst, off = measured(c, default, want)
    print(f"LARGE {name} [{info.split(';')[0]}] max |delta| {worst}, off by one {off:.5f}")
    if c.get("fused"):
        assert c["fused"] in info, (name, f"expected {c['fused']}", info)
    else:
        assert not any(k in info for k in G.FUSED_NAMES), (name, "no fused kernel expected", info)
    hold(c, default, want, f"{name} [{info}]")


def check_group(mpcvr, oracle, torch, cases):
    failed = []
    for c in cases:
        try:
            check_case(mpcvr, oracle, torch, c)
        except AssertionError as e:
            failed.append(f"{c['name']}: {str(e)[:600]}")
    assert not failed, f"{len(failed)} of {len(cases)} cases:\n" + "\n".join(failed)


def _params(family, size):
    g = G.groups(family, size)
    return pytest.mark.parametrize("cases", [x[1] for x in g], ids=[x[0] for x in g])


@_params("ladder", 13)
def test_tap_count_ladder(mpcvr, oracle, torch_cuda, cases):
    """ps_convolution at 16, 17, 64 and 128 taps per axis through all six downscalers: X only (k_resize_cols / k_resize), Y only (k_resize_rows),
    both axes (k_resize_2d where its gates allow; k_fused_strip's nt = 16 variant at 16 taps) and against a 4-tap upscale; rows whose own
    window is shorter than the table's ntaps run the zero-weight padding."""
    check_group(mpcvr, oracle, torch_cuda, cases)


@_params("strip", 11)
def test_strip_kernel_edges(mpcvr, oracle, torch_cuda, cases):
    """k_fused_strip with a ring of 32 rows, 16 taps on one axis against an upscale on the other, four and eight convert passes per row pair and
    the widest source window any plan reaches, from raw samples and from a surface, tails none / PQ / HLG; a 17th tap: the kernel steps aside."""
    check_group(mpcvr, oracle, torch_cuda, cases)


@_params("gates", 11)
def test_lds_gates_of_the_folded_kernels(mpcvr, oracle, torch_cuda, cases):
    check_group(mpcvr, oracle, torch_cuda, cases)


@_params("bigup", 9)
def test_upscales_of_16x_to_127x(mpcvr, oracle, torch_cuda, cases):
    check_group(mpcvr, oracle, torch_cuda, cases)


@_params("extent", 12)
def test_frames_at_the_largest_extents(mpcvr, oracle, torch_cuda, cases):
    """Thin frames 16384, 16380 and 15360 long, as width and as height: exact 2x (4 / 5 / 6 taps), Jinc2m 2x, 1.5x, 4:3, same size, a 2.5x
    downscale; source rects at columns / rows >= 13900; 8-bit dithered and R10G10B10A2 targets."""
    check_group(mpcvr, oracle, torch_cuda, cases)


@pytest.mark.parametrize("name", G.BATCH_CASES)
def test_batches_at_the_largest_extents_equal_single_frames(mpcvr, torch_cuda, name):
    torch = torch_cuda
    c = G.CASES[name]
    vp, (ww, wh) = make_vp(mpcvr, c)
    frames = [torch.from_numpy(case_frame(dict(c, seed=c["seed"] + 100 * (i + 1)))[0]).cuda() for i in range(3)]
    pitch = vp.GetFrameBytes()[1]
    singles = []
    for f in frames:
        dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
        vp.CopySample(f, pitch)
        vp.Process(dst, ww * 4)
        singles.append(dst)
    vp.Synchronize()
    info = vp.GetVPInfo()
    dsts = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in frames]
    vp.ProcessBatch(frames, dsts, ww * 4)
    vp.Synchronize()
    route = vp.GetLastBatchInfo()
    vp.close()
    assert route["frames"] == 3, (name, route)
    if c.get("fused"):
        assert c["fused"] in info, (name, info)
    for i in range(3):
        assert torch.equal(singles[i], dsts[i]), (name, i, info, route)
    assert not torch.equal(dsts[0], dsts[1]), name


# ---- family F: refusal at 129 taps and above ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in G.FAMILIES["refused"]])
def test_refusal_above_128_taps(mpcvr, oracle, torch_cuda, name):
    """Process fails with E_NOTIMPL on every tier, the render target and its guard bytes untouched; a batch is refused with nothing drawn; the
    context stays usable: back at a supported video rect its next frame equals a fresh context's (and the oracle's, on the plain tier)."""
    from videorenderer_amd import api
    torch = torch_cuda
    c = G.CASES[name]
    frame, pitch = case_frame(c)
    dev = torch.from_numpy(frame).cuda()
    back = dict(c, dst=c["back_to"])
    for flags in (api.FLAG_NO_FUSED, api.FLAG_NO_FAST_CONVERT, 0):
        vp, (ww, wh) = make_vp(mpcvr, c, flags)
        t = CarvedTargets(torch, ww, wh, ww * 4 + 64, [0, 8])
        vp.CopySample(dev, pitch)
        with pytest.raises(api.MpcvrError, match="resize ratio outside the supported range") as e:
            vp.Process(t.ptrs[0], t.pitch)
        assert e.value.hr == api.E_NOTIMPL, (name, flags, str(e.value))
        with pytest.raises(api.MpcvrError) as e:
            vp.ProcessBatch([dev, dev], [t.ptrs[0], t.ptrs[1]], t.pitch)
        assert e.value.hr == api.E_NOTIMPL, (name, flags, str(e.value))
        vp.Synchronize()
        t.assert_guards_intact(f"{name} flags {flags}")
        for i in range(2):
            assert bool((t.window(i) == BG).all()), f"{name} flags {flags}: a refused draw wrote window pixels of target {i}"
        # back to a supported size: the same context, then a fresh one
        bw, bh = back["dst"]
        vp.SetWindowRect((0, 0, bw, bh))
        vp.SetVideoRect((0, 0, bw, bh))
        dst = torch.full((bh, bw, 4), BG, dtype=torch.uint8, device="cuda")
        vp.CopySample(dev, pitch)
        vp.Process(dst, bw * 4)
        vp.Synchronize()
        info = vp.GetVPInfo()
        vp.close()
        fresh, info_fresh = run_product(mpcvr, torch, back, extra_flags=flags)
        assert info == info_fresh, (name, flags, info, info_fresh)
        assert np.array_equal(dst.cpu().numpy(), fresh), f"{name} flags {flags} [{info}]: the frame after a refusal differs from a fresh context's"
        if flags == api.FLAG_NO_FUSED:
            p = oracle_params(oracle, back)
            want = oracle.process(p, frame, pitch, dst=np.full((bh, bw, 4), BG, dtype=np.uint8))
            hold(back, fresh, want, f"{name} back at {bw} x {bh} plain [{info}]", exact=True)


def test_input_extents_above_the_limit_are_refused(mpcvr, oracle, torch_cuda):
    """mpcvr_set_input refuses 16385 columns or rows (E_INVALIDARG) and the context then takes a legal media type and draws it correctly."""
    from videorenderer_amd import api
    torch = torch_cuda
    c = G.CASES["gates_blk8_span_14_lanczos3_rgb32"]
    want = oracle_frame(oracle, c)
    fresh, info_fresh = run_product(mpcvr, torch, c)
    for cf, w, h in ((G.RGB32, G.MAX_EXTENT + 1, 8), (G.RGB32, 8, G.MAX_EXTENT + 1), (G.P010, G.MAX_EXTENT + 2, 8), (G.P010, 8, G.MAX_EXTENT + 2)):
        vp = api.VideoProcessor(api.default_settings(iUpscaling=c["iUpscaling"], flags=c["flags"]))
        with pytest.raises(api.MpcvrError) as e:
            vp.InitMediaType(cf, w, h)
        assert e.value.hr == api.E_INVALIDARG, (cf, w, h, str(e.value))
        vp.InitMediaType(c["cformat"], c["w"], c["h"], extfmt=c["exfmt"])
        ww, wh = c["dst"]
        vp.SetWindowRect((0, 0, ww, wh))
        vp.SetVideoRect((0, 0, ww, wh))
        frame, pitch = case_frame(c)
        dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
        vp.CopySample(torch.from_numpy(frame).cuda(), pitch)
        vp.Process(dst, ww * 4)
        vp.Synchronize()
        info = vp.GetVPInfo()
        vp.close()
        assert info == info_fresh and np.array_equal(dst.cpu().numpy(), fresh), (cf, w, h, info)
    hold(c, fresh, want, f"{c['name']} [{info_fresh}]")
