"""Parity tests proper: the HIP path (through the C-ABI) against the CPU oracle on the same seeded inputs.

Bar (BASELINE.json north_star): |delta| <= 1 LSB per 8-bit channel, dither table/indexing bit-exact.
Tighter where the arithmetic allows it:
  * pass-per-kernel path, SDR (no transcendental instruction on the path): BIT-EXACT with the oracle;
  * pass-per-kernel path with a PQ/HLG/gamma tail: <= 1 LSB, >= 99.5 % of channels identical;
  * fused 2x kernel (FMA contraction, LDS tone-map LUT): <= 1 LSB, >= 99 % identical.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.golden.cases import GOLDEN_CASES, SETTING_KEYS, case_frame, case_geometry, oracle_params, run_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

BG = 7      # background byte of the render target: pixels outside the video rect must stay untouched


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def has_tail(c):
    trc = (c.get("exfmt", 0) >> 27) & 0x1f
    prim = (c.get("exfmt", 0) >> 22) & 0x1f
    return (trc in (15, 16) and c.get("bConvertToSdr", 1)) or prim == 9 or "dovi" in c


def make_vp(mpcvr, c, extra_flags=0):
    from videorenderer_amd import api
    kw = {k: c[k] for k in SETTING_KEYS if k in c}
    kw["flags"] = kw.get("flags", 0) | extra_flags
    if "bDeintBlend" in c:
        kw["bDeintBlend"] = c["bDeintBlend"]
    vp = api.VideoProcessor(api.default_settings(**kw))
    (ww, wh), vr = case_geometry(c)
    pitch = c.get("pitch", 0)
    if c.get("bottom_up"):
        pitch = -api.plan_frame_layout(c["cformat"], c["w"], c["h"])[1]
    vp.InitMediaType(c["cformat"], c["w"], c["h"], pitch=pitch, src_rect=c.get("src_rect"), extfmt=c.get("exfmt", 0))
    vp.SetWindowRect((0, 0, ww, wh))
    vp.SetVideoRect(vr)
    if "procamp" in c:
        vp.SetProcAmpValues(*c["procamp"])
    if "sample_format" in c:
        vp.SetSampleFormat(c["sample_format"])
    if c.get("hdr_output"):
        vp.SetHdrOutput(True, c.get("hdr_tonemap", 0), c.get("hdr_display", 1000.0))
        if "hdr_meta" in c:
            vp.SetHdrMetadata(*c["hdr_meta"])
    elif "hdr_display" in c:
        vp.SetHdrOutput(False, 0, c["hdr_display"])
    if "dovi" in c:
        from videorenderer_amd import synth
        vp.SetDoviMetadata(synth.dovi_metadata(**c["dovi"]))
    if "rotation" in c:
        vp.SetRotation(c["rotation"])
    if "flip" in c:
        vp.SetFlip(bool(c["flip"]))
    return vp, (ww, wh)


def run_product(mpcvr, torch, c, extra_flags=0, host_upload=False):
    vp, (ww, wh) = make_vp(mpcvr, c, extra_flags)
    frame, pitch = case_frame(c)
    assert vp.GetFrameBytes() == (frame.size, abs(pitch))
    dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
    if host_upload:
        vp.CopySample(frame, pitch)
    else:
        dev = torch.from_numpy(frame).cuda()
        vp.CopySample(dev, pitch)
    vp.Process(dst, ww * 4)
    vp.Synchronize()
    info = vp.GetVPInfo()
    out = dst.cpu().numpy()
    vp.close()
    return out, info


# ---- render-target layouts ----------------------------------------------------------------------------------------------------------
# A host's back buffer is pitch-padded and sub-allocated more often than not.  Every layout draws into a target carved out of a larger device
# buffer that holds a non-constant byte pattern; the bytes in front of the target, behind it and between window_w * 4 and dst_pitch of every
# row must still hold the pattern afterwards, bit for bit (include/mpcvr.h: pixels outside dst_rect are not written).
#   name       first byte (from a 256-byte boundary)   pitch                                              what it reaches
#   tight      0                                       window_w * 4                                       the layout of a tensor of its own
#   padded16   0                                       window_w * 4 rounded up to 16, plus 64             the aligned epilogues with other row addresses
#   off4       4                                       window_w * 4 + 4                                   nothing aligned beyond a pixel: the per-pixel store paths
#   off8       8                                       a multiple of 8, not of 16, >= window_w * 4 + 8    the 8-byte paths, the 16-byte ones declining
LAYOUTS = ("tight", "padded16", "off4", "off8")


def layout_of(layout, ww):
    """(distance of the target's first byte from a 256-byte boundary, dst_pitch) of a layout for a window ww pixels wide."""
    row = ww * 4
    if layout == "tight":
        return 0, row
    if layout == "padded16":
        return 0, ((row + 15) & ~15) + 64
    if layout == "off4":
        return 4, row + 4
    if layout == "off8":
        pitch = (row + 8 + 7) & ~7
        return 8, pitch + 8 if pitch % 16 == 0 else pitch
    raise KeyError(layout)


def kernel_under(layout, expect):
    """The GetVPInfo fragment a layout is expected to show where `tight` shows `expect`: k_fused_period stores 8 bytes per lane and steps
    aside for a target or pitch that is not a multiple of 8 (`off4`) — the launch then goes to k_fused_strip, whose epilogue has a per-pixel
    form; it must step aside, so `off4` is held to the strip kernel's name.  `off8` is all k_fused_period needs and is held to ITS name:
    these layouts found single frames into an 8-byte-aligned target losing the kernel to a flag that asked for 16 bytes (batches never did)."""
    if layout == "off4" and "fused_period" in expect:
        return expect.split("(")[0].replace("fused_period", "fused_strip") + "("
    return expect


class CarvedTargets:
    """n render targets of ww x wh pixels, `pitch` bytes per row, inside ONE patterned device buffer: target i starts bases[i] bytes behind a
    256-byte boundary; a guard band of one row of `pitch` plus 4 KiB (a wave's worth of 16-byte stores is 1 KiB) lies in front of the first,
    between any two and behind the last.  Window pixels start as BG."""

    def __init__(self, torch, ww, wh, pitch, bases):
        self.torch, self.ww, self.wh, self.pitch = torch, ww, wh, pitch
        guard = pitch + 4096
        self.starts = []
        at = 0
        for b in bases:
            at = (at + guard + 255) // 256 * 256 + b
            self.starts.append(at)
            at += wh * pitch                      # (the last row's padding belongs to the target's rows: checked like every row's)
        total = at + guard
        i = torch.arange(total, dtype=torch.int32, device="cuda") & 255
        self.pattern = ((i * 131 + 17) & 255).to(torch.uint8)
        del i
        self.buf = self.pattern.clone()
        assert self.buf.data_ptr() % 256 == 0
        for s in self.starts:
            self._window(self.buf, s).fill_(BG)
        self.ptrs = [self.buf.data_ptr() + s for s in self.starts]

    def _window(self, t, start):
        return t.as_strided((self.wh, self.ww * 4), (self.pitch, 1), start)

    def window(self, i):
        """the pixels of target i as a (wh, ww, 4) view of the buffer (device)"""
        return self.buf.as_strided((self.wh, self.ww, 4), (self.pitch, 4, 1), self.starts[i])

    def pixels(self, i=0):
        return self.window(i).contiguous().cpu().numpy()

    def assert_guards_intact(self, what):
        """every byte that is not a window pixel equals the pattern (call after Synchronize; the pixels are read with pixels() / window())"""
        torch = self.torch
        rest = self.buf.clone()
        for s in self.starts:
            self._window(rest, s).copy_(self._window(self.pattern, s))
        if torch.equal(rest, self.pattern):
            return
        off = int(torch.nonzero(rest != self.pattern)[0])
        n_bad = int((rest != self.pattern).sum())
        where = f"{self.starts[0] - off} bytes in front of target 0"
        for k, s in enumerate(self.starts):
            if off >= s:
                r, x = divmod(off - s, self.pitch)
                where = (f"target {k}: row {r}, byte {x} of the row (pixels end at {self.ww * 4}, pitch {self.pitch})" if r < self.wh
                         else f"{off - s - self.wh * self.pitch} bytes behind the last row of target {k}")
        raise AssertionError(f"{what}: {n_bad} byte(s) outside the window pixels were written; the first is {where}: "
                             f"{int(rest[off])} where the pattern holds {int(self.pattern[off])}")


def run_layouts(mpcvr, torch, c, extra_flags=0, layouts=LAYOUTS, what=""):
    """One context, one sample, the case drawn once per layout: {layout: (pixels, GetVPInfo)}, the guard and padding bytes of every layout
    checked.  `padded16` runs the kernel variant `tight` runs wherever window_w * 4 is a multiple of 16 (only the row addresses differ), so
    it must then leave the same bytes."""
    vp, (ww, wh) = make_vp(mpcvr, c, extra_flags)
    frame, pitch = case_frame(c)
    assert vp.GetFrameBytes() == (frame.size, abs(pitch))
    dev = torch.from_numpy(frame).cuda()
    outs = {}
    for layout in layouts:
        base, dst_pitch = layout_of(layout, ww)
        t = CarvedTargets(torch, ww, wh, dst_pitch, [base])
        vp.CopySample(dev, pitch)
        vp.Process(t.ptrs[0], dst_pitch)
        vp.Synchronize()
        info = vp.GetVPInfo()
        t.assert_guards_intact(f"{what or c.get('name', '')} layout {layout} (first byte at +{base}, pitch {dst_pitch}) [{info}]")
        outs[layout] = (t.pixels(), info)
    vp.close()
    if "tight" in outs and "padded16" in outs and (ww * 4) % 16 == 0:
        assert outs["tight"][1] == outs["padded16"][1], (what, outs["tight"][1], outs["padded16"][1])
        assert np.array_equal(outs["tight"][0], outs["padded16"][0]), f"{what}: a padded pitch changed the pixels [{outs['tight'][1]}]"
    return outs


# whole frames (>= 0.4 M pixels): the smallest share of identical channels measured over every such comparison of the suite is 0.99922
# (profiles/r03/parity_identical_channels.jsonl, MPCVR_PARITY_LOG); the floor is 1 - 2 x (1 - that): twice today's worst fails
WHOLE_FRAME_FLOOR = 0.9984
# Dolby Vision frames through the fused resize kernels ("hdr" content: bright saturated colours behind the reshaping and both PQ chains)
# measure 0.99846 .. 0.99854 on every tier, the plain kernels included: the same rule gives them their own floor
DOVI_RESIZE_FLOOR = 0.9969
POW_ULPS = 4      # Direct3D's pow is exp2(y * log2 x): with 1-ulp log2 / exp2 the result is off by up to ~0.35 |y log2 x| + 1.5 ulp (4 at x = 1e-4, y = 1/2.2)
# How MANY channels may sit beyond 1 LSB behind their witness (compare_behind_tail), from what was measured, not from a blanket share:
# Dolby Vision frames (reshaping + two PQ chains in front of the cancelling 2020 -> 709 row): at most 16 per 2.07 M-pixel frame over the
# whole round-3 suite (profiles/r03/parity_identical_channels.jsonl: 1-16, 17 of 1,187 comparisons) = 7.7 per million pixels; the cap
# is twice that.  Every other frame: none — except the cases named here, each with the count it was witnessed with.
# Round 6 (the oracle's transcendentals are now defined functions; gpurun_out/r06/parity_log.jsonl -> profiles/r06/): at most 9 per 2.07 M-pixel
# Dolby Vision frame on the block convert (0 on the plain tier, which is bit-exact) = 4.3 per million pixels; the cap is 1.5 x that.
ILL_CONDITIONED_PER_MPX_DOVI = 6.5
KNOWN_ILL_CONDITIONED = {
    # one channel, 2 LSB, on the block-convert kernel only (the plain per-pixel kernel is within 1): a saturated BT.2020 colour whose
    # blue cancels to 2e-4 of its terms behind the 2020 -> 709 row — the table's interpolated tone-map value (5e-7 off the literal chain)
    # and the fused chain's roundings move pow(x, 1/2.2)'s argument by 2 % there; the oracle's own answer spans 3 codes under +-4 ulp of pow()
    "p010_cosited_pq_same_size": 1,
}


def _codes10(a):
    u = a.view(np.uint32)[..., 0]
    return np.stack([(u >> sh) & 1023 for sh in (0, 10, 20)], -1).astype(np.int16)


# The Dolby Vision block convert reads the PQ EOTF from a table (log2 of the EOTF over sqrt(x), 8,193 entries) whose interpolation is accurate to
# 1.2e-6 relative (tests/test_host_logic.py::test_pq_eotf_table holds it to 3e-6): that is TEN ulps of a pow() result, not four.  Where a channel of
# a Dolby Vision frame is so ill-conditioned that the oracle's own answer spans a dozen codes under +-8 ulp (soak case 1428: 0 .. 17), the table
# tier lands outside the +-4 ulp interval without being wrong by more than its documented accuracy: a caller may ask for the interval of THAT
# accuracy (pow_ulps=POW_ULPS_EOTF_TABLE) — the fuzz tool does, on Dolby Vision plans only; the suite's Dolby Vision tests keep +-4.
POW_ULPS_EOTF_TABLE = 10


def compare_behind_tail(oracle, p, frame, pitch, got, want, name, min_same=0.99, ten_bit=False, lim=1, dovi=False, cap=None, operator_input=False, convert_output=False,
                        pow_ulps=None):
    """Frames behind a PQ / HLG / Dolby Vision tail: |delta| <= 1 like everywhere else, EXCEPT on channels where the oracle's own
    answer is not defined to one code — shown per channel, not assumed: the oracle is run again with every pow() of the chain POW_ULPS
    ulps low, POW_ULPS ulps high, and eight times with each call off by its own hash-drawn amount within +-POW_ULPS
    (oracle.process_with_pow_bias; D3D's pow = exp2(y log2 x) is allowed that slack and more), and a channel beyond 1 LSB passes only
    if the product's code lies inside the interval those oracle runs span (+- 1).  Where that happens (measured: the oracle's own
    answer spans 0..13 codes on such a channel):
    a bright saturated colour whose third channel cancels to ~1e-4 behind the 2020 -> 709 matrix — the PQ EOTF's (c2 - c3 v) term
    amplifies an ulp of pow(x, 1/m2) ~100x, pow(., 1/m1) 6x more, and pow(x, 1/2.2) has a slope of ~70 down there.
    ten_bit: an R10G10B10A2 target, compared code for code with `lim` ten-bit codes in place of the one 8-bit code.
    operator_input (plans with an HDR10 tone-mapping operator, round 6): the fused tiers are held to ONE code at every stored intermediate, and
    the operator maps a code of the texture it reads with its own slope (operator 6 near black: seven ten-bit codes per code — soak case 2367,
    profiles/r06/case2367.txt); the interval then also spans the oracle's answers for that texture one code low / high as a whole, on each
    channel alone, and in eight per-texel draws (oracle.process_with_tonemap_input_bias).
    convert_output (fused tiers, UNORM internal formats, round 6): the block convert is held to ONE code of m_TexConvertOutput, and what a code
    becomes behind the draws is the reference's own business — its Bicubic / Lanczos downscale shaders divide by a weight sum that is small at
    some phases (soak case 5624, profiles/r06/cases_5624_1428.txt: one code of one luma sample moves one pixel of the ORACLE by 17 ten-bit
    codes); the interval then also spans the oracle's answers for that texture one code low / high as a whole, per channel, and in sixteen
    per-texel draws (oracle.process_with_convert_output_bias).
    Returns (share of identical channels, number of such channels)."""
    codes = _codes10 if ten_bit else (lambda a: a[..., :3].astype(np.int16))
    g3, w3 = codes(got), codes(want)
    d = np.abs(g3 - w3)
    same = float((d == 0).mean())
    assert same >= min_same, f"{name}: only {same:.5f} of channels identical"
    bad = d > lim
    n_bad = int(bad.sum())
    if n_bad:
        bg = np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8)
        lo, hi = w3.copy(), w3.copy()
        # all pow() calls low, all high, and eight draws of independent per-call errors (a uniform bias cancels in the gamut matrix,
        # whose rows sum to 1: the channels of a real approximate pow err independently)
        pu = POW_ULPS if pow_ulps is None else int(pow_ulps)
        for bias, seed in [(-pu, 0), (pu, 0)] + [(pu, k) for k in range(1, 9)]:
            run = codes(oracle.process_with_pow_bias(p, frame, pitch, bias, dst=bg.copy(), seed=seed))
            lo = np.minimum(lo, run); hi = np.maximum(hi, run)
        if operator_input:
            for bias, ch, seed in [(b, ch, 0) for b in (-1, 1) for ch in (-1, 0, 1, 2)] + [(1, -1, k) for k in range(1, 9)]:
                run = codes(oracle.process_with_tonemap_input_bias(p, frame, pitch, bias, channel=ch, seed=seed, dst=bg.copy()))
                lo = np.minimum(lo, run); hi = np.maximum(hi, run)
        if convert_output:
            for bias, ch, seed in [(b, ch, 0) for b in (-1, 1) for ch in (-1, 0, 1, 2)] + [(1, -1, k) for k in range(1, 17)]:
                run = codes(oracle.process_with_convert_output_bias(p, frame, pitch, bias, channel=ch, seed=seed, dst=bg.copy()))
                lo = np.minimum(lo, run); hi = np.maximum(hi, run)
        lo -= lim; hi += lim
        inside = (g3 >= lo) & (g3 <= hi)
        worst = np.argwhere(bad & ~inside)
        assert worst.size == 0, (f"{name}: {len(worst)} of {n_bad} channels beyond {lim} code(s) are NOT explained by +-{pu} ulp of pow(): "
                                 f"e.g. (y, x, ch) = {tuple(worst[0])}: got {g3[tuple(worst[0])]}, oracle {w3[tuple(worst[0])]}, interval [{lo[tuple(worst[0])] + lim}, {hi[tuple(worst[0])] - lim}]")
        mpx = d.size / 3 / 1e6
        if cap is None:
            cap = int(np.ceil(ILL_CONDITIONED_PER_MPX_DOVI * mpx)) if dovi else KNOWN_ILL_CONDITIONED.get(name.split(" ")[0], 0)
        assert n_bad <= cap, (f"{name}: {n_bad} channels beyond {lim} code(s) (each inside the oracle's own +-{POW_ULPS} ulp interval) — more than "
                              f"the {cap} this kind of frame was measured with ({'Dolby Vision: 16 per M pixels' if dovi else 'named cases only'})")
    if os.environ.get("MPCVR_PARITY_LOG"):
        import json
        with open(os.environ["MPCVR_PARITY_LOG"], "a") as f:
            f.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], "what": name, "pixels": int(d.size // 3), "identical": same,
                                "max_delta": int(d.max()), "beyond_1lsb_all_inside_pow_ulp_interval": n_bad, "floor": min_same}) + "\n")
    return same, n_bad


def path_ok(info, path):
    """GetVPInfo against an expected prefix; where the prefix names k_fused_strip the periodic-phase kernel (the same launch with the
    vertical window in registers, taken at 4:3 / 3:2 / 2:3 / 1:2 / 3:1) is the planner's choice and counts as well."""
    return (info.startswith(path) or info.startswith(path.replace("kernel=fused_strip(", "kernel=fused_period(")) or
            info.startswith(path.replace("kernel=fused_strip:surface(", "kernel=fused_period:surface(")))


def compare(got, want, name, exact=False, min_same=0.99):
    assert got.shape == want.shape, name
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    same = float((d == 0).mean())
    assert d.max() <= (0 if exact else 1), f"{name}: max |delta| = {d.max()} ({(d > 1).sum()} channels > 1 LSB, same={same:.5f})"
    assert same >= min_same, f"{name}: only {same:.5f} of channels identical"
    if os.environ.get("MPCVR_PARITY_LOG"):      # evidence: measured share of identical channels per comparison (profiles/rNN/parity_*.jsonl)
        import json
        with open(os.environ["MPCVR_PARITY_LOG"], "a") as f:
            f.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], "what": name, "pixels": int(d.size // d.shape[-1]),
                                "identical": same, "max_delta": int(d.max()), "floor": 0.0 if exact else min_same, "exact_required": bool(exact)}) + "\n")
    return same


def internal_is_8bit(c):
    """m_InternalTexFmt of a case (UpdateTexParams :1143-1155): 8-bit when forced, or AUTO on an 8-bit source."""
    t = c.get("iTexFormat", 0)
    return t == 8 or (t == 0 and c["cformat"] in (1, 4, 5, 11, 14, 15, 16, 17, 18, 19, 26, 29, 30, 31, 37))


def compare_rgb10(got, want, name, exact=False, tail=False, min_same=0.99, internal8=False):
    """R10G10B10A2 render targets carry their own LSB (1/1023): the bar is stated in 10-bit codes, not as the 8-bit bar rescaled.
    exact: plain / folded kernels without a transcendental tail; otherwise <= 1 code (FMA contraction of the fused / block kernels),
    <= 2 codes behind a PQ / HLG / gamma tail (pow(x, 1/2.2) has unbounded slope at 0: one ulp of the linear value moves dark
    10-bit codes by more than one), and >= min_same of the channels identical.  internal8: the intermediates are B8G8R8A8, so
    one LSB of THEM is 1023/255 = 4.01 ten-bit codes at the render target (<= 5 after its own rounding)."""
    g, w = got.view(np.uint32)[..., 0], want.view(np.uint32)[..., 0]
    lim = 0 if exact else (5 if internal8 else 2 if tail else 1)
    same = []
    for sh in (0, 10, 20):
        d = np.abs(((g >> sh) & 1023).astype(np.int32) - ((w >> sh) & 1023).astype(np.int32))
        assert d.max() <= lim, f"{name}: 10-bit delta {d.max()} > {lim} ({int((d > lim).sum())} channels)"
        same.append(float((d == 0).mean()))
    assert min(same) >= min_same, f"{name}: only {min(same):.5f} of the 10-bit channels identical"
    assert np.array_equal(g >> 30, w >> 30)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_pass_per_kernel_path_vs_oracle(mpcvr, oracle, torch_cuda, name):
    from videorenderer_amd import api
    c = GOLDEN_CASES[name]
    want = run_case(oracle, name, background=BG)
    # (every render-target layout: the oracle's frame once, the product's once per layout, guard and padding bytes checked by run_layouts)
    for layout, (got, info) in run_layouts(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FUSED, what=name).items():
        assert info.startswith("passes:"), info
        # bit-exact, behind a PQ / HLG / gamma / Dolby Vision tail too (round 6: the tier evaluates the transcendentals as the oracle defines
        # them — csrc/vp_crmath.h — where until round 5 v_log_f32 / v_exp_f32 left tails at "<= 1 LSB, >= 99.5 % identical")
        if c.get("output_format", 0) == 1:
            compare_rgb10(got, want, f"{name} <{layout}>", exact=True)
        else:
            compare(got, want, f"{name} <{layout}>", exact=True)


ADAPTER_DRIVER = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "adapter_driver")


@pytest.mark.parametrize("name,window,offset,ten", [("c3hdr_p010_pq_lanczos3_2x", None, None, 0), ("c1_nv12_bt709_passthrough", (160, 96), (12, 6), 0),
                                                    ("up_1p5x_lanczos3", None, None, 0)])
def test_one_frame_through_the_adapter_class(mpcvr, oracle, torch_cuda, tmp_path, name, window, offset, ten):
    """The drop-in boundary exercised AS a CVideoProcessor (review item: the adapter was only ever checked for syntax).
    examples/hip_video_processor_adapter.cpp — compiled against the reference's own method list (Source/VideoProcessor.h:171-236, cut out of
    the header when oracle/_ref/adapter_driver was built) and linked with libmpcvr.so — is driven through the BASE-CLASS pointer the way the
    filter drives a processor: Init -> VerifyMediaType / InitMediaType(CMediaType over a VIDEOINFOHEADER2) -> SetWindowRect / SetVideoRect ->
    ProcessSample(IMediaSample over a host buffer) -> GetDisplayedImage -> GetCurentImage -> GetVPInfo.  What comes back is compared with the
    oracle: the displayed image (the back buffer Render drew: the window, black outside the video rect) and the snapshot (source-rect sized)."""
    import subprocess
    if not os.path.exists(ADAPTER_DRIVER):
        pytest.skip("oracle/_ref/adapter_driver is built where /root/reference is mounted (tests/adapter_env/build_adapter.py)")
    c = dict(GOLDEN_CASES[name])
    if window:
        c["window"], c["offset"] = window, offset
    (ww, wh), vr = case_geometry(c)
    frame, pitch = case_frame(c)
    assert pitch > 0
    sample = tmp_path / "sample.bin"
    sample.write_bytes(np.ascontiguousarray(frame).tobytes())
    exf = (c.get("exfmt", 0) & ~0xff) | (0x81 if c.get("exfmt", 0) else 0)      # AMCONTROL_USED | AMCONTROL_COLORINFO_PRESENT: "the bits are valid" (:1763)
    args = [ADAPTER_DRIVER, str(c["cformat"]), str(c["w"]), str(c["h"]), str(exf), str(ww), str(wh), *(str(v) for v in vr), str(c.get("iUpscaling", 2)), str(ten),
            str(sample), str(tmp_path / "displayed.bin"), str(tmp_path / "snapshot.bin")]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-1500:])
    out = dict(l.split(" ", 1) for l in r.stdout.splitlines() if " " in l)
    assert out["DISPLAYED"].split() == [str(ww), str(wh), "32", str(ww * wh * 4)], out
    assert out["SNAPSHOT"].split() == [str(c["w"]), str(c["h"]), "32", str(c["w"] * c["h"] * 4)], out
    assert out["VPINFO"].startswith("HIP shader video processor: ") and out["TYPE"].startswith("12 "), out
    # the displayed image: Render clears the back buffer to black, Process fills the video rect (DX11VideoProcessor.cpp:2622, 3285)
    shown = np.frombuffer((tmp_path / "displayed.bin").read_bytes(), dtype=np.uint8).reshape(wh, ww, 4)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.zeros((wh, ww, 4), dtype=np.uint8))
    d = np.abs(shown[..., :3].astype(np.int16) - want[..., :3].astype(np.int16))
    assert d.max() <= 1, f"{name}: displayed image vs oracle: max {int(d.max())} [{out['VPINFO']}]"
    inside = np.zeros((wh, ww), bool)
    inside[max(vr[1], 0):min(vr[3], wh), max(vr[0], 0):min(vr[2], ww)] = True
    assert not shown[~inside][:, :3].any(), "the letterbox area is black"
    # the snapshot: the frame at source-rect size into a B8G8R8X8 image (:3493-3608)
    snap = np.frombuffer((tmp_path / "snapshot.bin").read_bytes(), dtype=np.uint8).reshape(c["h"], c["w"], 4)
    cs = {k: v for k, v in c.items() if k not in ("window", "offset")}
    cs["dst"] = (c["w"], c["h"])
    ps = oracle_params(oracle, cs)
    want_s = oracle.process(ps, frame, pitch, dst=np.zeros((c["h"], c["w"], 4), dtype=np.uint8))
    ds = np.abs(snap[..., :3].astype(np.int16) - want_s[..., :3].astype(np.int16))
    assert ds.max() <= 1, f"{name}: snapshot vs oracle: max {int(ds.max())}"


def test_get_displayed_image_formats(mpcvr, oracle, torch_cuda):
    """mpcvr_get_displayed_image (GetDisplayedImage, DX11VideoProcessor.cpp:3610-3683) on a 10-bit back buffer: BGR32 = the top eight bits of
    each channel (ConvertR10G10B10A2toBGR32, Helper.cpp:805), BGR48 with deep colour = the ten bits in the top of each word (:836), rows
    CalcDibRowPitch apart; an 8-bit back buffer comes back as it is; before the first Render the call is refused."""
    from videorenderer_amd import api
    c = dict(GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"], output_format=1)
    vp, (ww, wh) = make_vp(mpcvr, c)
    with pytest.raises(api.MpcvrError):
        vp.GetDisplayedImage()
    frame, pitch = case_frame(c)
    vp.CopySample(torch_cuda.from_numpy(frame).cuda(), pitch)
    vp.Render()
    ptr, bp, bw, bh = vp.GetBackBuffer()
    assert (bw, bh, bp) == (ww, wh, ww * 4)
    raw = np.empty((wh, ww), dtype=np.uint32)
    import ctypes as C
    vp.Synchronize()
    assert C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(raw.ctypes.data), C.c_void_p(ptr), C.c_size_t(raw.nbytes), 2) == 0      # hipMemcpyDeviceToHost
    px32, w, h, bits = vp.GetDisplayedImage()
    assert (w, h, bits) == (ww, wh, 32)
    want32 = ((raw & 0x3fc00000) >> 22) | ((raw & 0x000ff000) >> 4) | ((raw & 0x000003fc) << 14) | 0xff000000
    assert np.array_equal(px32.view(np.uint32).reshape(wh, ww), want32)
    px48, w, h, bits = vp.GetDisplayedImage(deep_color=True)
    pitch48 = ((ww * 48 + 31) & ~31) // 8
    assert bits == 48 and px48.size == pitch48 * wh
    rows = px48.reshape(wh, pitch48)[:, :ww * 6].view(np.uint16).reshape(wh, ww, 3)
    assert np.array_equal(rows[..., 0], ((raw >> 20) & 1023) << 6) and np.array_equal(rows[..., 1], ((raw >> 10) & 1023) << 6) and np.array_equal(rows[..., 2], (raw & 1023) << 6)
    vp.close()


# fuzz case 6375 of the round-6 final fuzz run (profiles/r06/fuzz_8000_found_case_6375.txt): Dolby Vision MMR + level-2 trims + ProcAmp, same size —
# the plain tier differed from the oracle on 2 of 162 k ten-bit channels.  The per-pixel arithmetic was identical (test_dovi_tail_stage_by_stage);
# the ORACLE's colour-matrix constant was one ulp off the reference's expression (gcc dropped two float roundings of `c -= m * offset`, see
# tests/test_oracle_pins.py::test_dovi_colour_matrix_with_procamp_rounds_every_step); the product's host code had it right.
FUZZ_6375 = {'cformat': 2, 'w': 240, 'h': 444, 'kind': 'noise', 'seed': 598584363, 'exfmt': 2051155200, 'iChromaScaling': 1, 'iUpscaling': 1, 'iDownscaling': 3,
             'bInterpolateAt50pct': 0, 'src_rect': (92, 78, 240, 444), 'dst': (148, 366), 'procamp': (-5.010828386886953, 1.1960476848026689, 26.2518030673696, 0.8615709989981972),
             'dovi': {'kind': 'mmr', 'l2': (100, 600, 1000)}}


def test_fuzz_case_6375_dovi_l2_procamp_plain_tier_is_exact(mpcvr, oracle, torch_cuda):
    from videorenderer_amd import api
    for c in (FUZZ_6375, dict(FUZZ_6375, output_format=1, bUseDither=0), dict(FUZZ_6375, output_format=1, bUseDither=0, iChromaScaling=0)):
        frame, pitch = case_frame(c)
        p = oracle_params(oracle, c)
        want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
        plain, info = run_product(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FUSED)
        if c.get("output_format", 0) == 1:
            assert np.array_equal(_codes10(plain), _codes10(want)), info
        else:
            assert np.array_equal(plain[..., :3], want[..., :3]), info
        vp, _ = make_vp(mpcvr, c, api.FLAG_NO_FUSED)
        cm = np.array(vp.GetColorMatrix(), np.float32)
        vp.close()
        assert np.array_equal(cm.view(np.uint32), np.asarray(oracle.color_matrix(p), np.float32).view(np.uint32)), "colour matrix: product != oracle"


# soak case 2367 (profiles/r06/case2367.txt; MPCVR_FUZZ_JINC=1 MPCVR_FUZZ_FLAGS=8, seed 2102): HLG -> one-draw Jinc2m 2x -> HDR10 tone-mapping
# operator 6 -> R10G10B10A2.  The plain tier equals the oracle bit for bit; every other tier draws Jinc2m from its phase table (weights at the
# nominal phase, not at the interpolated texture coordinate: one code of the 10-bit post-scale texture on a few texels, its bar) and ONE such
# texel is a blue of 1 / 1023 where the oracle has 0 — which operator 6 turns into seven ten-bit codes.  The +-4 ulp pow() witness says
# nothing about that (no pow() moved): the channel is shown to lie inside what the oracle answers for the operator's input one code off.
FUZZ_2367 = {'cformat': 13, 'w': 290, 'h': 436, 'kind': 'noise', 'seed': 116969516, 'exfmt': 2185372928, 'iChromaScaling': 0, 'iUpscaling': 5, 'iDownscaling': 2,
             'bInterpolateAt50pct': 1, 'dst': (580, 872), 'iTexFormat': 10, 'hdr_output': 1, 'output_format': 1, 'hdr_tonemap': 6, 'hdr_display': 400.0,
             'hdr_meta': (0.005, 4000.0, 800.0, 200.0)}


def test_soak_case_2367_one_code_in_front_of_tonemap_operator_6(mpcvr, oracle, torch_cuda):
    from videorenderer_amd import api
    c = FUZZ_2367
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    plain, info = run_product(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FUSED)
    assert np.array_equal(_codes10(plain), _codes10(want)), info
    for flags in (0, api.FLAG_NO_FAST_CONVERT, api.FLAG_NO_LUT):
        got, info = run_product(mpcvr, torch_cuda, c, extra_flags=flags)
        d = np.abs(_codes10(got) - _codes10(want))
        assert int((d > 4).sum()) >= 1, "the case no longer shows what it was recorded for: tighten this test"
        # without the operator-input runs the witness must REFUSE the channel (no pow() explains it) ...
        with pytest.raises(AssertionError, match="NOT explained"):
            compare_behind_tail(oracle, p, frame, pitch, got, want, f"soak 2367, flags {flags}", min_same=0.97, ten_bit=True, lim=4, cap=1)
        # ... and with them it lies inside the interval; one channel of 1.5 M, as measured
        _, n = compare_behind_tail(oracle, p, frame, pitch, got, want, f"soak 2367, flags {flags}", min_same=0.97, ten_bit=True, lim=4, cap=1, operator_input=True)
        assert n == 1, (n, info)
    # the operator's input one code off moves the oracle's own answer by that much: the slope the bar has to live with
    up = oracle.process_with_tonemap_input_bias(p, frame, pitch, 1, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    assert int(np.abs(_codes10(up) - _codes10(want)).max()) >= 7


# soak case 3549 (profiles/r06/case3549.txt; default mode, seed 4006): HLG -> HDR10 output through tone-mapping operator 2, rotated 270.  One red
# channel of the default tier is 71 ten-bit codes from the plain tier's — and the ORACLE answers that channel 511 or 582 depending on +-4 ulp of
# pow(): the operator branches there.  The plain tier is the oracle's exact answer; the default tier's is the oracle's other one.
FUZZ_3549 = {'cformat': 24, 'w': 606, 'h': 258, 'kind': 'noise', 'seed': 476592806, 'exfmt': 2185372928, 'iChromaScaling': 2, 'iUpscaling': 4, 'iDownscaling': 5,
             'bInterpolateAt50pct': 0, 'dst': (123, 837), 'rotation': 270, 'hdr_output': 1, 'output_format': 1, 'hdr_tonemap': 2, 'hdr_display': 400.0,
             'hdr_meta': (0.005, 1000.0, 0.0, 200.0)}


def test_soak_case_3549_tonemap_operator_branch(mpcvr, oracle, torch_cuda):
    from videorenderer_amd import api
    c = FUZZ_3549
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    bg = lambda: np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8)
    want = oracle.process(p, frame, pitch, dst=bg())
    plain, info = run_product(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FUSED)
    assert np.array_equal(_codes10(plain), _codes10(want)), info
    got, info = run_product(mpcvr, torch_cuda, c)
    _, n = compare_behind_tail(oracle, p, frame, pitch, got, want, "soak 3549", min_same=0.97, ten_bit=True, lim=4, cap=1, operator_input=True)
    assert n <= 1, (n, info)
    # the oracle's own two answers at the channel the case was recorded for
    y, x, ch = 700, 34, 0
    seen = {int(_codes10(oracle.process_with_pow_bias(p, frame, pitch, b, dst=bg(), seed=sd))[y, x, ch]) for b, sd in [(-4, 0), (4, 0), (4, 1), (4, 2), (4, 3), (4, 4)]}
    assert int(_codes10(want)[y, x, ch]) == 511 and {511, 582} <= seen | {511}, seen
    assert int(_codes10(got)[y, x, ch]) in seen | {511}


# soak case 5624 (profiles/r06/cases_5624_1428.txt; default mode, seed 5001): PQ -> HDR10 passthrough (no transcendental anywhere in the plan),
# Bicubic downscale across + Mitchell upscale along a frame rotated by 270: two vertically adjacent red channels 7 ten-bit codes from the plain
# tier.  The block convert's texture differs from the oracle's in 24 texels of 151 k, by one code each (its bar) — and the reference's Bicubic
# downscale at that output column turns one code into ten (the ORACLE moves by 17 for one code of one luma sample there).
FUZZ_5624 = {'cformat': 3, 'w': 574, 'h': 264, 'kind': 'noise', 'seed': 931924931, 'exfmt': 2051155200, 'iChromaScaling': 1, 'iUpscaling': 1, 'iDownscaling': 3,
             'bInterpolateAt50pct': 0, 'dst': (125, 1378), 'rotation': 270, 'hdr_output': 1, 'output_format': 1, 'hdr_tonemap': 0, 'hdr_display': 400.0,
             'hdr_meta': (0.005, 4000.0, 800.0, 0.0)}


def test_soak_case_5624_one_convert_code_in_front_of_a_bicubic_downscale(mpcvr, oracle, torch_cuda):
    from videorenderer_amd import api
    c = FUZZ_5624
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    bg = lambda: np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8)
    want = oracle.process(p, frame, pitch, dst=bg())
    for flags in (api.FLAG_NO_FUSED, api.FLAG_NO_FAST_CONVERT):          # the per-pixel convert kernel: the oracle's bits all the way
        plain, info = run_product(mpcvr, torch_cuda, c, extra_flags=flags)
        assert np.array_equal(_codes10(plain), _codes10(want)), info
    # the convert texture itself (a rotated copy draw shows it): within one code everywhere
    same = dict(c, dst=(c["h"], c["w"]))
    ps = oracle_params(oracle, same)
    ws = oracle.process(ps, frame, pitch, dst=np.full((ps.window_h, ps.window_w, 4), BG, dtype=np.uint8))
    gs, _ = run_product(mpcvr, torch_cuda, same)
    assert int(np.abs(_codes10(gs) - _codes10(ws)).max()) <= 1
    got, info = run_product(mpcvr, torch_cuda, c)
    with pytest.raises(AssertionError, match="NOT explained"):
        compare_behind_tail(oracle, p, frame, pitch, got, want, "soak 5624", min_same=0.97, ten_bit=True, lim=2, cap=2)
    _, n = compare_behind_tail(oracle, p, frame, pitch, got, want, "soak 5624", min_same=0.97, ten_bit=True, lim=2, cap=2, convert_output=True)
    assert n == 2, (n, info)
    # the oracle's own sensitivity there: one code of one luma sample
    f2 = frame.copy()
    Y = f2[:c["w"] * c["h"] * 2].view(np.uint16).reshape(c["h"], c["w"])
    Y[199, 543] = np.uint16(int(Y[199, 543]) + 64)
    moved = oracle.process(p, f2, pitch, dst=bg())
    assert int(np.abs(_codes10(moved) - _codes10(want)).max()) >= 10


# soak case 1428 (profiles/r06/case1428.txt; Jinc2m mode, seed 5102): Dolby Vision (polynomial curves) + level-2 trims + ProcAmp (contrast 1.18,
# brightness -4) -> Jinc2m 2x -> 8-bit target.  The block convert's table variant leaves 5 of 233 k channels beyond one code, and two of them — the
# blue of two saturated yellows, 6 and 16 where the oracle has 0 and 8 — lie outside the +-4 ulp interval.  Cause, by elimination (experiment
# builds): the PQ EOTF TABLE — with the EOTF evaluated literally (-DMPCVR_DV_EXP=1) the frame is within one code; the over-range codes, the trimmed
# codes above 1.0 and the PQ-encode table were built out and change nothing.  The table is accurate to 1.2e-6 (its tested property) = ten ulps of a
# pow(), and at these channels the ORACLE spans 0 .. 17 and 7 .. 30 under +-8 ulp: the table tier is inside the interval of its own accuracy and
# outside the suite's +-4.  Both statements are asserted below.
FUZZ_1428 = {'cformat': 2, 'w': 90, 'h': 216, 'kind': 'noise', 'seed': 897013636, 'exfmt': 2051155200, 'iChromaScaling': 0, 'iUpscaling': 5, 'iDownscaling': 3,
             'bInterpolateAt50pct': 0, 'dst': (180, 432), 'window': (171, 432), 'offset': (15, 20),
             'procamp': (-3.9689549383766405, 1.1823064992043373, -6.779328347755538, 1.053739126351976), 'dovi': {'kind': 'poly', 'l2': (100, 600, 1000)}}


def test_soak_case_1428_plain_and_per_pixel_tiers(mpcvr, oracle, torch_cuda):
    from videorenderer_amd import api
    c = FUZZ_1428
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    plain, info = run_product(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FUSED)
    assert np.array_equal(plain[..., :3], want[..., :3]), info
    for flags in (api.FLAG_NO_LUT, api.FLAG_NO_FAST_CONVERT):
        got, info = run_product(mpcvr, torch_cuda, c, extra_flags=flags)
        assert int(np.abs(got[..., :3].astype(int) - want[..., :3].astype(int)).max()) <= 1, info
    # the default tier as recorded: a handful of channels, none further than 8 codes (a regression beyond that fails here)
    got, info = run_product(mpcvr, torch_cuda, c)
    d = np.abs(got[..., :3].astype(int) - want[..., :3].astype(int))
    assert int((d > 1).sum()) <= 8 and int(d.max()) <= 8, (int((d > 1).sum()), int(d.max()), info)


def test_soak_case_1428_default_tier_inside_the_eotf_tables_own_accuracy(mpcvr, oracle, torch_cuda):
    c = FUZZ_1428
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    got, info = run_product(mpcvr, torch_cuda, c)
    with pytest.raises(AssertionError, match="NOT explained"):         # the suite's +-4 ulp witness refuses two of the channels
        compare_behind_tail(oracle, p, frame, pitch, got, want, "soak 1428", min_same=0.97, lim=1, cap=8, convert_output=True)
    _, n = compare_behind_tail(oracle, p, frame, pitch, got, want, "soak 1428", min_same=0.97, lim=1, cap=8, convert_output=True, pow_ulps=POW_ULPS_EOTF_TABLE)
    assert n <= 8, (n, info)


# soak5 case 4319 (profiles/r06/case4319.txt; left-out-scalers mode, seed 6701) — RECORDED STATE, not a bar: Dolby Vision MMR + ProcAmp (contrast 1.17,
# saturation 1.44), 8-bit internal format, nearest 1.7x, 10-bit target, noise.  The plain tier is the oracle's bits; the table tier (the PQ EOTF out of
# its LDS table: a 14 % faster Dolby Vision convert) leaves 17 of 1.5 M channels beyond five ten-bit codes (max 16; 20 with contrast 1.0), four of them
# outside even the +-10 ulp interval — at channels the oracle itself spans 128 .. 168 on.  The test pins the plain tier and fences the recorded figures.
FUZZ_4319 = {'cformat': 3, 'w': 598, 'h': 288, 'kind': 'noise', 'seed': 546315119, 'exfmt': 2051155200, 'iChromaScaling': 0, 'iUpscaling': 0, 'iDownscaling': 2,
             'bInterpolateAt50pct': 1, 'dst': (1027, 495), 'output_format': 1, 'iTexFormat': 8,
             'procamp': (-3.8196396258474365, 1.1730855112312484, -6.805298891179945, 1.4386824544891605), 'dovi': {'kind': 'mmr', 'l2': ()}}


def test_soak_case_4319_plain_tier_exact_table_tier_as_recorded(mpcvr, oracle, torch_cuda):
    from videorenderer_amd import api
    c = FUZZ_4319
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = _codes10(oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8)))
    plain, info = run_product(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FUSED)
    assert np.array_equal(_codes10(plain), want), info
    got, info = run_product(mpcvr, torch_cuda, c)
    d = np.abs(_codes10(got) - want)
    assert float((d == 0).mean()) >= 0.998 and int((d > 5).sum()) <= 34 and int(d.max()) <= 24, (float((d == 0).mean()), int((d > 5).sum()), int(d.max()), info)


def test_dovi_tail_stage_by_stage(mpcvr, oracle, torch_cuda):
    """The plain tier's Dolby Vision tail (mpcvr_eval_dovi_tail: k_eval_dovi_tail is compiled in the plain kernels' translation unit) against the
    oracle's, cut off after each of its six stages — PQ EOTF -> LMS -> PQ OETF; saturate + level-2 trims; ST2084ToLinear * scale; Hable; 2020 -> 709;
    pow 1/2.2 — on 300 k random PQ-coded triples (some outside 0..1) per metadata kind: bit for bit, NaNs in the same places."""
    import ctypes as C
    from videorenderer_amd import api, synth
    torch = torch_cuda
    L = api.load_library()
    rng = np.random.default_rng(11)
    n = 200_000
    rgb = np.concatenate([rng.uniform(0, 1, (n, 3)), rng.uniform(-0.05, 1.2, (n // 4, 3)), rng.uniform(0, 0.1, (n // 4, 3))]).astype(np.float32)
    fp = C.POINTER(C.c_float)
    d_in = torch.from_numpy(rgb).cuda()
    for kind, l2 in (("mmr", (100, 600, 1000)), ("poly", ())):
        pd = api.plan_dovi(synth.dovi_metadata(kind, l2=l2), 1000)
        lms, k = np.ascontiguousarray(pd["lms"], np.float32), np.ascontiguousarray(pd["l2k"], np.float32)
        for stage in range(6):
            d_out = torch.empty_like(d_in)
            assert L.mpcvr_eval_dovi_tail(stage, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()), rgb.shape[0], lms.ctypes.data_as(fp), k.ctypes.data_as(fp),
                                          int(pd["l2_enabled"]), 80.0, None) == 0
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            want = np.empty_like(rgb)
            oracle.lib().orc_eval_dovi_tail(stage, rgb.ctypes.data, want.ctypes.data, rgb.shape[0], lms.ctypes.data_as(fp), k.ctypes.data_as(fp), int(pd["l2_enabled"]), 80.0)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), (kind, stage)
            bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
            assert not bad.any(), f"{kind} stage {stage}: {int(bad.sum())} values differ, e.g. in {rgb[np.argwhere(bad)[0][0]].tolist()}"


def test_fused_jinc_steps_aside_where_the_device_grants_less_lds(mpcvr, torch_cuda):
    """The fused Jinc2m kernel claims 114 - 146 KiB of LDS per workgroup; UpdatePlan compares that with what the device grants and keeps the
    convert + k_jinc2 draws otherwise (advisor, round 5: the launch failed on every frame of such a plan).  MPCVR_LDS_LIMIT plans as if this
    MI355X granted 64 KiB (the limit is cached per process: a child process), and the frame still equals the default plan's to one code."""
    import subprocess
    import sys
    root = os.path.dirname(HERE)
    code = (
        "import sys, numpy as np, torch\n"
        "sys.path.insert(0, %r)\n"
        "from videorenderer_amd import api\n"
        "from tests.golden.cases import GOLDEN_CASES\n"
        "from tests.test_parity_gpu import run_product\n"
        "c = GOLDEN_CASES['jinc2_p010_2x_dither']\n"
        "got, info = run_product(api, torch, c)\n"
        "np.save(sys.argv[1], got)\n"
        "print('INFO', info)\n" % root)
    import tempfile
    outs = {}
    for limit in ("", "65536"):
        with tempfile.TemporaryDirectory() as d:
            env = dict(os.environ)
            env.pop("MPCVR_LDS_LIMIT", None)
            if limit:
                env["MPCVR_LDS_LIMIT"] = limit
            r = subprocess.run([sys.executable, "-c", code, os.path.join(d, "o.npy")], capture_output=True, text=True, timeout=600, env=env, cwd=root)
            assert r.returncode == 0, r.stderr[-2000:]
            info = [l for l in r.stdout.splitlines() if l.startswith("INFO")][0][5:]
            outs[limit] = (np.load(os.path.join(d, "o.npy")), info)
    assert outs[""][1] == "fused_jinc2x", outs[""][1]
    assert outs["65536"][1].startswith("passes:convert,resizeX"), outs["65536"][1]
    d = np.abs(outs[""][0].astype(np.int16) - outs["65536"][0].astype(np.int16))
    assert d.max() <= 1, int(d.max())


# ---- round 6: the shader transcendentals as DEFINED functions (csrc/vp_crmath.h, oracle/crmath.h, tests/test_crmath.py) ---------------
def test_defined_transcendentals_device_equals_host(mpcvr, oracle, torch_cuda):
    """log2f / exp2f / expf / pow / sinf / cosf of the plain tier evaluated ON THE GPU (fp64 there) == the oracle's CPU evaluation of the same definition,
    bit for bit, on 4 M arguments per function: every binade, the neighbourhood of 1, [0, 1], subnormals, infinities, NaN, and pow with the
    exponents of the PQ / HLG / gamma chains.  This is what lets the pass-per-kernel tier be held to the oracle bit for bit behind a tail."""
    import ctypes as C
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    rng = np.random.default_rng(2026)
    n = 1_000_000
    pos = rng.integers(1, 0x7f800000, n, dtype=np.uint32).view(np.float32)
    x = np.concatenate([pos, (1 + rng.uniform(-0.3, 0.42, n)).astype(np.float32), rng.uniform(0, 1, 2 * n).astype(np.float32),
                        np.arange(0, 65536, dtype=np.uint32).view(np.float32), np.float32(2.0) ** np.arange(-149, 128).astype(np.float32),
                        np.array([0.0, -0.0, -1.0, np.inf, -np.inf, np.nan], np.float32)]).astype(np.float32)
    t = np.concatenate([rng.uniform(-152, 129, n), rng.uniform(-1, 1, n), rng.uniform(-40, 4, 2 * n), np.arange(-152, 130, 0.25),
                        np.array([np.inf, -np.inf, np.nan, 1e9, -1e9], np.float32)]).astype(np.float32)
    y = rng.choice(np.array([1 / 2.2, 2.2, 2.4, 0.2, 2610 / 16384, 2523 / 32, 32 / 2523, 16384 / 2610, 1.961, 0.1, 1.0], np.float32), x.size).astype(np.float32)
    sc = np.concatenate([rng.uniform(-12, 12, 2 * n), rng.uniform(-1e5, 1e5, n // 2), np.arange(-4000, 4001) * (np.pi / 2),
                         np.array([0.0, -0.0, np.inf, -np.inf, np.nan])]).astype(np.float32)
    for fn, name, a, b in ((0, "log2", x, None), (1, "exp2", t, None), (2, "exp", t, None), (3, "pow", x, y), (4, "sin", sc, None), (5, "cos", sc, None)):
        da = torch.from_numpy(a).cuda()
        db = torch.from_numpy(b).cuda() if b is not None else da
        out = torch.empty_like(da)
        assert L.mpcvr_eval_transcendental(fn, C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()), C.c_void_p(out.data_ptr()), a.size, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        with np.errstate(all="ignore"):
            want = oracle.eval_transcendental(name, a, b)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), name
        diff = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
        assert not diff.any(), f"{name}: {int(diff.sum())} of {a.size} differ, e.g. x = {a[diff][0]!r}: device {got[diff][0]!r}, host {want[diff][0]!r}"


# fuzz case 1820 of profiles/r05/fuzz_2500_jinc_flags64.txt (seed 612561346) — the run that ended rc = 1 in round 5: Dolby Vision (MMR)
# P016 184 x 166, source rect (76, 36, 184, 166) -> 216 x 260 in a 236 x 284 window at (5, 19), two-draw Jinc2m, 10-bit target.  One texel of
# m_TexConvertOutput is a bright saturated colour whose red cancels behind the 2020 -> 709 row: the oracle says code 28, its +-4 ulp pow()
# runs 0 .. 28, the plain convert kernel said 33 — v_log_f32 / v_exp_f32 are good to an ulp each, and behind pow(x, 1/m1 = 6.28) one ulp of
# log2 is ~35 ulp of the result: the +-4 ulp witness was never a bound for that kernel — and the Jinc2m draw's anti-ringing clamp carried
# the five codes to the output as six (got 224, oracle 218, interval [181, 218]).  Round 6: the plain tier evaluates the transcendentals
# as the oracle defines them (correctly rounded steps), so it carries the oracle's code in every texel, this one included.
FUZZ_1820 = {'cformat': 3, 'w': 184, 'h': 166, 'kind': 'noise', 'seed': 612561346, 'exfmt': 2051155200, 'iChromaScaling': 0, 'iUpscaling': 5,
             'iDownscaling': 1, 'bInterpolateAt50pct': 0, 'src_rect': (76, 36, 184, 166), 'dst': (216, 260), 'window': (236, 284), 'offset': (5, 19),
             'output_format': 1, 'dovi': {'kind': 'mmr', 'l2': ()}}


def test_fuzz_case_1820_dovi_mmr_two_draw_jinc2m_10bit(mpcvr, oracle, torch_cuda):
    from videorenderer_amd import api
    c = FUZZ_1820
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    plain, info = run_product(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FUSED)
    assert info.startswith("passes:convert,resizeX"), info
    d = np.abs(_codes10(plain) - _codes10(want))
    assert d.max() == 0, f"plain tier [{info}]: {int((d > 0).sum())} channels differ from the oracle (max {int(d.max())}), e.g. {tuple(np.argwhere(d > 0)[0])}"
    assert _codes10(plain)[231, 107, 0] == _codes10(want)[231, 107, 0] == 218
    # the convert texel itself (the same source rect at 1:1 into a 10-bit target, no dither = m_TexConvertOutput's codes): the oracle's 28
    cs = {k: v for k, v in c.items() if k not in ("window", "offset")}
    cs.update(dst=(108, 130), bUseDither=0, iUpscaling=2)
    tex, info_t = run_product(mpcvr, torch_cuda, cs, extra_flags=api.FLAG_NO_FUSED)
    ps = oracle_params(oracle, cs)
    want_t = oracle.process(ps, frame, pitch, dst=np.full((ps.window_h, ps.window_w, 4), BG, dtype=np.uint8))
    assert np.array_equal(_codes10(tex), _codes10(want_t)), info_t
    assert _codes10(tex)[106, 51, 0] == 28
    # the default planner (block convert: PQ decoded from tables) against the bar of the fuzz tool: 4 ten-bit codes behind Dolby Vision
    got, info_d = run_product(mpcvr, torch_cuda, c)
    compare_behind_tail(oracle, p, frame, pitch, got, want, f"fuzz 1820 [{info_d}]", min_same=0.97, ten_bit=True, lim=4, cap=1)


def _is_exact_2x(c):
    if c.get("rotation", 0) in (90, 270):
        return False
    r = c.get("src_rect", (0, 0, c["w"], c["h"]))
    return c["dst"] == (2 * (r[2] - r[0]), 2 * (r[3] - r[1]))


FUSED = sorted(n for n, c in GOLDEN_CASES.items() if _is_exact_2x(c))


@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_default_path_vs_oracle(mpcvr, oracle, torch_cuda, name):
    """Default settings: whatever the planner picks — the fused 2x kernel where eligible, else the folded convert /
    row-tap / column-tap kernels, else the plain ones.  The folded kernels keep the plain kernels' arithmetic, so
    everything that does not run the fused kernel or a transcendental tail stays bit-exact."""
    c = GOLDEN_CASES[name]
    want = run_case(oracle, name, background=BG)
    for layout, (got, info) in run_layouts(mpcvr, torch_cuda, c, what=name).items():
        # 4:2:0 sources may go through the fused kernel or its block convert (FMA contraction, scale folded into the matrix)
        if c.get("output_format", 0) == 1:
            compare_rgb10(got, want, f"{name} <{layout}>", tail=has_tail(c), internal8=internal_is_8bit(c))
        else:
            compare(got, want, f"{name} <{layout}> [{info}]", min_same=0.99)


@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_folded_kernels_vs_oracle(mpcvr, oracle, torch_cuda, name):
    """MPCVR_FLAG_NO_FAST_CONVERT takes the fused kernel and its block convert out of the default planner: what runs are the
    compile-time-folded convert / row-tap / column-tap kernels (or the plain ones where no folded variant exists).  They
    keep the plain kernels' arithmetic, so everything without a transcendental tail stays bit-exact."""
    from videorenderer_amd import api
    c = GOLDEN_CASES[name]
    want = run_case(oracle, name, background=BG)
    got, info = run_product(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FAST_CONVERT)
    assert info != "fused_up2x"
    # (behind a tail the folded convert — built with the fused tiers' v_log_f32 / v_exp_f32 — keeps the fused tiers' bar; the plain tier
    # alone evaluates the transcendentals as the oracle defines them and is exact there too: test_pass_per_kernel_path_vs_oracle)
    if c.get("output_format", 0) == 1:
        compare_rgb10(got, want, name, exact=not has_tail(c))
    elif has_tail(c):
        compare(got, want, f"{name} [{info}]", min_same=0.99)
    else:
        compare(got, want, f"{name} [{info}]", exact=True)


# ---- round 4: the table-driven kernel families swept through their template-argument space -----------------------------------------
# k_resize_rows / k_resize_cols / k_resize_2d are instantiated per (tap count: 4, 6, run-time) x (format of the texture they read: 8-bit,
# 10-bit, fp16) x (epilogue: surface store / final pass into either swap chain format); k_convert_420 per (planes, bytes, tail, output
# format, destination).  The golden cases reach a third of them; this sweep walks the settings that select the rest — internal
# format x filter x swap chain x dither x source layout — through the tiers that use those kernels (MPCVR_FLAG_NO_STRIP: block convert +
# tiled two-draw kernel; MPCVR_FLAG_NO_FAST_CONVERT: folded per-pixel convert + folded row / column kernels), each against the oracle.
def _sweep_cases():
    """(label, case, tier flag name): every source layout the specialised loaders know x every tail x the internal formats x filters of
    4 / 6 / 8 / 16 taps x two-pass, one-axis and same-size geometries x both swap chain formats x dither x aligned / odd window offsets,
    thinned deterministically to a few hundred cases (every value of every dimension appears many times; P010 runs the full product of
    the dimensions the resize kernels are instantiated over)."""
    fmts = ((2, "p010"), (1, "nv12"), (20, "yuv420p10"), (14, "yv12"), (4, "yuy2"), (30, "rgb32"), (32, "r210"))
    tails = ("HDR10", "SDR", "HLG", "BT2020SDR")
    geos = (("up_mitchell", dict(iUpscaling=1, dst=(90, 66))), ("up_lanczos3", dict(iUpscaling=4, dst=(90, 66))),
            ("down_hamming8", dict(iDownscaling=2, dst=(24, 18))), ("down_bicubic16", dict(iDownscaling=3, dst=(28, 20))),
            ("x_only", dict(iUpscaling=4, dst=(90, 48))), ("y_only", dict(iUpscaling=1, dst=(64, 66))), ("y_only_down", dict(iDownscaling=2, dst=(64, 18))),
            ("same_size", dict(dst=(64, 48))), ("jinc_2x", dict(iUpscaling=5, dst=(128, 96))),
            # one-axis draws with the other filters, and two-pass geometries the tiled two-draw kernel does not take (a 3x downscale along
            # one axis outgrows its LDS windows): the folded column kernel filling m_TexResize and the row kernel reading it
            ("y_only_lanczos3", dict(iUpscaling=4, dst=(64, 66))), ("x_only_mitchell", dict(iUpscaling=1, dst=(90, 48))), ("x_only_down", dict(iDownscaling=2, dst=(24, 48))),
            ("x_up_mitchell_y_down3", dict(iUpscaling=1, iDownscaling=2, dst=(90, 16))), ("x_up_lanczos3_y_down3", dict(iUpscaling=4, iDownscaling=2, dst=(90, 16))),
            ("x_down3_y_up_lanczos3", dict(w=640, iUpscaling=4, iDownscaling=2, dst=(200, 66))), ("x_down3_y_up_mitchell", dict(w=640, iUpscaling=1, iDownscaling=2, dst=(200, 66))))
    tiers = ("DEFAULT", "FLAG_NO_LUT", "FLAG_NO_STRIP", "FLAG_NO_FAST_CONVERT", "NO_STRIP_NO_FAST_CONVERT")
    out = []
    k = 0
    for cf, fname in fmts:
        for tail in tails:
            if cf in (1, 14, 4, 30, 32) and tail != "SDR" and not (cf == 1 and tail == "HDR10"):      # 8-bit / RGB sources: SDR (and one 8-bit PQ stream)
                continue
            for itex in (8, 10, 16):
                for gname, g in geos:
                    # Jinc2m's 16 weights sum to |w| = 1.9 (negative ring): ONE code of difference in the texture it reads comes out as up
                    # to two.  Behind a PQ / HLG tail an 8-bit internal format (a setting AUTO never picks for such sources) holds such
                    # codes on every tier — the oracle's own +-4 ulp pow() runs differ there — so that corner is not swept; the 10-bit
                    # internal formats keep the same effect below half an 8-bit code (and within 2 ten-bit codes, see the test)
                    if gname == "jinc_2x" and itex == 8 and tail in ("HDR10", "HLG"):
                        continue
                    for outfmt in (0, 1):
                        for dither in (1, 0):
                            for off in ((0, 0), (3, 1)):
                                for tier in tiers:
                                    k += 1
                                    full = cf == 2 and tail == "HDR10" and off == (0, 0) and tier in ("FLAG_NO_STRIP", "NO_STRIP_NO_FAST_CONVERT")
                                    # interleaved RGB feeds the resize kernels its own texture format whatever the internal format is: the
                                    # (texture format, epilogue) pairs no YUV source produces
                                    full = full or (cf in (30, 32) and off == (0, 0) and tier == "FLAG_NO_STRIP" and gname != "jinc_2x")
                                    # the one-draw Jinc2m quad kernel: internal format x epilogue (integer final pass, straight store, generic)
                                    full = full or (gname == "jinc_2x" and tier == "DEFAULT" and ((cf == 2 and tail == "HDR10") or (cf == 1 and tail == "SDR")))
                                    if not full and (k * 2654435761 >> 7) % 23:
                                        continue
                                    c = dict(dict(cformat=cf, w=64, h=48, kind="noise", seed=7000 + k % 997, exfmt_name=tail, iTexFormat=itex, output_format=outfmt,
                                                  bUseDither=dither), **g)
                                    if off != (0, 0):
                                        c.update(window=(c["dst"][0] + 8, c["dst"][1] + 4), offset=off)
                                    out.append((f"{fname}_{tail}_tex{itex}_{gname}_out{outfmt}_d{dither}_off{off[0]}_{tier}", c, tier))
    # the strip kernel family in full: source loader x tail x tap count x epilogue (k_fused_strip<NT, PXL, TAIL, SRC, EPI>; PXL is the
    # planner's choice, steered here by the ratio: a 1.7x interpolated downscale and the 16-tap filters run one pixel per lane)
    strip_geos = (("s_up_mitchell", dict(iUpscaling=1, dst=(90, 66))), ("s_up_lanczos3fix", dict(iUpscaling=4, flags=1, dst=(90, 66))),
                  ("s_down17_mitchell", dict(iUpscaling=1, bInterpolateAt50pct=1, dst=(38, 28))), ("s_down17_lanczos3fix", dict(iUpscaling=4, flags=1, bInterpolateAt50pct=1, dst=(38, 28))),
                  ("s_down_hamming8", dict(iDownscaling=2, dst=(24, 18))), ("s_down_bicubic16", dict(iDownscaling=3, dst=(28, 20))))
    epis = (("dither8", dict(iTexFormat=10, output_format=0, bUseDither=1)), ("direct", dict(iTexFormat=0, bUseDither=0)),
            ("generic", dict(iTexFormat=10, output_format=0, bUseDither=1, offset=(3, 1))),
            # a video rectangle the window clips on every side: the per-pixel store_epilogue variant of every loader x tail x tap count
            ("clipped", dict(iTexFormat=10, output_format=0, bUseDither=1, clip=1)),
            # ... and behind an 8-bit internal format: the exact-form twins of the 8-bit and the run-time loader with that epilogue
            ("clipped8", dict(iTexFormat=0, bUseDither=0, clip=1)))
    for cf, fname in fmts:
        for tail in tails:
            if cf in (30, 32) and tail != "SDR":
                continue
            for gname, g in strip_geos:
                for ename, e in epis:
                    if ename == "clipped8" and not (cf in (1, 14, 4) and tail == "SDR"):
                        continue
                    for tier in ("DEFAULT", "FLAG_NO_LUT"):
                        if tier == "FLAG_NO_LUT" and tail in ("SDR", "BT2020SDR"):
                            continue
                        k += 1
                        c = dict(dict(cformat=cf, w=64, h=48, kind="noise", seed=9000 + k % 997, exfmt_name=tail, output_format=1 if (ename == "direct" and cf in (2, 20, 32)) else 0), **g)
                        c.update(e)
                        if ename == "direct" and cf in (2, 20, 32):
                            c["output_format"] = 1           # a 10-bit source into a 10-bit swap chain: the straight R10G10B10A2 store
                        if c.pop("clip", 0):
                            c.update(window=(c["dst"][0] - 10, c["dst"][1] - 6), offset=(-4, -2))
                        elif "offset" in c:
                            c["window"] = (c["dst"][0] + 8, c["dst"][1] + 4)
                        flags = c.pop("flags", 0)
                        if flags:
                            c["flags"] = flags
                        out.append((f"strip_{fname}_{tail}_{gname}_{ename}_{tier}", c, tier))
    # the convert kernels in full.  Same-size frames, bi-planar ones 66 columns wide (not a multiple of 4: the streaming kernel declines, the
    # 2x2-block kernel k_convert_blocks<TAIL, SRC, FINAL, DV, CHR> runs; three planes need 4-byte aligned chroma rows: 72): loader (P010 with centred chroma = the run-time variant) x tail x
    # bilinear / Catmull-Rom chroma x with / without the final pass; Dolby Vision: the three variants x both loaders x final pass
    conv_fmts = ((2, "p010", {}), (1, "nv12", {}), (20, "yuv420p10", dict(w=72, dst=(72, 48))), (14, "yv12", dict(w=72, dst=(72, 48))), (2, "p010centred", dict(chroma_loc=1)))
    for cf, fname, extra in conv_fmts:
        for tail in tails:
            if cf in (1, 14) and tail != "SDR" and not (cf == 1 and tail == "HDR10"):
                continue
            for chroma in (1, 2):
                for fin in (1, 0):
                    k += 1
                    c = dict(dict(cformat=cf, w=66, h=48, kind="noise", seed=11000 + k % 997, exfmt_name=tail, dst=(66, 48), iChromaScaling=chroma,
                                  iTexFormat=10 if fin else 0, output_format=0 if fin or cf in (1, 14) else 1, bUseDither=fin), **extra)
                    out.append((f"blocks_{fname}_{tail}_chroma{chroma}_final{fin}_DEFAULT", c, "DEFAULT"))
    dv_kinds = (("sdr", dict(dovi=dict(kind="poly"))), ("sdr_l2", dict(dovi=dict(kind="mixed", l2=(100, 600, 1000)), hdr_display=400.0)),
                ("hlg_tagged", dict(dovi=dict(kind="identity"), exfmt_name="HLG")), ("hdr_out", dict(dovi=dict(kind="mmr"), hdr_output=1)),
                ("no_sdr_convert", dict(dovi=dict(kind="poly"), bConvertToSdr=0)))
    for cf, fname in ((2, "p010"), (20, "yuv420p10")):
        for dname, dv in dv_kinds:
            for fin in (1, 0):
                k += 1
                ho = dv.get("hdr_output", 0)
                wd = 66 if cf == 2 else 72
                c = dict(dict(cformat=cf, w=wd, h=48, kind="hdr", seed=12000 + k % 997, exfmt_name="TVONLY", dst=(wd, 48), iTexFormat=(16 if ho else 10) if fin else 0,
                              output_format=1 if ho else (0 if fin else 1), bUseDither=fin), **dv)
                out.append((f"blocks_dovi_{fname}_{dname}_final{fin}_DEFAULT", c, "DEFAULT"))
    # the folded per-pixel convert k_convert_420<PLANES, BYTES, TAIL, OFMT, DMODE, DFMT, DV> (MPCVR_FLAG_NO_FAST_CONVERT): loader x tail x
    # internal format x {a resize behind it, the final pass folded in, a straight copy folded in}
    folded = (("resize", dict(iUpscaling=1, dst=(90, 66))), ("final8", dict(dst=(64, 48), output_format=0, bUseDither=1)),
              ("copy8", dict(dst=(64, 48), output_format=0, bUseDither=0)), ("out10", dict(dst=(64, 48), output_format=1, bUseDither=1)))
    for cf, fname in fmts[:4]:
        for tail in tails:
            if cf in (1, 14) and tail != "SDR":
                continue
            for itex in (8, 10, 16):
                for gname, g in folded:
                    k += 1
                    c = dict(dict(cformat=cf, w=64, h=48, kind="noise", seed=13000 + k % 997, exfmt_name=tail, iTexFormat=itex, output_format=0, bUseDither=1), **g)
                    out.append((f"folded_{fname}_{tail}_tex{itex}_{gname}_NO_STRIP_NO_FAST_CONVERT", c, "NO_STRIP_NO_FAST_CONVERT"))
    for cf, fname in ((2, "p010"), (20, "yuv420p10")):
        for dname, dv in (dv_kinds[0], dv_kinds[3], dv_kinds[4]):
            for itex in (8, 10, 16):
                for gname, g in folded:
                    if dv.get("hdr_output") and g.get("output_format", 0) == 0 and gname != "resize":
                        continue                # (an HDR passthrough goes to a 10-bit swap chain)
                    k += 1
                    c = dict(dict(cformat=cf, w=64, h=48, kind="hdr", seed=14000 + k % 997, exfmt_name="TVONLY", iTexFormat=itex, output_format=0, bUseDither=1), **g)
                    c.update(dv)
                    if dv.get("hdr_output"):
                        c["output_format"] = 1
                    out.append((f"folded_dovi_{fname}_{dname}_tex{itex}_{gname}_NO_STRIP_NO_FAST_CONVERT", c, "NO_STRIP_NO_FAST_CONVERT"))
    # the folded column kernel as the FIRST of two draws (it fills m_TexResize) from every texture format: 32 output rows of a 6x downscale
    # along Y read more source rows than the tiled two-draw kernel keeps (kResizeTileRowsMax); and the one-draw Jinc2m from an 8-bit RGB texture into a 10-bit post-scale one
    for gname, g in (("x_up_mitchell_y_down6", dict(h=192, iUpscaling=1, iDownscaling=2, dst=(90, 32))), ("x_up_lanczos3_y_down6", dict(h=192, iUpscaling=4, iDownscaling=2, dst=(90, 32))),
                     ("x_down2p5_y_down6", dict(w=500, h=192, iDownscaling=2, dst=(200, 32))),
                     ("x_down2p5_lanczos15_y_down6", dict(w=500, h=192, iDownscaling=5, dst=(200, 32)))):
        for cf, fname, tail in ((2, "p010", "HDR10"), (30, "rgb32", "SDR")):
            for itex in (8, 10, 16):
                k += 1
                c = dict(dict(cformat=cf, w=64, h=48, kind="noise", seed=15000 + k % 997, exfmt_name=tail, iTexFormat=itex, output_format=0, bUseDither=1), **g)
                out.append((f"cols_{fname}_{tail}_tex{itex}_{gname}_FLAG_NO_STRIP", c, "FLAG_NO_STRIP"))
    for cf, fname in ((30, "rgb32"), (32, "r210")):
        k += 1
        out.append((f"jinc_{fname}_tex10_final_DEFAULT", dict(cformat=cf, w=64, h=48, kind="noise", seed=16000 + k, exfmt_name="SDR", iTexFormat=10, output_format=0,
                                                          bUseDither=1, iUpscaling=5, dst=(128, 96)), "DEFAULT"))
    return out


SWEEP = _sweep_cases()


@pytest.mark.parametrize("label", [n for n, _, _ in SWEEP])
def test_kernel_family_sweep_vs_oracle(mpcvr, oracle, torch_cuda, label):
    from videorenderer_amd import api
    from tests.golden import cases as G
    c, tier = next((dict(c), t) for n, c, t in SWEEP if n == label)
    ex = c.pop("exfmt_name")
    c["exfmt"] = {"HDR10": G.HDR10, "HLG": G.HLG, "SDR": G.ext(matrix=G.M709), "BT2020SDR": G.ext(G.MPEG2, G.TV, G.M2020, G.P2020, G.T709),
                  "TVONLY": G.ext(G.MPEG2, G.TV)}[ex]
    if "chroma_loc" in c:           # (the chroma siting field of DXVA2_ExtendedFormat: bits 8..11)
        c["exfmt"] = (c["exfmt"] & ~(0xf << 8)) | (c.pop("chroma_loc") << 8)
    if c["cformat"] in (30, 32):
        c["exfmt"] = 0
    flags = {"DEFAULT": 0, "NO_STRIP_NO_FAST_CONVERT": api.FLAG_NO_STRIP | api.FLAG_NO_FAST_CONVERT}.get(tier)
    if flags is None:
        flags = getattr(api, tier)
    p = oracle_params(oracle, c)
    frame, pitch = case_frame(c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    # noise frames of a few thousand pixels: with an 8-bit internal format one code of the texture is four ten-bit codes of the target,
    # so the share of identical channels is held at 0.97 there (0.99 elsewhere); behind a PQ / HLG tail a channel beyond the bar needs
    # its witness (compare_behind_tail: inside the oracle's own +-4 ulp pow() interval), at most one per frame (round 6: what was measured)
    same_floor = 0.97 if internal_is_8bit(c) else 0.99
    # every render-target layout on every case (the oracle's frame once; run_layouts checks the bytes around the pixels)
    for layout, (got, info) in run_layouts(mpcvr, torch_cuda, c, extra_flags=flags, what=label).items():
        if has_tail(c):
            ten = c["output_format"] == 1
            compare_behind_tail(oracle, p, frame, pitch, got, want, f"{label} <{layout}> [{info}]", min_same=same_floor, ten_bit=ten,
                                lim=(5 if internal_is_8bit(c) else 2) if ten else 1, cap=1)       # (measured, round 6: 1 on two of the 2,975 cases)
        elif c["output_format"] == 1:
            # (Jinc2m: a one-code difference of the block convert in the 10-bit texture may come out as two ten-bit codes = half an 8-bit code)
            compare_rgb10(got, want, f"{label} <{layout}> [{info}]", tail=c.get("iUpscaling") == 5, internal8=internal_is_8bit(c), min_same=same_floor)
        else:
            compare(got, want, f"{label} <{layout}> [{info}]", min_same=same_floor)


def _is_same_size(c):
    r = c.get("src_rect", (0, 0, c["w"], c["h"]))
    return c["dst"] == (r[2] - r[0], r[3] - r[1]) and not c.get("rotation", 0) and not c.get("hdr_tonemap", 0)


SAME_SIZE = sorted(n for n, c in GOLDEN_CASES.items() if _is_same_size(c))


@pytest.mark.parametrize("name", SAME_SIZE)
def test_direct_convert_vs_oracle(mpcvr, oracle, torch_cuda, name):
    """Nothing to resize: the default planner folds the copy / final pass into the convert kernel (one launch, no
    m_TexConvertOutput round trip).  Same bars as the pass-per-kernel path: bit-exact without a transcendental tail."""
    c = GOLDEN_CASES[name]
    want = run_case(oracle, name, background=BG)
    got, info = run_product(mpcvr, torch_cuda, c)
    if info.startswith("passes:"):          # interleaved RGB without ProcAmp: no convert draw at all, or a flip that needs a draw
        assert info.startswith("passes:source") or c.get("flip"), info
    else:
        assert info.startswith("direct:convert"), info
    chroma = c.get("iChromaScaling", 1)
    # what the 2x2-block convert takes (FMA contraction, scale folded into the matrix => <= 1 LSB instead of bit-exact): 4:2:0 with
    # bilinear or Catmull-Rom chroma, planar / bi-planar 4:2:2 with bilinear chroma, planar 4:4:4 YUV
    blocks = ((c["cformat"] in (1, 2, 3, 14, 17, 20, 21) and chroma in (1, 2) and not c.get("dovi") or
               c["cformat"] in (1, 2, 3, 14, 17, 20, 21) and chroma == 1) or
              (c["cformat"] in (6, 7, 15, 18, 22, 23) and chroma == 1) or c["cformat"] in (16, 19, 24, 25))
    if c.get("output_format", 0) == 1:
        compare_rgb10(got, want, name, exact=not has_tail(c) and not blocks)
    elif has_tail(c) or blocks:
        compare(got, want, name, min_same=0.99)
    else:
        compare(got, want, name, exact=True)


@pytest.mark.parametrize("name", FUSED)
def test_fused_kernel_vs_oracle_and_the_retired_engine_flag(mpcvr, oracle, torch_cuda, name):
    """Every exact-2x golden case through k_fused_up2x against the oracle; MPCVR_FLAG_FUSED_MFMA (the matrix-core experiment kernel that left
    the build in round 6) is accepted, ignored, and draws the same frame bit for bit."""
    from videorenderer_amd import api
    c = GOLDEN_CASES[name]
    want = run_case(oracle, name, background=BG)
    got, info = run_product(mpcvr, torch_cuda, c, extra_flags=api.FLAG_FUSED_VALU)
    if c.get("output_format", 0) == 1:
        compare_rgb10(got, want, f"{name} [{info}]", tail=has_tail(c), internal8=internal_is_8bit(c))
    else:
        compare(got, want, f"{name} [{info}]", min_same=0.99)
    again, info2 = run_product(mpcvr, torch_cuda, c, extra_flags=api.FLAG_FUSED_MFMA)
    assert info2 == info and np.array_equal(again, got)


def test_fused_kernel_is_actually_used(mpcvr, torch_cuda):
    used = 0
    for name in FUSED:
        vp, _ = make_vp(mpcvr, GOLDEN_CASES[name])
        used += vp.GetVPInfo() == "fused_up2x"
        vp.close()
    assert used >= 15


@pytest.mark.parametrize("name", ["c3hdr_p010_pq_lanczos3_2x", "noise_p010_pq_lanczos3_2x", "p010_cosited_pq", "yuv420p16_mpeg1",
                                  "noise_nv12_catmull_2x", "c2_yuv420p10_catmull_2x", "ragged_2x"])
def test_fused_variants_agree(mpcvr, oracle, torch_cuda, name):
    """A/B of the fused kernel's internal shortcuts: LUT vs ALU tone-map, vectorised vs per-pixel convert."""
    from videorenderer_amd import api
    c = GOLDEN_CASES[name]
    want = run_case(oracle, name, background=BG)
    base, info = run_product(mpcvr, torch_cuda, c)
    assert info == "fused_up2x"
    for flags in (api.FLAG_NO_LUT, api.FLAG_NO_FAST_CONVERT, api.FLAG_NO_LUT | api.FLAG_NO_FAST_CONVERT):
        alt, _ = run_product(mpcvr, torch_cuda, c, extra_flags=flags)      # (without the fast convert: the folded pass-per-kernel path)
        compare(alt, want, f"{name} flags={flags}", min_same=0.99)
        compare(alt, base, f"{name} flags={flags} vs default", min_same=0.99)


# ------------------------------------------------------------------------------------------------
def test_host_upload_equals_zero_copy(mpcvr, torch_cuda):
    for name in ("c3hdr_p010_pq_lanczos3_2x", "c2_yuv420p10_catmull_2x", "down_hamming_3x", "v210_2x", "yuy2_bilinear_2x", "gbrp10_procamp"):
        a, _ = run_product(mpcvr, torch_cuda, GOLDEN_CASES[name], host_upload=True)
        b, _ = run_product(mpcvr, torch_cuda, GOLDEN_CASES[name], host_upload=False)
        assert np.array_equal(a, b), name


def test_get_current_image_and_render(mpcvr, oracle, torch_cuda):
    """GetCurentImage = Process at source-rect size into a BGRX target (DX11VideoProcessor.cpp:3493-3608);
    Render clears the letterbox to black and draws into the owned back buffer (:2599-2813)."""
    torch = torch_cuda
    c = dict(GOLDEN_CASES["crop_offset_letterbox"])
    vp, (ww, wh) = make_vp(mpcvr, c)
    frame, pitch = case_frame(c)
    vp.CopySample(frame, pitch)
    snap = vp.GetCurentImage().reshape(48, 64, 4)
    c2 = dict(c, dst=(64, 48), window=(64, 48), offset=(0, 0))
    want = oracle_params(oracle, c2)
    ref = oracle.process(want, frame, pitch)
    compare(snap, ref, "GetCurentImage", min_same=0.999)
    # rects are restored afterwards
    assert vp.Render(1) == 0
    ptr, bpitch, bw, bh = vp.GetBackBuffer()
    assert (bw, bh, bpitch) == (ww, wh, ww * 4)
    vp.Synchronize()
    back = torch.empty((wh, ww, 4), dtype=torch.uint8, device="cuda")
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(back.data_ptr()), ctypes.c_void_p(ptr), ww * wh * 4, 3) == 0
    full = run_case(oracle, "crop_offset_letterbox", background=0)
    compare(back.cpu().numpy(), full, "Render", min_same=0.99)
    vp.close()


# batches that go frame by frame by design (everything else in test_process_batch_equals_single must take a whole-batch route)
# — the fp16 internal format (a user-forced setting): its convert is the per-pixel kernel, which has no frame dimension
BATCH_FRAME_BY_FRAME = ("hdrout_tm6_st2094_hlg_fp16",)
# the first bytes of a batch's targets inside one buffer, from 256-byte boundaries: target 0 on the boundary, target 1 at +8, target 2 at +4, the rest alternate
MIXED_BASES = (0, 8, 4, 8, 4, 8, 4, 8)


def batch_vs_singles_in_carved_targets(torch, vp, frames, src_pitch, ww, wh, dst_pitch, bases, what):
    """mpcvr_process_batch into targets that are slices of ONE patterned buffer (guard bytes in front, between and behind; first bytes at
    `bases` from 256-byte boundaries, one pitch) against the same frames drawn one by one.  A whole-batch launch is planned from the batch's
    first target and runs EVERY frame through the kernel and stores its worst-aligned target allows (a target at +4 sends the whole launch
    from k_fused_period to k_fused_strip, say — two kernels that are held to one code of each other, not to the same bytes), so its frames
    are compared with single frames drawn at that worst alignment.  A batch that declines to frame by frame (GetLastBatchInfo: a launch
    per frame or more) draws every frame as a single one, with the kernel ITS target allows: those are compared with single frames
    drawn into the same first bytes.  Either way each target must hold its single frame's bytes, and every byte outside the window pixels
    the pattern.  Returns GetLastBatchInfo()."""
    assert len(bases) == len(frames)
    worst = min(bases, key=lambda b: (b & -b) if b else 256)
    alone = {}
    for how, at in (("worst", [worst] * len(frames)), ("own", list(bases))):
        alone[how] = CarvedTargets(torch, ww, wh, dst_pitch, at)
        for f, ptr in zip(frames, alone[how].ptrs):
            vp.CopySample(f, src_pitch)
            vp.Process(ptr, dst_pitch)
        vp.Synchronize()
        alone[how].assert_guards_intact(f"{what}: single frames at {at}, pitch {dst_pitch} [{vp.GetVPInfo()}]")
    batch = CarvedTargets(torch, ww, wh, dst_pitch, list(bases))
    vp.ProcessBatch(frames, batch.ptrs, dst_pitch)
    vp.Synchronize()
    info = vp.GetLastBatchInfo()
    batch.assert_guards_intact(f"{what}: batch into targets at {list(bases)}, pitch {dst_pitch} [{vp.GetVPInfo()}; {info}]")
    how = "own" if info["launches"] >= len(frames) else "worst"
    for i in range(len(frames)):
        assert torch.equal(batch.window(i), alone[how].window(i)), (f"{what}: frame {i} of the batch (target at +{bases[i]}, pitch {dst_pitch}) differs from the frame drawn "
                                                                    f"alone at +{worst if how == 'worst' else bases[i]} [{vp.GetVPInfo()}; {info}]")
    assert not bool((batch.window(0) == BG).all()), what
    return info


def test_process_batch_equals_single(mpcvr, torch_cuda):
    torch = torch_cuda
    # fused launch, plain per-frame loop, and the whole-batch launches of the pass-per-kernel path (two-pass, one-pass,
    # same-size direct, 8-bit and 10-bit sources, a source rect, a letterboxed window)
    by_frame = []
    for name, flags in (("noise_p010_pq_lanczos3_2x", 0), ("noise_p010_pq_lanczos3_2x", 2), ("down_lanczos_2p5x", 0),
                        ("up_1p5x_lanczos3", 0), ("x_only_resize", 0), ("y_only_resize", 0), ("c1_nv12_bt709_passthrough", 0),
                        ("mild_down_uses_upscaler", 0), ("crop_offset_letterbox", 0), ("down_hamming_3x", 0), ("c5_p010_hlg_lanczos3_2x", 8),
                        ("up_1p5x_lanczos3", 64), ("down_lanczos_2p5x", 64), ("jinc2_p010_2x_dither", 0), ("jinc2_nv12_noise_1p5x", 0),      # 64 = NO_STRIP: block convert + tiled two-draw kernel
                        # the layouts that joined the fused kernels in round 2: packed 4:2:2 / 4:4:4, gray, three-plane RGB (v210 batches frame by frame)
                        ("yuy2_bilinear_2x", 0), ("y210_lanczos3_2x", 0), ("yuy2_noise_same_size", 0), ("v210_2x", 0), ("ayuv_same_size", 0),
                        ("y410_pq_2x", 0), ("y416_fullrange", 0), ("gbrp8_2x", 0), ("gbrp16_down", 0), ("y8_gray_2x", 0), ("y16_gray_crop", 0),
                        # round 4: the HDR10 tone-mapping step as one launch per batch behind batched post-scale textures (2x, 1.5x, same size, an
                        # 8-bit target with the final pass behind it, the fp16 internal format), Dolby Vision through the block convert's frame
                        # dimension (same-size, resized, HDR output with the tone-mapping step), quarter turns (frame by frame: still equal)
                        ("hdrout_tm1_aces_2x", 0), ("hdrout_tm2_reinhard", 0), ("hdrout_tm3_habel_same_size", 0), ("hdrout_tm4_moebius_bgra8_dither", 0),
                        ("hdrout_tm5_bt2390", 0), ("hdrout_tm6_st2094_hlg_fp16", 0), ("hdrout_tm2_reinhard", 64),
                        ("dovi_poly_sdr", 0), ("dovi_poly_sdr_l2_between_2x", 0), ("dovi_mmr_sdr_l2_brighter", 0), ("dovi_hdrout_tm5_l1_l3_l2", 0),
                        ("rot90_same_shader_single_draw", 0), ("rot270_down_hamming", 0),
                        # round 4, second half: the one-kernel-fits-all draws have a frame dimension too — quarter turns (one draw, two draws, with
                        # a flip, a rotated Jinc2m), flips / half turns where the strip kernels' surface variant is switched off (64), the two-draw
                        # Jinc2m (one axis Jinc, the other the downscaler) and Jinc2m at a non-dyadic ratio
                        ("rot90_two_pass_down_up", 0), ("rot270_one_axis_only", 0), ("rot90_flip_mitchell", 0), ("rot90_copy_nv12", 0), ("jinc2_rot90_pq", 0),
                        ("flip_catmull_1p5x", 64), ("rot180_lanczos3_2x_dither", 64), ("flip_offset_rect_final_pass", 0),
                        ("jinc2_x_with_hamming_down_y", 0), ("jinc2_y_only", 0), ("jinc2_nv12_noise_1p5x", 64)):
        c = GOLDEN_CASES[name]
        vp, (ww, wh) = make_vp(mpcvr, c, flags)
        c = dict(c, kind="noise")        # distinct frames whatever the case's own content
        frames = [torch.from_numpy(case_frame(dict(c, seed=c["seed"] + 100 * i))[0]).cuda() for i in range(5)]
        pitch = vp.GetFrameBytes()[1]
        singles = []
        for f in frames:
            dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
            vp.CopySample(f, pitch)
            vp.Process(dst, ww * 4)
            singles.append(dst)
        dsts = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in frames]
        vp.ProcessBatch(frames, dsts, ww * 4)
        vp.Synchronize()
        for i in range(5):
            assert torch.equal(singles[i], dsts[i]), (name, flags, i)
        assert c["kind"] != "noise" or not torch.equal(dsts[0], dsts[1])       # (structure frames ignore the seed)
        # the whole-batch routes really run: one launch per stage (convert, up to two draws, the tone-mapping step), not one per frame.
        # Frame by frame by design: samples that are repacked one by one (v210 would be batched; interleaved RGB is not in this list),
        # MPCVR_FLAG_NO_FUSED (2) and the literal-tail tier (8) on the pass-per-kernel path
        route = vp.GetLastBatchInfo()
        assert route["frames"] == 5
        if flags in (0, 64) and route["launches"] > 4:
            by_frame.append((name, flags, route["launches"], vp.GetVPInfo()))
        assert vp.GetLastProcessMs() > 0
        # a second batch through the same context (frame-table slots, batched intermediates reused), odd frame count
        dsts = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in range(3)]
        vp.ProcessBatch(frames[2:], dsts, ww * 4)
        vp.Synchronize()
        for i in range(3):
            assert torch.equal(singles[2 + i], dsts[i]), (name, flags, "second batch", i)
        # the targets as slices of one patterned buffer with mixed first bytes: `off8`'s pitch, then `off4`'s (same route: the launch count stays)
        for layout in ("off8", "off4"):
            mixed = batch_vs_singles_in_carved_targets(torch, vp, frames, pitch, ww, wh, layout_of(layout, ww)[1], MIXED_BASES[:5], f"{name} flags={flags} <{layout}>")
            assert mixed["frames"] == 5, (name, flags, layout, route, mixed)
        vp.close()
    assert sorted(n for n, _, _, _ in by_frame) == sorted(BATCH_FRAME_BY_FRAME), by_frame


DOVI_BATCH_CASES = (
    # (label, case, expected GetVPInfo suffix): a stream whose RPU changes with every frame — curves (poly / MMR / mixed / identity), the
    # ycc_to_rgb matrix, level-2 trims appearing (a new kernel variant: a new run) and staying as last seen afterwards
    ("same_size_sdr", dict(cformat=2, w=128, h=64, kind="hdr", seed=700, dst=(128, 64), exfmt_name="TVONLY"), "dovi_batch=3:tables,4:tables"),
    ("resized_sdr", dict(cformat=2, w=128, h=64, kind="hdr", seed=701, dst=(192, 96), iUpscaling=4, exfmt_name="TVONLY"), "dovi_batch=3:tables,4:tables"),
    ("planar_2x_sdr", dict(cformat=20, w=128, h=64, kind="hdr", seed=702, dst=(256, 128), iUpscaling=2, exfmt_name="TVONLY"), "dovi_batch=3:tables,4:tables"),
    ("hdr_passthrough", dict(cformat=2, w=128, h=64, kind="hdr", seed=703, dst=(128, 64), output_format=1, hdr_output=1, exfmt_name="TVONLY"), "dovi_batch=3:tables,4:tables"),
    # the per-pixel convert (a source rect the 2x2-block kernel does not take) and the HDR10 tone-mapping step (level-1 constants by value): frame by frame
    ("odd_rect_per_pixel_convert", dict(cformat=2, w=128, h=64, kind="hdr", seed=704, src_rect=(3, 1, 125, 63), dst=(122, 62), exfmt_name="TVONLY"), "dovi_batch=3:frames,4:frames"),
    ("hdr_tonemap_l1", dict(cformat=2, w=128, h=64, kind="hdr", seed=705, dst=(192, 96), iUpscaling=2, output_format=1, hdr_output=1, hdr_tonemap=5, hdr_display=1000.0,
                            exfmt_name="TVONLY"), None),
)


@pytest.mark.parametrize("label", [c[0] for c in DOVI_BATCH_CASES])
def test_process_batch_dovi_one_rpu_per_frame(mpcvr, oracle, torch_cuda, label):
    """mpcvr_process_batch_dovi: frame i of the batch runs on rpus[i].  Must equal, bit for bit, the reference's own pattern — the RPU read
    from every sample: SetDoviMetadata + CopySample + Process frame after frame on a second context — and the oracle run with frame i's
    RPU; the whole-batch routes must really be taken (GetVPInfo names the runs), and the context must end up on the last RPU.  Nothing of a
    Dolby Vision batch outlives the call: a plain batch behind it runs on the context's own RPU and reports no runs, and a batch behind a
    refused one equals the loop as before."""
    torch = torch_cuda
    from videorenderer_amd import api, synth
    from tests.golden import cases as G
    _, c, want_info = next(x for x in DOVI_BATCH_CASES if x[0] == label)
    c = dict(c)
    c.pop("exfmt_name")
    c["exfmt"] = G.ext(G.MPEG2, G.TV)
    kinds = [dict(kind="poly"), dict(kind="mmr"), dict(kind="mixed"), dict(kind="mmr", l2=(100, 600, 1000)), dict(kind="poly"),
             dict(kind="identity", l2=(600,)), dict(kind="mixed")]
    if c.get("hdr_tonemap"):
        kinds[2] = dict(kind="mixed", l1=True)          # level-1 data appear on frame 2: the tone-mapping step switches on (a new plan, a new run)
    rpus = []
    for i, k in enumerate(kinds):
        md = api.DoviMetadata.from_dict(synth.dovi_metadata(**k))
        md.ycc_to_rgb_matrix[0] *= 1.0 - 0.01 * i       # every frame its own colour matrix
        md.ycc_to_rgb_matrix[5] += 0.004 * i
        md.ycc_to_rgb_offset[1] += 0.001 * i
        rpus.append(md)
    n = len(rpus)
    frames = [torch.from_numpy(case_frame(dict(c, seed=c["seed"] + 31 * i))[0]).cuda() for i in range(n)]
    # frame after frame
    one, (ww, wh) = make_vp(mpcvr, c)
    pitch = one.GetFrameBytes()[1]
    singles = []
    for f, md in zip(frames, rpus):
        dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
        one.SetDoviMetadata(md)
        one.CopySample(f, pitch)
        one.Process(dst, ww * 4)
        singles.append(dst)
    one.Synchronize()
    # the batch
    vp, _ = make_vp(mpcvr, c)
    dsts = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in frames]
    vp.ProcessBatchDovi(frames, dsts, ww * 4, rpus)
    vp.Synchronize()
    info = vp.GetVPInfo()
    route = vp.GetLastBatchInfo()
    for i in range(n):
        assert torch.equal(singles[i], dsts[i]), (label, i, info, route)
    assert not torch.equal(dsts[0], dsts[1])
    assert route["frames"] == n
    if want_info:
        assert route["dovi_runs"] == want_info.split("=")[1], route
        if "tables" in want_info:       # two runs, a convert launch each (+ the draws behind it): fewer launches than frames
            assert route["launches"] <= 4, route
        else:
            assert route["launches"] >= n, route
    else:           # (level-1 data from frame 2 on: the runs behind the tone-mapping step go frame by frame)
        assert ":frames" in route["dovi_runs"], route
    # the context holds the last frame's RPU (and the level-2 block frame 5 brought): a plain Process repeats the batch's last frame
    again = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
    vp.CopySample(frames[-1], pitch)
    vp.Process(again, ww * 4)
    vp.Synchronize()
    assert torch.equal(again, dsts[-1]), label
    if label in ("same_size_sdr", "resized_sdr"):
        # a plain batch behind it, on the RPU the context still holds: equals CopySample + Process of the same frames there, and its record is its
        # own (mpcvr.h: the string describes the last call) — no runs of the Dolby Vision batch before it
        plain = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in range(3)]
        vp.ProcessBatch(frames[:3], plain, ww * 4)
        vp.Synchronize()
        plain_route = vp.GetLastBatchInfo()
        for i in range(3):
            alone = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
            vp.CopySample(frames[i], pitch)
            vp.Process(alone, ww * 4)
            vp.Synchronize()
            assert torch.equal(plain[i], alone), (label, "plain batch after the Dolby Vision batch", i, plain_route)
        assert not torch.equal(plain[0], dsts[0])       # (frame 0 on the last RPU, not on its own)
        assert plain_route["frames"] == 3 and plain_route["dovi_runs"] == "", plain_route
    # a second batch through the same context: the table slots are reused; starts on the sticky level-2 state like the loop would
    dsts2 = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in range(3)]
    vp.ProcessBatchDovi(frames[:3], dsts2, ww * 4, rpus[:3])
    singles2 = []
    for f, md in zip(frames[:3], rpus[:3]):
        dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
        one.SetDoviMetadata(md)
        one.CopySample(f, pitch)
        one.Process(dst, ww * 4)
        singles2.append(dst)
    vp.Synchronize(); one.Synchronize()
    for i in range(3):
        assert torch.equal(singles2[i], dsts2[i]), (label, "second batch", i)
    # a malformed RPU anywhere in the batch: E_INVALIDARG and nothing drawn
    bad = api.DoviMetadata.from_dict(synth.dovi_metadata("poly"))
    bad.curves[1].num_pivots = 11
    untouched = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in range(2)]
    with pytest.raises(api.MpcvrError):
        vp.ProcessBatchDovi(frames[:2], untouched, ww * 4, [rpus[0], bad])
    vp.Synchronize()
    assert all(bool((u == BG).all()) for u in untouched)
    if label in ("same_size_sdr", "resized_sdr"):
        # ... and nothing of the refused call is left in the context: the batch before it, once more
        dsts3 = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in range(3)]
        vp.ProcessBatchDovi(frames[:3], dsts3, ww * 4, rpus[:3])
        vp.Synchronize()
        for i in range(3):
            assert torch.equal(singles2[i], dsts3[i]), (label, "batch after the refused one", i, vp.GetLastBatchInfo())
    vp.close(); one.close()
    if c.get("hdr_tonemap"):
        return          # (level-1 data stay as last seen: the loop above is the statement of that; the tone-mapping step has its own oracle tests)
    # frames 1 (MMR) and 3 (MMR + level-2 trims) against the oracle on their own RPUs
    for i in (1, 3):
        k = dict(kinds[i])
        p = oracle_params(oracle, dict(c, dovi=k))
        mdd = synth.dovi_metadata(**k)
        mdd["ycc_to_rgb_matrix"] = list(rpus[i].ycc_to_rgb_matrix)
        mdd["ycc_to_rgb_offset"] = list(rpus[i].ycc_to_rgb_offset)
        # (level-2 / level-1 blocks stay as last seen: frame 3 brings its own trims; nothing earlier in this stream carries any)
        oracle.set_params(p, dovi=mdd)
        frame = frames[i].cpu().numpy()
        want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
        got = dsts[i].cpu().numpy()
        if c.get("output_format", 0) == 1:
            compare_rgb10(got, want, f"{label} frame {i}", tail=True)
        else:
            compare_behind_tail(oracle, p, frame, pitch, got, want, f"{label} frame {i} [{info}]", min_same=0.99, dovi=True, cap=2)


def test_param_blob_roundtrip_and_override(mpcvr, torch_cuda):
    """Rank-0 blob adopted by another context gives identical pixels (the multi-GPU broadcast payload)."""
    torch = torch_cuda
    c = GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]
    a, _ = run_product(mpcvr, torch, c)
    vp0, _ = make_vp(mpcvr, c)
    blob = vp0.GetParamBlob()
    assert 16000 < len(blob) < 32768
    # the receiving context is deliberately configured with different nits: the blob must win
    vp1, (ww, wh) = make_vp(mpcvr, dict(c, iSDRDisplayNits=300))
    vp1.SetParamBlob(blob)
    frame, pitch = case_frame(c)
    dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
    vp1.CopySample(frame, pitch)
    vp1.Process(dst, ww * 4)
    vp1.Synchronize()
    assert np.array_equal(dst.cpu().numpy(), a)
    from videorenderer_amd import api
    with pytest.raises(api.MpcvrError):
        vp1.SetParamBlob(b"\0" * len(blob))
    vp0.close(); vp1.close()


def test_configure_rebuilds_only_what_changed(mpcvr, oracle, torch_cuda):
    torch = torch_cuda
    from videorenderer_amd import api
    c = GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]
    vp, (ww, wh) = make_vp(mpcvr, c)
    frame, pitch = case_frame(c)
    vp.CopySample(frame, pitch)
    assert vp.Configure(vp.settings.copy()) == api.S_FALSE                     # nothing changed
    assert vp.Configure(vp.settings.copy(iUpscaling=api.UPSCALE_Mitchell, iSDRDisplayNits=200)) == api.S_OK
    dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
    vp.Process(dst, ww * 4)
    vp.Synchronize()
    c2 = dict(c, iUpscaling=1, iSDRDisplayNits=200)
    p = oracle_params(oracle, c2)
    compare(dst.cpu().numpy(), oracle.process(p, frame, pitch), "after Configure", min_same=0.99)
    vp.close()


def test_dovi_metadata_lifecycle(mpcvr, oracle, torch_cuda):
    """RPUs change from frame to frame: the curves follow the latest one, level-2 trims persist while later RPUs carry none
    (m_DoviExtensionMetadata.L2 stays present until Flush, DX11VideoProcessor.cpp:2383-2469, :4082), a display-peak change
    re-selects the trims, and SetDoviMetadata(None) returns to the tagged colourimetry."""
    torch = torch_cuda
    from videorenderer_amd import synth
    c = dict(GOLDEN_CASES["dovi_poly_sdr_l2_between_2x"])
    vp, (ww, wh) = make_vp(mpcvr, c)
    frame, pitch = case_frame(c)
    vp.CopySample(torch.from_numpy(frame).cuda(), pitch)

    def product():
        dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
        vp.Process(dst, ww * 4)
        vp.Synchronize()
        return dst.cpu().numpy()

    def expect(case):
        p = oracle_params(oracle, case)
        return oracle.process(p, frame, pitch, dst=np.full((wh, ww, 4), BG, np.uint8))

    assert vp.GetVPInfo().startswith("passes:convert,resizeX,resizeY")   # never the fused kernel
    compare(product(), expect(c), "first RPU", min_same=0.99)
    l2 = c["dovi"]["l2"]
    vp.SetDoviMetadata(synth.dovi_metadata("mmr"))                    # no level-2 block: the previous trims stay
    compare(product(), expect(dict(c, dovi=dict(kind="mmr", l2=l2))), "sticky L2", min_same=0.99)
    vp.SetHdrOutput(False, 0, 900.0)                                  # new display peak, but this RPU has no L2 list to re-select from
    compare(product(), expect(dict(c, dovi=dict(kind="mmr", l2=l2), hdr_display=400.0)), "sticky L2 after display change", min_same=0.99)
    vp.Flush()
    vp.CopySample(torch.from_numpy(frame).cuda(), pitch)
    vp.SetDoviMetadata(synth.dovi_metadata("mmr"))
    compare(product(), expect(dict(c, dovi=dict(kind="mmr"))), "after Flush", min_same=0.99)
    vp.SetDoviMetadata(synth.dovi_metadata("mixed", l2=(100, 600, 1000)))
    compare(product(), expect(dict(c, dovi=dict(kind="mixed", l2=(100, 600, 1000)), hdr_display=900.0)), "third RPU", min_same=0.99)
    vp.SetDoviMetadata(None)
    plain = {k: v for k, v in c.items() if k != "dovi"}
    compare(product(), expect(plain), "Dolby Vision off", min_same=0.99)
    assert vp.GetVPInfo() == "fused_up2x"                             # and the fused kernel is eligible again
    vp.close()
    # rejected metadata leaves the state alone and reports E_INVALIDARG
    vp, _ = make_vp(mpcvr, c)
    bad = synth.dovi_metadata("poly")
    bad["curves"][0] = dict(bad["curves"][0], num_pivots=12)
    with pytest.raises(mpcvr.api.MpcvrError) as e:
        vp.SetDoviMetadata(bad)
    assert e.value.hr & 0xffffffff == 0x80070057
    vp.close()


DOVI_FULL = [
    ("poly_sdr", dict(dovi=dict(kind="poly")), "direct:convert+final"),
    ("mmr_sdr", dict(dovi=dict(kind="mmr")), "direct:convert+final"),
    ("mixed_l2_sdr", dict(dovi=dict(kind="mixed", l2=(100, 600, 1000))), "direct:convert+final"),
    ("mmr_hdr_passthrough", dict(dovi=dict(kind="mmr"), hdr_output=1, output_format=1), "direct:convert+copy"),
    ("poly_sdr_720p_to_1080p", dict(dovi=dict(kind="poly"), w=1280, h=720, dst=(1920, 1080), iUpscaling=4), "passes:convert,resizeX,resizeY+final"),
]


@pytest.mark.parametrize("label,extra,path", DOVI_FULL)
def test_dovi_block_convert_whole_frame(mpcvr, oracle, torch_cuda, label, extra, path):
    """Dolby Vision through the 2x2-block convert (round 2) at 1080p, every pixel against the oracle: polynomial and MMR curves
    behind the elided PQ round trip (no level-2 trims), mixed curves with level-2 trims (PQ decode and tone map from tables,
    encode and trims in ALU), the literal chain into a 10-bit HDR target, and the block convert feeding the tiled resize.
    >= 99.8 % identical, |delta| <= 1 except on channels the oracle itself does not define to one code (compare_behind_tail: per-channel
    witness, no blanket allowance; 10-bit target: <= 2 codes behind the tail)."""
    torch = torch_cuda
    from videorenderer_amd import api
    c = dict(cformat=2, w=1920, h=1080, kind="hdr", seed=401, dst=(1920, 1080), exfmt=GOLDEN_CASES["dovi_poly_sdr"]["exfmt"])
    c.update(extra)
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    for flags in (api.FLAG_NO_FUSED, api.FLAG_NO_FAST_CONVERT, 0):
        got, info = run_product(mpcvr, torch, c, extra_flags=flags)
        assert info.startswith(path) or flags == api.FLAG_NO_FUSED, info
        if flags == api.FLAG_NO_FUSED:          # the plain tier: the oracle's bits on every channel of the Dolby Vision frame (round 6)
            if c.get("output_format", 0) == 1:
                compare_rgb10(got, want, f"{label} flags={flags}", exact=True)
            else:
                compare(got, want, f"dovi {label} flags={flags} [{info}]", exact=True)
            continue
        if c.get("output_format", 0) == 1:
            compare_rgb10(got, want, f"{label} flags={flags}", tail=True)
            continue
        same, n_bad = compare_behind_tail(oracle, p, frame, pitch, got, want, f"dovi {label} flags={flags} [{info}]", min_same=0.998, dovi=True)
        print(f"dovi {label} flags={flags} [{info}]: identical {same:.6f}, channels beyond 1 LSB (all inside the oracle's own +-{POW_ULPS} ulp pow() interval) {n_bad}")


def test_frame_timers(mpcvr, torch_cuda):
    """mpcvr_get_last_timings (FrameStats.h:145-173: copyticks, paintticks + the snapshot's read-back): nothing timed -> -1; a host
    sample times its upload, a device sample does not touch the upload timer, a snapshot times its read-back."""
    torch = torch_cuda
    from videorenderer_amd import api
    c = GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]
    vp, (ww, wh) = make_vp(mpcvr, c)
    t = vp.GetLastTimings()
    assert t == dict(copy_host_ms=-1.0, upload_ms=-1.0, process_ms=-1.0, readback_ms=-1.0)
    frame, pitch = case_frame(c)
    dst = torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda")
    vp.CopySample(torch.from_numpy(frame).cuda(), pitch)
    vp.Process(dst, ww * 4)
    t = vp.GetLastTimings()
    assert t["copy_host_ms"] >= 0 and t["upload_ms"] == -1.0 and t["process_ms"] > 0 and t["readback_ms"] == -1.0
    assert abs(t["process_ms"] - vp.GetLastProcessMs()) < 1e-6
    vp.CopySample(frame, pitch)                      # pageable host memory: staged and uploaded on the copy stream
    vp.Process(dst, ww * 4)
    t = vp.GetLastTimings()
    assert t["upload_ms"] > 0 and t["copy_host_ms"] > 0
    vp.GetCurentImage()
    assert vp.GetLastTimings()["readback_ms"] > 0
    vp.close()


def test_error_behaviour(mpcvr, torch_cuda):
    torch = torch_cuda
    from videorenderer_amd import api
    vp = api.VideoProcessor()
    dst = torch.zeros((16, 16, 4), dtype=torch.uint8, device="cuda")

    def hr_of(fn):
        with pytest.raises(api.MpcvrError) as e:
            fn()
        return e.value.hr

    assert hr_of(lambda: vp.Process(dst, 64)) == api.E_NOT_VALID_STATE                  # no media type yet
    assert hr_of(lambda: vp.InitMediaType(40, 64, 64)) == api.E_NOTIMPL                 # no such ColorFormat_t
    assert hr_of(lambda: vp.InitMediaType(1, 64, 64, pitch=-64)) == api.E_INVALIDARG    # bottom-up is an RGB notion
    assert hr_of(lambda: vp.InitMediaType(4, 63, 64)) == api.E_INVALIDARG               # odd width, packed 4:2:2
    assert hr_of(lambda: vp.InitMediaType(10, 60, 64, pitch=96)) == api.E_INVALIDARG    # v210 row needs 10 groups of 16 bytes
    assert hr_of(lambda: vp.InitMediaType(1, 63, 64)) == api.E_INVALIDARG               # odd width, 4:2:0
    assert hr_of(lambda: vp.InitMediaType(1, 64, 64, src_rect=(0, 0, 65, 64))) == api.E_INVALIDARG
    vp.InitMediaType(1, 64, 64)
    assert hr_of(lambda: vp.Process(dst, 64)) == api.E_NOT_VALID_STATE                  # no sample yet
    assert vp.Render(1) == api.S_FALSE                                                  # nothing to draw
    buf = torch.zeros(64 * 96, dtype=torch.uint8, device="cuda")
    assert hr_of(lambda: vp.CopySample(buf, 128)) == api.E_UNEXPECTED                   # pitch != media type (:2545)
    vp.CopySample(buf, 64)
    assert hr_of(lambda: vp.Process(dst, 8)) == api.E_INVALIDARG                        # RT pitch too small
    assert hr_of(lambda: vp.Process(dst, 256, src_rect=(0, 0, 32, 32))) == api.E_INVALIDARG
    assert hr_of(lambda: vp.SetRotation(45)) == api.E_INVALIDARG
    assert hr_of(lambda: vp.SetSampleFormat(3)) == api.E_INVALIDARG
    assert hr_of(lambda: vp.Configure(vp.settings.copy(iSDRDisplayNits=5))) == api.E_INVALIDARG
    assert hr_of(lambda: vp.Configure(vp.settings.copy(iUpscaling=7))) == api.E_INVALIDARG      # past UPSCALE_Jinc2
    vp.close()
    # A render target is made of dwords (include/mpcvr.h): a first byte or a pitch that is not a multiple of 4 is refused by every entry point
    # that takes a target, in front of any launch — the target, and every byte around it, stays as it was.  The plain context, and one whose
    # batches end in the error-diffusion pass (a route of its own).
    import ctypes as C
    from videorenderer_amd import synth
    for kw in (dict(), dict(bUseDither=api.DITHER_ErrorDiffusion_EXT)):
        vp = api.VideoProcessor(api.default_settings(**kw))
        vp.InitMediaType(2, 64, 64, extfmt=GOLDEN_CASES["dovi_poly_sdr"]["exfmt"])
        vp.SetWindowRect((0, 0, 64, 64)); vp.SetVideoRect((0, 0, 64, 64))
        sample = torch.from_numpy(synth.make_frame(2, 64, 64, "noise", seed=5)[0].copy()).cuda()
        pitch = vp.GetFrameBytes()[1]
        t = CarvedTargets(torch, 64, 64, 64 * 4 + 16, [0, 0])
        before = t.buf.clone()
        rpu = synth.dovi_metadata(kind="poly")
        arr = C.c_void_p * 2
        L = api.load_library()
        for off, dp in ((1, 272), (2, 272), (3, 272), (0, 273), (0, 274), (0, 275), (2, 274)):
            a, b = t.ptrs[0] + off, t.ptrs[1]
            vp.CopySample(sample, pitch)
            assert hr_of(lambda: vp.Process(a, dp)) == api.E_INVALIDARG, (kw, off, dp)
            assert L.mpcvr_process_frames(vp._ctx, 2, arr(sample.data_ptr(), sample.data_ptr()), pitch, api.MEM_DEVICE, arr(b, a), dp) == api.E_INVALIDARG, (kw, off, dp)
            assert hr_of(lambda: vp.ProcessBatch([sample, sample], [b, a], dp)) == api.E_INVALIDARG, (kw, off, dp)
            assert hr_of(lambda: vp.ProcessBatchDovi([sample, sample], [b, a], dp, [rpu, rpu])) == api.E_INVALIDARG, (kw, off, dp)
            vp.Synchronize()
            if off and dp % 4 == 0:
                # (mpcvr_process_frames stops at the first failure: with a sound pitch its first frame — the aligned target — is drawn)
                assert not torch.equal(t.window(1), before.as_strided((64, 64, 4), (272, 4, 1), t.starts[1])), (kw, off, dp)
                t.window(1).fill_(BG)
            assert torch.equal(t.buf, before), (kw, off, dp, "a refused call wrote into the buffer")
        # (the same calls with a sound target and pitch are served)
        vp.CopySample(sample, pitch)
        vp.Process(t.ptrs[0], 272)
        vp.ProcessBatch([sample, sample], t.ptrs, 272)
        vp.Synchronize()
        t.assert_guards_intact(f"aligned calls {kw}")
        assert torch.equal(t.window(0), t.window(1)) and not bool((t.window(0) == BG).all())
        vp.close()


# ------------------------------------------------------------------------------------------------
# BASELINE.json full sizes: size-independent properties + oracle on sampled regions
# ------------------------------------------------------------------------------------------------
def reference_text_output(oracle, name):
    """B8G8R8A8 render target of the REFERENCE's own shader text for a tests/golden/cases.py FULL_SIZE_CASES entry.
    Where oracle/_ref/libref_hlsl.so exists (this container, and the GPU box: built .so files travel with the snapshot) the text is
    EXECUTED here (oracle/ref_hlsl/ref_pipeline.py: the real Shaders/*.hlsl + the convert shader the real Source/Shaders.cpp emits)
    and its hash checked against tests/golden/full_size_pins.json; where it does not, the oracle's output stands in — after ITS hash
    matched the recorded reference-text hash, so either way the array returned is the reference text's result bit for bit (alpha set
    opaque: the reference leaves the shader's A in the target and the swap chain ignores it)."""
    import hashlib
    import json
    import sys
    from tests.golden.cases import FULL_SIZE_CASES
    from tests.golden.make_ref_hlsl_golden import rgb_channels
    with open(os.path.join(HERE, "golden", "full_size_pins.json")) as f:
        pin = json.load(f)["cases"][name]
    c = FULL_SIZE_CASES[name]
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle", "ref_hlsl"))
    import ref_hlsl
    live = ref_hlsl.available()
    if live:
        import ref_pipeline
        try:
            out = ref_pipeline.process(p, frame, pitch)
        except RuntimeError:            # this convert shader is not in the prebuilt library and /root/reference is not mounted
            live = False
    if not live:
        out = oracle.process(p, frame, pitch)
    assert hashlib.sha256(rgb_channels(out).astype(np.uint16).tobytes()).hexdigest() == pin["rgb_sha256"], \
        f"{name}: {'reference text' if live else 'oracle'} output does not hash to the recorded reference-text result"
    out = out.copy()
    out[..., 3] = 255
    return out, live


# measured share of identical channels per (case, tier) on MI355X, round 3 (max |delta| = 1 everywhere); the asserted floor is
# 1 - 2 x (1 - measured): a rounding regression twice as bad as today's fails
FULL_SIZE_TIERS = {
    # name: ((flags attr or 0, expected GetVPInfo prefix, floor), ...)
    "c3hdr": (("FLAG_FUSED_VALU", "fused_up2x", 0.99856), ("FLAG_NO_FUSED", "passes:convert,resizeX,resizeY+final", 1.0)),        # 0.999280 0.999272 0.999962
    "c3_sdr": (("FLAG_FUSED_VALU", "fused_up2x", 0.99925), ("FLAG_NO_FUSED", "passes:convert,resizeX,resizeY+final", 1.0)),                  # 0.999625 0.999616 1.0
    "c5_hlg": (("FLAG_FUSED_VALU", "fused_up2x", 0.9979), ("FLAG_NO_FUSED", "passes:convert,resizeX,resizeY+final", 1.0)),          # 0.998948 0.998939 0.999648
    "c4_mitchell": (("FLAG_FUSED_VALU", "fused_up2x", 0.9988), ("FLAG_NO_FUSED", "passes:convert,resizeX,resizeY+final", 1.0)),    # 0.999401 0.999397 0.999969
    "C1": ((0, "direct:convert+copy", 0.99999),          # 0.999996 1.0 1.0
            ("FLAG_NO_FAST_CONVERT", "direct:convert+copy", 1.0), ("FLAG_NO_FUSED", "passes:convert,copy", 1.0)),
    "C2": ((0, "fused_up2x", 0.9996),        # 0.999804 1.0
            ("FLAG_NO_FUSED", "passes:convert,resizeX,resizeY+final", 1.0)),
    "up1440": ((0, "period", 0.99938), ("FLAG_NO_PERIOD", "strip", 0.99938), ("FLAG_NO_STRIP", "passes:convert,resizeX,resizeY", 0.99939), ("FLAG_NO_FUSED", "passes:convert,resizeX,resizeY+final", 1.0)),            # 0.999691 0.999698 0.999963
    "down1440": ((0, "period", 0.99938), ("FLAG_NO_PERIOD", "strip", 0.99938), ("FLAG_NO_STRIP", "passes:convert,resizeX,resizeY", 0.99939), ("FLAG_NO_FUSED", "passes:convert,resizeX,resizeY+final", 1.0)),          # 0.999692 0.999697 0.999965
    "up1080_from_720_nv12": (("FLAG_FORCE_PERIOD", "strip", 0.99996), (0, "strip", 0.99996), ("FLAG_NO_STRIP", "passes:convert,resizeX,resizeY", 0.99998),      # 0.999981 0.999991 1.0
                             ("FLAG_NO_FUSED", "passes:convert,resizeX,resizeY", 1.0)),
    "down1080_from_4k_hlg": ((0, "period", 0.99877), ("FLAG_NO_PERIOD", "strip", 0.99877), ("FLAG_NO_STRIP", "passes:convert,resizeX,resizeY", 0.9988), ("FLAG_NO_FUSED", "passes:convert,resizeX,resizeY+final", 1.0)),   # 0.999386 0.999401 0.999695
    # round 3's new paths against the reference text
    "up2160_from_720": ((0, "period", 0.99939), ("FLAG_NO_PERIOD", "strip", 0.99939), ("FLAG_NO_FUSED", "passes:convert,resizeX,resizeY+final", 1.0)),      # 0.999695 0.999695 0.999962
    "up720_from_240_nv12_catmull": (("FLAG_FORCE_PERIOD", "strip", 0.99997), (0, "strip", 0.99997), ("FLAG_NO_FUSED", "passes:convert,resizeX,resizeY", 1.0)),  # 0.999988 0.999988 1.0
    "flipped_540_to_720_nv12": ((0, "period", 0.99996), ("FLAG_NO_PERIOD", "strip", 0.99996), ("FLAG_NO_FUSED", "passes:convert,resizeX,resizeY", 1.0)),          # 0.999984 0.999984 1.0
    "rot180_540_to_720_pq": ((0, "period:surface", 0.99936), ("FLAG_NO_PERIOD", "strip:surface", 0.99936), ("FLAG_NO_FUSED", "passes:convert,resizeX,resizeY+final", 1.0)),   # 0.999683 0.999683 0.999960
    # round 5: the fused Jinc2m kernel (10-bit internal format behind a PQ tail; 8-bit internal format = the exact form of the convert stage)
    # (floors = 1 - 2 x (1 - measured), like the rows above)
    "jinc_4k_from_1080_pq": ((0, "fused_jinc2x", 0.99844), ("FLAG_NO_FAST_CONVERT", "passes:convert,resizeX+final", 0.99846),       # 0.999223 0.999230 0.999940
                             ("FLAG_NO_FUSED", "passes:convert,resizeX+final", 1.0)),
    "jinc_1440_from_720_nv12": ((0, "fused_jinc2x", 0.99968), ("FLAG_NO_FAST_CONVERT", "passes:convert,resizeX", 0.9997),          # 0.999844 0.999850 0.999994
                                ("FLAG_NO_FUSED", "passes:convert,resizeX", 1.0)),
    "down1080_from_4k_lanczos_convolution": ((0, "strip", 0.99925), ("FLAG_NO_STRIP", "passes:convert,resizeX,resizeY", 0.99928),         # 0.999629 0.999644 0.999960
                                             ("FLAG_NO_FUSED", "passes:convert,resizeX,resizeY+final", 1.0)),
}


# Jinc2m's weights sum to |w| = 1.9 (negative ring): behind a PQ tail, where dark saturated colours sit on pow()'s steep end, what the separable
# filters keep inside one code comes out at two on a handful of channels per frame — each must be shown ill-conditioned (compare_behind_tail),
# and their number is capped at 1.5 x what was measured (3 of 24.9 M channels on the fused and the tiled tier; the plain tier is bit-identical)
FULL_SIZE_BEHIND_A_TAIL = {"jinc_4k_from_1080_pq": 4}


@pytest.mark.parametrize("name", sorted(FULL_SIZE_TIERS))
def test_full_size_hip_vs_reference_shader_text(mpcvr, oracle, torch_cuda, name):
    """The parity triangle closed at the BASELINE sizes: EVERY output pixel of every GPU tier — the fused kernels (both tap engines of
    the exact-2x kernel; the periodic / strip kernels for the other ratios), the tiled kernels, the pass-per-kernel path — against
    what the REFERENCE's own shader text produces for the same frame (reference_text_output: executed live on this box).
    BASELINE.json's bar: |delta| <= 1 LSB per 8-bit channel.  Tiers whose floor is 1.0 must be bit-identical to the reference text
    (no transcendental on the path, -ffp-contract=off, and the tap tables restate FillVertices' fp32 corner coordinates)."""
    torch = torch_cuda
    from videorenderer_amd import api
    from tests.golden.cases import FULL_SIZE_CASES
    c = FULL_SIZE_CASES[name]
    want, live = reference_text_output(oracle, name)
    for flag, path, floor in FULL_SIZE_TIERS[name]:
        flags = getattr(api, flag) if flag else 0
        # (today's layout and `off4` — the per-pixel store paths at real widths, right edge and last strip included; the reference frame serves both)
        for layout, (got, info) in run_layouts(mpcvr, torch, c, extra_flags=flags, layouts=("tight", "off4"), what=f"{name} flags={flag}").items():
            assert info.startswith(path) or (path in ("period", "strip", "period:surface", "strip:surface") and kernel_under(layout, f"kernel=fused_{path}(") in info), (name, flag, layout, info)
            assert bool((got[..., 3] == 255).all())
            if name in FULL_SIZE_BEHIND_A_TAIL and floor < 1.0:     # channels beyond 1 LSB must each lie inside the oracle's own +-4 ulp pow() interval, and be few
                frame, pitch = case_frame(c)
                same, n_ill = compare_behind_tail(oracle, oracle_params(oracle, c), frame, pitch, got, want, f"{name} flags={flag} <{layout}> [{info}]", min_same=floor,
                                                  cap=FULL_SIZE_BEHIND_A_TAIL[name])
                print(f"FULLSIZE {name} {flag or 'default'} <{layout}>: {n_ill} ill-conditioned channel(s)")
            else:
                same = compare(got, want, f"{name} flags={flag} <{layout}> [{info}]", exact=(floor == 1.0), min_same=floor)
            print(f"FULLSIZE {name} {flag or 'default'} <{layout}> [{info}] vs reference text ({'live' if live else 'recorded hash'}): identical channels {same:.6f}")


@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_default_planner_vs_live_reference_shader_text(mpcvr, oracle, torch_cuda, name):
    """Every comparable golden case: the default planner's output against the reference's shader text EXECUTED ON THIS BOX
    (oracle/_ref/libref_hlsl.so travels with the snapshot) — the GPU suite's own contact with reference-derived output, no oracle in
    between.  Bars as for the oracle comparisons: <= 1 LSB (8-bit) / the 10-bit bars of compare_rgb10."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle", "ref_hlsl"))
    import ref_hlsl
    from tests.golden.make_ref_hlsl_golden import comparable
    c = GOLDEN_CASES[name]
    if not comparable(c):
        pytest.skip("interleaved RGB sample / our own Lanczos3 tap fix: no reference-text counterpart")
    if not ref_hlsl.available():
        pytest.skip("oracle/_ref/libref_hlsl.so not built")
    import ref_pipeline
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    try:
        ref = ref_pipeline.process(p, frame, pitch, background=BG)
    except RuntimeError as e:
        pytest.skip(str(e))
    got, info = run_product(mpcvr, torch_cuda, c)
    if c.get("output_format", 0) == 1:
        g, r = got.view(np.uint32)[..., 0], ref                # untouched pixels carry BG in both
        lim = 5 if internal_is_8bit(c) else 2 if has_tail(c) else 1
        for sh in (0, 10, 20):
            d = np.abs(((g >> sh) & 1023).astype(np.int32) - ((r >> sh) & 1023).astype(np.int32))
            assert d.max() <= lim, f"{name} [{info}]: 10-bit delta {d.max()} vs the reference text"
    else:
        d = np.abs(got[..., :3].astype(np.int16) - ref[..., :3].astype(np.int16))
        assert d.max() <= 1, f"{name} [{info}]: max |delta| = {d.max()} vs the reference text"


STRIP_FULL = [
    ("p010_pq_1080p_to_1440p_lanczos3", dict(cformat=2, w=1920, h=1080, kind="noise", seed=311, dst=(2560, 1440), iUpscaling=4,
                                             exfmt=GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]["exfmt"])),
    ("p010_pq_4k_to_1440p_hamming", dict(cformat=2, w=3840, h=2160, kind="noise", seed=312, dst=(2560, 1440), iDownscaling=2,
                                         exfmt=GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]["exfmt"])),
    ("nv12_720p_to_1080p_catmull_odd_window", dict(cformat=1, w=1280, h=720, kind="noise", seed=313, dst=(1919, 1079), iUpscaling=2,
                                                   window=(1931, 1090), offset=(5, 3),
                                                   exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"])),
    ("yuv420p10_up_x_down_y", dict(cformat=20, w=1280, h=1440, kind="noise", seed=314, dst=(1920, 800), iUpscaling=3, iDownscaling=5,
                                   exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"])),
    ("nv12_1080p_down_2p6x_hamming", dict(cformat=1, w=1920, h=1080, kind="noise", seed=316, dst=(738, 416), iDownscaling=2, bInterpolateAt50pct=0,
                                          exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"])),
    ("p010_1080p_down_1p2x_bicubic_no_interp", dict(cformat=2, w=1920, h=1080, kind="noise", seed=317, dst=(1600, 900), iDownscaling=3, bInterpolateAt50pct=0,
                                                    exfmt=GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]["exfmt"])),
    ("p010_hlg_4k_to_1080p_interp50", dict(cformat=2, w=3840, h=2160, kind="noise", seed=315, dst=(1920, 1080), iUpscaling=1,
                                           exfmt=GOLDEN_CASES["c5_p010_hlg_lanczos3_2x"]["exfmt"])),
    # 9..16 taps (ps_convolution beyond ~2x with the wider kernels): the 16-tap variant, one pixel per lane, a 32-row ring
    ("p010_pq_4k_to_1080p_lanczos_without_the_50pct_rule", dict(cformat=2, w=3840, h=2160, kind="noise", seed=320, dst=(1920, 1080), iDownscaling=5, bInterpolateAt50pct=0,
                                                               exfmt=GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]["exfmt"])),
    ("nv12_1080p_to_480p_bicubic", dict(cformat=1, w=1920, h=1080, kind="noise", seed=321, dst=(854, 480), iDownscaling=3,
                                        exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"])),
    ("yuv420p10_hlg_1440p_to_540p_bicubic_sharp_letterboxed", dict(cformat=20, w=2560, h=1440, kind="noise", seed=322, dst=(960, 540), iDownscaling=4,
                                                                   window=(1000, 560), offset=(20, 9), exfmt=GOLDEN_CASES["c5_p010_hlg_lanczos3_2x"]["exfmt"])),
    # a horizontal flip is the X draw's table read from the other end (FillVertices swaps src_l / src_r): same kernel
    ("p010_pq_flipped_1080p_to_1500p_lanczos3", dict(cformat=2, w=1920, h=1080, kind="noise", seed=318, dst=(2666, 1500), iUpscaling=4, flip=1,
                                                     exfmt=GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]["exfmt"])),
    ("nv12_flipped_letterboxed_2x_catmull", dict(cformat=1, w=640, h=360, kind="noise", seed=319, dst=(1280, 720), iUpscaling=2, flip=1,
                                                 window=(1300, 740), offset=(9, 10), exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"])),
]


@pytest.mark.parametrize("label,c", STRIP_FULL)
def test_strip_kernel_whole_frame_vs_oracle(mpcvr, oracle, torch_cuda, label, c):
    """The arbitrary-ratio fused kernel (k_fused_strip) at real sizes, every output pixel against the oracle: 1.33x Lanczos3 and
    1.5x Hamming down of HDR10 P010 (the up1440 / down1440 bench workloads), an odd-sized letterboxed NV12 upscale (8-bit
    internal format, no final pass, generic epilogue), up along x / down along y in one frame (8-tap variant), and the 2x
    downscale the interpolation shader takes at 50 %.  <= 1 LSB, >= 99 % of the channels identical; MPCVR_FLAG_NO_STRIP must
    take the kernel out again (block convert + tiled two-draw kernel) under the same bar."""
    torch = torch_cuda
    from videorenderer_amd import api
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    # every render-target layout (run_layouts checks the bytes around the pixels): the right edge and the last strip at real widths
    strips = run_layouts(mpcvr, torch, c, extra_flags=api.FLAG_NO_PERIOD, what=label)
    tiled = run_layouts(mpcvr, torch, c, extra_flags=api.FLAG_NO_STRIP, what=label)
    for layout in LAYOUTS:
        (got, info), (alt, info_alt) = strips[layout], tiled[layout]
        assert "kernel=fused_strip" in info, info
        same = compare(got, want, f"{label} <{layout}> [{info}]", min_same=WHOLE_FRAME_FLOOR)
        assert "kernel=fused_" not in info_alt and info_alt.startswith("passes:convert,resizeX,resizeY"), info_alt
        same_alt = compare(alt, want, f"{label} <{layout}> [{info_alt}]", min_same=WHOLE_FRAME_FLOOR)
        print(f"{label} <{layout}>: identical channels strip {same:.6f}, tiled {same_alt:.6f}  [{info}]")


_SDR = GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]
_PQ = GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]["exfmt"]
_HLG = GOLDEN_CASES["c5_p010_hlg_lanczos3_2x"]["exfmt"]
PERIOD_CASES = [
    # (label, case, (P, Q, taps the kernel runs))
    ("p010_pq_540p_to_720p_lanczos3", dict(cformat=2, w=960, h=540, kind="noise", seed=401, dst=(1280, 720), iUpscaling=4, exfmt=_PQ), (4, 3, 5)),
    ("nv12_540p_to_720p_catmull_direct8", dict(cformat=1, w=960, h=540, kind="noise", seed=402, dst=(1280, 720), iUpscaling=2, exfmt=_SDR), (4, 3, 4)),
    ("p010_hlg_360p_to_540p_mitchell", dict(cformat=2, w=640, h=360, kind="noise", seed=403, dst=(960, 540), iUpscaling=1, exfmt=_HLG), (3, 2, 4)),
    ("yuv420p10_360p_to_540p_lanczos3_fixed", dict(cformat=20, w=640, h=360, kind="noise", seed=404, dst=(960, 540), iUpscaling=4, flags=1, exfmt=_SDR), (3, 2, 6)),
    ("p010_pq_1080p_to_720p_lanczos3_interp", dict(cformat=2, w=1920, h=1080, kind="noise", seed=405, dst=(1280, 720), iUpscaling=4, exfmt=_PQ), (2, 3, 5)),
    ("nv12_1080p_to_720p_lanczos2", dict(cformat=1, w=1920, h=1080, kind="noise", seed=406, dst=(1280, 720), iUpscaling=3, exfmt=_SDR), (2, 3, 4)),
    ("p010_pq_1080p_to_540p_catmull_at_50pct", dict(cformat=2, w=1920, h=1080, kind="noise", seed=407, dst=(960, 540), iUpscaling=2, exfmt=_PQ), (1, 2, 4)),
    ("yv12_1080p_to_540p_lanczos3_at_50pct", dict(cformat=14, w=1920, h=1080, kind="noise", seed=408, dst=(960, 540), iUpscaling=4, exfmt=_SDR), (1, 2, 5)),
    ("p010_pq_hdr_passthrough_540p_to_720p", dict(cformat=2, w=960, h=540, kind="noise", seed=409, dst=(1280, 720), iUpscaling=4, exfmt=_PQ, hdr_output=1, output_format=1), (4, 3, 5)),
    ("nv12_odd_width_letterboxed_540p_to_720p", dict(cformat=1, w=958, h=540, kind="noise", seed=410, dst=(1277, 720), iUpscaling=2, exfmt=_SDR,
                                                 window=(1300, 736), offset=(10, 7)), (4, 3, 4)),
    ("p010_pq_spline36_ext_540p_to_720p", dict(cformat=2, w=960, h=540, kind="noise", seed=411, dst=(1280, 720), iUpscaling=6, exfmt=_PQ), (4, 3, 6)),
    ("p210_pq_360p_to_540p_lanczos3", dict(cformat=6, w=640, h=360, kind="noise", seed=412, dst=(960, 540), iUpscaling=4, exfmt=_PQ), (3, 2, 5)),
    ("tiny_p010_48x30_to_64x40", dict(cformat=2, w=48, h=30, kind="noise", seed=413, dst=(64, 40), iUpscaling=4, exfmt=_PQ), (4, 3, 5)),
    # 3:1 — every third output row sits exactly on a texel centre and the fp32 texcoord picks its tap rows (period_centre)
    ("p010_pq_360p_to_1080p_lanczos3", dict(cformat=2, w=640, h=360, kind="noise", seed=414, dst=(1920, 1080), iUpscaling=4, exfmt=_PQ), (3, 1, 5)),
    ("nv12_240p_to_720p_catmull_direct8", dict(cformat=1, w=426, h=240, kind="noise", seed=415, dst=(1278, 720), iUpscaling=2, exfmt=_SDR), (3, 1, 4)),
    ("p010_hlg_360p_to_1080p_lanczos3_fixed", dict(cformat=2, w=640, h=360, kind="noise", seed=416, dst=(1920, 1080), iUpscaling=4, flags=1, exfmt=_HLG), (3, 1, 6)),
    ("p010_pq_720p_to_2160p_lanczos3", dict(cformat=2, w=1280, h=720, kind="noise", seed=417, dst=(3840, 2160), iUpscaling=4, exfmt=_PQ), (3, 1, 5)),
    ("p010_pq_flipped_540p_to_720p_lanczos3", dict(cformat=2, w=960, h=540, kind="noise", seed=418, dst=(1280, 720), iUpscaling=4, flip=1, exfmt=_PQ), (4, 3, 5)),
    ("nv12_flipped_odd_width_1080p_to_720p_catmull", dict(cformat=1, w=1918, h=1080, kind="noise", seed=419, dst=(1279, 720), iUpscaling=2, flip=1, exfmt=_SDR,
                                                          window=(1300, 736), offset=(10, 7)), (2, 3, 4)),
]


@pytest.mark.parametrize("label,c,pqn", PERIOD_CASES)
def test_period_kernel_vs_oracle_and_strip_kernel(mpcvr, oracle, torch_cuda, label, c, pqn):
    """The periodic-phase fused kernel (k_fused_period: the vertical window in registers, compile-time tap rows) at every ratio it is
    built for (4:3, 3:2, 2:3, 1:2, 3:1), 4 / 5 / 6 taps, the three table tails, both epilogues (integer final pass, straight UNORM store incl.
    R10G10B10A2), an odd width inside a larger window, a frame smaller than one strip: whole frames against the oracle (<= 1 LSB), and
    against k_fused_strip on the same launch (MPCVR_FLAG_NO_PERIOD), which reads the same tables at run time — the two may differ only
    where an FMA contracts differently, so their outputs are held to <= 1 LSB of each other too."""
    torch = torch_cuda
    from videorenderer_amd import api
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    periods = run_layouts(mpcvr, torch, c, extra_flags=api.FLAG_FORCE_PERIOD, what=label)       # (SDR + 4 taps: the planner's own choice is k_fused_strip)
    strips = run_layouts(mpcvr, torch, c, extra_flags=api.FLAG_NO_PERIOD, what=label)
    P, Q, nt = pqn
    for layout in LAYOUTS:             # (every render-target layout: `off8` is the 8-byte store of k_fused_period, `off4` its per-pixel one)
        (got, info), (alt, info_alt) = periods[layout], strips[layout]
        if nt == 6 or (nt == 4 and not has_tail(c)):     # (round 5: six taps — MPCVR_FLAG_LANCZOS3_FIXED, the Spline36 extension — have no periodic variant any
            # more; round 6: nor have four taps without a tail (SDR through Mitchell / Catmull-Rom / Lanczos2), where the strip kernel was the planner's choice anyway)
            assert "kernel=fused_strip(" in info, info
        else:
            assert kernel_under(layout, f"kernel=fused_period(rows={P}:{Q},taps={nt},") in info, (layout, info)
        assert "kernel=fused_strip(" in info_alt, info_alt
        if c.get("output_format", 0) == 1:
            compare_rgb10(got, want, f"{label} <{layout}> [{info}]", tail=has_tail(c), min_same=0.99)
            compare_rgb10(alt, want, f"{label} <{layout}> [{info_alt}]", tail=has_tail(c), min_same=0.99)
            continue
        floor = 0.99 if c["w"] < 100 else 0.998
        same = compare(got, want, f"{label} <{layout}> [{info}]", min_same=floor)
        same_alt = compare(alt, want, f"{label} <{layout}> [{info_alt}]", min_same=floor)
        compare(got, alt, f"{label} <{layout}> period vs strip", min_same=floor)
        print(f"PERIOD {label} <{layout}>: identical channels period {same:.6f}, strip {same_alt:.6f}  [{info}]")


PERIOD_SURFACE_CASES = [
    ("dovi_poly_540p_to_720p_lanczos3", dict(cformat=2, w=960, h=540, kind="hdr", seed=431, dst=(1280, 720), iUpscaling=4, exfmt=GOLDEN_CASES["dovi_poly_sdr"]["exfmt"], dovi=dict(kind="poly")), (4, 3, 5)),
    ("dovi_mmr_l2_1080p_to_720p", dict(cformat=2, w=1920, h=1080, kind="hdr", seed=432, dst=(1280, 720), iUpscaling=2, exfmt=GOLDEN_CASES["dovi_poly_sdr"]["exfmt"],
                                       dovi=dict(kind="mmr", l2=(100, 600, 1000))), (2, 3, 4)),
    ("nv12_catmull_chroma_360p_to_540p", dict(cformat=1, w=640, h=360, kind="noise", seed=433, dst=(960, 540), iUpscaling=4, iChromaScaling=2, exfmt=_SDR), (3, 2, 5)),
    ("p010_pq_catmull_chroma_1080p_to_540p", dict(cformat=2, w=1920, h=1080, kind="noise", seed=434, dst=(960, 540), iUpscaling=2, iChromaScaling=2, exfmt=_PQ), (1, 2, 4)),
    ("dovi_poly_flipped_540p_to_720p_lanczos3", dict(cformat=2, w=960, h=540, kind="hdr", seed=436, dst=(1280, 720), iUpscaling=4, flip=1, exfmt=GOLDEN_CASES["dovi_poly_sdr"]["exfmt"], dovi=dict(kind="poly")), (4, 3, 5)),
    # interleaved RGB without a convert draw: the source texture itself is the surface
    ("r210_540p_to_720p_lanczos3", dict(cformat=32, w=960, h=540, kind="noise", seed=437, dst=(1280, 720), iUpscaling=4), (4, 3, 5)),
    ("rgb32_360p_to_540p_catmull_letterboxed", dict(cformat=30, w=640, h=360, kind="noise", seed=438, dst=(960, 540), iUpscaling=2, window=(980, 560), offset=(10, 9)), (3, 2, 4)),
    # the draw's row map: a frame turned upside down, an RGB sample with a source rect
    ("p010_pq_rot180_540p_to_720p_lanczos3", dict(cformat=2, w=960, h=540, kind="noise", seed=439, dst=(1280, 720), iUpscaling=4, rotation=180, exfmt=_PQ), (4, 3, 5)),
    ("rgb32_source_rect_528_rows_to_704", dict(cformat=30, w=960, h=540, kind="noise", seed=440, src_rect=(16, 6, 944, 534), dst=(1237, 704), iUpscaling=4,
                                               window=(1244, 710), offset=(2, 3)), (4, 3, 5)),
    ("uyvy_catmull_chroma_540p_to_720p_10bit_target", dict(cformat=5, w=960, h=540, kind="noise", seed=435, dst=(1280, 720), iUpscaling=3, iChromaScaling=2, iTexFormat=10, output_format=1, exfmt=_SDR), (4, 3, 4)),
]


@pytest.mark.parametrize("label,c,pqn", PERIOD_SURFACE_CASES)
def test_period_kernel_from_a_surface(mpcvr, oracle, torch_cuda, label, c, pqn):
    """k_fused_period<..., SRC_SURFACE>: what its own convert stage does not take — Dolby Vision reshaping, Catmull-Rom chroma, packed
    4:2:2 with Catmull-Rom chroma — is converted by its own kernel into m_TexConvertOutput and the periodic-phase kernel runs both draws and
    the final pass from that surface (B8G8R8A8 / R10G10B10A2 texels -> window codes).  Whole frames against the oracle, and against
    k_fused_strip:surface on the same launch (MPCVR_FLAG_NO_PERIOD)."""
    torch = torch_cuda
    from videorenderer_amd import api
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    got, info = run_product(mpcvr, torch, c)
    P, Q, nt = pqn
    assert f"kernel=fused_period:surface(rows={P}:{Q},taps={nt}," in info, info
    alt, info_alt = run_product(mpcvr, torch, c, extra_flags=api.FLAG_NO_PERIOD)
    assert "kernel=fused_strip:surface(" in info_alt, info_alt
    if c.get("output_format", 0) == 1:
        compare_rgb10(got, want, f"{label} [{info}]", tail=has_tail(c), min_same=0.99)
        compare_rgb10(alt, want, f"{label} [{info_alt}]", tail=has_tail(c), min_same=0.99)
        return
    for out, tag in ((got, info), (alt, info_alt)):
        if has_tail(c):
            same, _ = compare_behind_tail(oracle, p, frame, pitch, out, want, f"{label} [{tag}]", min_same=DOVI_RESIZE_FLOOR if c.get("dovi") else WHOLE_FRAME_FLOOR, dovi=bool(c.get("dovi")))
        else:
            same = compare(out, want, f"{label} [{tag}]", min_same=WHOLE_FRAME_FLOOR)
        print(f"PERIOD:SURFACE {label}: identical channels {same:.6f}  [{tag}]")


@pytest.mark.parametrize("over,kernel", [
    (dict(iTexFormat=8), "kernel=fused_period("),            # 8-bit m_TexsPostScale in front of a 10-bit swap chain: the straight store's scale is the texture's
    (dict(iTexFormat=10), "kernel=fused_period("),
    (dict(iTexFormat=8, iChromaScaling=2), "kernel=fused_period:surface("),
    (dict(iTexFormat=8, dst=(1300, 733)), "kernel=fused_strip("),
])
def test_fused_resize_in_front_of_the_hdr10_tone_mapping_step(mpcvr, oracle, torch_cuda, over, kernel):
    """With an HDR10 tone-mapping operator (DX11VideoProcessor.cpp:3359-3367) the resize draws go into m_TexsPostScale (internal format)
    and the step writes the swap chain: the fused kernels then store straight into a texture whose format is NOT the swap chain's —
    a fuzz case (8-bit internal format, 10-bit target, 3:1) found the periodic-phase kernel scaling that store with the swap chain's
    quantiser.  Every fused tier against the plain kernels and the oracle."""
    torch = torch_cuda
    from videorenderer_amd import api
    c = dict(dict(cformat=2, w=960, h=540, kind="noise", seed=450, dst=(1280, 720), iUpscaling=4, exfmt=_PQ, hdr_output=1, output_format=1,
                  hdr_tonemap=6, hdr_display=400.0, hdr_meta=(0.005, 4000.0, 800.0, 0.0)), **over)
    got, info = run_product(mpcvr, torch, c)
    assert kernel in info and "hdr10tonemap" in info, info
    plain, _ = run_product(mpcvr, torch, c, extra_flags=api.FLAG_NO_FUSED)
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    # one code of the intermediate (the fused tiers' own bar) through an operator whose slope reaches ~3 at this display peak: 3 x 4 ten-bit
    # codes behind an 8-bit intermediate, 3 (+ its own rounding) behind a 10-bit one — the fuzz's bars
    lim = 12 if c["iTexFormat"] == 8 else 4
    for name, out in (("fused", got), ("plain", plain)):
        d = np.abs(_codes10(out) - _codes10(want))
        assert d.max() <= lim and float((d == 0).mean()) >= 0.97, f"{name} [{info}]: max {int(d.max())}, identical {float((d == 0).mean()):.4f}"
    d = np.abs(_codes10(got) - _codes10(plain))
    assert d.max() <= lim and float((d == 0).mean()) >= 0.97, f"fused vs plain [{info}]: max {int(d.max())}, identical {float((d == 0).mean()):.4f}"


@pytest.mark.parametrize("over,kernel", [
    (dict(), "kernel=fused_period("),
    (dict(flip=1), "kernel=fused_period("),                                         # flipped: the X tables read from the other end, still one launch per batch
    (dict(cformat=1, iChromaScaling=2, exfmt=_SDR, flip=1), "kernel=fused_period:surface("),      # convert kernel per batch + the surface variant per batch
    (dict(cformat=1, iChromaScaling=2, exfmt=_SDR, dst=(1300, 700), flip=1), "kernel=fused_strip:surface("),
    (dict(rotation=180), "kernel=fused_period:surface("),                                           # upside down: the row map of the surface variant
    (dict(rotation=180, flip=1, dst=(1300, 733)), "kernel=fused_strip:surface("),
    # interleaved RGB without a convert draw: a repack launch per frame into a batch texture, ONE resize launch per batch
    (dict(cformat=30, exfmt=None), "kernel=fused_period:surface("),
    (dict(cformat=32, exfmt=None, src_rect=(8, 4, 952, 536), dst=(1300, 733)), "kernel=fused_strip:surface("),
    (dict(cformat=29, exfmt=None, dst=(1301, 733), window=(1320, 740), offset=(6, 3)), "kernel=fused_strip:surface("),
    # v210: a repack launch per frame into the batch texture (CopyFrameV210), then the whole-batch launches of any 4:2:2 sample
    (dict(cformat=10), "kernel=fused_period("),
    (dict(cformat=10, dst=(1920, 1080)), "fused_up2x"),
    (dict(cformat=10, dst=(960, 540)), "direct:convert"),
    (dict(cformat=10, dst=(1300, 733), iChromaScaling=2), "kernel=fused_strip:surface("),
])
def test_period_kernel_batches_equal_single_frames(mpcvr, torch_cuda, over, kernel):
    """mpcvr_process_batch through the periodic-phase kernel (and, flipped, through the strip kernel's surface variant): every frame of
    a batch equals its single-frame result bit for bit."""
    torch = torch_cuda
    from videorenderer_amd import api
    c = dict(dict(cformat=2, w=960, h=540, kind="noise", seed=420, dst=(1280, 720), iUpscaling=4, exfmt=_PQ), **over)
    if c["exfmt"] is None:
        del c["exfmt"]
    vp, (ww, wh) = make_vp(mpcvr, c)
    frames = [torch.from_numpy(case_frame(dict(c, seed=420 + i))[0]).cuda() for i in range(5)]
    pitch = case_frame(c)[1]
    singles = []
    for f in frames:
        d = torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda")
        vp.CopySample(f, pitch)
        vp.Process(d, ww * 4)
        singles.append(d)
    vp.Synchronize()
    assert kernel in vp.GetVPInfo(), vp.GetVPInfo()
    outs = [torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda") for _ in frames]
    vp.ProcessBatch(frames, outs, ww * 4)
    vp.Synchronize()
    for a, b in zip(singles, outs):
        assert torch.equal(a, b)
    whole = vp.GetLastBatchInfo()
    # the targets as slices of one patterned buffer with mixed first bytes: `off8`'s pitch, then `off4`'s
    for layout in ("off8", "off4"):
        mixed = batch_vs_singles_in_carved_targets(torch, vp, frames, pitch, ww, wh, layout_of(layout, ww)[1], MIXED_BASES[:5], f"{over} <{layout}>")
        assert kernel_under("off4", kernel) in vp.GetVPInfo(), (layout, vp.GetVPInfo())        # (a target at +4: the 8-byte stores step aside)
        # (still one launch per stage — except same-size frames: the block convert needs 16-byte targets, so such a batch declines to frame by frame)
        assert mixed["frames"] == 5 and (mixed["launches"] == whole["launches"] or kernel == "direct:convert"), (layout, whole, mixed)
    vp.close()


# Same-size frames (DirectConvert) are the one route a misaligned target takes away: k_convert_blocks stores 16 bytes per lane and has no
# per-pixel epilogue, so a batch with such a target goes frame by frame — its aligned frames through k_convert_blocks, the others through
# the per-pixel convert kernel, each as the single frame into that target would.
MIXED_ALIGNMENT_DECLINES = ("DirectConvert",)
MIXED_ALIGNMENT_ROUTES = {
    # route: (case, extra flags, the GetVPInfo fragment of an aligned batch)
    "FusedUp2x": (GOLDEN_CASES["noise_p010_pq_lanczos3_2x"], 0, "fused_up2x"),
    "Strip:k_fused_strip": (dict(cformat=2, w=960, h=540, kind="noise", seed=420, dst=(1300, 733), iUpscaling=4, exfmt=_PQ), 0, "kernel=fused_strip("),
    "Strip:k_fused_period": (dict(cformat=2, w=960, h=540, kind="noise", seed=420, dst=(1280, 720), iUpscaling=4, exfmt=_PQ), 0, "kernel=fused_period("),
    "DirectConvert": (GOLDEN_CASES["c1_nv12_bt709_passthrough"], 0, "direct:convert"),
    "WholeBatchLaunches": (GOLDEN_CASES["down_lanczos_2p5x"], 64, "passes:"),                       # 64 = NO_STRIP: block convert + tiled two-draw kernel
    "StripToneMap": (GOLDEN_CASES["hdrout_tm2_reinhard"], 0, "hdr10tonemap"),
    "RgbSurfaceStrip": (dict(cformat=30, w=960, h=540, kind="noise", seed=420, dst=(1280, 720), iUpscaling=4), 0, "kernel=fused_period:surface("),
    "ErrorDiffusion": (dict(GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"], bUseDither=2), 0, "errdiff"),
}


@pytest.mark.parametrize("order", ["aligned_first_misaligned_later", "misaligned_first_aligned_later"])
@pytest.mark.parametrize("route", sorted(MIXED_ALIGNMENT_ROUTES))
def test_batch_whose_targets_differ_in_alignment(mpcvr, torch_cuda, route, order):
    """The launch parameters of a batch are planned from its FIRST target; the epilogue has to be the one its worst-aligned target allows.
    Per whole-batch route: a batch whose first target sits on a 256-byte boundary and whose later ones do not, and the other way round, at a
    pitch that is a multiple of 16 (the aligned targets alone would take the 16-byte stores).  Every frame must equal the frame drawn alone,
    the bytes around every target must keep their pattern, and the batch must stay on its whole-batch route (a handful of launches;
    MIXED_ALIGNMENT_DECLINES names the one route that steps aside)."""
    torch = torch_cuda
    c, flags, fragment = MIXED_ALIGNMENT_ROUTES[route]
    vp, (ww, wh) = make_vp(mpcvr, c, flags)
    c = dict(c, kind="noise")
    frames = [torch.from_numpy(case_frame(dict(c, seed=c["seed"] + 100 * i))[0]).cuda() for i in range(5)]
    pitch = vp.GetFrameBytes()[1]
    dst_pitch = layout_of("padded16", ww)[1]
    # what an aligned batch of this case runs (the route under test), then the mixed one
    aligned = CarvedTargets(torch, ww, wh, dst_pitch, [0] * 5)
    vp.ProcessBatch(frames, aligned.ptrs, dst_pitch)
    vp.Synchronize()
    aligned.assert_guards_intact(f"{route}: aligned batch")
    info, whole = vp.GetVPInfo(), vp.GetLastBatchInfo()
    assert fragment in info and whole["frames"] == 5 and whole["launches"] <= 4, (route, info, whole)
    bases = (0, 4, 0, 8, 4) if order.startswith("aligned") else (4, 0, 0, 8, 0)
    mixed = batch_vs_singles_in_carved_targets(torch, vp, frames, pitch, ww, wh, dst_pitch, bases, f"{route} {order}")
    info = vp.GetVPInfo()
    vp.close()
    assert kernel_under("off4", fragment) in info, (route, order, info)
    if route in MIXED_ALIGNMENT_DECLINES:
        assert mixed["frames"] == 5 and mixed["launches"] == 5, (route, order, info, mixed)
    else:
        assert mixed["frames"] == 5 and mixed["launches"] <= 4, (route, order, info, mixed)


# ---- instantiation sweeps: every template instantiation of the two headline kernel families is launched by the suite ----
# (tests/test_kernel_coverage.py checks it against the kernel trace of the suite: a planner typo cannot select a variant nothing ran)
_SWEEP_TAILS = {"none": (_SDR, 0), "pq": (_PQ, 0), "hlg": (_HLG, 0), "alu": (_PQ, 4)}          # name -> (extfmt, extra flags: 4 = MPCVR_FLAG_NO_LUT)
_SWEEP_TAPS = {4: dict(iUpscaling=2), 5: dict(iUpscaling=4), 6: dict(iUpscaling=4, flags=1)}   # Catmull-Rom, Lanczos3 (Q1 folded), Lanczos3 fixed
# (source, epilogue) pairs the launchers instantiate: name -> (cformat, case overrides)
_SWEEP_UP2X_SRC = {
    "p01x_dither8": (2, {}), "p01x_direct10": (2, dict(output_format=1, hdr_output_if_tail=1)), "p01x_generic": (2, dict(misalign=1)),
    "nv12_direct8": (1, {}), "nv12_generic": (1, dict(misalign=1)),
    "planar16_dither8": (20, {}), "planar8_direct8": (14, {}),
    "generic_dither8": (8, {}), "generic_generic": (8, dict(misalign=1)),          # Y210: packed 4:2:2 reads its layout at run time
}
# The exact-form twins (round 5: kernels that can meet an 8-bit internal format in front of a resize exist twice — k_*<..., XC_ALWAYS> where
# FusedArgs::exact_cv asks for the convert stage that rounds like the reference's, <..., XC_NEVER> otherwise; tail-less only).  The pairs
# above run the 8-bit loaders in their exact form (AUTO = an 8-bit internal format) and the run-time loader in the fast one (Y210: 10 bits);
# these are the other halves: the 8-bit loaders behind a forced 10-bit internal format and a 10-bit target (no final pass: the straight and
# the generic store), the run-time loader behind an 8-bit one (YUY2).
_SWEEP_UP2X_TWINS = {
    "nv12_direct10_fast": (1, dict(iTexFormat=10, output_format=1)), "nv12_generic10_fast": (1, dict(iTexFormat=10, output_format=1, misalign=1)),
    "planar8_direct10_fast": (14, dict(iTexFormat=10, output_format=1)), "generic_generic8_exact": (4, dict(misalign=1)),
}
_SWEEP_PERIOD_TWINS = {"nv12_direct10_fast": (1, dict(iTexFormat=10, output_format=1)), "generic_direct10_fast": (14, dict(iTexFormat=10, output_format=1))}
_SWEEP_STRIP_TWINS = dict(_SWEEP_UP2X_TWINS, planar8_generic10_fast=(14, dict(iTexFormat=10, output_format=1, misalign=1)),
                          generic_direct10_fast=(8, dict(output_format=1)), generic_direct8_exact=(4, {}))
_SWEEP_PERIOD_SRC = {"p01x_dither8": (2, {}), "p01x_direct10": (2, dict(output_format=1, hdr_output_if_tail=1)), "nv12_direct8": (1, {}),
                     "generic_dither8": (20, {}), "generic_direct8": (14, {})}
_SWEEP_PERIOD_GEO = {"4:3": ((48, 30), (64, 40)), "3:2": ((48, 32), (72, 48)), "2:3": ((96, 48), (64, 32)), "1:2": ((96, 48), (48, 24)), "3:1": ((32, 16), (96, 48))}


def _sweep_case(cformat, over, tail, taps, src_wh, dst_wh, seed):
    ex, tflags = _SWEEP_TAILS[tail]
    c = dict(cformat=cformat, w=src_wh[0], h=src_wh[1], kind="noise", seed=seed, dst=dst_wh, exfmt=ex)
    c.update(_SWEEP_TAPS[taps])
    c["flags"] = c.get("flags", 0) | tflags
    if over.get("output_format"):
        c["output_format"] = 1          # R10G10B10A2 target, no final pass: the straight 10-bit store
    if over.get("iTexFormat"):
        c["iTexFormat"] = over["iTexFormat"]
    if over.get("misalign"):            # a window column that is not a multiple of 4: the generic epilogue
        c["window"] = (dst_wh[0] + 8, dst_wh[1] + 4); c["offset"] = (2, 1)
    return c


def _tiers_agree(mpcvr, torch, c, fast_flags, expect):
    from videorenderer_amd import api
    # every render-target layout, both tiers: a source / epilogue pair whose specialised store needs an aligned target runs its generic twin
    # under `off4` / `off8` (run_layouts checks the bytes around the pixels; the oracle's frame is computed once)
    fast = run_layouts(mpcvr, torch, c, extra_flags=fast_flags, what=f"{expect} sweep {c}")
    plain = run_layouts(mpcvr, torch, c, extra_flags=api.FLAG_NO_FUSED, what=f"plain tier {c}")
    # Round 6: the plain tier carries the ORACLE's bits (tails included), so "the fast tier within the bar of the plain one" below IS "within the
    # bar of the oracle" — checked here on every sweep case instead of assumed (round 5's review: ~90 sweep tests compared two GPU tiers only)
    from oracle import oracle as O
    frame, pitch = case_frame(c)
    po = oracle_params(O, c)
    want = O.process(po, frame, pitch, dst=np.full((po.window_h, po.window_w, 4), BG, dtype=np.uint8))
    for layout in LAYOUTS:
        (got, info), (ref, info_ref) = fast[layout], plain[layout]
        assert kernel_under(layout, expect) in info, (c, layout, info)
        assert info_ref.startswith("passes:"), info_ref
        if c.get("output_format", 0) == 1:
            assert np.array_equal(_codes10(ref), _codes10(want)), (c, layout, info_ref, "plain tier != oracle")
        else:
            assert np.array_equal(ref[..., :3], want[..., :3]), (c, layout, info_ref, "plain tier != oracle", int(np.abs(ref[..., :3].astype(int) - want[..., :3].astype(int)).max()))
        if c.get("output_format", 0) == 1:
            g, r = got.view(np.uint32)[..., 0], ref.view(np.uint32)[..., 0]
            lim = 5 if internal_is_8bit(c) else 2 if has_tail(c) else 1
            if c.get("iUpscaling") == 5:     # Jinc2m's weights sum to |w| = 1.9: one code of the block convert in the 10-bit texture comes out as up to two
                lim = max(lim, 2)
            for sh in (0, 10, 20):
                d = np.abs(((g >> sh) & 1023).astype(np.int32) - ((r >> sh) & 1023).astype(np.int32))
                assert d.max() <= lim, (c, layout, info, int(d.max()))
        else:
            d = np.abs(got[..., :3].astype(np.int16) - ref[..., :3].astype(np.int16))
            assert d.max() <= 1, (c, layout, info, int(d.max()), int((d > 1).sum()))        # two GPU tiers of one frame
            assert np.array_equal(got[..., 3], ref[..., 3])


@pytest.mark.parametrize("taps", sorted(_SWEEP_TAPS))
@pytest.mark.parametrize("tail", sorted(_SWEEP_TAILS))
def test_sweep_every_fused_up2x_instantiation(mpcvr, torch_cuda, tail, taps):
    """k_fused_up2x<taps, tail, source, epilogue>: all nine (source, epilogue) pairs the launcher instantiates, per tap count and tail
    kind, on small frames against the plain kernels of the same frame."""
    for i, (name, (cf, over)) in enumerate(sorted(_SWEEP_UP2X_SRC.items()) + (sorted(_SWEEP_UP2X_TWINS.items()) if tail == "none" else [])):
        c = _sweep_case(cf, over, tail, taps, (64, 40), (128, 80), 500 + 17 * i + taps)
        _tiers_agree(mpcvr, torch_cuda, c, 0, "fused_up2x")


_SWEEP_JINC_SRC = {"p01x_dither8": (2, {}), "p01x_generic": (2, dict(misalign=1)), "p01x_direct10": (2, dict(output_format=1)),
                   "generic_dither8": (20, {}), "generic_generic": (20, dict(misalign=1))}
_SWEEP_JINC_TAIL_LESS = {"nv12_direct8": (1, {}), "nv12_generic": (1, dict(misalign=1)), "nv12_direct10_fast": (1, dict(iTexFormat=10, output_format=1)),
                         "nv12_generic10_fast": (1, dict(iTexFormat=10, output_format=1, misalign=1)), "generic_generic8_exact": (4, dict(misalign=1)),
                         "planar8_direct8": (14, {})}


@pytest.mark.parametrize("tail", sorted(_SWEEP_TAILS))
def test_sweep_every_fused_jinc_instantiation(mpcvr, torch_cuda, tail):
    """k_fused_jinc2x<tail, source, epilogue[, exact form]> (vp_fused_jinc.hip: convert + the one-draw Jinc2m at exactly 2x + final pass in one
    kernel): every (source, epilogue) pair the launcher instantiates per tail kind — and, without a tail, NV12's own loader and both halves
    of the exact-form twins — against the per-pixel kernels of the same frame."""
    items = sorted(_SWEEP_JINC_SRC.items()) + (sorted(_SWEEP_JINC_TAIL_LESS.items()) if tail == "none" else [])
    for i, (name, (cf, over)) in enumerate(items):
        ex, tflags = _SWEEP_TAILS[tail]
        c = dict(cformat=cf, w=64, h=40, kind="noise", seed=1500 + 7 * i, dst=(128, 80), exfmt=ex, iUpscaling=5, flags=tflags)
        for k in ("output_format", "iTexFormat"):
            if over.get(k):
                c[k] = over[k]
        if over.get("misalign"):
            c["window"] = (136, 84); c["offset"] = (2, 1)
        _tiers_agree(mpcvr, torch_cuda, c, 0, "fused_jinc2x")


def test_two_draw_jinc_whose_one_to_one_axis_sits_on_the_floor_step(mpcvr, oracle, torch_cuda):
    """fuzz_strip.py's Jinc2m mode, seed 9, case 3109: X downscaled by the convolution shader, Y exactly 2x by Jinc2m — the second draw runs 1:1
    along x over an 88-texel-wide texture, where Tex * wh of four columns lands one ulp below k + 0.5 and the shader's 4 x 4 window sits one
    texel further left.  The phase-table kernels took the tap base from org + (o + 0.5) * step (up to 53 codes off in those columns on every
    tier but the plain one); BuildJincPhases now checks every output index against TexCenter and leaves such a draw to the per-pixel kernel."""
    c = dict(cformat=15, w=438, h=68, kind="noise", seed=426369876, exfmt=_SDR, iChromaScaling=2, iUpscaling=5, iDownscaling=3, bInterpolateAt50pct=0,
             src_rect=(40, 14, 258, 68), dst=(88, 108))
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    from videorenderer_amd import api
    for flags in (0, api.FLAG_NO_FAST_CONVERT, api.FLAG_NO_STRIP):
        got, info = run_product(mpcvr, torch_cuda, c, extra_flags=flags)
        compare(got, want, f"two-draw Jinc2m, 1:1 axis on the floor step [{info}] flags={flags}", min_same=0.99)


def test_block_convert_in_front_of_a_tone_mapping_operator_carries_the_exact_codes(mpcvr, torch_cuda):
    """fuzz_strip.py with the tier flags on the product side, seed 208, case 600: HDR10 output through tone-mapping operator 5 — one code of the
    10-bit intermediate by which the block convert (contracted FMAs) differed from the per-pixel convert came out of the operator's curve as
    FIVE ten-bit codes.  Plans with an operator now take the exact form of the convert stage for 10-bit internal formats too
    (FusedParams::exact_wide): the tier with the block convert and the tier with the per-pixel convert draw the same frame, bit for bit."""
    from videorenderer_amd import api
    c = dict(cformat=2, w=608, h=156, kind="noise", seed=173819605, exfmt=2051155200, iChromaScaling=2, iUpscaling=2, iDownscaling=5, bInterpolateAt50pct=0,
             dst=(137, 332), rotation=90, hdr_output=1, output_format=1, hdr_tonemap=5, hdr_display=400.0, hdr_meta=(0.005, 4000.0, 0.0, 0.0))
    block, info_b = run_product(mpcvr, torch_cuda, c)
    pixel, info_p = run_product(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FAST_CONVERT)
    assert "hdr10tonemap" in info_b and "hdr10tonemap" in info_p, (info_b, info_p)
    assert np.array_equal(block, pixel), f"{(block != pixel).any(axis=2).sum()} pixels differ between the block convert and the per-pixel convert in front of the operator"
    for cf, chroma in ((2, 1), (1, 1), (20, 2)):        # bilinear chroma, an 8-bit source, three planes: the other loaders' exact twins in front of an operator
        c2 = dict(c, cformat=cf, iChromaScaling=chroma, rotation=0, dst=(760, 208), w=608, h=156)
        if cf == 1:
            c2["iTexFormat"] = 10
        block, _ = run_product(mpcvr, torch_cuda, c2)
        pixel, _ = run_product(mpcvr, torch_cuda, c2, extra_flags=api.FLAG_NO_FAST_CONVERT | api.FLAG_NO_STRIP)
        ref, _ = run_product(mpcvr, torch_cuda, c2, extra_flags=api.FLAG_NO_FUSED)
        g, r = block.view(np.uint32)[..., 0], ref.view(np.uint32)[..., 0]
        d = max(int(np.abs(((g >> sh) & 1023).astype(np.int32) - ((r >> sh) & 1023).astype(np.int32)).max()) for sh in (0, 10, 20))
        assert d <= 2, (cf, d)          # the fused resize tiers keep their own <= 1-code bar on the post-scale texture; the operator may double it


def test_jinc_quad_kernel_behind_a_convert_kernel_of_its_own(mpcvr, torch_cuda):
    """k_jinc2_quad (vp_jinc.hip) still draws the exact-2x Jinc2m frames the fused kernel does not take: Catmull-Rom chroma (the convert is a
    kernel of its own; 8-bit texture, straight store and 10-bit texture, integer final pass) and interleaved RGB (no convert at all)."""
    for i, (cf, over) in enumerate(((1, dict(iChromaScaling=2)), (2, dict(iChromaScaling=2)), (30, {}))):
        c = dict(cformat=cf, w=64, h=40, kind="noise", seed=1600 + i, dst=(128, 80), exfmt=0 if cf == 30 else _SDR, iUpscaling=5, **over)
        _tiers_agree(mpcvr, torch_cuda, c, 0, "passes:")


@pytest.mark.parametrize("taps", sorted(_SWEEP_TAPS))
@pytest.mark.parametrize("tail", ["none", "pq", "hlg"])
@pytest.mark.parametrize("ratio", sorted(_SWEEP_PERIOD_GEO))
def test_sweep_every_fused_period_instantiation(mpcvr, torch_cuda, ratio, tail, taps):
    """k_fused_period<P, Q, taps, tail, source, epilogue>: the five (source, epilogue) pairs per ratio, tap count and table tail
    (MPCVR_FLAG_FORCE_PERIOD: the planner's own choice for SDR content with 4 taps is k_fused_strip)."""
    from videorenderer_amd import api
    src_wh, dst_wh = _SWEEP_PERIOD_GEO[ratio]
    for i, (name, (cf, over)) in enumerate(sorted(_SWEEP_PERIOD_SRC.items()) + (sorted(_SWEEP_PERIOD_TWINS.items()) if tail == "none" else [])):
        c = _sweep_case(cf, over, tail, taps, src_wh, dst_wh, 700 + 13 * i + taps)
        # (six taps — the as-intended Lanczos3 of MPCVR_FLAG_LANCZOS3_FIXED, Spline36 — have no periodic variant since round 5: the strip kernel draws them)
        # (... and four taps without a tail since round 6)
        periodic = taps == 5 or (taps == 4 and tail != "none")
        _tiers_agree(mpcvr, torch_cuda, c, api.FLAG_FORCE_PERIOD, ("kernel=fused_period(rows=" + ratio) if periodic else "kernel=fused_strip(")
    if tail == "none":      # SRC_SURFACE (no tail of its own): Catmull-Rom chroma puts the convert into its own kernel; 8-bit surface -> straight store, 10-bit -> final pass
        for i, cf in enumerate((1, 2)):
            c = _sweep_case(cf, {}, "none", taps, src_wh, dst_wh, 800 + i + taps)
            c["iChromaScaling"] = 2
            _tiers_agree(mpcvr, torch_cuda, c, 0, ("kernel=fused_period:surface(rows=" + ratio) if taps != 6 else "kernel=fused_strip:surface(")


_SWEEP_STRIP_SRC = dict(_SWEEP_UP2X_SRC, planar16_generic=(20, dict(misalign=1)), planar8_generic=(14, dict(misalign=1)), p01x_direct10=(2, dict(output_format=1)))
_SWEEP_STRIP_GEO = {4: ((64, 40), (100, 62), dict(iUpscaling=2)), 6: ((64, 40), (100, 62), dict(iUpscaling=4)),
                    8: ((208, 104), (80, 40), dict(iDownscaling=2)),          # Hamming 2.6x down: 7 taps -> the 8-tap variant
                    16: ((208, 104), (80, 40), dict(iDownscaling=3))}         # bicubic 2.6x down: 13 taps -> the 16-tap variant


@pytest.mark.parametrize("taps", sorted(_SWEEP_STRIP_GEO))
@pytest.mark.parametrize("tail", sorted(_SWEEP_TAILS))
def test_sweep_fused_strip_instantiations(mpcvr, torch_cuda, tail, taps):
    """k_fused_strip<taps, px per lane, tail, source, epilogue> at a ratio that is no period (1.5625 / 2.6x): every source specialisation
    with every epilogue it can meet (integer final pass, straight 8- / 10-bit store, the generic store behind a misaligned window
    column), per tap count and tail kind, against the plain kernels of the same frame."""
    src_wh, dst_wh, scaler = _SWEEP_STRIP_GEO[taps]
    for i, (name, (cf, over)) in enumerate(sorted(_SWEEP_STRIP_SRC.items()) + (sorted(_SWEEP_STRIP_TWINS.items()) if tail == "none" else [])):
        ex, tflags = _SWEEP_TAILS[tail]
        c = dict(cformat=cf, w=src_wh[0], h=src_wh[1], kind="noise", seed=900 + 11 * i + taps, dst=dst_wh, exfmt=ex, flags=tflags, **scaler)
        if over.get("output_format"):
            c["output_format"] = 1
        if over.get("iTexFormat"):
            c["iTexFormat"] = over["iTexFormat"]
        if over.get("misalign"):
            c["window"] = (dst_wh[0] + 8, dst_wh[1] + 4); c["offset"] = (3, 1)
        _tiers_agree(mpcvr, torch_cuda, c, 0, "kernel=fused_strip(")


@pytest.mark.parametrize("label,cf,over", [
    ("nv12_bilinear", 1, dict(w=66)), ("nv12_catmull", 1, dict(w=66, iChromaScaling=2)),
    ("yv12_bilinear", 14, dict(w=72)), ("yv12_catmull", 14, dict(w=72, iChromaScaling=2)),
    ("nv12_centred_bilinear", 1, dict(w=66, chroma_loc=1)), ("nv12_centred_catmull", 1, dict(w=66, chroma_loc=1, iChromaScaling=2)),
    ("p010_tex8_catmull", 2, dict(w=66, iTexFormat=8, iChromaScaling=2)),
])
def test_sweep_exact_twins_of_the_block_convert_kernel(mpcvr, torch_cuda, label, cf, over):
    """k_convert_blocks<TAILK_NONE, source, no final pass, no DV, chroma filter, XC_ALWAYS>: a convert draw of its own into an 8-bit internal
    format with a resize behind it — Catmull-Rom chroma (no fused kernel takes it), or the fused kernels switched off — for the NV12, the
    three-plane and the run-time loader (centred chroma; 16-bit samples behind a forced 8-bit format).  (The XC_NEVER halves are the
    same-size cases of the kernel-family sweep: blocks_*_final0.)"""
    from videorenderer_amd import api
    c = dict(cformat=cf, h=48, kind="noise", seed=970 + len(label), dst=(100, 62), iUpscaling=2, exfmt=_SDR, **over)
    if "chroma_loc" in c:           # (the chroma siting field of DXVA2_ExtendedFormat: bits 8..11)
        c["exfmt"] = (c["exfmt"] & ~(0xf << 8)) | (c.pop("chroma_loc") << 8)
    for fast_flags in (0, api.FLAG_NO_STRIP):
        _tiers_agree(mpcvr, torch_cuda, c, fast_flags, "")


@pytest.mark.parametrize("tail", sorted(_SWEEP_TAILS))
def test_sweep_wide_block_convert_instantiations(mpcvr, torch_cuda, tail):
    """k_convert_blocks_wide<tail, source, final> (same-size frames, four 2x2 blocks per lane): P01x and NV12, each into a final pass
    (10-bit internal format — forced for NV12 — and an 8-bit target) and into a straight store."""
    ex, tflags = _SWEEP_TAILS[tail]
    for i, (cf, over) in enumerate(((2, {}), (2, dict(output_format=1)), (1, {}), (1, dict(iTexFormat=10)))):
        c = dict(cformat=cf, w=256, h=64, kind="noise", seed=960 + i, dst=(256, 64), exfmt=ex, flags=tflags, **over)
        _tiers_agree(mpcvr, torch_cuda, c, 0, "direct:convert")


SURFACE_STRIP = [
    ("r210_1080p_to_1440p", dict(cformat=32, w=1920, h=1080, kind="noise", seed=331, dst=(2560, 1440), iUpscaling=4)),
    ("y216_catmull_chroma_720p_to_1080p_hamming_down_y", dict(cformat=9, iChromaScaling=2, w=1280, h=1440, kind="noise", seed=332, dst=(1920, 1080), iUpscaling=2, iDownscaling=2,
                                                exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"])),
    ("rgb32_crop_1080p_to_1440p", dict(cformat=30, w=1920, h=1080, kind="noise", seed=333, src_rect=(16, 8, 1904, 1072), dst=(2511, 1419), iUpscaling=4,
                                       window=(2560, 1440), offset=(21, 11))),
    ("nv12_catmull_chroma_1080p_to_1440p_fp16", dict(cformat=1, w=1920, h=1080, kind="noise", seed=334, dst=(2560, 1440), iUpscaling=3, iChromaScaling=2,
                                                     iTexFormat=16, exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"])),
    ("rgb32_flipped_crop_720p_to_1000p", dict(cformat=30, w=1280, h=720, kind="noise", seed=335, src_rect=(10, 6, 1270, 714), dst=(1777, 1000), iUpscaling=4, flip=1)),
    # rotation 180: the X tables from the other end AND the first draw's row map reversed — a 4:2:0 source then takes its convert kernel
    # and this variant instead of the strip kernel's own convert stage
    ("p010_pq_rot180_1080p_to_1440p", dict(cformat=2, w=1920, h=1080, kind="noise", seed=336, dst=(2560, 1440), iUpscaling=4, rotation=180,
                                           exfmt=GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]["exfmt"])),
    ("nv12_rot180_flipped_720p_to_1000p_letterboxed", dict(cformat=1, w=1280, h=720, kind="noise", seed=337, dst=(1778, 1000), iUpscaling=2, rotation=180, flip=1,
                                                           window=(1800, 1020), offset=(12, 9), exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"])),
    ("rgb32_rot180_720p_to_1000p", dict(cformat=30, w=1280, h=720, kind="noise", seed=338, dst=(1778, 1000), iUpscaling=4, rotation=180)),
]


@pytest.mark.parametrize("label,c", SURFACE_STRIP)
def test_strip_kernel_from_a_surface_whole_frame(mpcvr, oracle, torch_cuda, label, c):
    """The arbitrary-ratio fused kernel WITHOUT its convert stage: what the block convert inside the strip kernel does not take
    (Catmull-Rom chroma, an fp16 internal format) goes through its convert kernel into m_TexConvertOutput and from there through
    k_fused_strip<SRC_SURFACE>; an interleaved RGB sample (no convert draw at all, a source rect => the draw's row map) is
    sampled in place.  Whole frames against the oracle, and against the tiled two-draw kernel it replaces (bit-exact with the
    plain kernels on this SDR content): <= 1 LSB, >= 99 % identical."""
    torch = torch_cuda
    from videorenderer_amd import api
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    surf = run_layouts(mpcvr, torch, c, extra_flags=api.FLAG_NO_PERIOD, what=label)      # (4:3 and friends would go to k_fused_period:surface)
    tiled = run_layouts(mpcvr, torch, c, extra_flags=api.FLAG_NO_STRIP, what=label)
    for layout in LAYOUTS:             # every render-target layout (run_layouts checks the bytes around the pixels)
        (got, info), (alt, info_alt) = surf[layout], tiled[layout]
        assert "kernel=fused_strip:surface" in info, info
        same = compare(got, want, f"{label} <{layout}> [{info}]", min_same=WHOLE_FRAME_FLOOR)
        assert "kernel=" not in info_alt, info_alt
        if has_tail(c) or (c.get("rotation") and c["cformat"] < 29):
            # (a 4:2:0 source turned by 180 degrees: the alternative is the fused block convert + the tiled kernel — a fused tier, <= 1 LSB)
            compare(alt, want, f"{label} <{layout}> [{info_alt}]", min_same=WHOLE_FRAME_FLOOR)
        else:
            compare(alt, want, f"{label} <{layout}> [{info_alt}]", exact=True)
        print(f"{label} <{layout}>: identical channels {same:.6f}  [{info}]")


def _cr_cases():
    from tests.golden.cases import ext, MPEG1, MPEG2, COSITED, TV, FULL, M709, M2020, P2020, TPQ
    return [
        ("nv12_mpeg2_same_size", dict(cformat=1, w=1920, h=1080, kind="noise", seed=341, dst=(1920, 1080), exfmt=ext(MPEG2, TV, M709))),
        ("p010_cosited_pq_same_size", dict(cformat=2, w=1920, h=1080, kind="noise", seed=342, dst=(1920, 1080), exfmt=ext(COSITED, TV, M2020, P2020, TPQ))),
        ("yuv420p10_mpeg1_to_1440p", dict(cformat=20, w=1920, h=1080, kind="noise", seed=343, dst=(2560, 1440), iUpscaling=4, exfmt=ext(MPEG1, FULL, M709))),
        ("yv12_mpeg2_rect_down", dict(cformat=14, w=1920, h=1080, kind="noise", seed=344, src_rect=(8, 4, 1912, 1076), dst=(1270, 716), iDownscaling=2,
                                      exfmt=ext(MPEG2, TV, M709))),
    ]


@pytest.mark.parametrize("label,c", _cr_cases())
def test_catmull_rom_chroma_block_convert_whole_frame(mpcvr, oracle, torch_cuda, label, c):
    """CHROMA_CatmullRom on the 2x2-block convert (round 2: a block's four pixels share one 4-column x 5-row chroma
    neighbourhood; weights per column / row parity and siting from the shader's own expressions): bi-planar and three-plane
    sources, all three sitings, same size (one kernel) and in front of a resize (block convert -> k_fused_strip:surface), whole
    1080p frames against the oracle — and against the per-pixel kernel it replaces (MPCVR_FLAG_NO_FAST_CONVERT)."""
    torch = torch_cuda
    from videorenderer_amd import api
    c = dict(c, iChromaScaling=2)
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    got, info = run_product(mpcvr, torch, c)
    ref, info_ref = run_product(mpcvr, torch, c, extra_flags=api.FLAG_NO_FAST_CONVERT)
    compare(ref, want, f"{label} [{info_ref}]", exact=True)          # the per-pixel kernel: the oracle's bits, behind the PQ tail too (round 6)
    if not has_tail(c):
        same = compare(got, want, f"{label} [{info}]", min_same=WHOLE_FRAME_FLOOR)
    else:
        # behind the PQ tail: a channel of the block convert beyond 1 LSB must be one the oracle itself does not define to a code (compare_behind_tail)
        same, _ = compare_behind_tail(oracle, p, frame, pitch, got, want, f"{label} [{info}]", min_same=WHOLE_FRAME_FLOOR, dovi=bool(c.get("dovi")))
    print(f"{label}: identical channels {same:.6f}  [{info}]")


@pytest.mark.parametrize("label,c,path", [
    ("p210_pq_1080p_to_4k", dict(cformat=6, w=1920, h=1080, kind="noise", seed=351, dst=(3840, 2160), iUpscaling=4,
                                 exfmt=GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]["exfmt"]), "fused_up2x"),
    ("yuv422p10_same_size", dict(cformat=22, w=1920, h=1080, kind="noise", seed=352, dst=(1920, 1080),
                                 exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]), "direct:convert+final"),
    ("yv16_1080p_to_1440p", dict(cformat=15, w=1920, h=1080, kind="noise", seed=353, dst=(2560, 1440), iUpscaling=2,
                                 exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]), "passes:convert,resizeX,resizeY;kernel=fused_strip("),
    ("yv24_720p_to_1440p", dict(cformat=16, w=1280, h=720, kind="noise", seed=355, dst=(2560, 1440), iUpscaling=4,
                                exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]), "fused_up2x"),
    ("yuv444p10_pq_1080p_to_1440p", dict(cformat=24, w=1920, h=1080, kind="noise", seed=356, dst=(2560, 1440), iUpscaling=4, iChromaScaling=2,
                                         exfmt=GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]["exfmt"]), "passes:convert,resizeX,resizeY+final;kernel=fused_strip("),
    ("yuv444p16_same_size", dict(cformat=25, w=1920, h=1080, kind="noise", seed=357, dst=(1920, 1080), iChromaScaling=0,
                                 exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]), "direct:convert+final"),
    ("gbrp10_360p_to_540p", dict(cformat=27, w=640, h=360, kind="noise", seed=358, dst=(960, 540), iUpscaling=2), "passes:convert,resizeX,resizeY+final;kernel=fused_strip("),
    ("p216_rect_down_1p5x", dict(cformat=7, w=1920, h=1080, kind="noise", seed=354, src_rect=(8, 4, 1912, 1076), dst=(1270, 714), iDownscaling=2,
                                 exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]), "passes:convert,resizeX,resizeY+final;kernel=fused_strip("),
])
def test_planar_422_and_444_on_the_fused_paths(mpcvr, oracle, torch_cuda, label, c, path):
    """Planar / bi-planar 4:2:2 (P210, P216, YV16, YUV422P10) on the 2x2-block convert (round 2): chroma rows are luma rows, so a
    row pair takes row 0 from chroma row sy and row 1 from sy + 1 with weight 1 — the 4:2:0 block code with a different row
    rule; planar 4:4:4 (YV24, YUV444P8/10/16) likewise with a chroma sample per pixel and no filter.  The exact-2x kernel, the strip
    kernel and the same-size convert take these formats now, three-plane RGB (GBRP: the same loads behind a rotated matrix) too.
    Whole frames against the oracle."""
    torch = torch_cuda
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    got, info = run_product(mpcvr, torch, c)
    assert path_ok(info, path), info
    if has_tail(c):
        same, _ = compare_behind_tail(oracle, p, frame, pitch, got, want, f"{label} [{info}]", min_same=WHOLE_FRAME_FLOOR, dovi=bool(c.get("dovi")))
    else:
        same = compare(got, want, f"{label} [{info}]", min_same=WHOLE_FRAME_FLOOR)
    print(f"{label}: identical channels {same:.6f}  [{info}]")


@pytest.mark.gpu
@pytest.mark.parametrize("label,c,path", [
    ("yuy2_same_size_nearest_is_bilinear", dict(cformat=4, w=1920, h=1080, kind="noise", seed=361, dst=(1920, 1080), iChromaScaling=0,
                                                exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]), "direct:convert"),
    ("uyvy_720p_to_1440p", dict(cformat=5, w=1280, h=720, kind="noise", seed=362, dst=(2560, 1440), iUpscaling=4,
                                exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]), "fused_up2x"),
    ("y210_pq_1080p_to_1440p", dict(cformat=8, w=1920, h=1080, kind="noise", seed=363, dst=(2560, 1440), iUpscaling=4,
                                    exfmt=GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]["exfmt"]), "passes:convert,resizeX,resizeY+final;kernel=fused_strip("),
    ("y216_rect_down_1p5x", dict(cformat=9, w=1920, h=1080, kind="noise", seed=364, src_rect=(8, 4, 1912, 1076), dst=(1270, 714), iDownscaling=2,
                                 exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]), "passes:convert,resizeX,resizeY+final;kernel=fused_strip("),
    ("v210_1080p_to_4k", dict(cformat=10, w=1920, h=1080, kind="noise", seed=365, dst=(3840, 2160), iUpscaling=2,
                              exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]), "fused_up2x"),
    ("yuy2_catmull_chroma_stays_per_pixel", dict(cformat=4, w=640, h=360, kind="noise", seed=366, dst=(960, 540), iUpscaling=2, iChromaScaling=2),
     "passes:convert,resizeX,resizeY;kernel=fused_strip:surface("),
])
def test_packed_422_on_the_fused_paths(mpcvr, oracle, torch_cuda, label, c, path):
    """Packed 4:2:2 (YUY2, UYVY, Y210, Y216, and v210 behind its unpack) on the 2x2-block convert: one texel holds the block's two
    luma samples and its own chroma, the next texel the neighbour's (Shaders.cpp:195-229: even pixel = own chroma, odd pixel = the
    mean with the next texel; CHROMA_Nearest is not distinguished) — the planar 4:2:2 block code behind a whole-texel loader.
    CATMULLROM_05 chroma stays on the per-pixel convert.  Whole frames against the oracle."""
    torch = torch_cuda
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    got, info = run_product(mpcvr, torch, c)
    assert path_ok(info, path), info
    if has_tail(c):
        same, _ = compare_behind_tail(oracle, p, frame, pitch, got, want, f"{label} [{info}]", min_same=WHOLE_FRAME_FLOOR, dovi=bool(c.get("dovi")))
    else:
        same = compare(got, want, f"{label} [{info}]", min_same=WHOLE_FRAME_FLOOR)
    print(f"{label}: identical channels {same:.6f}  [{info}]")


NEAREST_CHROMA = [
    ("nv12_same_size", dict(cformat=1, w=1920, h=1080, kind="noise", seed=381, dst=(1920, 1080), iChromaScaling=0,
                            exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]), "direct:convert"),
    ("p010_pq_mpeg1_siting_ignored_2x", dict(cformat=2, w=1920, h=1080, kind="noise", seed=382, dst=(3840, 2160), iUpscaling=4, iChromaScaling=0,
                                             exfmt=(GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]["exfmt"] & ~0xF00) | (1 << 8)), "fused_up2x"),
    ("yv12_rect_1080p_to_1440p", dict(cformat=14, w=1920, h=1080, kind="noise", seed=383, src_rect=(8, 6, 1912, 1074), dst=(2540, 1424), iUpscaling=2, iChromaScaling=0,
                                      exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]), "passes:convert,resizeX,resizeY;kernel=fused_strip("),
    ("p210_4k_down_to_1080p", dict(cformat=6, w=3840, h=2160, kind="noise", seed=384, dst=(1920, 1080), iDownscaling=3, iChromaScaling=0,
                                   exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]), "passes:convert,resizeX,resizeY+final;kernel=fused_strip("),
    ("yuv420p10_cosited_odd_height_pairs", dict(cformat=20, w=1280, h=722, kind="noise", seed=385, dst=(1280, 722), iChromaScaling=0,
                                                exfmt=(GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"] & ~0xF00) | (7 << 8)), "direct:convert"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("label,c,path", NEAREST_CHROMA)
def test_nearest_chroma_on_the_fused_paths(mpcvr, oracle, torch_cuda, label, c, path):
    """CHROMA_Nearest on 4:2:0 and planar 4:2:2 (Shaders.cpp:239-241: the chroma texel under the pixel, (sx / div_w, sy / div_h), whatever
    the stream's siting says): the block code with one texel per block column pair and whole-row vertical weights.  No arithmetic is
    left between texel and matrix, so SDR cases must be as close to the oracle as the bilinear ones.  Whole frames."""
    torch = torch_cuda
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    got, info = run_product(mpcvr, torch, c)
    assert path_ok(info, path), info
    if has_tail(c):
        same, _ = compare_behind_tail(oracle, p, frame, pitch, got, want, f"{label} [{info}]", min_same=WHOLE_FRAME_FLOOR, dovi=bool(c.get("dovi")))
    else:
        same = compare(got, want, f"{label} [{info}]", min_same=WHOLE_FRAME_FLOOR)
    print(f"{label}: identical channels {same:.6f}  [{info}]")


@pytest.mark.gpu
@pytest.mark.parametrize("label,c,path", [
    ("ayuv_same_size", dict(cformat=11, w=1920, h=1080, kind="noise", seed=371, dst=(1920, 1080),
                            exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]), "direct:convert"),
    ("y410_pq_1080p_to_4k", dict(cformat=12, w=1920, h=1080, kind="noise", seed=372, dst=(3840, 2160), iUpscaling=4,
                                 exfmt=GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]["exfmt"]), "fused_up2x"),
    ("y416_catmull_setting_1080p_to_1440p", dict(cformat=13, w=1920, h=1080, kind="noise", seed=373, dst=(2560, 1440), iUpscaling=4, iChromaScaling=2,
                                                 exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]), "passes:convert,resizeX,resizeY+final;kernel=fused_strip("),
    ("y8_gray_rect_720p_down", dict(cformat=37, w=1280, h=720, kind="noise", seed=374, src_rect=(8, 4, 1272, 716), dst=(846, 476), iDownscaling=2),
     "passes:convert,resizeX,resizeY;kernel=fused_strip("),
    ("y10_gray_2x", dict(cformat=38, w=640, h=360, kind="noise", seed=375, dst=(1280, 720), iUpscaling=2, exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]), "fused_up2x"),
    ("y16_gray_same_size", dict(cformat=39, w=1280, h=720, kind="noise", seed=376, dst=(1280, 720)), "direct:convert"),
    ("gbrp8_2x", dict(cformat=26, w=1280, h=720, kind="noise", seed=377, dst=(2560, 1440), iUpscaling=4), "fused_up2x"),
    ("gbrp16_same_size_procamp", dict(cformat=28, w=1280, h=720, kind="noise", seed=378, dst=(1280, 720), procamp=(8.0, 1.1, 0.0, 1.0)), "direct:convert"),
])
def test_packed_444_gray_and_gbrp_on_the_fused_paths(mpcvr, oracle, torch_cuda, label, c, path):
    """The remaining one-sample-per-pixel layouts on the 2x2-block convert: packed 4:4:4 (AYUV / Y410 / Y416: two consecutive texels
    are the block's two columns, components by the format's swizzle, Shaders.cpp:186-193), gray (Y8 / Y10 / Y16: luma only, U = V = 0,
    :184 and the cbuffer fix-up :863-873) and three-plane RGB (GBRP8/10/16: the planar 4:4:4 loads behind the rotated matrix).  No chroma
    filter exists for any of them, so every chroma setting is accepted.  Whole frames against the oracle."""
    torch = torch_cuda
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    got, info = run_product(mpcvr, torch, c)
    assert path_ok(info, path), info
    if has_tail(c):
        same, _ = compare_behind_tail(oracle, p, frame, pitch, got, want, f"{label} [{info}]", min_same=WHOLE_FRAME_FLOOR, dovi=bool(c.get("dovi")))
    else:
        same = compare(got, want, f"{label} [{info}]", min_same=WHOLE_FRAME_FLOOR)
    print(f"{label}: identical channels {same:.6f}  [{info}]")


@pytest.mark.gpu
@pytest.mark.parametrize("label,c,path", [
    ("p010_pq_1080p_to_4k", dict(cformat=2, w=1920, h=1080, kind="noise", seed=391, dst=(3840, 2160), iUpscaling=6,
                                 exfmt=GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]["exfmt"]), "fused_up2x"),
    ("nv12_720p_to_1080p", dict(cformat=1, w=1280, h=720, kind="structure", seed=392, dst=(1920, 1080), iUpscaling=6,
                                exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]), "passes:convert,resizeX,resizeY;kernel=fused_strip("),
    ("yuv420p10_rect_odd_ratio", dict(cformat=20, w=640, h=360, kind="noise", seed=393, src_rect=(8, 4, 632, 356), dst=(1501, 777), iUpscaling=6,
                                      window=(1520, 800), offset=(9, 11)), "passes:convert,resizeX,resizeY+final;kernel=fused_strip("),
    ("rgb32_rot90", dict(cformat=30, w=320, h=200, kind="structure", seed=394, dst=(300, 480), iUpscaling=6, rotation=90), "passes:"),
])
def test_spline36_extension_vs_oracle(mpcvr, oracle, torch_cuda, label, c, path):
    """The Spline36 extension (no reference shader: unpinned by construction — the oracle states the kernel, the product must agree with
    it like with every reference scaler): exact 2x through the fused kernel's plain six-tap variant, other ratios through the strip
    kernel, a rotated RGB frame through the per-draw kernels; and the plain tier bit-exact on SDR content."""
    torch = torch_cuda
    from videorenderer_amd import api
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    got, info = run_product(mpcvr, torch, c)
    assert path_ok(info, path), info
    plain, info_plain = run_product(mpcvr, torch, c, extra_flags=api.FLAG_NO_FUSED)
    compare(plain, want, f"{label} [{info_plain}]", exact=True)       # the plain tier: the oracle's bits, behind a tail too (round 6)
    if has_tail(c):
        same, _ = compare_behind_tail(oracle, p, frame, pitch, got, want, f"{label} [{info}]", min_same=WHOLE_FRAME_FLOOR, dovi=bool(c.get("dovi")))
    else:
        same = compare(got, want, f"{label} [{info}]", min_same=WHOLE_FRAME_FLOOR)
    print(f"{label}: identical channels {same:.6f}  [{info}]")


def test_full_size_flat_frame_and_dither_period(mpcvr, torch_cuda):
    """Constant input at 4K: every pass keeps it constant; the only variation is the 32x32 dither tile."""
    torch = torch_cuda
    w, h = 3840, 2160
    buf = np.zeros(w * h * 3 // 2, dtype=np.uint16)
    buf[: w * h] = 600 << 6
    buf[w * h:] = 512 << 6
    c = dict(cformat=2, w=w, h=h, dst=(2 * w, 2 * h), exfmt=GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]["exfmt"], iUpscaling=4)
    vp, (ww, wh) = make_vp(mpcvr, c)
    dst = torch.empty((wh, ww, 4), dtype=torch.uint8, device="cuda")
    vp.CopySample(torch.from_numpy(buf.view(np.uint8)).cuda(), w * 2)
    vp.Process(dst, ww * 4)
    vp.Synchronize()
    tile = dst[:32, :32]
    assert int(tile[..., :3].max()) - int(tile[..., :3].min()) <= 1
    tiled = tile.repeat(wh // 32, ww // 32, 1)
    assert torch.equal(tiled, dst)
    vp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("label,c", [
    ("C1", dict(cformat=1, w=1920, h=1080, kind="structure", seed=201, dst=(1920, 1080), exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"])),
    ("C2", dict(cformat=20, w=1920, h=1080, kind="noise", seed=202, dst=(3840, 2160), exfmt=GOLDEN_CASES["c2_yuv420p10_catmull_2x"]["exfmt"], iUpscaling=2)),
    ("C2_nv12_2x", dict(cformat=1, w=1920, h=1080, kind="noise", seed=203, dst=(3840, 2160), exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"], iUpscaling=4)),
])
def test_full_size_baseline_configs_whole_frame(mpcvr, oracle, torch_cuda, label, c):
    """BASELINE.json C1 / C2 (and the everyday NV12 2x) at their full sizes: every output pixel against the oracle."""
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch)
    got, info = run_product(mpcvr, torch_cuda, c)
    if label == "C1":
        from videorenderer_amd import api
        assert info.startswith("direct:convert+copy")
        compare(got, want, label, min_same=WHOLE_FRAME_FLOOR)              # block convert (FMA contraction): <= 1 LSB
        got, info = run_product(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FAST_CONVERT)
        assert info.startswith("direct:convert+copy")
        compare(got, want, label + " folded", exact=True)     # folded per-pixel kernel, SDR: bit-exact
    else:
        assert info == "fused_up2x"
        compare(got, want, label, min_same=WHOLE_FRAME_FLOOR)


@pytest.mark.parametrize("label,c", [
    ("p010_1080p_to_1440p_lanczos3", dict(cformat=2, w=1920, h=1080, kind="noise", seed=301, dst=(2560, 1440), iUpscaling=4,
                                          exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"])),
    ("nv12_4k_to_1440p_hamming", dict(cformat=1, w=3840, h=2160, kind="noise", seed=302, dst=(2560, 1440), iDownscaling=2,
                                      exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"])),
    ("yuv420p10_1080p_to_4k_jinc2", dict(cformat=20, w=1920, h=1080, kind="noise", seed=303, dst=(3840, 2160), iUpscaling=5,
                                         exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"])),
])
def test_full_size_general_ratio_tiers_agree(mpcvr, torch_cuda, label, c):
    """Everyday geometries at their real sizes, every output pixel, GPU tiers against each other (the oracle would need
    minutes): the folded / tiled kernels (k_convert_420, k_resize_2d, k_jinc2_phases) must reproduce the plain kernels bit for
    bit on SDR content — tile edges, XCD bands, ragged last tiles included — and the default planner (block convert) must stay
    within 1 LSB of them."""
    from videorenderer_amd import api
    plain, info_p = run_product(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FUSED)
    folded, info_f = run_product(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FAST_CONVERT)
    default, info_d = run_product(mpcvr, torch_cuda, c)
    # (Jinc2m at exactly 2x: the default tier is the fused kernel since round 5 — a full-size frame of it against the per-pixel kernels)
    assert info_p.startswith("passes:convert") and info_f.startswith("passes:convert") and info_d.startswith("fused_jinc2x" if c.get("iUpscaling") == 5 else "passes:convert")
    if c.get("iUpscaling") == 5:     # Jinc2m: the phase table holds the weights of the NOMINAL phases (k + 1/4, k + 3/4), the per-pixel kernel — like
        # the shader — evaluates them at the interpolated texture coordinate, which sits an ulp beside the nominal position on some columns / rows
        compare(folded, plain, label + " phase table vs per-pixel weights", min_same=0.999)
    else:
        assert np.array_equal(plain, folded), f"{label}: folded kernels differ from the plain ones in {(plain != folded).sum()} bytes"
    compare(default, plain, label + " default vs plain", min_same=WHOLE_FRAME_FLOOR)


def _random_case(rng):
    cformat = int(rng.choice([1, 2, 20, 17, 14]))
    w, h = int(rng.integers(8, 120)) * 2, int(rng.integers(8, 80)) * 2
    c = dict(cformat=cformat, w=w, h=h, kind="noise", seed=int(rng.integers(1, 1 << 30)),
             exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"],
             iUpscaling=int(rng.choice([1, 2, 3, 4])), iDownscaling=int(rng.integers(0, 6)),
             bInterpolateAt50pct=int(rng.integers(0, 2)))
    rw, rh = w, h
    if rng.random() < 0.5:                       # a source rect, sometimes on the alignment the fast kernels need, sometimes not
        l = int(rng.integers(0, w // 4)) * (4 if rng.random() < 0.6 else 1)
        t = int(rng.integers(0, h // 4)) * (2 if rng.random() < 0.6 else 1)
        r = min(w, l + max(8, int(rng.integers(w // 3, w))))
        b = min(h, t + max(8, int(rng.integers(h // 3, h))))
        c["src_rect"] = (l, t, r, b)
        rw, rh = r - l, b - t
    fx, fy = (float(rng.uniform(0.45, 2.6)), float(rng.uniform(0.45, 2.6)))
    if rng.random() < 0.25:
        fy = fx
    if rng.random() < 0.15:
        fx = 1.0
    if rng.random() < 0.15:
        fy = 1.0
    dw, dh = max(4, int(round(rw * fx))), max(4, int(round(rh * fy)))
    c["dst"] = (dw, dh)
    if rng.random() < 0.4:                        # letterboxed / partly outside the window
        ww, wh = dw + int(rng.integers(0, 40)), dh + int(rng.integers(0, 40))
        ox, oy = int(rng.integers(-12, 24)), int(rng.integers(-12, 24))
        c["window"] = (max(8, ww), max(8, wh)); c["offset"] = (ox, oy)
    if rng.random() < 0.2:
        c["output_format"] = 1
    if rng.random() < 0.2:
        c["iTexFormat"] = int(rng.choice([8, 10, 16]))
    if rng.random() < 0.25:                       # rotated / mirrored first draw (plain kernel) feeding a folded second draw
        c["rotation"] = int(rng.choice([90, 180, 270]))
    if rng.random() < 0.15:
        c["flip"] = 1
    return c


def test_random_geometries_tiers_agree(mpcvr, oracle, torch_cuda):
    """240 random geometries (sizes, crops, ratios 0.45x .. 2.6x per axis, window offsets and clipping, scaler choices, internal
    formats, rotations and flips) on SDR content: the folded / tiled kernels must equal the plain kernels bit for bit, the default planner must stay
    within 1 LSB of them."""
    from videorenderer_amd import api
    rng = np.random.default_rng(20260924)
    paths = set()
    for n in range(240):
        c = _random_case(rng)
        try:
            plain, _ = run_product(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FUSED)
        except api.MpcvrError as e:                       # e.g. a ratio outside the supported tap range: same answer on every tier
            for fl in (api.FLAG_NO_FAST_CONVERT, 0):
                with pytest.raises(api.MpcvrError):
                    run_product(mpcvr, torch_cuda, c, extra_flags=fl)
            continue
        if n < 80:                                        # ... and the plain kernels must equal the oracle bit for bit
            frame, pitch = case_frame(c)
            p = oracle_params(oracle, c)
            want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
            if c.get("output_format", 0) == 1:
                compare_rgb10(plain, want, f"random {n} vs oracle {c}", exact=True)
            else:
                compare(plain, want, f"random {n} vs oracle {c}", exact=True)
        folded, _ = run_product(mpcvr, torch_cuda, c, extra_flags=api.FLAG_NO_FAST_CONVERT)
        default, info = run_product(mpcvr, torch_cuda, c)
        paths.add(info.split(";")[0])
        assert np.array_equal(plain, folded), (n, c, int((plain != folded).sum()))
        if c.get("output_format", 0) == 1:
            compare_rgb10(default, plain, f"random {n} {c}", internal8=internal_is_8bit(c))
        else:
            compare(default, plain, f"random {n} {c}", min_same=0.98)
    assert len(paths) >= 4, paths


def test_random_formats_and_tails_vs_oracle(mpcvr, oracle, torch_cuda):
    """120 random (format, colourimetry, chroma mode, geometry) combinations over all 39 ColorFormat_t values, SDR / HDR10 / HLG /
    BT.2020-gamma tagging, HDR output on or off, through the plain kernels and the default planner against the oracle."""
    from videorenderer_amd import api
    from tests.golden.cases import HDR10, HLG, ext, MPEG1, MPEG2, COSITED, TV, FULL, M709, M601, M2020, P709, P2020, T709, T22
    rng = np.random.default_rng(424242)
    sdr = [ext(MPEG2, TV, M709), ext(MPEG1, TV, M601), ext(COSITED, FULL, M709, P709, T709), ext(MPEG2, TV, M2020, P2020, T22), 0]
    refused = 0
    for n in range(120):
        c = _random_case(rng)
        c.pop("rotation", None); c.pop("flip", None)
        c["cformat"] = int(rng.integers(1, 40))
        c["exfmt"] = int(rng.choice([HDR10, HLG])) if rng.random() < 0.35 else int(rng.choice(sdr))
        c["iChromaScaling"] = int(rng.integers(0, 3))
        if rng.random() < 0.2:
            c["hdr_output"] = 1; c["output_format"] = 1
        if c["cformat"] in (29, 30, 31, 32, 33, 34, 35, 36):       # interleaved RGB: the texture copy loops need whole frames
            c.pop("src_rect", None)
            c["dst"] = (max(4, int(c["w"] * rng.uniform(0.5, 2.2))), max(4, int(c["h"] * rng.uniform(0.5, 2.2))))
            c.pop("window", None); c.pop("offset", None)
        if c["cformat"] == 10:                                     # v210: widths in multiples of 6 keep the test frame simple
            c["w"] = max(12, c["w"] // 6 * 6); c.pop("src_rect", None)
            c["dst"] = (max(4, int(c["w"] * rng.uniform(0.5, 2.2))), max(4, int(c["h"] * rng.uniform(0.5, 2.2))))
            c.pop("window", None); c.pop("offset", None)
        frame, pitch = case_frame(c)
        p = oracle_params(oracle, c)
        want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
        for flags in (api.FLAG_NO_FUSED, 0):
            try:
                got, info = run_product(mpcvr, torch_cuda, c, extra_flags=flags)
            except api.MpcvrError:                        # refused combinations (e.g. odd sizes of subsampled formats) are refused by
                refused += 1                              # both planners alike
                continue
            tail = has_tail(c) or c.get("hdr_output")
            name = f"random format {n} flags={flags} [{info}] {c}"
            if c.get("output_format", 0) == 1:
                compare_rgb10(got, want, name, exact=(flags != 0), tail=tail, internal8=internal_is_8bit(c))
            elif flags != 0:
                compare(got, want, name, exact=True)          # the plain tier: bit-exact, tails included (round 6)
            else:
                compare(got, want, name, min_same=0.98)
    assert refused % 2 == 0 and refused <= 24, refused


@pytest.mark.parametrize("kind", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("src_fmt,dst_fmt", [(0, 0), (1, 1), (1, 0)])
def test_correction_passes_vs_oracle(mpcvr, oracle, torch_cuda, kind, src_fmt, dst_fmt):
    """The m_pPSCorrection shaders as standalone passes: random surfaces plus the corners of the cube, against the oracle."""
    torch = torch_cuda
    from videorenderer_amd import api
    rng = np.random.default_rng(1000 + kind * 10 + src_fmt * 3 + dst_fmt)
    w, h = 200, 64
    src = rng.integers(0, 1 << 32, size=(h, w), dtype=np.uint64).astype(np.uint32)
    src[0, :8] = [0, 0xffffffff, 0x3ff, 0x3ff << 10, 0x3ff << 20, 0x00ff0000, 0x0000ff00, 0x000000ff]
    want = oracle.correction_pass(kind, src, 10 if src_fmt else 8, 10 if dst_fmt else 8, sdr_nits=125)
    d_src = torch.from_numpy(src.view(np.int32)).cuda()
    # the pass writes through dst_pitch: every render-target layout, the bytes around the w x h texels untouched
    outs = {}
    for layout in LAYOUTS:
        base, dst_pitch = layout_of(layout, w)
        t = CarvedTargets(torch, w, h, dst_pitch, [base])
        api.correction_pass(kind, d_src, w * 4, src_fmt, t.ptrs[0], dst_pitch, dst_fmt, w, h, sdr_nits=125)
        torch.cuda.synchronize()
        t.assert_guards_intact(f"correction {kind} layout {layout}")
        outs[layout] = t.pixels()
        if dst_fmt:
            compare_rgb10(outs[layout], want.reshape(h, w, 1).view(np.uint8).reshape(h, w, 4), f"correction {kind} <{layout}>", exact=(kind == 2))
        else:
            compare(outs[layout], want.view(np.uint8).reshape(h, w, 4), f"correction {kind} <{layout}>", exact=(kind == 2), min_same=0.99)
    assert np.array_equal(outs["tight"], outs["padded16"])
    got = np.ascontiguousarray(outs["tight"]).view(np.uint32)[..., 0]
    # in place
    api.correction_pass(kind, d_src, w * 4, src_fmt, d_src, w * 4, src_fmt, w, h, sdr_nits=125)
    torch.cuda.synchronize()
    if src_fmt == dst_fmt:
        assert np.array_equal(d_src.cpu().numpy().view(np.uint32), got)


def test_context_reuse_across_geometries_and_batches(mpcvr, torch_cuda):
    """One context driven the way a player would: the video rect changes between batches (tiled two-draw kernel -> fused 2x ->
    same-size direct -> Jinc2m phases -> one-pass), batch sizes vary (1, 2, 33, 70 > the frame-table slot), settings change
    through Configure, Dolby Vision comes and goes.  Every batch must equal frame-by-frame Process on a fresh context."""
    torch = torch_cuda
    from videorenderer_amd import api, synth
    w, h = 96, 64
    exf = GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]["exfmt"]
    frames_np = [synth.make_frame(2, w, h, "noise", seed=900 + i)[0] for i in range(70)]
    frames = [torch.from_numpy(f).cuda() for f in frames_np]
    vp = api.VideoProcessor(api.default_settings(iUpscaling=4))
    vp.InitMediaType(2, w, h, extfmt=exf)

    def reference(settings, dst_wh, n, dovi=None):
        ref = api.VideoProcessor(settings)
        ref.InitMediaType(2, w, h, extfmt=exf)
        ref.SetWindowRect((0, 0) + dst_wh); ref.SetVideoRect((0, 0) + dst_wh)
        if dovi:
            ref.SetDoviMetadata(dovi)
        outs = []
        for i in range(n):
            d = torch.zeros((dst_wh[1], dst_wh[0], 4), dtype=torch.uint8, device="cuda")
            ref.CopySample(frames[i], w * 2); ref.Process(d, dst_wh[0] * 4); outs.append(d)
        ref.Synchronize(); ref.close()
        return outs

    steps = [((128, 86), 33, dict(), None), ((192, 128), 2, dict(), None), ((96, 64), 70, dict(), None),
             ((192, 128), 5, dict(iUpscaling=5), None), ((96, 100), 1, dict(), None), ((144, 96), 7, dict(iUpscaling=1), None),
             ((144, 96), 4, dict(iUpscaling=1), synth.dovi_metadata("poly", l2=(100, 600))), ((128, 86), 9, dict(iUpscaling=4), None)]
    for dst_wh, n, cfg, dovi in steps:
        settings = api.default_settings(iUpscaling=4, **cfg) if "iUpscaling" not in cfg else api.default_settings(**cfg)
        vp.Configure(settings)
        vp.SetWindowRect((0, 0) + dst_wh); vp.SetVideoRect((0, 0) + dst_wh)
        vp.SetDoviMetadata(dovi)
        dsts = [torch.zeros((dst_wh[1], dst_wh[0], 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
        vp.ProcessBatch(frames[:n], dsts, dst_wh[0] * 4)
        vp.Synchronize()
        want = reference(settings, dst_wh, n, dovi)
        for i in range(n):
            assert torch.equal(dsts[i], want[i]), (dst_wh, n, cfg, bool(dovi), i, vp.GetVPInfo())
    vp.close()


def test_context_reuse_walks_through_plan_tables(mpcvr, torch_cuda):
    """One context walks through plans whose tables differ in kind, each step leaving behind what the next must not read: a reversed row
    map, no tap tables at all, periodic tables, a first draw that is a Y shader, one pass, normalising taps (wsum), a flipped 4:3, exact 2x
    without tables, and back to the first.  Window = video rect throughout.  At every step one Process and one ProcessBatch of 3 frames
    equal a fresh context's bit for bit, and so does GetVPInfo."""
    torch = torch_cuda
    from videorenderer_amd import api, synth
    w, h = 96, 72
    frames = [torch.from_numpy(synth.make_frame(2, w, h, "noise", seed=1200 + i)[0]).cuda() for i in range(3)]
    L3, J2 = api.UPSCALE_Lanczos3, api.UPSCALE_Jinc2

    def run(vp, settings, dst_wh, rotation, flip):
        vp.Configure(settings)
        vp.SetRotation(rotation); vp.SetFlip(flip)
        vp.SetWindowRect((0, 0) + dst_wh); vp.SetVideoRect((0, 0) + dst_wh)
        outs = [torch.zeros((dst_wh[1], dst_wh[0], 4), dtype=torch.uint8, device="cuda") for _ in range(4)]
        vp.CopySample(frames[0], w * 2); vp.Process(outs[0], dst_wh[0] * 4)
        vp.ProcessBatch(frames, outs[1:], dst_wh[0] * 4)
        vp.Synchronize()
        return outs, vp.GetVPInfo()

    #        upscaling, target, rotation, flip, what GetVPInfo must name
    steps = [(L3, (144, 108), 180, False, ":surface("),          # strip kernel on the convert output, reversed row map
             (J2, (144, 108), 0, False, "passes:convert,resizeX"),      # no tap tables
             (L3, (144, 108), 0, False, "kernel=fused_period(rows=3:2"),
             (L3, (108, 144), 90, False, ";rot90"),              # the first draw is a Y shader
             (L3, (96, 100), 0, False, "passes:convert,resizeY"),       # one pass
             (L3, (64, 48), 0, False, "kernel=fused_strip("),    # ps_convolution: normalising taps
             (L3, (128, 96), 0, True, "kernel=fused_period(rows=4:3"),  # the X table read from the other end
             (L3, (192, 144), 0, False, "fused_up2x")]           # exact 2x: no tables
    steps.append(steps[0])
    vp = api.VideoProcessor(api.default_settings(iUpscaling=L3, bInterpolateAt50pct=0))
    vp.InitMediaType(2, w, h)
    for i, (up, dst_wh, rotation, flip, route) in enumerate(steps):
        settings = api.default_settings(iUpscaling=up, bInterpolateAt50pct=0)
        got, info = run(vp, settings, dst_wh, rotation, flip)
        fresh = api.VideoProcessor(settings)
        fresh.InitMediaType(2, w, h)
        want, want_info = run(fresh, settings, dst_wh, rotation, flip)
        fresh.close()
        print(i + 1, info)
        assert info == want_info and route in info, (i + 1, info, want_info, route)
        for k in range(4):
            assert torch.equal(got[k], want[k]), (i + 1, k, info)
    vp.close()


def test_c_abi_demo_program(mpcvr, oracle, torch_cuda, tmp_path):
    """examples/c_abi_demo.c — plain C, host memory in, host memory out — against the oracle on the same frame."""
    import subprocess
    from tests.test_host_logic import build_c_demo
    w, h = 128, 72
    out = subprocess.run([build_c_demo(tmp_path), str(w), str(h)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    fields = dict(f.split("=") for f in out.stdout.split() if "=" in f)
    # the demo's frame, rebuilt here
    frame = np.zeros(w * h * 3 // 2, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    frame[: w * h] = (16 + (xx * 219) // (w - 1) - (((xx >> 3) ^ (yy >> 3)) & 1) * 8).astype(np.uint8).reshape(-1)
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    uv = np.zeros((h // 2, w), np.uint8)
    uv[:, 0::2] = 64 + (cx * 128) // (w // 2)
    uv[:, 1::2] = 192 - (cy * 128) // (h // 2)
    frame[w * h:] = uv.reshape(-1)
    p = oracle.default_params(cformat=1, width=w, height=h, exfmt=(5 << 8) | (2 << 12) | (1 << 15), window_w=w, window_h=h,
                              video_rect=(0, 0, w, h))
    want = oracle.process(p, frame, w)
    want[..., 3] = 255
    fnv = 2166136261
    for b in want.tobytes():
        fnv = ((fnv ^ b) * 16777619) & 0xffffffff
    assert out.stdout.startswith("direct:convert+copy"), out.stdout
    assert int(fields["bytes"]) == w * h * 4
    assert fields["fnv1a"] == f"{fnv:08x}", (out.stdout, f"{fnv:08x}")


def test_two_contexts_interleaved(mpcvr, torch_cuda):
    """Two contexts (own streams, different formats and geometries) fed alternately without synchronising in between — a
    transcoding server's pattern — must give what each gives alone: no state is shared between contexts."""
    torch = torch_cuda
    from videorenderer_amd import api, synth
    specs = [dict(cf=2, w=128, h=72, dst=(256, 144), ext=GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"]["exfmt"], st=dict(iUpscaling=4)),
             dict(cf=1, w=160, h=96, dst=(212, 128), ext=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"], st=dict(iUpscaling=3))]
    ctxs, frames, alone = [], [], []
    for sp in specs:
        vp = api.VideoProcessor(api.default_settings(**sp["st"]))
        vp.InitMediaType(sp["cf"], sp["w"], sp["h"], extfmt=sp["ext"])
        vp.SetWindowRect((0, 0) + sp["dst"]); vp.SetVideoRect((0, 0) + sp["dst"])
        fr = [torch.from_numpy(synth.make_frame(sp["cf"], sp["w"], sp["h"], "noise", seed=700 + i)[0]).cuda() for i in range(6)]
        outs = [torch.zeros((sp["dst"][1], sp["dst"][0], 4), dtype=torch.uint8, device="cuda") for _ in fr]
        vp.ProcessBatch(fr, outs, sp["dst"][0] * 4)
        vp.Synchronize()
        ctxs.append(vp); frames.append(fr); alone.append(outs)
    both = [[torch.zeros_like(o) for o in outs] for outs in alone]
    for rep in range(4):
        for k in (0, 1, 1, 0):
            ctxs[k].ProcessBatch(frames[k][rep:rep + 3], both[k][rep:rep + 3], specs[k]["dst"][0] * 4)
    for vp in ctxs:
        vp.Synchronize()
    for k in (0, 1):
        for i in range(6):
            assert torch.equal(both[k][i], alone[k][i]), (k, i)
    for vp in ctxs:
        vp.close()

# ------------------------------------------------------------------------------------------------
# device samples that do not start on a dword; rotated / HDR snapshots
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3hdr_p010_pq_lanczos3_2x", "c1_nv12_bt709_passthrough", "up_1p5x_lanczos3", "noise_nv12_catmull_2x"])
def test_misaligned_device_sample(mpcvr, torch_cuda, name):
    """A zero-copy sample at +2 / +1 bytes from an allocation: the kernels' dword loads never see it — the sample is copied
    into the context's own texture first (the reference copies EVERY decoder sample, :2563-2569).  Single frames and batches."""
    torch = torch_cuda
    c = GOLDEN_CASES[name]
    frame, pitch = case_frame(c)
    want, info = run_product(mpcvr, torch, c)
    for shift in (2, 1):
        vp, (ww, wh) = make_vp(mpcvr, c)
        big = torch.zeros(frame.size + 64, dtype=torch.uint8, device="cuda")
        big[shift:shift + frame.size] = torch.from_numpy(frame).cuda()
        sample = big[shift:shift + frame.size]
        assert sample.data_ptr() % 4 == shift
        dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
        vp.CopySample(sample, pitch)
        vp.Process(dst, ww * 4)
        vp.Synchronize()
        assert np.array_equal(dst.cpu().numpy(), want), f"{name} +{shift}"
        dsts = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in range(3)]
        vp.ProcessBatch([sample, torch.from_numpy(frame).cuda(), sample], dsts, ww * 4)
        vp.Synchronize()
        for d in dsts:
            assert np.array_equal(d.cpu().numpy(), want), f"{name} +{shift} batch"
        vp.close()


def test_get_current_image_rotated_and_hdr(mpcvr, oracle, torch_cuda):
    """GetCurentImage swaps width and height for 90 / 270 degrees (:3500-3502) and shows an HDR source as SDR even while the
    processor is in HDR-output mode (m_bHdrPassthrough cleared around the draw, :3530-3545)."""
    c = dict(GOLDEN_CASES["rot90_copy_nv12"])
    vp, _ = make_vp(mpcvr, c)
    frame, pitch = case_frame(c)
    vp.CopySample(frame, pitch)
    snap = vp.GetCurentImage()
    assert snap.size == 64 * 40 * 4
    snap = snap.reshape(64, 40, 4)                                   # 64 x 40 source, rotated: 40 wide, 64 high
    want = oracle.process(oracle_params(oracle, dict(c, dst=(40, 64))), frame, pitch)
    compare(snap, want, "rotated GetCurentImage", min_same=0.999)
    vp.close()
    c = dict(GOLDEN_CASES["hdrout_pq_passthrough_2x"])
    vp, _ = make_vp(mpcvr, c)
    frame, pitch = case_frame(c)
    vp.CopySample(frame, pitch)
    snap = vp.GetCurentImage().reshape(32, 64, 4)
    sdr = dict(c, dst=(64, 32), output_format=0)
    sdr.pop("hdr_output")
    want = oracle.process(oracle_params(oracle, sdr), frame, pitch)
    compare(snap, want, "HDR-mode GetCurentImage is SDR", min_same=0.99)
    # ... and the processor is back in HDR-output mode afterwards
    got, _ = run_product(mpcvr, torch_cuda, c)
    assert got.shape[0] == 64
    vp.close()


# ------------------------------------------------------------------------------------------------
# N > 1 on the one GPU of this box: two ranks over gloo (MPCVR_DIST_BACKEND), the real parameter blob, the real bench.py
# ------------------------------------------------------------------------------------------------
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, q):
    import hashlib
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MPCVR_DIST_BACKEND="gloo")
    import torch
    from videorenderer_amd import api, dist as vdist
    from tests.golden.cases import GOLDEN_CASES as G, case_frame as cf
    vdist.init_from_env()
    torch.cuda.set_device(0)
    c = G["c3hdr_p010_pq_lanczos3_2x"]
    # rank 1 is configured DIFFERENTLY on purpose (display nits, scaler): after sync_params it must render like rank 0
    st = api.default_settings(iUpscaling=4 if rank == 0 else 1, iSDRDisplayNits=125 if rank == 0 else 300)
    vp = api.VideoProcessor(st, device=0)
    vp.InitMediaType(c["cformat"], c["w"], c["h"], extfmt=c["exfmt"])
    w2, h2 = c["dst"]
    vp.SetWindowRect((0, 0, w2, h2))
    vp.SetVideoRect((0, 0, w2, h2))
    frame, pitch = cf(c)

    def render():
        dst = torch.zeros((h2, w2, 4), dtype=torch.uint8, device="cuda")
        vp.CopySample(torch.from_numpy(frame).cuda(), pitch)
        vp.Process(dst, w2 * 4)
        vp.Synchronize()
        return hashlib.sha256(dst.cpu().numpy().tobytes()).hexdigest()
    before = render()
    vdist.sync_params(vp)                      # the real mpcvr_get_param_blob payload, broadcast from rank 0
    after = render()
    shard = vdist.shard_frames(7, rank, world)
    q.put((rank, before, after, shard))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
    vp.close()


def test_c_multi_gpu_example_degrades_to_one_device(mpcvr, torch_cuda, tmp_path):
    """examples/c_multi_gpu.c: a context per device 0..N-1 in one plain-C process, rank 0's parameter blob given to the others,
    frames dealt by index.  Here N is whatever the box has (1): every frame must come out identical."""
    import subprocess
    from tests.test_host_logic import build_c_demo
    out = subprocess.run([build_c_demo(tmp_path, "c_multi_gpu"), "8", "6"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert "identical=yes" in last and "frames=6" in last, out.stdout
    assert int(last.split("devices=")[1].split()[0]) == torch_cuda.cuda.device_count()


@pytest.mark.parametrize("name", ["c3hdr_p010_pq_lanczos3_2x", "up_1p5x_lanczos3", "c1_nv12_bt709_passthrough", "c3hdr_p010_pq_lanczos3_2x@1080p"])
def test_frame_lanes_equal_one_after_the_other(mpcvr, torch_cuda, name):
    """mpcvr_process frame after frame (Render -> Process per frame, DX11VideoProcessor.cpp:2730) on a context that owns its stream: the
    frames overlap on its frame lanes — same bytes as strictly one after the other (MPCVR_FLAG_NO_FRAME_LANES), also when later
    frames reuse a render target (frames into the same target keep their order), and nothing is read before mpcvr_synchronize."""
    from videorenderer_amd import api, synth
    torch = torch_cuda
    c = dict(GOLDEN_CASES[name.split("@")[0]])
    if name.endswith("@1080p"):                    # kernels long enough (~15 us) that consecutive frames really overlap
        c.update(w=1920, h=1080, dst=(3840, 2160))
    (ww, wh), vr = case_geometry(c)
    n_frames, n_targets = 13, 5                     # frame i -> target i % 5: later frames overwrite what earlier ones wrote (4 lanes, 5 targets: the writers of a target sit on different lanes)
    frames = []
    for i in range(n_frames):
        f, pitch = synth.make_frame(c["cformat"], c["w"], c["h"], "noise", seed=900 + i)
        frames.append(torch.from_numpy(np.ascontiguousarray(f)).cuda())
    torch.cuda.synchronize()
    outs = {}
    for label, extra in (("lanes", 0), ("serial", api.FLAG_NO_FRAME_LANES)):
        kw = {k: c[k] for k in SETTING_KEYS if k in c}
        kw["flags"] = kw.get("flags", 0) | extra
        vp = api.VideoProcessor(api.default_settings(**kw), use_torch_stream=False)       # the context's own stream, as in a C host
        vp.InitMediaType(c["cformat"], c["w"], c["h"], extfmt=c.get("exfmt", 0))
        vp.SetWindowRect((0, 0, ww, wh))
        vp.SetVideoRect(vr)
        dsts = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in range(n_targets)]
        torch.cuda.synchronize()
        for i in range(n_frames):
            vp.CopySample(frames[i], pitch)
            vp.Process(dsts[i % n_targets], ww * 4)
        vp.Synchronize()
        outs[label] = [d.cpu().numpy() for d in dsts]
        info = vp.GetVPInfo()
        vp.close()
    for t in range(n_targets):
        assert np.array_equal(outs["lanes"][t], outs["serial"][t]), f"{name} [{info}]: target {t} differs between the frame lanes and strict order"
    # and the last frame written to each target is the one that is there: compare with that frame processed alone
    vp, _ = make_vp(mpcvr, c)
    for t in range(n_targets):
        last = max(i for i in range(n_frames) if i % n_targets == t)
        d = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
        vp.CopySample(frames[last], pitch)
        vp.Process(d, ww * 4)
        vp.Synchronize()
        assert np.array_equal(d.cpu().numpy(), outs["lanes"][t]), f"{name}: target {t} does not hold frame {last}"
    vp.close()


def test_c_multi_gpu_rccl_example(mpcvr, torch_cuda, tmp_path):
    """examples/c_multi_gpu_rccl.c: SURVEY.md 8e without Python — ncclCommInitAll over the box's devices, ONE ncclBroadcast of rank 0's
    parameter blob issued by the library (mpcvr_broadcast_param_blob_begin / _end, librccl resolved at run time), frames by index.  On
    this box N = 1: the collective is degenerate, but RCCL is loaded, a communicator exists and ncclBroadcast runs on the context's stream."""
    import subprocess
    from tests.test_host_logic import build_c_demo
    out = subprocess.run([build_c_demo(tmp_path, "c_multi_gpu_rccl", rccl=True), "8", "6"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    head = [l for l in lines if l.startswith("rccl=")]             # (RCCL prints its own banner first)
    assert len(head) == 1 and "broadcast=ok" in head[0], out.stdout
    assert int(head[0].split("ranks=")[1].split()[0]) == torch_cuda.cuda.device_count()
    assert "identical=yes" in lines[-1] and "frames=6" in lines[-1], out.stdout


def test_two_ranks_share_rank0_parameters(mpcvr, torch_cuda):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, b0, a0, s0), (_, b1, a1, s1) = res
    assert b0 != b1, "the two ranks were configured differently"
    assert a0 == b0, "rank 0 keeps its own parameters"
    assert a1 == a0, "rank 1 renders with rank 0's parameter blob after sync_params"
    assert sorted(s0 + s1) == list(range(7))


def test_bench_two_ranks_one_gpu(mpcvr, torch_cuda):
    """bench.py's N > 1 branch end to end (torchrun launch line of the driver, barriers, max-over-ranks timing, rank-0 JSON)
    with two ranks sharing this box's one GPU over gloo."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(HERE)
    env = dict(os.environ, MPCVR_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--batch", "2", "--ring", "2", "--src", "256x144", "--no-cpu-baseline", "--no-host-path"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["steps"] == 2 and r["scaling"] == "weak"
    assert r["value"] > 0 and r["config"]["path"] == "fused_up2x"
    assert abs(r["config"]["fps_per_gpu"] * 2 - r["value"]) < 1e-2 * r["value"]


def test_bench_gpus_2_starts_its_own_ranks(mpcvr, torch_cuda):
    """`python bench.py --gpus 2` from a plain shell (no torchrun, no WORLD_SIZE): the script starts its own two ranks (round 6: it used to
    warn and measure one GPU) — here over gloo on this box's one device, the rehearsal mode — and the line describes a world of two."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(HERE)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["MPCVR_DIST_BACKEND"] = "gloo"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--batch", "2", "--ring", "2", "--src", "256x144", "--no-cpu-baseline", "--no-host-path"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    d = r["config"]["distributed"]
    assert r["n_gpus"] == 2 and d["world_size"] == 2 and d["backend"] == "gloo" and len(d["devices"]) == 2
    assert sorted(x["rank"] for x in d["devices"]) == [0, 1]
    assert r["value"] > 0 and abs(r["config"]["fps_per_gpu"] * 2 - r["value"]) < 1e-2 * r["value"]
    # without the rehearsal backend two ranks on ONE device are refused before anything is spawned (the box has one GPU)
    if torch_cuda.cuda.device_count() < 2:
        env.pop("MPCVR_DIST_BACKEND")
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=root)
        assert out.returncode != 0 and "refusing" in out.stderr, (out.returncode, out.stderr[-500:])
        assert not [l for l in out.stdout.splitlines() if l.startswith("{")], "a refused run must not print a line"


# ------------------------------------------------------------------------------------------------
# 8-bit internal formats in front of a resize (round 5): the convert stage of the block / fused kernels takes its EXACT form there
# (FusedArgs::exact_cv, convert_block_exact in csrc/vp_fused_dev.h): every texel of m_TexConvertOutput carries the oracle's code, so a
# negative-lobe filter has no one-code-off texel to amplify to two codes.  Until round 4 the fuzz tool counted that class (1-3 channels
# per 1e6 on NV12 / YV12 resizes) instead of failing on it.
def _exact8_cases():
    from tests.golden.cases import ext, MPEG1, MPEG2, COSITED, TV, FULL, M709, M601
    sdr = GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]
    out = []
    # (label, cformat, extra): every source layout the block convert reads, every siting / chroma filter with an exact form of its own
    for label, cf, extra in [
            ("nv12", 1, {}), ("yv12", 14, {}), ("yuv420p8_mpeg1", 17, dict(exfmt=ext(MPEG1, TV, M601))), ("nv12_cosited_full", 1, dict(exfmt=ext(COSITED, FULL, M709))),
            ("nv12_nearest", 1, dict(iChromaScaling=0)), ("yuv420p8_catmull", 17, dict(iChromaScaling=2)), ("nv12_catmull_mpeg1", 1, dict(iChromaScaling=2, exfmt=ext(MPEG1, TV, M709))),
            ("yuy2", 4, {}), ("uyvy", 5, {}), ("ayuv", 11, {}), ("yv16", 15, {}), ("yuv422p8_nearest", 18, dict(iChromaScaling=0)), ("yv24", 16, {}), ("yuv444p8", 19, {}),
            ("gbrp8", 26, dict(exfmt=0)), ("y8", 37, {}),
            # deeper sources behind a forced 8-bit internal format: the 16-bit loaders, the CopyPlane10to16 shift, the 10:10:10:2 texel
            ("p010_tex8", 2, dict(iTexFormat=8)), ("yuv420p10_tex8", 20, dict(iTexFormat=8)), ("yuv422p10_tex8", 22, dict(iTexFormat=8)),
            ("y410_tex8", 12, dict(iTexFormat=8)), ("y416_tex8", 13, dict(iTexFormat=8)), ("y210_tex8", 8, dict(iTexFormat=8)), ("yuv444p10_tex8", 24, dict(iTexFormat=8))]:
        c = dict(cformat=cf, w=320, h=200, kind="noise", seed=8800 + len(out), exfmt=sdr, iUpscaling=4, dst=(270, 430), rotation=90)
        c.update(extra)
        out.append((label, c))
    return out


@pytest.mark.parametrize("label,c", _exact8_cases())
def test_exact_convert_stage_carries_the_oracles_codes(mpcvr, oracle, torch_cuda, label, c):
    """A quarter turn keeps the draws on the plain kernels (bit-exact with the oracle on SDR content) while the convert draw is the 2x2-block
    kernel: the whole frame is then identical to the oracle bit for bit exactly when every convert texel is (192,000 channels per case;
    the fast form of the stage differs in ~1e-4 of them)."""
    from videorenderer_amd import api
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    got, info = run_product(mpcvr, torch_cuda, c)
    assert info.startswith("passes:convert"), info
    compare(got, want, f"{label} [{info}]", exact=True)


FUZZ_8000_CASE_1250 = dict(cformat=17, w=544, h=98, kind="noise", seed=46112843, exfmt=32768, iChromaScaling=1, iUpscaling=2, iDownscaling=0,
                           bInterpolateAt50pct=1, dst=(981, 133))


def test_amplified_convert_code_replay_of_fuzz_8000_case_1250(mpcvr, oracle, torch_cuda):
    """profiles/r04/fuzz_8000.txt case 1250 (YUV420P8 544x98 -> 981x133 Catmull-Rom through k_fused_strip): one channel came out two codes off
    the oracle with the contracted convert stage."""
    c = FUZZ_8000_CASE_1250
    frame, pitch = case_frame(c)
    want = oracle.process(oracle_params(oracle, c), frame, pitch)
    got, info = run_product(mpcvr, torch_cuda, c)
    assert "fused_strip" in info or "fused_period" in info, info
    compare(got, want, f"fuzz_8000 case 1250 [{info}]", min_same=0.98)


def _hunt_case(rng, i):
    """8-bit internal format x negative-lobe filter x a ratio that is not 2x (a third of the cases exactly 2x: the other fused kernel)"""
    sdr = GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"]
    cf = int(rng.choice([1, 1, 14, 17, 4, 5, 11, 15, 18, 16, 19, 2, 20]))
    w, h = int(rng.integers(120, 330)) * 2, int(rng.integers(60, 150)) * 2
    c = dict(cformat=cf, w=w, h=h, kind="noise", seed=int(rng.integers(1, 1 << 30)), exfmt=sdr, iChromaScaling=int(rng.choice([0, 1, 1, 1])),
             iUpscaling=int(rng.choice([1, 2, 2, 3, 4, 4])), iDownscaling=int(rng.choice([3, 4, 5])), bInterpolateAt50pct=int(rng.integers(0, 2)))
    if cf in (2, 20):
        c["iTexFormat"] = 8
    mode = rng.random()
    if mode < 0.3:
        fx = fy = 2.0
    elif mode < 0.55:       # a periodic row ratio
        P_, Q_ = [(4, 3), (3, 2), (2, 3), (1, 2), (3, 1)][int(rng.integers(0, 5))]
        h -= h % (2 * Q_); c["h"] = h
        fx = fy = P_ / Q_
        c["bInterpolateAt50pct"] = 1
    else:
        fx, fy = float(rng.uniform(0.45, 2.6)), float(rng.uniform(0.45, 2.6))
    dw, dh = max(8, int(round(w * fx))), max(8, int(round(h * fy)))
    if mode >= 0.55:
        dw += dw == w; dh += dh == h
    c["dst"] = (dw, dh)
    return c


def test_hunt_8bit_internal_formats_behind_negative_lobe_filters(mpcvr, oracle, torch_cuda):
    """300 seeded shapes where the amplified-convert-code class lived (8-bit internal format, Catmull-Rom / Lanczos / bicubic, any ratio):
    the default planner within ONE code of the oracle on every channel — no count of exceptions.  (A net, not the detector: the class was
    one channel in ~1e8 on these shapes and the contracted convert stage passes this hunt too — profiles/r05/exact8_tests_with_fast_form_call1.txt;
    what tells the two forms apart is test_exact_convert_stage_carries_the_oracles_codes and the replay below it.)"""
    from videorenderer_amd import api
    rng = np.random.default_rng(20260925)
    kernels = {}
    channels = 0
    for i in range(300):
        c = _hunt_case(rng, i)
        frame, pitch = case_frame(c)
        want = oracle.process(oracle_params(oracle, c), frame, pitch)
        got, info = run_product(mpcvr, torch_cuda, c)
        d = np.abs(got[..., :3].astype(np.int16) - want[..., :3].astype(np.int16))
        assert d.max() <= 1, f"hunt {i}: {int((d > 1).sum())} channel(s) beyond one code (max {int(d.max())}) [{info}] {c}"
        assert float((d == 0).mean()) >= 0.97, f"hunt {i} [{info}] {c}"
        channels += d.size
        k = [q for q in info.split(";") if q.startswith("kernel=")]
        key = k[0].split("(")[0] if k else info.split(";")[0]
        kernels[key] = kernels.get(key, 0) + 1
    assert sum(v for k, v in kernels.items() if "fused" in k) >= 200, kernels
    if os.environ.get("MPCVR_PARITY_LOG"):
        import json
        with open(os.environ["MPCVR_PARITY_LOG"], "a") as f:
            f.write(json.dumps({"test": "hunt_8bit_internal", "cases": 300, "channels": int(channels), "kernels": kernels, "beyond_one_code": 0}) + "\n")


def test_full_size_up1440_nv12_within_one_code(mpcvr, oracle, torch_cuda):
    """bench.py's up1440_nv12 at its real size (1080p NV12 -> Catmull-Rom 4:3 -> 1440p, 8-bit internal format): all 11 M channels within one code."""
    c = dict(cformat=1, w=1920, h=1080, kind="noise", seed=1440, dst=(2560, 1440), iUpscaling=2, exfmt=GOLDEN_CASES["c1_nv12_bt709_passthrough"]["exfmt"])
    frame, pitch = case_frame(c)
    want = oracle.process(oracle_params(oracle, c), frame, pitch)
    got, info = run_product(mpcvr, torch_cuda, c)
    assert "fused_strip" in info or "fused_period" in info, info
    compare(got, want, f"up1440_nv12 [{info}]", min_same=WHOLE_FRAME_FLOOR)


def test_single_frames_queued_behind_a_batch_stay_behind_it(mpcvr, torch_cuda):
    """mpcvr_process_batch into dst[0..n) followed IMMEDIATELY, without a sync, by mpcvr_process into dst[0] (and by one out of a misaligned device
    sample, which is copied on the context stream first): the single frame runs on a frame lane and must neither overtake nor overlap the
    batch still running on the context stream (include/mpcvr.h: frames into the same target stay in order).  The batch is ~0.4 ms of 4K -> 8K
    frames, the single frame 45 us: without the context-stream -> lane edge the batch overwrites it."""
    from videorenderer_amd import api, synth
    torch = torch_cuda
    c = dict(GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"])
    c.update(w=3840, h=2160, dst=(7680, 4320))
    (ww, wh), vr = case_geometry(c)
    n = 6
    frames = []
    for i in range(n + 2):
        f, pitch = synth.make_frame(c["cformat"], c["w"], c["h"], "noise", seed=700 + i)
        frames.append(torch.from_numpy(np.ascontiguousarray(f)).cuda())
    kw = {k: c[k] for k in SETTING_KEYS if k in c}
    vp = api.VideoProcessor(api.default_settings(**kw), use_torch_stream=False)
    vp.InitMediaType(c["cformat"], c["w"], c["h"], extfmt=c.get("exfmt", 0))
    vp.SetWindowRect((0, 0, ww, wh))
    vp.SetVideoRect(vr)
    dsts = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in range(n)]
    # what frames n and n + 1 look like on their own
    alone = []
    for k in (n, n + 1):
        d = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
        vp.CopySample(frames[k], pitch); vp.Process(d, ww * 4); vp.Synchronize()
        alone.append(d.clone())
    # the second single frame arrives as a device sample that does not start on a dword: PrepareSample copies it on the context stream
    odd = torch.empty(frames[n + 1].numel() + 16, dtype=torch.uint8, device="cuda")
    odd[2:2 + frames[n + 1].numel()] = frames[n + 1]
    torch.cuda.synchronize()
    for rep in range(4):
        vp.ProcessBatch(frames[:n], dsts, ww * 4)
        vp.CopySample(frames[n], pitch)
        vp.Process(dsts[0], ww * 4)                  # a lane frame into the batch's first target
        vp.CopySample(odd[2:2 + frames[n + 1].numel()], pitch)
        vp.Process(dsts[1], ww * 4)                  # ... and one whose sample is still being copied
        vp.Synchronize()
        assert torch.equal(dsts[0], alone[0]), f"round {rep}: target 0 does not hold the frame queued behind the batch"
        assert torch.equal(dsts[1], alone[1]), f"round {rep}: target 1 does not hold the frame queued behind the batch (misaligned sample)"
    info = vp.GetVPInfo()
    vp.close()
    assert info.startswith("fused_up2x"), info


# (explicit ids: those of the cases that predate the expected-lanes column stay as they were)
@pytest.mark.parametrize("name,size,dst,route,lanes_off,expect", [
    pytest.param("c3hdr_p010_pq_lanczos3_2x", (1920, 1080), (3840, 2160), "fused_up2x", 0, (0, 1), id="c3hdr_p010_pq_lanczos3_2x-size0-dst0-fused_up2x-0"),
    pytest.param("c3hdr_p010_pq_lanczos3_2x", (1920, 1080), (2560, 1440), "kernel=fused_period", 0, (0, 1), id="c3hdr_p010_pq_lanczos3_2x-size1-dst1-kernel=fused_period-0"),
    pytest.param("c3hdr_p010_pq_lanczos3_2x", (1920, 1080), (2304, 1296), "kernel=fused_strip", 0, (0, 1), id="c3hdr_p010_pq_lanczos3_2x-size2-dst2-kernel=fused_strip-0"),
    pytest.param("c3hdr_p010_pq_lanczos3_2x", (1920, 1080), (2560, 1440), "kernel=fused_period", 1, (0, 1), id="c3hdr_p010_pq_lanczos3_2x-size3-dst3-kernel=fused_period-1"),
    pytest.param("c1_nv12_bt709_passthrough", (1920, 1080), (1920, 1080), "direct:convert", 0, (0, 1), id="c1_nv12_bt709_passthrough-size4-dst4-direct:convert-0"),
    # not on the lanes: a v210 batch on the exact-2x kernel reads its samples from the one shared batch texture they are repacked into, and a
    # quarter turn takes the whole-batch launches through the shared intermediate surfaces
    pytest.param("v210_2x", (1920, 1080), (3840, 2160), "fused_up2x", 0, (-1,), id="v210_2x-repacked-fused_up2x-context_stream"),
    pytest.param("rot90_two_pass_down_up", (96, 32), (48, 40), "resizeY;rot90", 0, (-1,), id="rot90_two_pass_down_up-whole_batch-context_stream")])
def test_batches_on_the_lanes_equal_batches_in_stream_order(mpcvr, torch_cuda, name, size, dst, route, lanes_off, expect):
    """(round 6) Consecutive mpcvr_process_batch calls of a context that owns its stream take turns on two lanes when the batch is one launch
    with nothing shared (exact 2x, strip / periodic kernel, same-size block convert): two launches in flight fill each other's ramp-up and
    tail.  What that must not change: every target holds exactly what the same sequence of calls leaves on a context bound to the caller's
    stream — also when consecutive batches write the SAME targets (the later batch waits for the earlier one's event), when the ring of
    targets wraps, and when a single frame follows into a target a batch in flight still writes.  MPCVR_NO_BATCH_LANES=1 (read once per
    process: a child process) keeps every batch on the context stream; `expect`: the lanes the batches take otherwise."""
    if lanes_off:
        code = ("import os, sys\nsys.path.insert(0, os.getcwd())\nimport torch\nfrom videorenderer_amd import api\nimport tests.test_parity_gpu as t\n"
                f"t.test_batches_on_the_lanes_equal_batches_in_stream_order(api, torch, {name!r}, {size!r}, {dst!r}, {route!r}, 0, {expect!r})\nprint('ok')\n")
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MPCVR_NO_BATCH_LANES="1"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
        return
    expect_lanes = {-1} if os.environ.get("MPCVR_NO_BATCH_LANES") == "1" else set(expect)
    from videorenderer_amd import api, synth
    torch = torch_cuda
    c = dict(GOLDEN_CASES[name])
    c.update(w=size[0], h=size[1], dst=dst)
    (ww, wh), vr = case_geometry(c)
    nb, n = 5, 8
    frames = []
    for i in range(nb * n + 1):
        f, pitch = synth.make_frame(c["cformat"], c["w"], c["h"], "noise", seed=900 + i)
        frames.append(torch.from_numpy(np.ascontiguousarray(f)).cuda())
    kw = {k: c[k] for k in SETTING_KEYS if k in c}

    def play(own):
        if not own:
            with torch.cuda.stream(torch.cuda.Stream()):         # (torch's default stream is NULL = "the context's own stream")
                return play_on(False)
        return play_on(True)

    def play_on(own):
        vp = api.VideoProcessor(api.default_settings(**kw), use_torch_stream=not own)
        vp.InitMediaType(c["cformat"], c["w"], c["h"], extfmt=c.get("exfmt", 0))
        vp.SetWindowRect((0, 0, ww, wh)); vp.SetVideoRect(vr)
        if "rotation" in c:
            vp.SetRotation(c["rotation"])
        ring = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in range(3 * n)]
        lanes = set()
        torch.cuda.synchronize()
        # five batches over a ring of three batches' worth of targets (the fourth and fifth write what the first and second wrote), then the
        # same targets again straight away from other samples, then a single frame into the first target of the batch still in flight
        for b in range(nb):
            k = (b * n) % len(ring)
            vp.ProcessBatch(frames[b * n:(b + 1) * n], ring[k:k + n], ww * 4)
            lanes.add(vp.GetLastBatchInfo()["lane"])
        k = ((nb - 1) * n) % len(ring)
        vp.ProcessBatch(frames[0:n], ring[k:k + n], ww * 4)
        lanes.add(vp.GetLastBatchInfo()["lane"])
        vp.CopySample(frames[nb * n], pitch)
        vp.Process(ring[k], ww * 4)
        vp.Synchronize()
        torch.cuda.synchronize()
        out = [t.clone() for t in ring]
        info = vp.GetVPInfo()
        vp.close()
        return out, lanes, info

    want, lanes_ref, info = play(False)
    assert route in info, info
    assert lanes_ref == {-1}, lanes_ref              # a caller's stream promises stream order: no lanes
    for rep in range(3):
        got, lanes, _ = play(True)
        assert lanes == expect_lanes, lanes
        for i, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(g, w), f"round {rep}: target {i} differs from the stream-ordered run"


@pytest.mark.parametrize("name,size,dst,route", [
    ("c3hdr_p010_pq_lanczos3_2x", (1920, 1080), (3840, 2160), "fused_up2x"),
    ("c3hdr_p010_pq_lanczos3_2x", (1920, 1080), (2560, 1440), "kernel=fused_period"),
    ("c3hdr_p010_pq_lanczos3_2x", (1920, 1080), (2304, 1296), "kernel=fused_strip"),
    ("c1_nv12_bt709_passthrough", (1920, 1080), (1920, 1080), "direct:convert")])
def test_overlapping_targets_keep_their_order_on_the_lanes(mpcvr, torch_cuda, name, size, dst, route):
    """Two writers of the same MEMORY stay in the order they were queued whatever pointers they were given (include/mpcvr.h): a window a few
    rows further down in one surface, the same surface addressed from another base.  Like test_batches_on_the_lanes_equal_batches_in_stream_order:
    a context on a caller's stream gives the stream-ordered truth, a context that owns its stream (batches and single frames on the lanes) must
    leave the same bytes, three rounds.  All targets are rows of ONE allocation of 3n * window_h + window_h (+ r) rows, addressed by pointer.
    Each sequence makes the race decide: the earlier writer is long (8 frames), the later, overlapping one short and aimed at what the long one
    writes last, both from different noise frames — "the earlier one finished last" leaves other bytes.
      shifted_batch        batch into rows k * window_h, then a batch window_h // 2 rows further down (each target over two targets in flight)
      frame_into_batch     mpcvr_process into a pointer inside a target of the batch in flight                          (PickFrameLane)
      batch_over_frames    a batch over single frames still in flight on a frame lane                                   (PickBatchLane, the rings)
      other_base           the allocation from its base pointer, then from base + dst_pitch * r, window unchanged
      adjacent             targets that touch (end of one == start of the next) and rows whose PADDING interleaves: still on both lanes,
                           and touching targets wait for nothing (GetLastBatchInfo: waits=0) — the order is kept without serialising everything"""
    import ctypes as C
    from videorenderer_amd import api, synth
    torch = torch_cuda
    c = dict(GOLDEN_CASES[name])
    c.update(w=size[0], h=size[1], dst=dst)
    (ww, wh), vr = case_geometry(c)
    n, r = 8, 16
    frames = []
    for i in range(2 * n + 4):
        f, pitch = synth.make_frame(c["cformat"], c["w"], c["h"], "noise", seed=1900 + i)
        frames.append(torch.from_numpy(np.ascontiguousarray(f)).cuda())
    kw = {k: c[k] for k in SETTING_KEYS if k in c}
    row = ww * 4
    rows_total = 3 * n * wh + wh + r

    def shifted_batch(vp, at, note):
        vp.ProcessBatch(frames[0:n], [at(i * wh) for i in range(n)], row); note(vp)
        vp.ProcessBatch(frames[n:n + 2], [at((n - 2 + j) * wh + wh // 2) for j in range(2)], row); note(vp)      # over targets 6, 7 (and free rows)
        vp.ProcessBatch(frames[n + 2:n + 4], [at((n + 2 + j) * wh) for j in range(2)], row); note(vp)              # disjoint: beside them

    def frame_into_batch(vp, at, note):
        vp.CopySample(frames[n + 2], pitch); vp.Process(at(2 * n * wh), row)         # (takes the first frame lane: the next frame gets another lane than the batch)
        vp.ProcessBatch(frames[0:n], [at(i * wh) for i in range(n)], row); note(vp)
        vp.CopySample(frames[n], pitch); vp.Process(at((n - 1) * wh + wh // 2), row)

    def batch_over_frames(vp, at, note):
        vp.CopySample(frames[n + 3], pitch); vp.Process(at(2 * n * wh), row)         # (the first frame lane — the lane the batch below takes)
        # seven frames into ONE target queue up on the second lane (mpcvr_process_frames: no interpreter between them, so they do queue up)
        arr = C.c_void_p * 7
        assert api.load_library().mpcvr_process_frames(vp._ctx, 7, arr(*[f.data_ptr() for f in frames[:7]]), pitch, api.MEM_DEVICE, arr(*[at(2 * wh)] * 7), row) == 0
        vp.ProcessBatch(frames[n:n + 2], [at(wh + wh // 2), at(2 * wh + wh // 2)], row); note(vp)

    def other_base(vp, at, note):
        vp.ProcessBatch(frames[0:n], [at(i * wh) for i in range(n)], row); note(vp)
        vp.ProcessBatch(frames[n:n + 2], [at(r + (n - 2 + j) * wh) for j in range(2)], row); note(vp)             # the same surface, r rows further down

    def adjacent(vp, at, note):
        for b in range(4):                    # every batch starts on the byte the one before ended on
            vp.ProcessBatch(frames[b * 4:b * 4 + 4], [at((b * 4 + i) * wh) for i in range(4)], row); note(vp, touching=b > 0)
        # a surface twice as wide: the left halves of its rows, then the right halves (each target's padding is the other's pixels)
        vp.ProcessBatch(frames[0:2], [at(4 * n * wh // 2 + 2 * i * wh) for i in range(2)], 2 * row); note(vp)
        vp.ProcessBatch(frames[2:4], [at(4 * n * wh // 2 + 2 * i * wh) + row for i in range(2)], 2 * row); note(vp)

    def play(seq, own):
        if not own:
            with torch.cuda.stream(torch.cuda.Stream()):         # (torch's default stream is NULL = "the context's own stream")
                return play_on(seq, False)
        return play_on(seq, True)

    def play_on(seq, own):
        vp = api.VideoProcessor(api.default_settings(**kw), use_torch_stream=not own)
        vp.InitMediaType(c["cformat"], c["w"], c["h"], extfmt=c.get("exfmt", 0))
        vp.SetWindowRect((0, 0, ww, wh)); vp.SetVideoRect(vr)
        surf = torch.full((rows_total * row,), BG, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        lanes, waits_touching = [], []

        def note(vp, touching=False):
            b = vp.GetLastBatchInfo()
            lanes.append(b["lane"])
            if touching:
                waits_touching.append(b["waits"])

        seq(vp, lambda first_row: surf.data_ptr() + first_row * row, note)
        vp.Synchronize()
        torch.cuda.synchronize()
        info = vp.GetVPInfo()
        vp.close()
        return surf, lanes, waits_touching, info

    failed = []
    for seq in (shifted_batch, frame_into_batch, batch_over_frames, other_base, adjacent):
        want, lanes_ref, _, info = play(seq, False)
        assert route in info, info
        assert set(lanes_ref) == {-1}, lanes_ref              # a caller's stream promises stream order: no lanes
        assert int((want != BG).sum()) >= 2 * wh * row        # (every sequence draws at least two frames)
        for rep in range(3):
            got, lanes, waits_touching, _ = play(seq, True)
            # the batches still take turns on the two lanes
            assert lanes == [i % 2 for i in range(len(lanes))], (seq.__name__, lanes)
            assert not any(waits_touching), (seq.__name__, "targets that only touch were ordered behind each other", waits_touching)
            if not torch.equal(got, want):
                bad = torch.nonzero((got != want).view(rows_total, row).any(dim=1)).flatten()
                failed.append(f"{seq.__name__} round {rep}: rows {int(bad[0])}..{int(bad[-1])} ({bad.numel()} rows) differ from the stream-ordered run")
                break
            del got
    assert not failed, failed


def test_bench_through_rccl_in_a_world_of_one(mpcvr, torch_cuda):
    """The `nccl` branch of videorenderer_amd/dist.py on hardware, as far as one GPU allows: bench.py under torchrun with ONE rank and
    MPCVR_DIST_FORCE=1 — init_process_group("nccl"), the parameter-blob broadcast, the max-over-ranks all_reduce and all_gather_object all
    execute over RCCL (a world of one), and the line says which RCCL it was.  No scaling curve comes out of this; that is the driver's run."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(HERE)
    env = dict(os.environ, MPCVR_DIST_FORCE="1")
    env.pop("MPCVR_DIST_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--batch", "2", "--ring", "2", "--src", "256x144", "--no-cpu-baseline", "--no-host-path"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    d = r["config"]["distributed"]
    assert d["backend"] == "nccl" and d["world_size"] == 1 and d.get("rccl_version") and "unavailable" not in d["rccl_version"], d
    assert r["n_gpus"] == 1 and r["value"] > 0 and r["config"]["path"] == "fused_up2x"


def _bench_line(args, timeout=600):
    import json
    root = os.path.dirname(HERE)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_dump_outputs_is_the_last_step(mpcvr, torch_cuda, tmp_path):
    """bench.py --dump-outputs: the render targets of the last timed step as float32 codes, the same arrays from two runs with the same
    arguments, and the very bytes mpcvr_process_batch gives for those ring frames; a plain run does none of --full's side measurements."""
    from bench import WORKLOADS, noise_frame_gpu
    from videorenderer_amd import api
    torch = torch_cuda
    small = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--settle", "0", "--batch", "2", "--ring", "3", "--src", "256x144"]
    r = _bench_line(small + ["--dump-outputs", str(tmp_path / "a")])
    _bench_line(small + ["--dump-outputs", str(tmp_path / "b")])
    assert r["steps"] == 3 and r["ms_per_step"] > 0 and r["config"]["side_measurements"] is False
    assert "cpu_baseline" not in r and "process_per_frame" not in r and r["roofline"]["empirical_copy_peak_GBps"] is None
    a = np.load(tmp_path / "a" / "render_targets.npy")
    assert a.dtype == np.float32 and a.shape == (2, 288, 512, 4)
    assert np.array_equal(a, np.load(tmp_path / "b" / "render_targets.npy"))
    assert not (tmp_path / "a" / "render_targets_pixel_index.npy").exists()
    # the last step is step 1 + 3 - 1 = 3: ring offset 3 * 2 % 3 = 0, i.e. the ring's frames 0 and 1 (bench.py's seeded noise)
    wl = dict(WORKLOADS["c3hdr"], w=256, h=144)
    vp = api.VideoProcessor(api.default_settings(iUpscaling=wl["iUpscaling"], iDownscaling=2, flags=0, output_format=0, bUseDither=1), device=0)
    vp.InitMediaType(wl["cformat"], 256, 144, extfmt=api.make_extfmt(**wl["ext"]))
    vp.SetWindowRect((0, 0, 512, 288))
    vp.SetVideoRect((0, 0, 512, 288))
    nbytes, pitch = vp.GetFrameBytes()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x4D50)
    srcs = [noise_frame_gpu(torch, wl, nbytes, pitch, gen) for _ in range(2)]
    dsts = [torch.zeros((288, 512, 4), dtype=torch.uint8, device="cuda") for _ in range(2)]
    vp.ProcessBatch(vp.PrepareBatch(srcs, dsts), None, 512 * 4)
    vp.Synchronize()
    vp.close()
    assert np.array_equal(a, np.stack([d.cpu().numpy() for d in dsts]).astype(np.float32))
    # a full-size batch is a seeded sample at the same pixels of every frame, under the 64 MB cap
    big = ["--gpus", "1", "--steps", "1", "--warmup", "0", "--settle", "0", "--batch", "2", "--ring", "2"]
    _bench_line(big + ["--dump-outputs", str(tmp_path / "c")])
    s = np.load(tmp_path / "c" / "render_targets.npy")
    idx = np.load(tmp_path / "c" / "render_targets_pixel_index.npy")
    assert s.dtype == np.float32 and idx.dtype == np.float64 and s.shape == (2, idx.size, 4)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 7680 * 4320
    assert sum(os.path.getsize(tmp_path / "c" / f) for f in os.listdir(tmp_path / "c")) <= 64e6


def test_bandwidth_probe_moves_what_it_says(mpcvr, torch_cuda):
    """mpcvr_bandwidth_probe (csrc/vp_probe.hip, bench.py's traffic-shaped ceiling): every 16-byte word of the source read once, `fan` words written."""
    import ctypes as C
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    n, fan = 1 << 16, 5
    src = torch.randint(0, 1 << 31, (n // 4,), dtype=torch.int32, device="cuda")
    dst = torch.zeros((fan, n // 4), dtype=torch.int32, device="cuda")
    assert L.mpcvr_bandwidth_probe(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), C.c_size_t(n), fan, None) == 0
    torch.cuda.synchronize()
    s4 = src.view(-1, 4)
    for k in range(fan):
        d4 = dst[k].view(-1, 4)
        assert torch.equal(d4[:, 1:], s4[:, 1:]) and torch.equal(d4[:, 0], s4[:, 0] + k)
    assert L.mpcvr_bandwidth_probe(None, C.c_void_p(dst.data_ptr()), C.c_size_t(n), fan, None) < 0
    assert L.mpcvr_bandwidth_probe(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), C.c_size_t(n), 0, None) < 0


def test_up2x_shape_probe_writes_the_kernels_pattern(mpcvr, torch_cuda):
    """mpcvr_bandwidth_probe_up2x (csrc/vp_probe.hip: the exact-2x kernel's own traffic shape over a batch in one launch): mode 0 writes, for
    every source row pair, four target rows whose 16-byte pieces carry the luma / chroma dwords the lane read (so every byte of a target is
    written exactly once, by the lane and row the kernel would write it from); mode 1 writes without reading; mode 2 writes nothing."""
    import ctypes as C
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    w, h, n = 256, 48, 3
    srcs = [torch.randint(0, 1 << 31, (w * h * 3 // 4,), dtype=torch.int32, device="cuda") for _ in range(n)]
    arr = C.c_void_p * n
    for cols in (120, 128):
        for mode in (0, 1, 2):
            dsts = [torch.full((2 * h, 2 * w), -1, dtype=torch.int32, device="cuda") for _ in range(n)]
            assert L.mpcvr_bandwidth_probe_up2x(mode, n, arr(*[t.data_ptr() for t in srcs]), arr(*[t.data_ptr() for t in dsts]), w, h, 12, cols, None) == 0
            torch.cuda.synchronize()
            for z in range(n):
                d = dsts[z].cpu().numpy().reshape(2 * h, w // 2, 4)           # [row][16-byte piece][dword]
                if mode == 2:
                    assert (d == -1).all()
                    continue
                assert (d != -1).any(axis=2).all(), "every 16-byte piece of the target is written"
                rows = np.arange(2 * h)
                assert np.array_equal(d[:, :, 3], np.broadcast_to(((rows // 4) * 2)[:, None], d[:, :, 3].shape))      # the source row of the pair
                if mode == 0:
                    s = srcs[z].cpu().numpy()
                    luma = s[: w * h // 2].reshape(h, w // 2)                  # one dword = two 16-bit luma samples
                    chroma = s[w * h // 2:].reshape(h // 2, w // 2)
                    r0 = (rows // 4) * 2
                    assert np.array_equal(d[:, :, 0], luma[r0] + (rows % 4)[:, None]) and np.array_equal(d[:, :, 1], luma[r0 + 1])
                    assert np.array_equal(d[:, :, 2], chroma[r0 // 2])
    assert L.mpcvr_bandwidth_probe_up2x(3, n, arr(*[t.data_ptr() for t in srcs]), arr(*[t.data_ptr() for t in srcs]), w, h, 12, 120, None) < 0
    assert L.mpcvr_bandwidth_probe_up2x(0, n, arr(*[t.data_ptr() for t in srcs]), arr(*[t.data_ptr() for t in srcs]), w, h, 12, 130, None) < 0


def test_process_frames_equals_frame_by_frame_calls(mpcvr, torch_cuda):
    """mpcvr_process_frames (the per-frame loop — mpcvr_copy_sample + mpcvr_process — behind one call, so that a scripting-language caller
    does not time its own FFI): the same targets, bit for bit, as the calls made one by one; on the frame lanes and strictly in order."""
    import ctypes as C
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    c = GOLDEN_CASES["noise_p010_pq_lanczos3_2x"]
    frames = [torch.from_numpy(case_frame(dict(c, seed=c["seed"] + 5 * k))[0]).cuda() for k in range(6)]
    for extra in (0, api.FLAG_NO_FRAME_LANES):
        vp = api.VideoProcessor(api.default_settings(iUpscaling=c["iUpscaling"], flags=extra), device=0, use_torch_stream=False)
        vp.InitMediaType(c["cformat"], c["w"], c["h"], extfmt=c.get("exfmt", 0))
        w2, h2 = c["dst"]
        vp.SetWindowRect((0, 0, w2, h2)); vp.SetVideoRect((0, 0, w2, h2))
        pitch = vp.GetFrameBytes()[1]
        one = [torch.zeros((h2, w2, 4), dtype=torch.uint8, device="cuda") for _ in frames]
        for f, d in zip(frames, one):
            vp.CopySample(f, pitch); vp.Process(d, w2 * 4)
        vp.Synchronize()
        many = [torch.zeros((h2, w2, 4), dtype=torch.uint8, device="cuda") for _ in frames]
        arr = C.c_void_p * len(frames)
        assert L.mpcvr_process_frames(vp._ctx, len(frames), arr(*[f.data_ptr() for f in frames]), pitch, api.MEM_DEVICE, arr(*[d.data_ptr() for d in many]), w2 * 4) == 0
        vp.Synchronize()
        for a, b in zip(one, many):
            assert torch.equal(a, b)
        assert not torch.equal(many[0], many[1])
        assert L.mpcvr_process_frames(vp._ctx, 2, None, pitch, api.MEM_DEVICE, None, w2 * 4) < 0
        vp.close()
