"""The oracle pinned to the REFERENCE's own shader text (oracle/ref_hlsl/).

The reference has no tests and its arithmetic is HLSL.  oracle/ref_hlsl compiles that HLSL — the fixed shaders
of /root/reference/Shaders and the convert shader the real Source/Shaders.cpp generates — for the CPU behind a small execution
model of Direct3D (hlsl_shim.h) and runs the whole Process() with it (ref_pipeline.py).  These tests hold the oracle to it:

  * every comparable golden / pinning case (172) AND the BASELINE configurations at their real sizes (4K -> 8K, 1080p -> 4K,
    1080p, 1080p -> 1440p, 4K -> 1440p ...: tests/golden/cases.py FULL_SIZE_CASES): B, G, R of the oracle's render target against
    the reference-text result — recorded as sha256 in tests/golden/ref_hlsl_pins.json / full_size_pins.json, so the check runs
    without /root/reference; and live whenever oracle/_ref/libref_hlsl.so is built (here, and on the GPU box where it travels);
  * bar: BIT-IDENTICAL, every case (round 3).  Until round 2 nine cases sat at <= 1 code and ps_convolution's box filter at a
    2.4x ratio differed by whole taps: the oracle computed Tex * wh as `src_l + (i + .5) * src / dst` where the reference rounds
    the quad's corner coordinates to fp32 first (FillVertices, DX11VideoProcessor.cpp:133-138: src_dx = 1.0f / texW; src_l =
    src_dx * rect.left ...).  With those three roundings restated (oracle axis_center, product TexCenter) every tap decision —
    the box filter's `x < 0.5` edge included — falls the way the shader text's does, at every size;
  * "bit-identical" is UNDER THE MODELLED INTERPOLATOR: the shader text is the reference's, the rasteriser that hands it texture
    coordinates is oracle/ref_hlsl/ref_draw.h's model (interpolation in double, one rounding to fp32) — the same model TexCenter and
    axis_center restate.  Channels that hang on the last ulp of a coordinate (exact texel centres at 3:1, the box filter's x < 0.5 edge)
    are decided by that model on both sides; real hardware's fixed-point interpolators are not claimed to agree there;
  * alpha is not compared: the reference leaves the shader's A there (not 1 after the float4-wide HLG / Dolby Vision tails) and the
    swap chain ignores it; the oracle and the product write opaque alpha.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_hlsl"))

from tests.golden import cases  # noqa: E402
from tests.golden.make_ref_hlsl_golden import all_cases, comparable, rgb_channels  # noqa: E402

with open(os.path.join(HERE, "golden", "ref_hlsl_pins.json")) as _f:
    PINS = json.load(_f)["cases"]
OUTS = np.load(os.path.join(HERE, "golden", "ref_hlsl_outputs.npz"))
CASES = {k: v for k, v in all_cases().items() if comparable(v)}

with open(os.path.join(HERE, "golden", "full_size_pins.json")) as _f:
    FULL_PINS = json.load(_f)["cases"]


def oracle_rgb(oracle, name):
    a = cases.run_case(oracle, name)
    c = CASES[name]
    if c.get("output_format", 0) == 1:
        a = a.view(np.uint32).reshape(a.shape[0], a.shape[1])
    return rgb_channels(a)


def sha(ch):
    return hashlib.sha256(ch.astype(np.uint16).tobytes()).hexdigest()


def test_every_comparable_case_is_pinned():
    assert set(PINS) == set(CASES)
    assert len(PINS) >= 185
    assert set(c["cformat"] for c in CASES.values()) == set(range(1, 40))          # every ColorFormat_t (Helper.h:86-127), interleaved RGB included
    for n, p in PINS.items():
        assert p["oracle_max"] == 0 and p["oracle_differing"] == 0.0, (n, p)       # bit-identical to the reference shader text
    assert len(OUTS.files) == 0                                                     # ... so no reference output needs storing
    assert set(FULL_PINS) == set(cases.FULL_SIZE_CASES)
    for n, p in FULL_PINS.items():
        assert p["oracle_max"] == 0, (n, p)


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_against_recorded_reference_hlsl(oracle, name):
    assert sha(oracle_rgb(oracle, name)) == PINS[name]["rgb_sha256"], "oracle no longer bit-identical to the reference shader text"


@pytest.mark.parametrize("name", sorted(cases.FULL_SIZE_CASES))
def test_oracle_full_size_against_recorded_reference_hlsl(oracle, name):
    """BASELINE configurations at their real sizes (33 M output pixels at 4K -> 8K): the oracle's render target hashes to what the
    reference's shader text produced (tests/golden/make_full_size_pins.py)."""
    got = rgb_channels(cases.run_case(oracle, name))
    assert sha(got) == FULL_PINS[name]["rgb_sha256"], "oracle no longer bit-identical to the reference shader text at full size"


def _live():
    import ref_hlsl
    if not ref_hlsl.available():
        pytest.skip("oracle/_ref/libref_hlsl.so not built (no /root/reference here)")
    import ref_pipeline
    return ref_pipeline


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_against_live_reference_hlsl(oracle, name):
    RP = _live()
    c = CASES[name]
    frame, pitch = cases.case_frame(c)
    p = cases.oracle_params(oracle, c)
    try:
        ref = RP.process(p, frame, pitch)
    except RuntimeError as e:
        pytest.skip(str(e))
    ref = rgb_channels(ref)
    assert sha(ref) == PINS[name]["rgb_sha256"], "reference-text result changed: regenerate tests/golden/ref_hlsl_pins.json"
    d = np.abs(oracle_rgb(oracle, name) - ref)
    assert int(d.max()) == 0


@pytest.mark.parametrize("name", sorted(cases.FULL_SIZE_CASES))
def test_oracle_full_size_against_live_reference_hlsl(oracle, name):
    """The same at full size, live: the reference shader text is executed here (5 - 15 s per 8K frame on 8 threads)."""
    RP = _live()
    c = cases.FULL_SIZE_CASES[name]
    frame, pitch = cases.case_frame(c)
    p = cases.oracle_params(oracle, c)
    try:
        ref = rgb_channels(RP.process(p, frame, pitch))
    except RuntimeError as e:
        pytest.skip(str(e))
    assert sha(ref) == FULL_PINS[name]["rgb_sha256"], "reference-text result changed: regenerate tests/golden/full_size_pins.json"
    got = rgb_channels(oracle.process(p, frame, pitch))
    assert np.array_equal(got, ref)


def test_headline_convert_shader_is_the_generators_text():
    """The text comes out of the real GetShaderConvertColor: spot-check SURVEY.md appendix A's lines (Shaders.cpp:819-921)."""
    RP = _live()
    import ref_hlsl
    from oracle import oracle as O
    p = cases.oracle_params(O, dict(cformat=2, w=3840, h=2160, dst=(7680, 4320), exfmt=cases.HDR10, iUpscaling=4))
    text = ref_hlsl.convert_shader_text(*RP.convert_args(p))
    if text is None:
        pytest.skip("reference tree not mounted")
    for line in ("#define w 3840", "#define dx (1.0/3840)", "static const float2 wh = {3840, 2160};",
                 "float2 pos = input.Tex+float2(dx*0.5,0);", "colorUV = texUV.Sample(sampL, pos).rg;",
                 "color.rgb = float3(mul(cm_r, color.rgb), mul(cm_g, color.rgb), mul(cm_b, color.rgb)) + cm_c;",
                 "color = ST2084ToLinear(color, LuminanceScale);", "color.rgb = ToneMappingHable(color.rgb);",
                 "color.rgb = mul(matrix_conv_prim, color.rgb);", "color = pow(color, 1.0/2.2);"):
        assert line in text, line
    assert "1.660497, -0.58765674, -0.072839946" in text             # std::format("{}") of the real gamut matrix (:634-645)


CORR = {1: "fix_bt2020", 2: "fix_ycgco", 3: "fixconvert_pq_to_sdr", 4: "fixconvert_hlg_to_sdr", 5: "convert_pq_to_sdr", 6: "convert_hlg_to_pq"}


@pytest.mark.parametrize("kind", sorted(CORR))
@pytest.mark.parametrize("fmts", [(8, 8), (10, 10), (10, 8)])
def test_correction_shaders_against_live_reference_hlsl(oracle, kind, fmts):
    """m_pPSCorrection shaders (ps_fix_*.hlsl, ps_fixconvert_*.hlsl, ps_convert_*.hlsl) vs orc_correction_pass.  Kinds 3, 4 and 5 read
    LuminanceScale = 10000 / nits: they run at every value of tests/tone_params.py's SDR_NITS (both ends of 25 .. 400, their neighbours, the
    default 125 and values in between); kinds 1, 2 and 6 do not read it and keep their single run."""
    _live()
    import ref_hlsl as R
    from tests.tone_params import SDR_NITS
    assert 125 in SDR_NITS
    src_fmt, dst_fmt = fmts
    rng = np.random.default_rng(100 * kind + src_fmt + dst_fmt)
    h, w = 24, 64
    src = rng.integers(0, 2 ** 32, size=(h, w), dtype=np.uint32)
    tex = np.zeros((h, w, 4), np.float32)
    if src_fmt == 10:
        for k in range(3):
            tex[..., k] = ((src >> (10 * k)) & 1023).astype(np.float32) / np.float32(1023)
        tex[..., 3] = (src >> 30).astype(np.float32) / np.float32(3)
    else:
        for k, sh_ in enumerate((16, 8, 0, 24)):
            tex[..., k] = ((src >> sh_) & 255).astype(np.float32) / np.float32(255)
    fn = R.find_shader("ps_" + CORR[kind])
    seen = set()
    for nits in (SDR_NITS if kind in (3, 4, 5) else (125,)):
        got = oracle.correction_pass(kind, src, src_fmt, dst_fmt, sdr_nits=nits)
        rt = np.zeros((h, w, 4), np.float32)
        lum = R.words(np.float32(10000.0) / np.float32(nits), np.float32(0))
        R.draw(fn, [tex], rt, dst_fmt, (0, 0, w, h), ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0)), samplers=[(0, 0)], cbs=[lum])
        if dst_fmt == 10:
            ref = np.stack([np.floor(rt[..., k] * np.float32(1023) + np.float32(0.5)) for k in range(3)], -1).astype(np.int32)
            gch = np.stack([(got >> (10 * k)) & 1023 for k in range(3)], -1).astype(np.int32)
        else:
            ref = np.stack([np.floor(rt[..., k] * np.float32(255) + np.float32(0.5)) for k in range(3)], -1).astype(np.int32)
            gch = np.stack([(got >> sh_) & 255 for sh_ in (16, 8, 0)], -1).astype(np.int32)
        d = np.abs(ref - gch)
        assert d.max() == 0, (nits, int(d.max()), float((d > 0).mean()))
        seen.add(ref.tobytes())
    assert len(seen) == (len(SDR_NITS) if kind in (3, 4, 5) else 1)        # the nits reach the shader: nine different surfaces


# ---- the rewrite itself (host logic; no reference needed) ----
def test_hlsl2cpp_rules():
    import hlsl2cpp
    lit = lambda s: hlsl2cpp._FLOAT_LIT.sub(lambda m: m.group(1) + "f", s)
    assert lit("a = 1.0 / x + .5 - 2. * 1e-6 + 3.0f + float4x4(1) + v.x2") == "a = 1.0f / x + .5f - 2.f * 1e-6f + 3.0f + float4x4(1) + v.x2"
    assert lit("#define w 3840") == "#define w 3840"
    src = ("cbuffer PS_CONSTANTS : register(b0)\n{\n float2 wh;\n float pad[2];\n};\nTexture2D tex : register(t0);\n"
           "SamplerState samp : register(s0);\nstatic const float k = 0.5;\nstruct PS_INPUT { float4 Pos : SV_POSITION; float2 Tex : TEXCOORD; };\n"
           "float4 main(PS_INPUT input) : SV_Target\n{\n float3 rgb = tex.Sample(samp, input.Tex).rgb;\n"
           " rgb = (rgb <= 0.5)\n  ? rgb * 2.0\n  : rgb;\n [unroll(3)]\n for (uint c = 0; c < 3; c++) {}\n return float4(rgb, 1);\n}\n")
    out = hlsl2cpp.transform(src, "t")
    assert "float2 wh = hlsl::cb_pop<float2 >(0);" in out and "hlsl::arr<float, 2> pad = hlsl::cb_pop<hlsl::arr<float, 2> >(0);" in out
    assert "register" not in out and "SV_" not in out and "unroll" not in out and "TEXCOORD" not in out
    assert "\nconst float k = 0.5f;" in out
    assert "rgb = hlsl::select((rgb <= 0.5f), (rgb * 2.0f), (rgb));" in out
    assert "tex.s = &rd__.tex[0];" in out and "samp.filter = rd__.samp_filter[0];" in out
    assert 'extern "C" void t(const RefDraw* rd__)' in out
