"""tests/sample_layouts.py itself, and the condition every GPU comparison of tests/test_sample_layout_gpu.py rests on: THE ORACLE READS NO
PADDING.  A sample re-laid at a padded pitch with its padding poisoned gives the oracle's picture of the tight sample bit for bit — for every
one of the 39 formats, on the plain convert and on one resize — so a library frame that differs between two poisons, or from its tight frame,
has read a byte that is not a pixel.

The exceptions are the interleaved RGB formats, whose copy functions loop over line_pixels = |pitch| / bytes-per-pixel instead of the width
(Helper.cpp, restated line by line in oracle/mpcvr_oracle.c::orc_repack_rgb), so the PITCH decides how many texels of a row are filled:
  * RGB48 (CopyFrameRGB48, Helper.cpp:541-565) copies whole groups of four and has no remainder branch: at the tight pitch a width of 4k + r
    leaves the last r texels black; a pitch of at least (4k + 4) * 6 bytes fills them.  Padded and tight differ whenever width % 4 != 0 and the
    pitch reaches the next group (46 x 12 at pitch 288 and above: texels 44 and 45).
  * RGB24 (CopyFrameRGB24, Helper.cpp:446-482) handles a remainder of line_pixels % 4 by its parity alone: odd => one texel.  A remainder of
    three therefore fills one texel and leaves two black.  The default pitch (3 w rounded up to 4) never gives a remainder of three; a pitch with
    |pitch| // 3 == width == 4k + 3 does (47 x 12 at pitch 141 .. 143: texels 45 and 46 black, filled at the default pitch 144), and so does
    |pitch| // 3 == width + 1 == 4k + 3 (46 x 12 at pitch 141 .. 143: texel 45).
  * BGR48 (CopyFrameBGR48, Helper.cpp:600-645) has a branch for every remainder, RGB32 / r210 / BGRA64 / b64a copy line_pixels texels
    (:414-428, :770-787, :647-683): always the whole width — padded equals tight.
Which texels a pitch fills is rgb_texels_written(); the test below holds the oracle to it.  In NO case does a padding byte reach a sampled texel
(the loops write pad bytes only into texels at or behind `width`, and into the X / A byte of RGB24's raw dword copies, which no shader reads):
poison A == poison B holds for every format and no case is kept out of the GPU test's A/B assertion.
"""
import numpy as np
import pytest

from tests.golden.cases import ext, M709
from tests.sample_layouts import (ALL_FORMATS, PITCH_CLASSES, RGB_BPP, RGB_FORMATS, bottom_up, frame_bytes, pitch_of, pixel_mask, relayout,
                                  rgb_texels_written, row_bytes, sample_bytes, strip)
from videorenderer_amd import synth

W, H = 22, 8        # v210: 3 groups and 4 pixels of a fourth; 4:2:0: 11 x 4 chroma samples; RGB: 22 = 4 * 5 + 2
POISON_A, POISON_B = 1, 2


def test_all_39_formats():
    assert len(ALL_FORMATS) == 39


def pitches_for(cformat, w):
    """every pitch class the format admits, plus a pitch 12 bytes above the (4-byte aligned) tight row"""
    ps = {pitch_of(cls, cformat, w) for cls in PITCH_CLASSES} - {None}
    ps.add(((row_bytes(cformat, w) + 3) & ~3) + 12)
    if cformat in synth.FORMATS and synth.FORMATS[cformat][:2] == (3, 2):
        ps = {p for p in ps if (p // synth.FORMATS[cformat][2]) % 2 == 0}       # 16-bit chroma rows start on even addresses (include/mpcvr.h)
    return sorted(ps)


@pytest.mark.parametrize("cformat", ALL_FORMATS)
def test_relayout_to_the_default_pitch_returns_the_frame(cformat):
    for w, h in ((W, H), (46, 4), (62, 6)):         # (default pitches with padding of their own: NV12 / Y8 / RGB24 / BGR48 at 22, 46, 62; v210 always)
        frame, pitch = synth.make_frame(cformat, w, h, "noise", seed=900 + cformat)
        assert frame.size == frame_bytes(cformat, w, h, pitch)
        assert np.array_equal(relayout(frame, cformat, w, h, pitch, None), frame)
        poisoned = relayout(frame, cformat, w, h, pitch, POISON_A)
        mask = pixel_mask(cformat, w, h, pitch)
        assert np.array_equal(poisoned[mask], frame[mask])
        assert mask.all() or poisoned[~mask].any()


@pytest.mark.parametrize("cformat", ALL_FORMATS)
def test_stripping_a_relaid_frame_gives_the_tight_frame_back(cformat):
    frame, tight = synth.make_frame(cformat, W, H, "noise", seed=910 + cformat)
    pixels = strip(frame, cformat, W, H, tight)
    ps = pitches_for(cformat, W)
    assert len(ps) >= 3
    for p in ps:
        a, b = relayout(frame, cformat, W, H, p, POISON_A), relayout(frame, cformat, W, H, p, POISON_B)
        assert a.size == b.size == frame_bytes(cformat, W, H, p)
        assert np.array_equal(strip(a, cformat, W, H, p), pixels) and np.array_equal(strip(b, cformat, W, H, p), pixels)
        mask = pixel_mask(cformat, W, H, p)
        assert not mask.all() and (a[~mask] != b[~mask]).all(), "the two poisons differ in every padding byte"
        assert a[~mask].any() and b[~mask].any()
        # synth at that pitch is the same picture with zeroed padding (three-plane formats: its chroma planes follow pitch // div_w as well)
        direct, _ = synth.make_frame(cformat, W, H, "noise", seed=910 + cformat, pitch=p)
        z = relayout(frame, cformat, W, H, p, None)
        assert np.array_equal(z[:direct.size], direct) and not z[direct.size:].any()


def test_pitch_classes():
    for cf in ALL_FORMATS:
        t, b = row_bytes(cf, 136), sample_bytes(cf)
        for cls, (mod, res) in {"mod16=8": (16, 8), "mod8=4": (8, 4), "mod4=2": (4, 2), "odd": (2, 1)}.items():
            p = pitch_of(cls, cf, 136)
            if p is None:
                assert (cls == "odd" and b > 1) or (cls == "mod4=2" and b == 4)
                continue
            assert t < p <= t + mod and p % mod == res and p % b == 0
        p = pitch_of("wide", cf, 136)
        assert p % 256 == 0 and t < p <= t + 256


def params_for(oracle, cformat, w, h, dst):
    return oracle.default_params(cformat=cformat, width=w, height=h, exfmt=ext(matrix=M709), window_w=dst[0], window_h=dst[1],
                                 video_rect=(0, 0, dst[0], dst[1]), iUpscaling=2)


@pytest.mark.parametrize("cformat", ALL_FORMATS)
def test_the_oracle_reads_no_padding(oracle, cformat):
    frame, tight = synth.make_frame(cformat, W, H, "noise", seed=920 + cformat)
    kind = synth.PACKED[cformat][0] if cformat in synth.PACKED else None
    for dst in ((W, H), (2 * W, 2 * H)):            # the plain convert (RGB: the copy), and Catmull-Rom 2x
        p = params_for(oracle, cformat, W, H, dst)
        want = oracle.process(p, frame, tight)
        for pitch in pitches_for(cformat, W):
            a = oracle.process(p, relayout(frame, cformat, W, H, pitch, POISON_A), pitch)
            b = oracle.process(p, relayout(frame, cformat, W, H, pitch, POISON_B), pitch)
            assert np.array_equal(a, b), f"cformat {cformat} pitch {pitch} -> {dst}: the oracle's picture depends on the padding bytes"
            if kind in synth.RGB_FAMILIES and rgb_texels_written(kind, pitch, W) != rgb_texels_written(kind, tight, W):
                assert not np.array_equal(a, want), (cformat, pitch)        # (the module docstring: RGB48 / RGB24, pitch-driven copy loops)
                continue
            assert np.array_equal(a, want), f"cformat {cformat} pitch {pitch} -> {dst}: padded differs from tight"


@pytest.mark.parametrize("cformat", RGB_FORMATS)
@pytest.mark.parametrize("w", [45, 46, 47])
def test_the_oracles_rgb_copy_loops_fill_what_the_pitch_says(oracle, cformat, w):
    """Same-size copy of an interleaved RGB sample (no convert draw: the texture is what is shown) for every |pitch| // bpp from the width to the
    width + 5, top-down and bottom-up: columns below rgb_texels_written() show the tight frame's pixels, the rest of the row is black, and the
    poison shows nowhere."""
    h = 4
    kind = synth.PACKED[cformat][0]
    bpp = RGB_BPP[kind]
    frame, tight = synth.make_frame(cformat, w, h, "noise", seed=930 + cformat)
    p = params_for(oracle, cformat, w, h, (w, h))
    full_pitch = ((w + 4) * bpp + 3) & ~3                   # a pitch that fills every texel of the row whatever the loop
    assert rgb_texels_written(kind, full_pitch, w) == w
    full = oracle.process(p, relayout(frame, cformat, w, h, full_pitch, None), full_pitch)
    step = 4 if sample_bytes(cformat) == 4 else 2 if sample_bytes(cformat) == 2 else 1
    seen = set()
    for pitch in range(w * bpp, (w + 6) * bpp, step):
        n = rgb_texels_written(kind, pitch, w)
        seen.add((pitch // bpp) % 4)
        for up in (False, True):
            outs = []
            for poison in (POISON_A, POISON_B):
                buf, sp = relayout(frame, cformat, w, h, pitch, poison), pitch
                if up:
                    buf, sp = bottom_up(buf, h, pitch)
                outs.append(oracle.process(p, buf, sp))
            assert np.array_equal(outs[0], outs[1]), (cformat, w, pitch, up)
            assert np.array_equal(outs[0][:, :n], full[:, :n]), (cformat, w, pitch, up, n)
            assert not outs[0][:, n:, :3].any(), (cformat, w, pitch, up, n)
    assert seen == {0, 1, 2, 3}
