"""tests/sample_bits.py itself, and the condition the metamorphic assertion of tests/test_sample_bits_gpu.py rests on: THE ORACLE IGNORES the
`high`, `alpha` and `pad` bits of a sample — for every one of the 39 formats, on the default convert and through a 1.5x Lanczos3 resize, a
legal noise frame and its two with_ignored_bits twins give the same picture bit for bit — and READS the `low` bits of P010 / P210 / Y210.

What the reference does with the LSB-aligned 10-bit planes is CopyPlane10to16 (Helper.cpp:789-803): dst16[i] = src16[i] << 6 stored into a
uint16_t, so bits 10..15 of the word fall off the top; oracle/mpcvr_oracle.c::load_luma / load_chroma restate it as (uint16_t)(v << shift), and
tests/test_oracle_pins.py pins both over all 65,536 words.

One wording of the issue is narrowed here: "code + low bits are exactly those make_frame can set when full_range=True" — make_frame never sets
a `low` bit (it shifts the 10-bit code up by six), so the test holds the bits it can set to `code` exactly and `low`, `high`, `pad` to zero.
"""
import numpy as np
import pytest

from tests.golden.cases import M709, ext
from tests.sample_bits import (CLASSES, CYCLE, IGNORED, LSB10, LSB10_EXTRA, MSB10, SEEDS, container_noise, corner_frame, corner_values, field_map,
                               fields, get_field, legal_range, sparse_edges, with_ignored_bits, with_low_bits)
from tests.sample_layouts import ALL_FORMATS, pitch_of, pixel_mask, relayout
from videorenderer_amd import synth

W, H = 48, 16
SIZES = {10: ((48, 16), (46, 16), (50, 16))}         # v210: whole groups, and two widths whose last group has fields past the width
HAS_IGNORED = set(LSB10) | {10, 11, 12, 13, 30, 31, 32, 35, 36}


def sizes(cformat):
    return SIZES.get(cformat, ((W, H),))


# ---- field_map -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cformat", ALL_FORMATS)
def test_the_classes_partition_the_pixel_bytes(cformat):
    for w, h in ((W, H), (46, 16)):
        for pitch in (synth.default_pitch(cformat, w), pitch_of("wide", cformat, w)):
            fm = field_map(cformat, w, h, pitch)
            assert set(fm) == set(CLASSES)
            union = np.zeros_like(fm["code"])
            bits = 0
            for c in CLASSES:
                union |= fm[c]
                bits += int(np.unpackbits(fm[c]).sum())
            inside = pixel_mask(cformat, w, h, pitch)
            assert (union[inside] == 0xff).all(), "a bit of a pixel byte is in no class"
            assert not union[~inside].any(), "pitch padding is in a class"
            assert bits == 8 * int(inside.sum()), "two classes share a bit"
            assert bool(sum(int(fm[c].any()) for c in IGNORED)) == (cformat in HAS_IGNORED)
            assert fm["low"].any() == (cformat in MSB10)
            assert fm["high"].any() == (cformat in LSB10)


@pytest.mark.parametrize("cformat", ALL_FORMATS)
def test_code_bits_are_the_bits_synth_can_set(cformat):
    """over 24 full-range noise frames every `code` bit is seen both set and clear and no other bit ever changes: `low`, `high`, `pad` are
    zero and `alpha` all ones in every frame (the module docstring on `low`)"""
    w, h = 46, 16
    fm = field_map(cformat, w, h)
    frames = [synth.make_frame(cformat, w, h, "noise", seed=3000 + k, full_range=True)[0] for k in range(24)]
    seen_or, seen_and = np.bitwise_or.reduce(frames), np.bitwise_and.reduce(frames)
    assert np.array_equal(seen_or & ~seen_and, fm["code"])
    assert not (seen_or & (fm["low"] | fm["high"] | fm["pad"])).any()
    assert np.array_equal(seen_and & fm["alpha"], fm["alpha"])
    legal = synth.make_frame(cformat, w, h, "noise", seed=1)[0]
    for f in fields(cformat, w, h):
        if f.cls == "code" and f.comp in CYCLE:
            lo, hi, _ = legal_range(cformat, f.comp)
            v = get_field(legal, f)
            assert lo <= v.min() and v.max() <= hi, (cformat, f.comp, int(v.min()), int(v.max()))


def test_the_two_twins_differ_from_the_frame_and_from_each_other():
    for cformat in ALL_FORMATS:
        frame, _ = synth.make_frame(cformat, W, H, "noise", seed=10)
        a, b = (with_ignored_bits(frame, cformat, W, H, s) for s in SEEDS)
        fm = field_map(cformat, W, H)
        keep = fm["code"] | fm["low"]
        assert np.array_equal(a & keep, frame & keep) and np.array_equal(b & keep, frame & keep)
        assert (cformat in HAS_IGNORED) == (not np.array_equal(a, frame)) == (not np.array_equal(a, b))
        low = with_low_bits(frame, cformat, W, H, SEEDS[0])
        assert (cformat in MSB10) == (not np.array_equal(low, frame))
        assert np.array_equal(low & ~fm["low"], frame)


def test_container_noise_covers_the_container():
    for cformat in ALL_FORMATS:
        buf, pitch = container_noise(cformat, 136, 24, 5)
        inside = pixel_mask(cformat, 136, 24, pitch)
        assert not buf[~inside].any()
        for f in fields(cformat, 136, 24):
            v = get_field(buf, f)
            if f.bits <= 10:
                assert np.bitwise_or.reduce(v.ravel()) == (1 << f.bits) - 1 and np.bitwise_and.reduce(v.ravel()) == 0, (cformat, f.comp, f.cls)
        if cformat in LSB10:
            words = buf[inside].view("<u2")
            assert (words >= 1024).mean() > 0.9


def test_corner_frame_cycles():
    from math import gcd
    assert all(gcd(a, b) == 1 for a, b in ((13, 11), (13, 7), (11, 7)))
    for cformat in ALL_FORMATS:
        buf, pitch = corner_frame(cformat, 136, 24)
        legal = synth.make_frame(cformat, 136, 24, "noise", seed=1)[0]
        fm = field_map(cformat, 136, 24)
        other = fm["low"] | fm["alpha"] | fm["pad"]
        assert np.array_equal(buf & other, legal & other)
        fs = fields(cformat, 136, 24)
        for comp in "YUV":
            code = [f for f in fs if f.comp == comp and f.cls == "code"]
            if not code:
                assert comp != "Y"
                continue
            words = get_field(buf, code[0]).astype(np.uint32)
            high = [f for f in fs if f.comp == comp and f.cls == "high"]
            if high:
                words |= get_field(buf, high[0]) << 10
            vals = corner_values(cformat, comp)
            assert set(np.unique(words).tolist()) == set(vals), (cformat, comp)
            assert np.array_equal(words[0, :CYCLE[comp]], words[0, CYCLE[comp]: 2 * CYCLE[comp]])          # the period along a row
            assert len(vals) >= 4 and (cformat not in LSB10 or set(LSB10_EXTRA) <= set(vals))
            top = (1 << code[0].bits) - 1
            assert {0, 1, top - 1, top} <= set(vals)
    # 8-bit Y'CbCr: the eight values of the issue's list
    assert corner_values(1, "Y") == [0, 1, 15, 16, 235, 236, 254, 255] and corner_values(1, "U")[4:6] == [240, 241]
    assert corner_values(20, "Y") == [0, 1, 63, 64, 940, 941, 1022, 1023, 1024, 1025, 0xFC00, 0xFFFF]


def test_sparse_edges_replaces_every_seventh_sample():
    for cformat in (2, 20, 10, 12, 32):
        frame, _ = synth.make_frame(cformat, 136, 24, "noise", seed=3)
        corner, _ = corner_frame(cformat, 136, 24)
        out = sparse_edges(frame, cformat, 136, 24)
        for f in fields(cformat, 136, 24):
            if f.cls != "code" or f.comp not in CYCLE:
                continue
            got, was, want = get_field(out, f).ravel(), get_field(frame, f).ravel(), get_field(corner, f).ravel()
            pick = np.arange(got.size) % 7 == 6
            assert np.array_equal(got[pick], want[pick]) and np.array_equal(got[~pick], was[~pick])


# ---- the oracle -------------------------------------------------------------------------------------------------------------------------
def params_for(oracle, cformat, w, h, dst):
    return oracle.default_params(cformat=cformat, width=w, height=h, exfmt=ext(matrix=M709), window_w=dst[0], window_h=dst[1],
                                 video_rect=(0, 0, dst[0], dst[1]), iUpscaling=4)


def geometries(w, h):
    return ((w, h), (w * 3 // 2, h * 3 // 2))       # the default convert; a 1.5x Lanczos3 resize


@pytest.mark.parametrize("cformat", ALL_FORMATS)
def test_the_oracle_ignores_high_alpha_and_pad_bits(oracle, cformat):
    for w, h in sizes(cformat):
        frame, pitch = synth.make_frame(cformat, w, h, "noise", seed=940 + cformat)
        twins = [with_ignored_bits(frame, cformat, w, h, s) for s in SEEDS]
        for dst in geometries(w, h):
            p = params_for(oracle, cformat, w, h, dst)
            want = oracle.process(p, frame, pitch)
            for s, twin in zip(SEEDS, twins):
                got = oracle.process(p, twin, pitch)
                assert np.array_equal(got, want), f"cformat {cformat} {w}x{h} -> {dst} seed {s:#x}: the oracle's picture depends on an ignored bit"


@pytest.mark.parametrize("cformat", [10, 20, 32, 33])
def test_the_oracle_ignores_them_at_a_padded_pitch_too(oracle, cformat):
    """(the classes are defined on the pixel bytes: pitch padding stays in none — tests/test_sample_layouts.py has the padding itself)"""
    w, h = 46, 16
    frame, tight = synth.make_frame(cformat, w, h, "noise", seed=980 + cformat)
    pitch = pitch_of("wide", cformat, w)
    wide = relayout(frame, cformat, w, h, pitch, 1)
    p = params_for(oracle, cformat, w, h, (w, h))
    want = oracle.process(p, wide, pitch)
    for s in SEEDS:
        assert np.array_equal(oracle.process(p, with_ignored_bits(wide, cformat, w, h, s, pitch), pitch), want), (cformat, s)


@pytest.mark.parametrize("cformat", MSB10)
def test_the_oracle_reads_the_low_bits(oracle, cformat):
    frame, pitch = synth.make_frame(cformat, W, H, "noise", seed=960 + cformat)
    low = with_low_bits(frame, cformat, W, H, SEEDS[0])
    for dst in geometries(W, H):
        p = params_for(oracle, cformat, W, H, dst)
        assert not np.array_equal(oracle.process(p, low, pitch), oracle.process(p, frame, pitch)), (cformat, dst)


@pytest.mark.parametrize("cformat", LSB10)
def test_the_oracle_wraps_words_above_1023(oracle, cformat):
    """a word of 1024 + k reads as k: container noise equals the same frame with every word masked to ten bits, and differs from the frame
    saturated to 1023 (what a loader without the truncation would be closer to)"""
    buf, pitch = container_noise(cformat, W, H, 7)
    masked = (buf.view("<u2") & 0x3ff).view(np.uint8)
    p = params_for(oracle, cformat, W, H, (W, H))
    want = oracle.process(p, buf, pitch)
    assert np.array_equal(oracle.process(p, masked, pitch), want)
    assert not np.array_equal(oracle.process(p, np.minimum(buf.view("<u2"), 1023).view(np.uint8), pitch), want)
