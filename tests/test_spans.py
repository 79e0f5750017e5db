"""The span algebra that orders writers on the frame lanes (videorenderer_amd/csrc/vp_spans.h), without a GPU.

A frame or a batch in flight is remembered as the bytes [lo, hi) its render targets cover; a new writer is ordered behind every writer in
flight whose bytes it shares.  The lanes keep a batch's spans sorted and merged and answer with a binary search (SpansOverlap) or one walk
through two lists (SpanListsOverlap).  Here both are compared with the definition they stand for: RtSpan::Overlaps against every original
span, one by one.  tests/tools/spans_shim.cpp puts the header behind a C interface.

Empty spans (lo == hi) are left out on purpose: an empty span inside another overlaps it by RtSpan::Overlaps but covers no byte, so the
merged and the unmerged answers differ for it — and the product never builds one (a window with pixels covers at least 4 bytes).
"""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
U64 = C.c_uint64


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("spans") / "libspans_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, os.path.join(HERE, "tools", "spans_shim.cpp")])
    L = C.CDLL(out)
    L.span_overlaps.argtypes = [U64] * 4
    L.spans_sort_and_merge.argtypes = [C.POINTER(U64), C.c_int, C.POINTER(U64)]
    L.spans_overlap.argtypes = [C.POINTER(U64), C.c_int, U64, U64]
    L.spans_overlap_every.argtypes = [C.POINTER(U64), C.c_int, C.c_int, C.c_void_p]
    L.spans_overlap_every.restype = None
    L.span_lists_overlap.argtypes = [C.POINTER(U64), C.c_int, C.POINTER(U64), C.c_int]
    return L


def _pack(spans):
    return (U64 * (2 * len(spans) + 2))(*[w for s in spans for w in s])          # (+2: never a zero-length array)


def merge(L, spans):
    out = (U64 * (2 * len(spans) + 2))()
    m = L.spans_sort_and_merge(_pack(spans), len(spans), out)
    return [(out[2 * i], out[2 * i + 1]) for i in range(m)]


def overlaps(L, a, b):
    return bool(L.span_overlaps(a[0], a[1], b[0], b[1]))


def spans_overlap(L, merged, s):
    return bool(L.spans_overlap(_pack(merged), len(merged), s[0], s[1]))


def lists_overlap(L, a, b):
    return bool(L.span_lists_overlap(_pack(a), len(a), _pack(b), len(b)))


def covered(spans):
    return {x for lo, hi in spans for x in range(lo, hi)}


def random_spans(rng):
    """up to 12 non-empty spans, lo in 0..64, length 1..8"""
    return [(lo, lo + rng.randint(1, 8)) for lo in (rng.randint(0, 64) for _ in range(rng.randint(0, 12)))]


LIMIT = 64 + 8 + 1      # no span of a case ends behind byte 72: the probes reach one byte further
PROBES = np.array([(lo, hi) for lo in range(LIMIT) for hi in range(lo + 1, LIMIT + 1)], dtype=np.int64)     # every non-empty span in range, lo-major


def spans_overlap_every(L, merged):
    out = np.zeros(len(PROBES), dtype=np.uint8)
    L.spans_overlap_every(_pack(merged), len(merged), LIMIT, out.ctypes.data)
    return out.astype(bool)


def some_span_overlaps_every(spans):
    """the definition, RtSpan::Overlaps (lo < o.hi && o.lo < hi) of every original span against every probe"""
    hit = np.zeros(len(PROBES), dtype=bool)
    for lo, hi in spans:
        hit |= (lo < PROBES[:, 1]) & (PROBES[:, 0] < hi)
    return hit


def test_random_lists_against_the_quadratic_definition(shim):
    rng = random.Random(20261018)
    for case in range(2000):
        a, b = random_spans(rng), random_spans(rng)
        ma, mb = merge(shim, a), merge(shim, b)
        # sorted, disjoint, and no two spans touch; every span non-empty
        assert all(lo < hi for lo, hi in ma), (case, a, ma)
        assert all(ma[i][1] < ma[i + 1][0] for i in range(len(ma) - 1)), (case, a, ma)
        # exactly the same bytes
        assert covered(ma) == covered(a), (case, a, ma)
        # one span against the merged list == against every original span: every non-empty span in range ...
        got, want = spans_overlap_every(shim, ma), some_span_overlaps_every(a)
        assert np.array_equal(got, want), (case, a, ma, PROBES[np.flatnonzero(got != want)[:4]].tolist())
        for s in b + a:         # ... and, through the shim's own RtSpan::Overlaps, the spans of the case
            assert spans_overlap(shim, ma, s) == any(overlaps(shim, x, s) for x in a), (case, a, ma, s)
        # two merged lists in one walk == some pair of original spans overlaps
        assert lists_overlap(shim, ma, mb) == any(overlaps(shim, x, y) for x in a for y in b), (case, a, b)
        assert lists_overlap(shim, mb, ma) == lists_overlap(shim, ma, mb), (case, a, b)


def test_overlaps_is_sharing_a_byte(shim):
    """RtSpan::Overlaps itself, for non-empty spans: the two share a byte, and it is the expression the random test restates"""
    small = [(lo, hi) for lo in range(7) for hi in range(lo + 1, 8)]
    for a in small:
        for b in small:
            assert overlaps(shim, a, b) == (not covered([a]).isdisjoint(covered([b]))) == (a[0] < b[1] and b[0] < a[1]), (a, b)


def test_spans_that_touch_are_merged_and_do_not_overlap(shim):
    a, b = (16, 32), (32, 40)           # a.hi == b.lo
    assert not overlaps(shim, a, b) and not overlaps(shim, b, a)
    assert merge(shim, [b, a]) == [(16, 40)]
    assert not spans_overlap(shim, [a], b) and not lists_overlap(shim, [a], [b])


def test_a_window_two_rows_down_in_one_surface_overlaps_the_one_above(shim):
    """pitch 64, windows of 10 pixels x 4 rows: [base, base + 3 * 64 + 40) — the row padding in between counts as written"""
    pitch, w, h = 64, 10, 4
    span = lambda base: (base, base + (h - 1) * pitch + w * 4)
    top, lower, below = span(4096), span(4096 + 2 * pitch), span(4096 + h * pitch)
    assert overlaps(shim, top, lower) and overlaps(shim, lower, top)
    assert spans_overlap(shim, merge(shim, [top]), lower)
    assert lists_overlap(shim, merge(shim, [top]), merge(shim, [lower]))
    assert merge(shim, [lower, top]) == [(top[0], lower[1])]
    # the window that starts under the last row shares nothing with it
    assert not overlaps(shim, top, below) and not spans_overlap(shim, [top], below)


def test_the_empty_list(shim):
    assert merge(shim, []) == []
    assert not spans_overlap(shim, [], (0, 8))
    assert not lists_overlap(shim, [], []) and not lists_overlap(shim, [], [(0, 8)]) and not lists_overlap(shim, [(0, 8)], [])
