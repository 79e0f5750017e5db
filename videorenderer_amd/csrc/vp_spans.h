// vp_spans.h — what is in flight, as memory: two writers are ordered when the bytes their render targets cover overlap, whatever pointers
// they were given (a window a few rows further down in one surface, the same surface from another base); targets that merely touch run
// side by side.  Host arithmetic only (no HIP): the frame lanes (vp_lanes.h) use it, tests/test_spans.py checks it against its definition.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace mpcvr {

// what a frame in flight writes: the bytes [lo, hi) from the first pixel of its render target to the last pixel of its last row (the padding
// of the rows in between counts as written: rows of two targets that interleave in one surface are ordered like rows that overlap)
struct RtSpan { uintptr_t lo = 0, hi = 0; bool Overlaps(const RtSpan &o) const { return lo < o.hi && o.lo < hi; } };
// ... of a surface or a plane of `rows` rows of rowBytes at `pitch`: the one definition of what a target, a source or a plane covers
inline RtSpan RowsSpan(const void *p, size_t pitch, int rows, size_t rowBytes) { return RtSpan{(uintptr_t)p, (uintptr_t)p + (size_t)std::max(rows - 1, 0) * pitch + rowBytes}; }

// sorted by address, spans that overlap or touch merged into one: the result is disjoint, so both ends ascend
inline void SortAndMergeSpans(std::vector<RtSpan> &v)
{
    std::sort(v.begin(), v.end(), [](const RtSpan &a, const RtSpan &b) { return a.lo < b.lo; });
    size_t m = 0;
    for (size_t i = 0; i < v.size(); i++) {
        if (m && v[i].lo <= v[m - 1].hi) v[m - 1].hi = std::max(v[m - 1].hi, v[i].hi);
        else v[m++] = v[i];
    }
    v.resize(m);
}

// do any two of the (non-empty) spans share a byte?  Sorted by address, a span overlaps an earlier one exactly when it starts in front of the
// furthest end seen so far; spans that touch do not overlap, two spans from one address do.  (mpcvr_process_batch_yuv: the 2n planes of a batch)
inline bool AnyTwoSpansOverlap(std::vector<RtSpan> v)
{
    std::sort(v.begin(), v.end(), [](const RtSpan &a, const RtSpan &b) { return a.lo < b.lo; });
    uintptr_t end = 0;
    for (size_t i = 0; i < v.size(); i++) {
        if (i && v[i].lo < end) return true;
        end = std::max(end, v[i].hi);
    }
    return false;
}

// the 2n planes of a batch of 4:2:0 frames as spans, frame i at [2i] (Y: h rows) and [2i + 1] (UV: h / 2 rows), rows of rowBytes
inline std::vector<RtSpan> BatchPlaneSpans(int n, void *const *y, int yPitch, void *const *uv, int uvPitch, int h, size_t rowBytes)
{
    std::vector<RtSpan> v((size_t)2 * (size_t)n);
    for (int i = 0; i < n; i++) {
        v[2 * i] = RowsSpan(y[i], (size_t)yPitch, h, rowBytes);
        v[2 * i + 1] = RowsSpan(uv[i], (size_t)uvPitch, h / 2, rowBytes);
    }
    return v;
}

// does `s` share a byte with one of `sorted` (SortAndMergeSpans' result)?
inline bool SpansOverlap(const std::vector<RtSpan> &sorted, const RtSpan &s)
{
    // the first span that ends behind s.lo is the only candidate: the ones in front end too early, the ones behind start later still
    const auto it = std::upper_bound(sorted.begin(), sorted.end(), s.lo, [](uintptr_t lo, const RtSpan &x) { return lo < x.hi; });
    return it != sorted.end() && it->lo < s.hi;
}

// do two such lists share a byte?  One walk through both: the span that ends first cannot meet anything further down the other list
inline bool SpanListsOverlap(const std::vector<RtSpan> &a, const std::vector<RtSpan> &b)
{
    for (size_t i = 0, j = 0; i < a.size() && j < b.size();) {
        if (a[i].Overlaps(b[j])) return true;
        if (a[i].hi <= b[j].lo) i++; else j++;
    }
    return false;
}

}  // namespace mpcvr
