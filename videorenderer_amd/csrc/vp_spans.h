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
