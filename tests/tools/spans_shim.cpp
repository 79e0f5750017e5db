// tests/tools/spans_shim.cpp — TEST TOOL (never linked into libmpcvr.so): the span algebra of the frame lanes
// (videorenderer_amd/csrc/vp_spans.h) behind a C interface, built from the product's own header.  tests/test_spans.py compares it with
// the quadratic definition (RtSpan::Overlaps against every span).  A span travels as two uint64 words, lo then hi.
// With -DSPANS_SHIM_MAIN it is a stand-alone program that walks seeded random lists through every function (for a sanitizer build:
// g++ -fsanitize=address,undefined -DSPANS_SHIM_MAIN); it checks the merge-free answers against the merged ones and returns 1 on a mismatch.
#include <cstdint>
#include <vector>

#include "../../videorenderer_amd/csrc/vp_spans.h"

using namespace mpcvr;

static std::vector<RtSpan> unpack(const uint64_t *lohi, int n)
{
    std::vector<RtSpan> v((size_t)n);
    for (int i = 0; i < n; i++) { v[i].lo = (uintptr_t)lohi[2 * i]; v[i].hi = (uintptr_t)lohi[2 * i + 1]; }
    return v;
}

extern "C" int span_overlaps(uint64_t alo, uint64_t ahi, uint64_t blo, uint64_t bhi)
{
    RtSpan a, b;
    a.lo = (uintptr_t)alo; a.hi = (uintptr_t)ahi; b.lo = (uintptr_t)blo; b.hi = (uintptr_t)bhi;
    return a.Overlaps(b) ? 1 : 0;
}

// out: room for n spans; returns how many the merged list has
extern "C" int spans_sort_and_merge(const uint64_t *lohi, int n, uint64_t *out)
{
    std::vector<RtSpan> v = unpack(lohi, n);
    SortAndMergeSpans(v);
    for (size_t i = 0; i < v.size(); i++) { out[2 * i] = v[i].lo; out[2 * i + 1] = v[i].hi; }
    return (int)v.size();
}

extern "C" int spans_overlap(const uint64_t *sorted, int n, uint64_t lo, uint64_t hi)
{
    RtSpan s;
    s.lo = (uintptr_t)lo; s.hi = (uintptr_t)hi;
    return SpansOverlap(unpack(sorted, n), s) ? 1 : 0;
}

// every non-empty span [lo, hi) with 0 <= lo < hi <= limit against the list, lo-major: out[k] = SpansOverlap(sorted, span k)
extern "C" void spans_overlap_every(const uint64_t *sorted, int n, int limit, uint8_t *out)
{
    const std::vector<RtSpan> v = unpack(sorted, n);
    for (int lo = 0; lo < limit; lo++)
        for (int hi = lo + 1; hi <= limit; hi++) { RtSpan s; s.lo = (uintptr_t)lo; s.hi = (uintptr_t)hi; *out++ = SpansOverlap(v, s) ? 1 : 0; }
}

extern "C" int span_lists_overlap(const uint64_t *a, int na, const uint64_t *b, int nb)
{
    return SpanListsOverlap(unpack(a, na), unpack(b, nb)) ? 1 : 0;
}

#ifdef SPANS_SHIM_MAIN
#include <cstdio>
int main()
{
    uint32_t s = 12345u;
    auto rnd = [&s](uint32_t m) { s = s * 1664525u + 1013904223u; return (s >> 8) % m; };
    auto draw = [&rnd](std::vector<uint64_t> &v) {
        v.clear();
        for (uint32_t i = 0, n = rnd(13); i < n; i++) { const uint64_t lo = rnd(65); v.push_back(lo); v.push_back(lo + 1 + rnd(8)); }
    };
    std::vector<uint64_t> a, b, ma, mb;
    for (int it = 0; it < 2000; it++) {
        draw(a); draw(b);
        ma.assign(a.size() + 2, 0); mb.assign(b.size() + 2, 0);
        const int na = spans_sort_and_merge(a.data(), (int)a.size() / 2, ma.data()), nb = spans_sort_and_merge(b.data(), (int)b.size() / 2, mb.data());
        bool any = false;
        for (size_t i = 0; i + 1 < b.size(); i += 2) {
            bool hit = false;
            for (size_t j = 0; j + 1 < a.size(); j += 2) hit = hit || span_overlaps(a[j], a[j + 1], b[i], b[i + 1]);
            if (hit != (spans_overlap(ma.data(), na, b[i], b[i + 1]) != 0)) { std::printf("case %d: SpansOverlap differs\n", it); return 1; }
            any = any || hit;
        }
        if (any != (span_lists_overlap(ma.data(), na, mb.data(), nb) != 0)) { std::printf("case %d: SpanListsOverlap differs\n", it); return 1; }
    }
    std::printf("ok\n");
    return 0;
}
#endif
