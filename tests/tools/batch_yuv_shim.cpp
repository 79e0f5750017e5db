// tests/tools/batch_yuv_shim.cpp — TEST TOOL (never linked into libmpcvr.so): the plane-overlap scan of mpcvr_process_batch_yuv behind a C
// interface, built from the product's own header (videorenderer_amd/csrc/vp_spans.h: BatchPlaneSpans, AnyTwoSpansOverlap).
// tests/test_batch_yuv.py compares it with the quadratic definition.  Planes travel as addresses (uint64).
// With -DBATCH_YUV_SHIM_MAIN it is a stand-alone program that walks seeded random batches through the scan and compares it with every pair
// (for a sanitizer build: g++ -fsanitize=address,undefined -DBATCH_YUV_SHIM_MAIN); it returns 1 on a mismatch.
#include <cstdint>
#include <vector>

#include "../../videorenderer_amd/csrc/vp_spans.h"

using namespace mpcvr;

static std::vector<RtSpan> spans_of(const uint64_t *y, const uint64_t *uv, int n, int h, int y_pitch, int uv_pitch, int row_bytes)
{
    std::vector<void *> yp((size_t)n), cp((size_t)n);
    for (int i = 0; i < n; i++) { yp[i] = (void *)(uintptr_t)y[i]; cp[i] = (void *)(uintptr_t)uv[i]; }
    return BatchPlaneSpans(n, yp.data(), y_pitch, cp.data(), uv_pitch, h, (size_t)row_bytes);
}

// out (optional): room for 4 n words, the spans as lo, hi: Y of frame 0, UV of frame 0, Y of frame 1, ...
extern "C" int batch_planes_overlap(const uint64_t *y, const uint64_t *uv, int n, int h, int y_pitch, int uv_pitch, int row_bytes, uint64_t *out)
{
    const std::vector<RtSpan> v = spans_of(y, uv, n, h, y_pitch, uv_pitch, row_bytes);
    if (out)
        for (size_t i = 0; i < v.size(); i++) { out[2 * i] = v[i].lo; out[2 * i + 1] = v[i].hi; }
    return AnyTwoSpansOverlap(v) ? 1 : 0;
}

#ifdef BATCH_YUV_SHIM_MAIN
#include <cstdio>
int main()
{
    uint32_t s = 2026u;
    auto rnd = [&s](uint32_t m) { s = s * 1664525u + 1013904223u; return (s >> 8) % m; };
    for (int it = 0; it < 4000; it++) {
        const int n = 1 + (int)rnd(6), h = 2 * (1 + (int)rnd(3)), row = 4 * (1 + (int)rnd(4)), yp = row + 4 * (int)rnd(3), cp = row + 4 * (int)rnd(3);
        std::vector<uint64_t> y((size_t)n), uv((size_t)n), out((size_t)4 * n);
        for (int i = 0; i < n; i++) { y[i] = 4096 + 4 * rnd(160); uv[i] = 4096 + 4 * rnd(160); }
        const int got = batch_planes_overlap(y.data(), uv.data(), n, h, yp, cp, row, out.data());
        int want = 0;
        for (int a = 0; a < 2 * n; a++)
            for (int b = a + 1; b < 2 * n; b++)
                if (out[2 * a] < out[2 * b + 1] && out[2 * b] < out[2 * a + 1]) want = 1;
        if (got != want) { std::printf("case %d: scan %d, pairs %d\n", it, got, want); return 1; }
    }
    std::printf("ok\n");
    return 0;
}
#endif
