"""mpcvr_process_batch_yuv without a GPU (extension: a batch written as NV12 / P010, include/mpcvr.h): the layout integers of
mpcvr_plan_batch_yuv against values worked by hand, and the scan that refuses a batch whose planes overlap (vp_spans.h: BatchPlaneSpans,
AnyTwoSpansOverlap, through tests/tools/batch_yuv_shim.cpp) against its definition — some pair of the 2n planes shares a byte, a plane
being the bytes from its first pixel to the last pixel of its last row.  What the call writes: tests/test_batch_yuv_gpu.py."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U64 = C.c_uint64


def plan(mpcvr, w, h, n, budget):
    from videorenderer_amd import api
    d = api.plan_batch_yuv(w, h, n, budget)
    return d["surface_pitch"], d["frame_stride"], d["frames_per_chunk"], d["chunks"]


def test_layout_integers_worked_by_hand(mpcvr):
    # 258 = 2 (mod 4): 4 * 258 = 1032 = 64 * 16 + 8 -> 1040; 1040 * 38 = 39520 = 154 * 256 + 96 -> 155 * 256 = 39680
    assert plan(mpcvr, 258, 38, 1, 1 << 30)[:2] == (1040, 39680)
    # 256 wide: the pitch is the row, 1024 * 36 = 36864 = 144 * 256 — nothing to round
    assert plan(mpcvr, 256, 36, 1, 1 << 30)[:2] == (1024, 36864)
    # 62 = 2 (mod 4): 248 -> 256; 256 * 34 = 8704 = 34 * 256
    assert plan(mpcvr, 62, 34, 1, 1 << 30)[:2] == (256, 8704)
    # the smallest frame: one row piece of 16 bytes, two rows, a whole 256-byte stride
    assert plan(mpcvr, 2, 2, 1, 1 << 30)[:2] == (16, 256)
    # 8K: 30720 * 4320 = 132710400 = 518400 * 256
    assert plan(mpcvr, 7680, 4320, 1, 1 << 30)[:2] == (30720, 132710400)
    # the largest window
    assert plan(mpcvr, 32768, 32768, 1, 1)[:2] == (131072, 131072 * 32768)


def test_chunks_under_a_budget(mpcvr):
    stride = 39680                                      # 258 x 38, above
    # a budget below one frame: one frame per chunk, n chunks
    assert plan(mpcvr, 258, 38, 5, 1000)[2:] == (1, 5)
    assert plan(mpcvr, 258, 38, 5, 1)[2:] == (1, 5)
    assert plan(mpcvr, 258, 38, 5, 2 * stride - 1)[2:] == (1, 5)
    # two frames fit: n = 5 is no multiple of the chunk — 2, 2 and 1
    assert plan(mpcvr, 258, 38, 5, 2 * stride)[2:] == (2, 3)
    assert plan(mpcvr, 258, 38, 5, 3 * stride - 1)[2:] == (2, 3)
    assert plan(mpcvr, 258, 38, 5, 3 * stride)[2:] == (3, 2)
    assert plan(mpcvr, 258, 38, 5, 4 * stride)[2:] == (4, 2)
    # at or above n frames: one chunk of n, never more frames than the batch has
    assert plan(mpcvr, 258, 38, 5, 5 * stride)[2:] == (5, 1)
    assert plan(mpcvr, 258, 38, 5, 1 << 40)[2:] == (5, 1)
    assert plan(mpcvr, 258, 38, 1, 1)[2:] == (1, 1)
    # 32 frames of 8K under 1 GiB: 2^30 / 132710400 = 8.09 -> 8 per chunk, 4 chunks; under 4 GiB 32.4 -> one chunk; 256 MiB: 2.02 -> 16 chunks
    assert plan(mpcvr, 7680, 4320, 32, 1 << 30)[2:] == (8, 4)
    assert plan(mpcvr, 7680, 4320, 32, 4 << 30)[2:] == (32, 1)
    assert plan(mpcvr, 7680, 4320, 32, 256 << 20)[2:] == (2, 16)
    assert plan(mpcvr, 7680, 4320, 33, 4 << 30)[2:] == (32, 2)


def test_budget_zero_is_the_headers_default(mpcvr):
    text = open(os.path.join(ROOT, "include", "mpcvr.h")).read()
    m = re.search(r"#define\s+MPCVR_BATCH_YUV_DEFAULT_BUDGET\s+\(\(size_t\)(\d+)\s*<<\s*(\d+)\)", text)
    assert m, "include/mpcvr.h does not name the default budget"
    default = int(m.group(1)) << int(m.group(2))
    assert (256 << 20) <= default <= (4 << 30)
    for w, h, n in ((7680, 4320, 32), (2560, 1440, 32), (258, 38, 5)):
        assert plan(mpcvr, w, h, n, 0) == plan(mpcvr, w, h, n, default)
    stride = plan(mpcvr, 7680, 4320, 1, 0)[1]
    assert plan(mpcvr, 7680, 4320, 1000, 0)[2] == default // stride


def test_refusals_and_null_out_pointers(mpcvr):
    from videorenderer_amd import api
    L = api.load_library()

    def hr(w, h, n):
        return L.mpcvr_plan_batch_yuv(w, h, n, 1 << 20, None, None, None, None)

    assert hr(258, 38, 5) == 0                          # (every out pointer may be NULL)
    for w, h, n in ((257, 38, 5), (258, 37, 5), (0, 38, 5), (258, 0, 5), (-2, 38, 5), (32770, 38, 5), (258, 32770, 5), (258, 38, 0), (258, 38, -1)):
        assert hr(w, h, n) == api.E_INVALIDARG, (w, h, n)
        with pytest.raises(api.MpcvrError):
            api.plan_batch_yuv(w, h, n, 1 << 20)
    assert hr(32768, 32768, 1) == 0 and hr(2, 2, 1) == 0


# ---- the plane-overlap scan ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_yuv")
    out = str(d / "libbatch_yuv_shim.so")
    src = os.path.join(HERE, "tools", "batch_yuv_shim.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, src])
    L = C.CDLL(out)
    L.batch_planes_overlap.argtypes = [C.POINTER(U64), C.POINTER(U64), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(U64)]
    L.program = (str(d / "batch_yuv_shim"), src)
    return L


def scan(L, ys, uvs, h, y_pitch, uv_pitch, row):
    """(the scan's answer, the 2n spans it was given)"""
    n = len(ys)
    out = (U64 * (4 * n))()
    got = L.batch_planes_overlap((U64 * n)(*ys), (U64 * n)(*uvs), n, h, y_pitch, uv_pitch, row, out)
    return bool(got), [(out[2 * i], out[2 * i + 1]) for i in range(2 * n)]


def some_pair_shares_a_byte(spans):
    return any(a[0] < b[1] and b[0] < a[1] for i, a in enumerate(spans) for b in spans[i + 1:])


W, H = 24, 6                        # NV12 rows of 24 bytes
Y_BYTES, UV_BYTES = W * H, W * H // 2
BASE = 1 << 20


def test_spans_are_first_pixel_to_last_pixel_of_the_last_row(shim):
    got, spans = scan(shim, [BASE], [BASE + 4096], H, 32, 40, W)
    assert spans == [(BASE, BASE + 5 * 32 + W), (BASE + 4096, BASE + 4096 + 2 * 40 + W)] and not got


def test_planes_that_touch_do_not_overlap(shim):
    # tight planes back to back: Y0 | UV0 | Y1 | UV1, every plane starting on the byte the one before ended on
    frame = Y_BYTES + UV_BYTES
    ys = [BASE, BASE + frame]
    uvs = [BASE + Y_BYTES, BASE + frame + Y_BYTES]
    got, spans = scan(shim, ys, uvs, H, W, W, W)
    assert not got and not some_pair_shares_a_byte(spans)
    assert spans[0][1] == spans[1][0] and spans[1][1] == spans[2][0]
    # one dword earlier and UV0 starts in Y0's last row
    got, _ = scan(shim, ys, [uvs[0] - 4, uvs[1]], H, W, W, W)
    assert got
    # padded rows: the last row's padding is not part of the plane, so the next plane may start right behind the last pixel
    pitch = W + 8
    y_end = BASE + (H - 1) * pitch + W
    assert not scan(shim, [BASE], [y_end], H, pitch, pitch, W)[0]
    assert scan(shim, [BASE], [y_end - 4], H, pitch, pitch, W)[0]


def test_interleaved_rows_count_as_overlapping(shim):
    # two Y planes side by side in one surface of double pitch: each plane's padding is the other's pixels
    uv_far = [BASE + (1 << 16), BASE + (2 << 16)]
    got, spans = scan(shim, [BASE, BASE + W], uv_far, H, 2 * W, W, W)
    assert got and some_pair_shares_a_byte(spans)
    # the same for two UV planes
    assert scan(shim, [BASE + (1 << 16), BASE + (2 << 16)], [BASE, BASE + W], H, W, 2 * W, W)[0]


def test_luma_of_one_frame_over_chroma_of_another(shim):
    ys = [BASE, BASE + 3 * 4096]
    uvs = [BASE + 4096, BASE + 2 * 4096]
    assert not scan(shim, ys, uvs, H, W, W, W)[0]
    # Y of frame 1 starts inside UV of frame 0, each frame's own pair apart
    ys[1] = uvs[0] + W
    got, spans = scan(shim, ys, uvs, H, W, W, W)
    assert got and some_pair_shares_a_byte(spans)
    assert not scan(shim, ys[1:], uvs[1:], H, W, W, W)[0] and not scan(shim, ys[:1], uvs[:1], H, W, W, W)[0]


def test_identical_pointers(shim):
    far = [BASE + (1 << 16), BASE + (2 << 16)]
    assert scan(shim, [BASE, BASE], far, H, W, W, W)[0]                 # one Y plane given twice
    assert scan(shim, far, [BASE, BASE], H, W, W, W)[0]                 # one UV plane given twice
    assert scan(shim, [BASE], [BASE], H, W, W, W)[0]                    # a frame whose Y and UV are one pointer
    assert not scan(shim, [BASE], [BASE + (1 << 16)], H, W, W, W)[0]


def test_random_batches_against_every_pair(shim):
    rng = random.Random(20261019)
    hits = 0
    for case in range(3000):
        n = rng.randint(1, 6)
        h = 2 * rng.randint(1, 3)
        row = 4 * rng.randint(1, 4)
        yp, cp = row + 4 * rng.randint(0, 2), row + 4 * rng.randint(0, 2)
        span = rng.choice((40, 160, 1200))             # crowded, mixed and sparse address ranges
        ys = [BASE + 4 * rng.randint(0, span) for _ in range(n)]
        uvs = [BASE + 4 * rng.randint(0, span) for _ in range(n)]
        got, spans = scan(shim, ys, uvs, h, yp, cp, row)
        assert got == some_pair_shares_a_byte(spans), (case, ys, uvs, h, yp, cp, row)
        hits += got
    assert 300 < hits < 2700, hits                      # (both answers occur often)


def test_the_shims_own_walk_as_a_program(shim):
    """the stand-alone form (what a sanitizer build runs): seeded random batches, scan against pairs"""
    exe, src = shim.program
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DBATCH_YUV_SHIM_MAIN", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
