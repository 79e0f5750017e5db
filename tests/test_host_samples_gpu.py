"""Samples that arrive in HOST memory: mpcvr_copy_sample(MPCVR_MEM_HOST / MPCVR_MEM_HOST_PINNED) -> mpcvr_process, the reference's
ProcessSample -> CopySample (MemCopyToTexSrcVideo) -> Render.  CHipVideoProcessor::CopySample cycles three upload slots (pinned staging
buffer, device buffer, an `uploaded` and a `consumed` event each) on a non-blocking copy stream that runs ahead of the context stream and
of the four frame lanes; what keeps a slot from being refilled under a frame that still reads it are host and stream waits that decide
nothing while the GPU is idle when the next sample arrives.  Here the GPU is BEHIND the host while the samples arrive.

Reference of every comparison: frame k of a case, handed to a FRESH context as a device tensor (zero-copy), MPCVR_FLAG_NO_FRAME_LANES set,
drawn alone and followed by Synchronize — the tier tests/test_parity_gpu.py holds to the oracle; frame 0 of every case is held to the oracle
here as well, under the bars of test_default_path_vs_oracle.  A host-path frame equals its zero-copy frame bit for bit, and the context
reports the same kernel (GetVPInfo).  Frame k of a case is case_frame(seed + 5 k); frames k / k + 1 and k / k + 3 (the two that share an
upload slot) are asserted to differ, so a slot handed out too early shows.

Termination: the only thing anything here waits for is the stall of `gpu_behind` — a fixed number of torch.mm calls, finite work.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

from tests.golden.cases import GOLDEN_CASES, HDR10, case_frame, oracle_params, run_case
from tests.test_parity_gpu import BG, compare, compare_rgb10, has_tail, internal_is_8bit, make_vp, run_product

pytestmark = pytest.mark.gpu

N_FRAMES = 7            # two turns of the three-slot ring plus one
RING = 3                # CHipVideoProcessor::kUploadSlots: the fourth host sample takes the first one's slot

# ---- the GPU behind the host ------------------------------------------------------------------------------------------------------------
# The stall is STALL_MMS products of two 8192 x 8192 fp32 matrices, queued on the stream the context is ordered behind.  Sized on an MI355X
# in one run: the host time of three CopySample(host) + Process pairs of a fresh context with no stall queued, at the frame sizes used here,
# per route and mode; the stall's own duration between two events; the factor between the two (>= 20 asked: host jitter of a shared machine).
#   three pairs, no stall:  13.9 ms  the slowest: 128 x 72 P010 -> 256 x 144 on the lanes as the FIRST context of the process (its first pair alone
#                                    13.1 ms: pinned allocations, copy stream, lanes and the kernel's code object all load there); v210 8.2 ms;
#                                    other fresh contexts on the lanes 2.4 - 3.6 ms, off the lanes or on a caller's stream 0.23 - 0.41 ms
#   the stall, by events:   313 - 315 ms (three repeats; 44 launches queued in 0.8 - 1.0 ms of host time)
#   factor:                 22.6 over the slowest three pairs
# With the stall queued the three pairs returned in 0.3 - 1.6 ms with its event pending, and the fourth CopySample took 312 ms: it waits.
STALL_DIM = 8192
STALL_MMS = 44


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def stall_mats(torch_cuda):
    """The stall's operands, allocated and multiplied once (the first torch.mm of a process loads its kernel: not inside a window)."""
    torch = torch_cuda
    g = torch.Generator(device="cuda").manual_seed(1)
    a = torch.rand((STALL_DIM, STALL_DIM), device="cuda", generator=g)
    b = torch.rand((STALL_DIM, STALL_DIM), device="cuda", generator=g)
    out = torch.empty_like(a)
    torch.mm(a, b, out=out)
    torch.cuda.synchronize()
    return a, b, out


def gpu_behind(torch, mats, n=STALL_MMS):
    """Queues the stall on torch's CURRENT stream and returns the event recorded behind it.
      * a context on its own stream: the current stream is torch's default (the legacy null) stream.  The context stream and the frame
        lanes are blocking streams and do not start behind it; the library's copy stream is non-blocking and runs on — the hazard.
      * a context on a caller's stream: the test runs inside `with torch.cuda.stream(s)`, the context was created there and the stall goes
        onto s itself.
    Everything the window must not contain has to be done before: allocations through torch, the context's plan (UpdatePlan synchronizes)."""
    a, b, out = mats
    if torch.cuda.current_stream().cuda_stream != 0:       # (a side stream starts behind the operands' producer)
        torch.cuda.current_stream().wait_stream(torch.cuda.default_stream())
    for _ in range(n):
        torch.mm(a, b, out=out)
    ev = torch.cuda.Event()
    ev.record()
    return ev


def still_behind(ev, what):
    """Condition, not measurement: the host has returned from its calls and the stall has not completed.  One attempt; a missed window is a failure."""
    assert not ev.query(), f"{what}: the stall had completed when the host calls returned — the window was missed, nothing was tested"


# ---- expectations -----------------------------------------------------------------------------------------------------------------------
def frame_case(c, k):
    """Frame k of a case: its seed moved on by 5 k.  Only the "noise" pictures of videorenderer_amd.synth depend on the seed ("structure" and
    "hdr" are fixed patterns), so frames 1 .. of such a case are noise pictures: frame 0 stays the case's own frame, the one the oracle test draws."""
    if k == 0 or c["kind"] == "noise":
        return dict(c, seed=c["seed"] + 5 * k)
    return dict(c, seed=c["seed"] + 5 * k, kind="noise")


_EXPECT = {}
_ORACLE_DONE = set()


def case_key(c):
    return repr(sorted((k, repr(v)) for k, v in c.items()))


def expected(mpcvr, torch, oracle, c, n, name):
    """[(pixels, GetVPInfo)] of frames 0 .. n-1 of `c`: zero-copy, fresh context each, no lanes, alone.  Computed once and shared (read-only)."""
    from videorenderer_amd import api
    key = case_key(c)
    have = _EXPECT.setdefault(key, [])
    while len(have) < n:
        out, info = run_product(mpcvr, torch, frame_case(c, len(have)), extra_flags=api.FLAG_NO_FRAME_LANES)
        out.setflags(write=False)
        have.append((out, info))
    for k in range(n):
        for step in (1, RING):
            if k + step < n:
                assert not np.array_equal(have[k][0], have[k + step][0]), f"{name}: expected frames {k} and {k + step} are the same picture"
    if oracle is not None and key not in _ORACLE_DONE:
        # frame 0 against the oracle, the bars of test_default_path_vs_oracle: the file does not rest on the library alone
        if name in GOLDEN_CASES and GOLDEN_CASES[name] == c:
            want = run_case(oracle, name, background=BG)
        else:
            frame, pitch = case_frame(c)
            p = oracle_params(oracle, c)
            want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
        if c.get("output_format", 0) == 1:
            compare_rgb10(have[0][0], want, f"{name} zero-copy", tail=has_tail(c), internal8=internal_is_8bit(c))
        else:
            compare(have[0][0], want, f"{name} zero-copy [{have[0][1]}]", min_same=0.99)
        _ORACLE_DONE.add(key)
    return have[:n]


def check(outs, want, info, name):
    for k, (got, (pix, winfo)) in enumerate(zip(outs, want)):
        diff = int((got != pix).sum())
        assert diff == 0, f"{name}: frame {k} differs from its zero-copy frame in {diff} bytes" + "".join(
            f" (it IS frame {j})" for j in range(len(want)) if j != k and np.array_equal(got, want[j][0]))
        assert info == winfo, f"{name}: host samples run [{info}], zero-copy runs [{winfo}]"


MODES = ("own_stream_lanes", "own_stream_no_lanes", "callers_stream")


@contextlib.contextmanager
def context_of(mpcvr, torch, c, mode):
    """A context for `c` in one of MODES, its plan settled; inside the block torch's current stream is the one a stall has to go on."""
    from videorenderer_amd import api
    s = torch.cuda.Stream() if mode == "callers_stream" else None
    with (torch.cuda.stream(s) if s is not None else contextlib.nullcontext()):
        vp, (ww, wh) = make_vp(mpcvr, c, api.FLAG_NO_FRAME_LANES if mode == "own_stream_no_lanes" else 0)
        try:
            vp.GetVPInfo()                  # UpdatePlan synchronizes the context stream: not inside the window
            yield vp, ww, wh
        finally:
            torch.cuda.synchronize()
            vp.close()


def targets(torch, n, ww, wh):
    t = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    return t


def stream_one_buffer(mpcvr, torch, mats, c, mode, name, n=N_FRAMES):
    """n frames through ONE numpy buffer, refilled with frame k + 1 as soon as CopySample(k) + Process(k) have returned ("the caller's buffer is
    free again when the call returns", include/mpcvr.h); the GPU behind the host for the first turn of the ring; one Synchronize at the end."""
    frames = [case_frame(frame_case(c, k)) for k in range(n)]
    pitch = frames[0][1]
    with context_of(mpcvr, torch, c, mode) as (vp, ww, wh):
        dsts = targets(torch, n, ww, wh)
        buf = frames[0][0].copy()
        ev = gpu_behind(torch, mats)
        for k in range(n):
            vp.CopySample(buf, pitch)
            vp.Process(dsts[k], ww * 4)
            if k + 1 < n:
                buf[:] = frames[k + 1][0]
            if k == RING - 1:
                still_behind(ev, f"{name} <{mode}>")        # (the next CopySample waits for frame 0, that is for the stall)
        vp.Synchronize()
        info = vp.GetVPInfo()
        return [d.cpu().numpy() for d in dsts], info


# ---- 1: seven distinct host frames through one context, the GPU behind --------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["c3hdr_p010_pq_lanczos3_2x",       # the exact-2x fused kernel
                                  "c1_nv12_bt709_passthrough",       # the same-size block convert
                                  "up_1p5x_lanczos3",                # the strip / periodic kernel
                                  "down_hamming_3x"])                # pass per kernel: off the lanes
def test_seven_host_frames_one_buffer_gpu_behind(mpcvr, oracle, torch_cuda, stall_mats, name, mode):
    c = GOLDEN_CASES[name]
    want = expected(mpcvr, torch_cuda, oracle, c, N_FRAMES, name)
    outs, info = stream_one_buffer(mpcvr, torch_cuda, stall_mats, c, mode, name)
    check(outs, want, info, f"{name} <{mode}>")


# ---- 2: the same through mpcvr_process_frames ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["own_stream_lanes", "own_stream_no_lanes"])
@pytest.mark.parametrize("name", ["c3hdr_p010_pq_lanczos3_2x", "c1_nv12_bt709_passthrough"])
def test_process_frames_from_host_pointers_gpu_behind(mpcvr, oracle, torch_cuda, stall_mats, name, mode):
    """mpcvr_process_frames(MPCVR_MEM_HOST) over ONE array of seven host pointers.  The entry point is the per-frame loop behind one call, and
    the fourth frame's CopySample waits for the stall: the array goes in as its first three frames, the window is checked, then its last four."""
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    c = GOLDEN_CASES[name]
    want = expected(mpcvr, torch, oracle, c, N_FRAMES, name)
    frames = [case_frame(frame_case(c, k)) for k in range(N_FRAMES)]
    pitch = frames[0][1]
    with context_of(mpcvr, torch, c, mode) as (vp, ww, wh):
        dsts = targets(torch, N_FRAMES, ww, wh)
        arr = C.c_void_p * N_FRAMES
        srcs, tgts = arr(*[f.ctypes.data for f, _ in frames]), arr(*[d.data_ptr() for d in dsts])
        rest = lambda a: (C.c_void_p * (N_FRAMES - RING)).from_buffer(a, RING * C.sizeof(C.c_void_p))       # (the same array, from its fourth entry)
        ev = gpu_behind(torch, stall_mats)
        assert L.mpcvr_process_frames(vp._ctx, RING, srcs, pitch, api.MEM_HOST, tgts, ww * 4) == 0
        still_behind(ev, f"{name} <{mode}>")
        assert L.mpcvr_process_frames(vp._ctx, N_FRAMES - RING, rest(srcs), pitch, api.MEM_HOST, rest(tgts), ww * 4) == 0
        vp.Synchronize()
        check([d.cpu().numpy() for d in dsts], want, vp.GetVPInfo(), f"{name} <{mode}> process_frames")


# ---- 3: the MPCVR_MEM_HOST_PINNED contract ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3hdr_p010_pq_lanczos3_2x", "v210_2x"])
def test_host_pinned_buffers_are_free_after_the_third_following_copy_sample(mpcvr, oracle, torch_cuda, stall_mats, name):
    """include/mpcvr.h: a page-locked buffer handed over as MPCVR_MEM_HOST_PINNED is DMA'd from directly and "must stay untouched until
    mpcvr_synchronize or the third following copy_sample".  Four page-locked buffers in rotation, nine frames: frame k comes from buffer k % 4,
    and as soon as CopySample(k + 3) has returned — the earliest moment allowed — the buffer of frame k is overwritten with 0xA5.  Then, in a
    fresh context: four frames handed over, Synchronize, EVERY buffer overwritten at once."""
    from videorenderer_amd import api
    torch = torch_cuda
    n, nbuf = 9, 4
    c = GOLDEN_CASES[name]
    want = expected(mpcvr, torch, oracle, c, n, name)
    frames = [case_frame(frame_case(c, k)) for k in range(n)]
    pitch = frames[0][1]
    pins = [torch.empty(frames[0][0].size, dtype=torch.uint8).pin_memory() for _ in range(nbuf)]
    views = [p.numpy() for p in pins]
    with context_of(mpcvr, torch, c, "own_stream_lanes") as (vp, ww, wh):
        dsts = targets(torch, n, ww, wh)
        ev = gpu_behind(torch, stall_mats)
        for k in range(n):
            views[k % nbuf][:] = frames[k][0]              # (its last frame, k - 4, was released by CopySample(k - 1))
            vp.CopySample(pins[k % nbuf], pitch, mem_kind=api.MEM_HOST_PINNED)
            if k >= RING:
                views[(k - RING) % nbuf][:] = 0xA5         # the third copy_sample following frame k - 3 has returned
            vp.Process(dsts[k], ww * 4)
            if k == RING - 1:
                still_behind(ev, name)
        vp.Synchronize()
        check([d.cpu().numpy() for d in dsts], want, vp.GetVPInfo(), f"{name} MEM_HOST_PINNED")
    with context_of(mpcvr, torch, c, "own_stream_lanes") as (vp, ww, wh):
        dsts = targets(torch, nbuf, ww, wh)
        for k in range(nbuf):
            views[k][:] = frames[k][0]
        ev = gpu_behind(torch, stall_mats)
        for k in range(nbuf):
            vp.CopySample(pins[k], pitch, mem_kind=api.MEM_HOST_PINNED)
            vp.Process(dsts[k], ww * 4)
            if k == RING - 1:
                still_behind(ev, name + " (synchronize)")
        vp.Synchronize()
        for v in views:
            v[:] = 0xA5
        check([d.cpu().numpy() for d in dsts], want[:nbuf], vp.GetVPInfo(), f"{name} MEM_HOST_PINNED, scribbled after Synchronize")


# ---- 4: a page-locked buffer passed as plain MPCVR_MEM_HOST is still staged ------------------------------------------------------------------
def test_page_locked_buffer_passed_as_mem_host_is_staged(mpcvr, torch_cuda):
    """PROBABILISTIC — the one such test of this file: a library that skipped its staging copy, or DMA'd from the caller's pointer, would lose
    a race here most of the time, not every time.  A 1920 x 1080 P010 frame (6 MB: a DMA long enough to race), converted at the same size,
    lies in a page-locked tensor and is handed over as plain MPCVR_MEM_HOST — "the caller's buffer is free again when the call returns" — and
    is overwritten in the very next statement.  (With pageable memory the runtime's own staging would hide the mistake.)  The expectation
    is the zero-copy frame; no oracle run at this size."""
    from videorenderer_amd import api
    torch = torch_cuda
    c = dict(cformat=2, w=1920, h=1080, kind="noise", seed=700, dst=(1920, 1080), exfmt=HDR10)
    frame, pitch = case_frame(c)
    want, winfo = run_product(mpcvr, torch, c, extra_flags=api.FLAG_NO_FRAME_LANES)
    pin = torch.empty(frame.size, dtype=torch.uint8).pin_memory()
    view = pin.numpy()
    view[:] = frame
    with context_of(mpcvr, torch, c, "own_stream_lanes") as (vp, ww, wh):
        dst = targets(torch, 1, ww, wh)[0]
        vp.CopySample(pin, pitch, mem_kind=api.MEM_HOST)
        view[:] = 0xA5
        vp.Process(dst, ww * 4)
        vp.Synchronize()
        got = dst.cpu().numpy()
        diff = int((got != want).sum())
        assert diff == 0, f"{diff} bytes differ from the zero-copy frame: the sample was read from the caller's buffer after CopySample returned"
        assert vp.GetVPInfo() == winfo


# ---- 5: the repack families, streamed --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v210_ragged_width",                  # CopyFrameV210 into m_TexSrcVideo
                                  "rgb24_bottom_up_procamp",            # negative pitch: the host pointer is the lowest address
                                  "rgb48_width_not_multiple_of_4",      # remainder texels stay zero
                                  "r210_2x_dither",
                                  "p010_pitch_padded",                  # the upload carries the padding
                                  "c2_yuv420p10_catmull_2x",            # the <<6 applied at load
                                  "dovi_poly_sdr"])                     # per-frame constants, off the lanes
def test_repack_families_streamed_gpu_behind(mpcvr, oracle, torch_cuda, stall_mats, name):
    c = GOLDEN_CASES[name]
    want = expected(mpcvr, torch_cuda, oracle, c, N_FRAMES, name)
    outs, info = stream_one_buffer(mpcvr, torch_cuda, stall_mats, c, "own_stream_lanes", name)
    check(outs, want, info, name)


def retarget(vp, c):
    """InitMediaType and the rects of another case on a context that has drawn already (make_vp's order)."""
    w2, h2 = c["dst"]
    vp.InitMediaType(c["cformat"], c["w"], c["h"], pitch=c.get("pitch", 0), extfmt=c.get("exfmt", 0))
    vp.SetWindowRect((0, 0, w2, h2))
    vp.SetVideoRect((0, 0, w2, h2))
    return w2, h2


def test_source_texture_reused_across_rgb48_v210_rgb48(mpcvr, oracle, torch_cuda):
    """One context: RGB48 (46 wide: remainder texels) -> InitMediaType(v210) -> InitMediaType(RGB48) again, two host frames each.  The one
    m_TexSrcVideo is reused: the v210 repack leaves its bytes where RGB48's never-written texels lie, so it has to be zeroed again."""
    torch = torch_cuda
    rgb, v210 = GOLDEN_CASES["rgb48_width_not_multiple_of_4"], GOLDEN_CASES["v210_ragged_width"]
    want = {id(rgb): expected(mpcvr, torch, oracle, rgb, 4, "rgb48_width_not_multiple_of_4"),
            id(v210): expected(mpcvr, torch, oracle, v210, 2, "v210_ragged_width")}
    with context_of(mpcvr, torch, rgb, "own_stream_lanes") as (vp, ww, wh):
        for c, first in ((rgb, 0), (v210, 0), (rgb, 2)):
            w2, h2 = retarget(vp, c)
            dsts = targets(torch, 2, w2, h2)
            for i, d in enumerate(dsts):
                frame, pitch = case_frame(frame_case(c, first + i))
                vp.CopySample(frame, pitch)
                vp.Process(d, w2 * 4)
            vp.Synchronize()
            check([d.cpu().numpy() for d in dsts], want[id(c)][first:first + 2], vp.GetVPInfo(), f"cformat {c['cformat']} from frame {first}")


# ---- 6: the media type grows and shrinks between host samples --------------------------------------------------------------------------------
def test_media_type_grows_and_shrinks_between_host_samples(mpcvr, oracle, torch_cuda, stall_mats):
    """P010 64 x 40, then 248 x 40, then 64 x 40 again on one context, three host frames each (exact 2x, on the lanes): the slots' staging and
    device buffers are re-created for the larger sample while the three frames of the first size have not run yet (the GPU is behind)."""
    torch = torch_cuda
    big = GOLDEN_CASES["noise_p010_pq_lanczos3_2x"]
    small = dict(big, w=64, h=40, dst=(128, 80), seed=600)
    assert (big["w"], big["h"]) == (248, 40)
    want_small = expected(mpcvr, torch, oracle, small, 6, "p010_64x40")
    want_big = expected(mpcvr, torch, oracle, big, 3, "noise_p010_pq_lanczos3_2x")
    with context_of(mpcvr, torch, small, "own_stream_lanes") as (vp, ww, wh):
        runs, infos = [], []
        for c, want, first in ((small, want_small, 0), (big, want_big, 0), (small, want_small, 3)):
            w2, h2 = c["dst"]
            runs.append((c, want[first:first + 3], first, targets(torch, 3, w2, h2)))
        ev = gpu_behind(torch, stall_mats)
        for i, (c, want, first, dsts) in enumerate(runs):
            if i:
                retarget(vp, c)             # (the next Process re-plans, which waits for the frames in flight; CopySample re-creates the slot buffers)
            w2, h2 = c["dst"]
            for j, d in enumerate(dsts):
                frame, pitch = case_frame(frame_case(c, first + j))
                vp.CopySample(frame, pitch)
                vp.Process(d, w2 * 4)
            infos.append(vp.GetVPInfo())    # (the plan Process has just settled: nothing is re-planned, nothing waits)
            if i == 0:
                still_behind(ev, "64 x 40, first three frames")
        vp.Synchronize()
        for (c, want, first, dsts), info in zip(runs, infos):
            check([d.cpu().numpy() for d in dsts], want, info, f"{c['w']} x {c['h']} from frame {first}")


# ---- 7: one host sample, several readers ------------------------------------------------------------------------------------------------------
REPAINTS = 6            # fewer than a lane's ring of frames in flight (kLaneDepth = 8): the host must not wait inside the window


def read_back_buffer(vp):
    ptr, pitch, w, h = vp.GetBackBuffer()
    out = np.empty((h, w, 4), dtype=np.uint8)
    assert pitch == w * 4
    assert C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.size), 2) == 0
    return out


@pytest.mark.parametrize("snapshot", [False, True])
def test_one_host_sample_drawn_into_two_targets_and_the_back_buffer(mpcvr, oracle, torch_cuda, stall_mats, snapshot):
    """CopySample(host H), Process -> A (repainted a few times), Process -> B (another target: another lane), Render; then either three more
    CopySample + Process pairs of other frames, the last of which takes H's slot, or GetCurentImage.  A, B and the back buffer hold H's picture
    (the window is the video rect: Render's clear leaves nothing), the snapshot equals a zero-copy context's.  The slot's one `consumed` event
    has to stand for ALL of H's readers: recorded behind the latest reader only, it fires while A's lane still draws from the slot."""
    from videorenderer_amd import api
    torch = torch_cuda
    name = "c3hdr_p010_pq_lanczos3_2x"
    c = GOLDEN_CASES[name]
    want = expected(mpcvr, torch, oracle, c, 4, name)
    frames = [case_frame(frame_case(c, k)) for k in range(4)]
    pitch = frames[0][1]
    if snapshot:
        zvp, _ = make_vp(mpcvr, c, api.FLAG_NO_FRAME_LANES)
        zvp.CopySample(torch.from_numpy(frames[0][0]).cuda(), pitch)
        want_snap = zvp.GetCurentImage()
        zvp.close()
    with context_of(mpcvr, torch, c, "own_stream_lanes") as (vp, ww, wh):
        a, b, *others = targets(torch, 5, ww, wh)
        ev = gpu_behind(torch, stall_mats)
        buf = frames[0][0].copy()
        vp.CopySample(buf, pitch)
        for _ in range(REPAINTS):           # (frames into one target share a lane: A's lane is REPAINTS kernels long, B's and Render's one each)
            vp.Process(a, ww * 4)
        vp.Process(b, ww * 4)
        assert vp.Render(1) == 0
        if snapshot:
            still_behind(ev, "A, B and Render queued")
            snap = vp.GetCurentImage()
            assert np.array_equal(snap, want_snap), "the snapshot of a host sample differs from the zero-copy snapshot"
        else:
            for k in (1, 2, 3):
                if k == RING:
                    still_behind(ev, "H and two more samples queued")
                buf[:] = frames[k][0]
                vp.CopySample(buf, pitch)
                vp.Process(others[k - 1], ww * 4)
        vp.Synchronize()
        info = vp.GetVPInfo()
        check([a.cpu().numpy(), b.cpu().numpy()], [want[0], want[0]], info, "H into A and B")
        if snapshot:
            check([read_back_buffer(vp)], [want[0]], info, "H in the back buffer")
        else:
            # (the back buffer's frame was followed by three samples: it must still be H)
            check([read_back_buffer(vp)] + [d.cpu().numpy() for d in others], [want[0]] + want[1:4], info, "back buffer, then frames 1 .. 3")


@pytest.mark.parametrize("name", ["c3hdr_p010_pq_lanczos3_2x", "v210_2x"])
def test_a_host_sample_that_is_never_drawn(mpcvr, oracle, torch_cuda, stall_mats, name):
    """The dropped frame: CopySample(H1), CopySample(H2), Process shows H2 — on the lanes and through the v210 repack, the GPU behind."""
    torch = torch_cuda
    c = GOLDEN_CASES[name]
    want = expected(mpcvr, torch, oracle, c, 2, name)
    (h1, pitch), (h2, _) = case_frame(frame_case(c, 0)), case_frame(frame_case(c, 1))
    with context_of(mpcvr, torch, c, "own_stream_lanes") as (vp, ww, wh):
        dst = targets(torch, 1, ww, wh)[0]
        ev = gpu_behind(torch, stall_mats)
        vp.CopySample(h1, pitch)
        vp.CopySample(h2, pitch)
        vp.Process(dst, ww * 4)
        still_behind(ev, name)
        vp.Synchronize()
        check([dst.cpu().numpy()], [want[1]], vp.GetVPInfo(), f"{name}: H2 behind a dropped H1")


# ---- 8: refusals leave the context usable ----------------------------------------------------------------------------------------------------
def hr_of(api, fn):
    with pytest.raises(api.MpcvrError) as e:
        fn()
    return e.value.hr


@pytest.mark.parametrize("mode", ["own_stream_lanes", "own_stream_no_lanes"])
def test_refused_copy_sample_keeps_the_current_sample(mpcvr, oracle, torch_cuda, stall_mats, mode):
    """include/mpcvr.h: a refused mpcvr_copy_sample changes nothing — the sample handed over before it stays current, with its upload slot.
    A good host sample, three refusals, Process: the good sample's picture; three more samples (the last one takes its slot), the GPU behind."""
    from videorenderer_amd import api
    torch = torch_cuda
    name = "c3hdr_p010_pq_lanczos3_2x"
    c = GOLDEN_CASES[name]
    want = expected(mpcvr, torch, oracle, c, 4, name)
    frames = [case_frame(frame_case(c, k)) for k in range(4)]
    pitch = frames[0][1]
    with context_of(mpcvr, torch, c, mode) as (vp, ww, wh):
        dsts = targets(torch, 4, ww, wh)
        ev = gpu_behind(torch, stall_mats)
        vp.CopySample(frames[0][0], pitch)
        other = frames[1][0]
        assert hr_of(api, lambda: vp.CopySample(other, pitch + 2, mem_kind=api.MEM_HOST)) == api.E_UNEXPECTED      # pitch != media type
        assert hr_of(api, lambda: vp.CopySample(other, pitch, mem_kind=7)) == api.E_INVALIDARG
        assert hr_of(api, lambda: vp.CopySample(0, pitch, mem_kind=api.MEM_HOST)) == api.E_POINTER
        vp.Process(dsts[0], ww * 4)
        for k in (1, 2, 3):
            if k == RING:
                still_behind(ev, f"refusals <{mode}>")
            vp.CopySample(frames[k][0], pitch)
            vp.Process(dsts[k], ww * 4)
        vp.Synchronize()
        check([d.cpu().numpy() for d in dsts], want, vp.GetVPInfo(), f"refusals <{mode}>")


def test_flush_drops_the_sample_and_the_next_host_sample_draws(mpcvr, oracle, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    name = "c3hdr_p010_pq_lanczos3_2x"
    c = GOLDEN_CASES[name]
    want = expected(mpcvr, torch, oracle, c, 2, name)
    with context_of(mpcvr, torch, c, "own_stream_lanes") as (vp, ww, wh):
        dsts = targets(torch, 2, ww, wh)
        frame, pitch = case_frame(frame_case(c, 0))
        vp.CopySample(frame, pitch)
        vp.Process(dsts[0], ww * 4)
        vp.Flush()
        assert hr_of(api, lambda: vp.Process(dsts[1], ww * 4)) == api.E_NOT_VALID_STATE
        assert vp.Render(1) == api.S_FALSE
        frame, pitch = case_frame(frame_case(c, 1))
        vp.CopySample(frame, pitch)
        vp.Process(dsts[1], ww * 4)
        vp.Synchronize()
        check([d.cpu().numpy() for d in dsts], want, vp.GetVPInfo(), "around Flush")


# ---- 9: one slot ring under three kinds of sample ---------------------------------------------------------------------------------------------
def test_host_tensor_and_field_samples_share_the_slot_ring_gpu_behind(mpcvr, torch_cuda, stall_mats):
    """mpcvr_copy_sample(MPCVR_MEM_HOST), mpcvr_copy_sample_tensor and mpcvr_copy_sample_fields fill the SAME three upload slots.  Seven
    samples of a 16 x 8 GBRP8 input (the one format all three take) in the order host, tensor, fields, host, tensor, fields, host — more
    than two turns of the ring — each drawn into its own 32 x 16 target before the next arrives, the GPU behind the host for the first turn.
    Expected, element for element: the same sample written into device memory by the caller (the bytes themselves, mpcvr_sample_pass,
    mpcvr_deint_pass), handed to a FRESH context as MPCVR_MEM_DEVICE and drawn alone.  A refused mpcvr_copy_sample_fields between two of
    them (field = 2) changes nothing: the next draw shows the sample before it."""
    from tests import deint_model as DM
    from tests import tensor_in_model as TM
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    w, h, cformat, kinds = 16, 8, TM.GBRP8, ("host", "tensor", "fields")
    ww, wh = 2 * w, 2 * h
    planes = api.plan_deint_planes(cformat, w, h)
    nbytes, pitch = DM.sample_size(planes), planes[0]["pitch"]
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(909)

    def context():
        vp = api.VideoProcessor(api.default_settings(iUpscaling=2), device=0)
        vp.InitMediaType(cformat, w, h)
        vp.SetWindowRect((0, 0, ww, wh))
        vp.SetVideoRect((0, 0, ww, wh))
        assert vp.GetFrameBytes() == (nbytes, pitch)
        return vp

    # the seven samples, and each as the bytes a caller would hand over as device memory
    given, as_device = [], []
    for k in range(N_FRAMES):
        kind = kinds[k % 3]
        dev = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        if kind == "host":
            data = rng.integers(0, 256, nbytes, dtype=np.uint8)
            dev.copy_(torch.from_numpy(data))
            given.append(data)
        elif kind == "tensor":
            t = torch.from_numpy(rng.random((3, h, w), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).cuda().to(torch.float16)
            d, _, _ = api._frame_tensor_desc(t, (255.0,) * 3, (0.0,) * 3, "rgb")
            api.sample_pass(t, d, w, h, cformat, dev, pitch, stream)
            given.append(t)
        else:
            s = [torch.from_numpy(x).cuda() for x in DM.noise_samples(planes, 3, 60 + k)]
            order, field, mode = 1 + k % 2, (k // 3) % 2, k % 2
            keep, first = DM.field_parity(order, field)
            api.deint_pass(s[0], s[1], s[2], cformat, w, h, 0, keep, first, mode, dev, 0, stream)
            given.append((s, order, field, mode))
        as_device.append(dev)
    want = []
    for dev in as_device:
        ref = context()
        dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
        ref.CopySample(dev, pitch, mem_kind=api.MEM_DEVICE)
        ref.Process(dst, ww * 4)
        ref.Synchronize()
        want.append((dst.cpu().numpy(), ref.GetVPInfo()))
        ref.close()
    for k in range(N_FRAMES):
        for step in (1, RING):
            if k + step < N_FRAMES:
                assert not np.array_equal(want[k][0], want[k + step][0]), f"expected frames {k} and {k + step} are the same picture"

    vp = context()
    try:
        vp.GetVPInfo()                      # UpdatePlan synchronizes the context stream: not inside the window
        dsts = targets(torch, N_FRAMES + 1, ww, wh)
        again = dsts.pop()
        ev = gpu_behind(torch, stall_mats)
        for k in range(N_FRAMES):
            kind = kinds[k % 3]
            if kind == "host":
                vp.CopySample(given[k], pitch, mem_kind=api.MEM_HOST)
            elif kind == "tensor":
                vp.CopySampleTensor(given[k])
            else:
                s, order, field, mode = given[k]
                vp.CopySampleFields(s[0], s[1], s[2], order, field, mode)
            vp.Process(dsts[k], ww * 4)
            if k == 1:                      # between the tensor sample and the fields sample: refused, the tensor sample stays current
                s = given[2][0]
                assert L.mpcvr_copy_sample_fields(vp._ctx, C.c_void_p(s[0].data_ptr()), C.c_void_p(s[1].data_ptr()), C.c_void_p(s[2].data_ptr()), 1, 2, 0) == api.E_INVALIDARG
                vp.Process(again, ww * 4)
            if k == RING - 1:
                still_behind(ev, "host, tensor, fields")        # (the next CopySample waits for sample 0, that is for the stall)
        vp.Synchronize()
        info = vp.GetVPInfo()
    finally:
        torch.cuda.synchronize()
        vp.close()
    check([d.cpu().numpy() for d in dsts], want, info, "host / tensor / fields samples")
    check([again.cpu().numpy()], [want[1]], info, "the draw behind a refused mpcvr_copy_sample_fields")
