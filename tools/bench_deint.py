"""tools/bench_deint.py — what the deinterlacing pass (motion-adaptive, at field rate) sustains on resident samples, in one process.

    python tools/bench_deint.py [--launches 200] [--warmup 20] [--repeats 5] [--steps 8] [--batch-warmup 3] [--frames 16] [--out FILE]

1. mpcvr_deint_pass (k_deint) at 1920x1080 and 3840x2160, NV12 and P010, both modes, beside a device-to-device hipMemcpyAsync of the same
   payload — the method of tools/bench_tensor_in.py: device events around `launches` back-to-back calls after `warmup` calls, `repeats`
   windows with the copy alternating, the median window and the spread (min .. max).  Payload = 2.5 frames read (the frame holding the other
   field contributes only the lines beside the kept ones) + 1 frame written; the copy reads AND writes that many bytes, so its own traffic
   is twice the payload: the ratio compares time for the same payload.  A pass is two launches for these bi-planar formats (Y, UV).  The
   samples are resident and the calls repeat: the last-level cache (256 MiB) holds all of them at both sizes.
2. mpcvr_process_batch_deint, `frames` interior frames -> 2 x `frames` pictures per call, 1080i NV12 -> 1080p and -> 1440p BGRA8, against
   its composition, alternating window by window on a caller's stream:
       a    2 x frames mpcvr_deint_pass calls into samples of the caller's, then mpcvr_process_batch — the composition
       a2   the same again: a against itself is the spread a difference has to exceed
       b    mpcvr_process_batch_deint (one pass per chunk, everything in stream order)
Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--batch-warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from videorenderer_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("bench_deint: no GPU visible")
    L = api.load_library()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lines = []

    # ---- 1. the pass ----
    stream = torch.cuda.current_stream().cuda_stream
    sp = C.c_void_p(stream) if stream else None
    lines += ["# 1. mpcvr_deint_pass vs hipMemcpyAsync(device to device) of the same payload; %d calls per window after %d warm-up, median of %d windows (min .. max)"
              % (a.launches, a.warmup, a.repeats),
              "# device: %s" % torch.cuda.get_device_name(0),
              "# payload = 2.5 frames read + 1 frame written; the copy reads AND writes that many bytes; a pass = 2 k_deint launches (Y plane, UV plane)",
              "# resident samples, repeated calls: the last-level cache can hold all of them",
              "# case                          payload_MB    pass_us    pass_GBps (min..max)      copy_us  copy_GBps (min..max)        pass/copy"]

    def window(fn):
        for _ in range(a.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / a.launches

    ratios = {}
    for w, h in ((1920, 1080), (3840, 2160)):
        for cformat, fname, by in ((api.CF_NV12, "nv12", 1), (api.CF_P010, "p010", 2)):
            frame = w * by * h * 3 // 2
            src = [torch.randint(0, 256, (frame,), dtype=torch.uint8, device="cuda") for _ in range(3)]
            dst = torch.empty(frame, dtype=torch.uint8, device="cuda")
            payload = frame * 7 // 2
            a_buf = torch.empty(payload, dtype=torch.uint8, device="cuda")
            b_buf = torch.empty(payload, dtype=torch.uint8, device="cuda")
            for mode, mname in ((api.DEINT_ADAPTIVE_EXT, "check"), (api.DEINT_ADAPTIVE_NOCHECK_EXT, "nocheck")):
                field = [0]

                def run():
                    field[0] ^= 1                       # the two fields of the frame in turn: keep = field, first = (field == 0)
                    hr = L.mpcvr_deint_pass(C.c_void_p(src[0].data_ptr()), C.c_void_p(src[1].data_ptr()), C.c_void_p(src[2].data_ptr()), cformat, w, h, w * by,
                                            field[0], 1 - field[0], mode, C.c_void_p(dst.data_ptr()), w * by, sp)
                    assert hr == 0, hr

                def cpy():
                    rc = hip.hipMemcpyAsync(C.c_void_p(b_buf.data_ptr()), C.c_void_p(a_buf.data_ptr()), payload, 3, sp)
                    assert rc == 0, rc

                tp, tc = [], []
                for _ in range(a.repeats):              # alternating: both see the same neighbours on a shared machine
                    tp.append(window(run))
                    tc.append(window(cpy))
                g = lambda t: payload / t * 1e-9
                mp, mc = float(np.median(tp)), float(np.median(tc))
                ratios["%dx%d %s %s" % (w, h, fname, mname)] = mc / mp
                lines.append("%-10s %-5s %-8s %15.1f %10.1f %9.0f (%.0f..%.0f) %12.1f %9.0f (%.0f..%.0f) %12.2f"
                             % ("%dx%d" % (w, h), fname, mname, payload * 1e-6, mp * 1e6, g(mp), g(max(tp)), g(min(tp)), mc * 1e6, g(mc), g(max(tc)), g(min(tc)), mc / mp))
            del src, dst, a_buf, b_buf
            torch.cuda.empty_cache()
    r = list(ratios.values())
    lines.append("# pass / copy (rate for the same payload): %.2f .. %.2f over the %d cases, median %.2f; below 1.0: %s"
                 % (min(r), max(r), len(r), float(np.median(r)), ", ".join(k for k, v in ratios.items() if v < 1.0) or "none"))

    # ---- 2. the batch call ----
    n, fpf = a.frames, 2
    n_out = n * fpf
    lines += ["#", "# 2. mpcvr_process_batch_deint (1080i NV12, top field first, both fields, mode check -> BGRA8) against its composition; %d interior frames -> %d pictures per call,"
              % (n, n_out), "# %d calls per window after %d warm-up calls, median of %d alternating windows (min .. max), all on a caller's stream" % (a.steps, a.batch_warmup, a.repeats),
              "# a = %d x mpcvr_deint_pass + mpcvr_process_batch (the composition); a2 = the same again; b = the new call" % n_out,
              "# target    contender  chunks  launches    ms_per_call (min..max)        pictures_per_s   a/x: median (min..max) over the windows"]
    caller = torch.cuda.Stream()
    w, h = 1920, 1080
    for name, (dw, dh) in (("1080p", (1920, 1080)), ("1440p", (2560, 1440))):
        settings = api.default_settings(iUpscaling=2, output_format=0)

        def context():
            with torch.cuda.stream(caller):
                vp = api.VideoProcessor(settings)
            vp.InitMediaType(api.CF_NV12, w, h)
            vp.SetWindowRect((0, 0, dw, dh))
            vp.SetVideoRect((0, 0, dw, dh))
            return vp

        vps = {"a": context(), "a2": context(), "b": context()}
        nbytes, pitch = vps["a"].GetFrameBytes()
        with torch.cuda.stream(caller):
            frames = torch.randint(0, 256, (n + 2, nbytes), dtype=torch.uint8, device="cuda")
            samples = torch.empty((n_out, nbytes), dtype=torch.uint8, device="cuda")
            rgb = torch.empty((n_out, dh, dw, 4), dtype=torch.uint8, device="cuda")
        fa = (C.c_void_p * (n + 2))(*[frames[i].data_ptr() for i in range(n + 2)])
        ra = (C.c_void_p * n_out)(*[rgb[i].data_ptr() for i in range(n_out)])
        batches = {c: vps[c].PrepareBatch([samples[i] for i in range(n_out)], [rgb[i] for i in range(n_out)]) for c in ("a", "a2")}
        pass_args = [(C.c_void_p(frames[k // fpf].data_ptr()), C.c_void_p(frames[1 + k // fpf].data_ptr()), C.c_void_p(frames[2 + k // fpf].data_ptr()), api.CF_NV12, w, h, pitch,
                      k % fpf, 1 - k % fpf, api.DEINT_ADAPTIVE_EXT, C.c_void_p(samples[k].data_ptr()), pitch, C.c_void_p(caller.cuda_stream)) for k in range(n_out)]

        def composition(c):
            def call():
                for args in pass_args:
                    assert L.mpcvr_deint_pass(*args) == 0
                vps[c].ProcessBatch(batches[c], None, dw * 4)
            return call

        def call_b():
            hr = L.mpcvr_process_batch_deint(vps["b"]._ctx, n, fa, api.FIELD_ORDER_TFF, fpf, api.DEINT_ADAPTIVE_EXT, ra, dw * 4)
            assert hr == 0, (hr, L.mpcvr_last_error(vps["b"]._ctx))

        def bwindow(fn, vp):
            with torch.cuda.stream(caller):
                for _ in range(a.batch_warmup):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    fn()
                e1.record()
                vp.Synchronize()
                e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / a.steps

        contenders = [("a", composition("a")), ("a2", composition("a2")), ("b", call_b)]
        times = {c[0]: [] for c in contenders}
        infos = {}
        for _ in range(a.repeats):
            for cname, fn in contenders:
                times[cname].append(bwindow(fn, vps[cname]))
                infos[cname] = vps[cname].GetLastBatchInfo()
        for cname, _ in contenders:
            t = times[cname]
            m = float(np.median(t))
            info = infos[cname]
            per = [x / y for x, y in zip(times["a"], t)]      # window by window: neighbours in time
            launches = info["launches"] + (2 * n_out if cname != "b" else 0)
            lines.append("%-9s %-10s %6s %9d %11.3f (%.3f..%.3f) %16.0f   %.3f (%.3f..%.3f)"
                         % (name, cname, info.get("deint_chunks", "-"), launches, m * 1e3, min(t) * 1e3, max(t) * 1e3, n_out / m, float(np.median(per)), min(per), max(per)))
        for vp in vps.values():
            vp.close()
        del frames, samples, rgb, batches
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
