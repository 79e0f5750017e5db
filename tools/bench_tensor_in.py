"""tools/bench_tensor_in.py — what the sample pass (a model's float tensor as a planar RGB sample) sustains on resident buffers, in one process.

    python tools/bench_tensor_in.py [--launches 200] [--warmup 20] [--repeats 5] [--steps 8] [--batch-warmup 3] [--batch 32] [--out FILE]

1. mpcvr_sample_pass (k_sample_from_tensor: fp32 / fp16 / bf16, C,H,W or H,W,C, into GBRP8 / GBRP16), all 12 instantiations at 3840x2160
   and 7680x4320, beside a device-to-device hipMemcpyAsync of the same number of bytes — the method of tools/bench_tensor.py: device events
   around `launches` back-to-back launches after `warmup` launches, `repeats` windows with the copy alternating, the median window and the
   spread (min .. max).  Bytes moved = the tensor read once (12 or 6 bytes per pixel) + the sample written (3 or 6); the copy reads AND
   writes that many bytes, so its own traffic is twice the pass's: the ratio compares time for the same payload.  The buffers are resident
   and the launches repeat: at 3840x2160 the last-level cache (256 MiB) holds them, at 7680x4320 part of them.
2. mpcvr_process_batch_from_tensors, 32 frames per call, fp16 N x 3 x H x W into a GBRP16 input -> BGRA8 targets, 1080p -> 1440p and
   4K -> 8K, against what it replaces, alternating window by window on a caller's stream:
       a   32 mpcvr_sample_pass calls into 32 samples of the caller's, then mpcvr_process_batch — the composition
       t   the torch formulation (multiply, add, round, clamp, cast, permute to G, B, R planes), then mpcvr_process_batch
       b   mpcvr_process_batch_from_tensors (one pass per chunk, everything in stream order)
Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def factors(maxcode):
    """a tensor normalised with ImageNet's mean / std -> codes"""
    return tuple(maxcode * s for s in IMAGENET_STD), tuple(maxcode * m for m in IMAGENET_MEAN)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--batch-warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--workloads", default="up1440,c3hdr")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from videorenderer_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("bench_tensor_in: no GPU visible")
    L = api.load_library()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lines = []

    # ---- 1. the pass ----
    stream = torch.cuda.current_stream().cuda_stream
    sp = C.c_void_p(stream) if stream else None
    lines += ["# 1. mpcvr_sample_pass vs hipMemcpyAsync(device to device) of the same payload; %d launches per window after %d warm-up, median of %d windows (min .. max)"
              % (a.launches, a.warmup, a.repeats),
              "# device: %s" % torch.cuda.get_device_name(0),
              "# payload = tensor read (12 B/pixel fp32, 6 B/pixel fp16 / bf16) + sample written (3 B/pixel GBRP8, 6 B/pixel GBRP16); the copy reads AND writes that many bytes",
              "# resident buffers, repeated launches: the last-level cache serves part of the traffic (all of it may fit at 3840x2160)",
              "# case                              payload_MB    pass_us    pass_GBps (min..max)      copy_us  copy_GBps (min..max)        pass/copy"]

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
    for w, h in ((3840, 2160), (7680, 4320)):
        for dtype, dname, es, tdt in ((api.TENSOR_F32, "f32", 4, torch.float32), (api.TENSOR_F16, "f16", 2, torch.float16), (api.TENSOR_BF16, "bf16", 2, torch.bfloat16)):
            src = (torch.rand(3 * h * w, dtype=torch.float32, device="cuda") * 5.0 - 2.3).to(tdt)      # codes inside and just outside the format
            for cformat, fname, by, maxcode in ((api.CF_GBRP8, "gbrp8", 1, 255), (api.CF_GBRP16, "gbrp16", 2, 65535)):
                scale, bias = factors(maxcode)
                dst = torch.empty(3 * h * w * by, dtype=torch.uint8, device="cuda")
                payload = 3 * w * h * (es + by)
                a_buf = torch.empty(payload, dtype=torch.uint8, device="cuda")
                b_buf = torch.empty(payload, dtype=torch.uint8, device="cuda")
                for layout, lname in ((api.TENSOR_PLANAR, "chw"), (api.TENSOR_INTERLEAVED, "hwc")):
                    d = api.tensor_desc(dtype, layout, w * es * (1 if layout == api.TENSOR_PLANAR else 3), w * h * es, scale, bias)

                    def run():
                        hr = L.mpcvr_sample_pass(C.c_void_p(src.data_ptr()), C.byref(d), w, h, cformat, C.c_void_p(dst.data_ptr()), w * by, sp)
                        assert hr == 0, hr

                    def cpy():
                        rc = hip.hipMemcpyAsync(C.c_void_p(b_buf.data_ptr()), C.c_void_p(a_buf.data_ptr()), payload, 3, sp)
                        assert rc == 0, rc

                    tp, tc = [], []
                    for _ in range(a.repeats):          # alternating: both see the same neighbours on a shared machine
                        tp.append(window(run))
                        tc.append(window(cpy))
                    g = lambda t: payload / t * 1e-9
                    mp, mc = float(np.median(tp)), float(np.median(tc))
                    ratios["%dx%d %s %s %s" % (w, h, dname, lname, fname)] = mc / mp
                    lines.append("%-10s %-5s %-4s %-7s %15.1f %10.1f %9.0f (%.0f..%.0f) %12.1f %9.0f (%.0f..%.0f) %12.2f"
                                 % ("%dx%d" % (w, h), dname, lname, fname, payload * 1e-6, mp * 1e6, g(mp), g(max(tp)), g(min(tp)), mc * 1e6, g(mc), g(max(tc)), g(min(tc)),
                                    mc / mp))
                del dst, a_buf, b_buf
            del src
            torch.cuda.empty_cache()
    r = list(ratios.values())
    lines.append("# pass / copy (rate for the same payload): %.2f .. %.2f over the %d cases, median %.2f; below 1.0: %s"
                 % (min(r), max(r), len(r), float(np.median(r)), ", ".join(k for k, v in ratios.items() if v < 1.0) or "none"))

    # ---- 2. the batch call ----
    n = a.batch
    lines += ["#", "# 2. mpcvr_process_batch_from_tensors (fp16 N x 3 x H x W, ImageNet mean / std, GBRP16 input -> BGRA8) against what it replaces; %d frames per call,"
              % n, "# %d calls per window after %d warm-up calls, median of %d alternating windows (min .. max), all on a caller's stream" % (a.steps, a.batch_warmup, a.repeats),
              "# a = %d x mpcvr_sample_pass + mpcvr_process_batch (the composition); t = torch (multiply, add, round, clamp, cast, permute) + mpcvr_process_batch; b = the new call" % n,
              "# workload  contender  chunks  launches    ms_per_call (min..max)        frames_per_s   vs_a"]
    caller = torch.cuda.Stream()
    scale, bias = factors(65535)
    for name in a.workloads.split(","):
        wl = dict(bench.WORKLOADS[name])
        w, h, s = wl["w"], wl["h"], wl["scale"]
        dw, dh = wl.get("dst", (w * s, h * s))
        settings = api.default_settings(iUpscaling=wl["iUpscaling"], iDownscaling=wl.get("iDownscaling", 2), output_format=0, bUseDither=wl.get("bUseDither", 1))

        def context():
            with torch.cuda.stream(caller):
                vp = api.VideoProcessor(settings)
            vp.InitMediaType(api.CF_GBRP16, w, h)
            vp.SetWindowRect((0, 0, dw, dh))
            vp.SetVideoRect((0, 0, dw, dh))
            return vp

        vp_a, vp_t, vp_b = context(), context(), context()
        nbytes, pitch = vp_a.GetFrameBytes()
        assert pitch == 2 * w and nbytes == 3 * pitch * h
        with torch.cuda.stream(caller):
            # two sets of tensors taken in turn (a model writes one while the other is read)
            ts = [(torch.rand((n, 3, h, w), dtype=torch.float32, device="cuda") * 5.0 - 2.3).to(torch.float16) for _ in range(2)]
            samples = torch.empty((n, 3, h, w), dtype=torch.int16, device="cuda")
            rgb = torch.empty((n, dh, dw, 4), dtype=torch.uint8, device="cuda")
            scale_t = torch.tensor(scale, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
            bias_t = torch.tensor(bias, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
        arr = C.c_void_p * n
        d = api.tensor_desc(api.TENSOR_F16, api.TENSOR_PLANAR, w * 2, w * h * 2, scale, bias)
        ta = [arr(*[t.data_ptr() + i * 3 * h * w * 2 for i in range(n)]) for t in ts]
        ra = arr(*[rgb[i].data_ptr() for i in range(n)])
        batch = vp_a.PrepareBatch([samples[i] for i in range(n)], [rgb[i] for i in range(n)])
        pass_args = [[(C.c_void_p(ts[k].data_ptr() + i * 3 * h * w * 2), C.byref(d), w, h, api.CF_GBRP16, C.c_void_p(samples[i].data_ptr()), pitch, C.c_void_p(caller.cuda_stream))
                      for i in range(n)] for k in range(2)]

        def call_a(i):
            for args in pass_args[i & 1]:
                assert L.mpcvr_sample_pass(*args) == 0
            vp_a.ProcessBatch(batch, None, dw * 4)

        def call_t(i):
            x = ts[i & 1].to(torch.float32).mul_(scale_t).add_(bias_t).round_().clamp_(0, 65535)      # multiply, add, round, clamp
            samples.copy_(x[:, [1, 2, 0]].to(torch.int32))                                              # permute to G, B, R, cast (int16 keeps the low 16 bits)
            vp_t.ProcessBatch(batch, None, dw * 4)

        def call_b(i):
            hr = L.mpcvr_process_batch_from_tensors(vp_b._ctx, n, ta[i & 1], C.byref(d), ra, dw * 4)
            assert hr == 0, (hr, L.mpcvr_last_error(vp_b._ctx))

        def bwindow(fn, vp):
            with torch.cuda.stream(caller):
                for i in range(a.batch_warmup):
                    fn(i)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.steps):
                    fn(a.batch_warmup + i)
                e1.record()
                vp.Synchronize()
                e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / a.steps

        contenders = [("a", call_a, vp_a), ("t", call_t, vp_t), ("b", call_b, vp_b)]
        times = {c[0]: [] for c in contenders}
        infos = {}
        for _ in range(a.repeats):
            for cname, fn, vp in contenders:
                times[cname].append(bwindow(fn, vp))
                infos[cname] = vp.GetLastBatchInfo()
        base = float(np.median(times["a"]))
        for cname, _, _ in contenders:
            t = times[cname]
            m = float(np.median(t))
            info = infos[cname]
            launches = "%d" % (info["launches"] + n) if cname == "a" else "%d+torch" % info["launches"] if cname == "t" else "%d" % info["launches"]
            lines.append("%-9s %-10s %6s %9s %11.3f (%.3f..%.3f) %14.0f %6.3f"
                         % (name, cname, info.get("sample_chunks", "-"), launches, m * 1e3, min(t) * 1e3, max(t) * 1e3, n / m, base / m))
        for vp in (vp_a, vp_t, vp_b):
            vp.close()
        del ts, samples, rgb, batch
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
