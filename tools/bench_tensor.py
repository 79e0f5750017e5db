"""tools/bench_tensor.py — what the tensor extension sustains on resident surfaces, in one process.

    python tools/bench_tensor.py [--launches 200] [--warmup 20] [--repeats 5] [--steps 8] [--batch-warmup 3] [--batch 32] [--out FILE]

1. mpcvr_tensor_pass (k_tensor: a rendered RGB surface written as fp32 / fp16 / bf16, C,H,W or H,W,C), all 12 instantiations at 3840x2160
   and 7680x4320, beside a device-to-device hipMemcpyAsync of the same number of bytes — the method of tools/bench_encode.py: device
   events around `launches` back-to-back launches after `warmup` launches, `repeats` windows with the copy alternating, the median window
   and the spread (min .. max).  Bytes moved = the surface read once (4 bytes per texel) + the elements written (6 or 12 per texel); the
   copy reads AND writes that many bytes, so its own traffic is twice the pass's: the ratio compares time for the same payload.
2. mpcvr_process_batch_tensor, 32 frames per call, fp16 C,H,W, for bench.py's c3hdr (4K P010 PQ -> 8K) and up1440 (1080p -> 1440p),
   against what it replaces, alternating window by window (the method of tools/bench_batch_yuv.py):
       a   mpcvr_process_batch into 32 RGB targets, then 32 mpcvr_tensor_pass calls, on a caller's stream — the bar
       t   mpcvr_process_batch, then the torch formulation (unpack, permute, cast, normalise), on a caller's stream
       b   mpcvr_process_batch_tensor on a caller's stream (everything in stream order)
       c   mpcvr_process_batch_tensor on a context that owns its stream (chunks on the two batch lanes)
Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SCALE = tuple(1 / (255 * s) for s in IMAGENET_STD)
BIAS = tuple(-m / s for m, s in zip(IMAGENET_MEAN, IMAGENET_STD))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--batch-warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--workloads", default="c3hdr,up1440")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from videorenderer_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("bench_tensor: no GPU visible")
    L = api.load_library()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lines = []

    # ---- 1. the pass ----
    stream = torch.cuda.current_stream().cuda_stream
    sp = C.c_void_p(stream) if stream else None
    lines += ["# 1. mpcvr_tensor_pass vs hipMemcpyAsync(device to device) of the same payload; %d launches per window after %d warm-up, median of %d windows (min .. max)"
              % (a.launches, a.warmup, a.repeats),
              "# device: %s" % torch.cuda.get_device_name(0),
              "# payload = surface read (4 B/texel) + elements written (12 B/texel fp32, 6 B/texel fp16 / bf16); the copy reads AND writes that many bytes",
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
        src = torch.randint(0, 2 ** 31 - 1, (h, w), dtype=torch.int32, device="cuda")
        for dtype, dname, es in ((api.TENSOR_F32, "f32", 4), (api.TENSOR_F16, "f16", 2), (api.TENSOR_BF16, "bf16", 2)):
            dst = torch.empty(3 * h * w * es, dtype=torch.uint8, device="cuda")
            payload = w * h * 4 + 3 * w * h * es
            a_buf = torch.empty(payload, dtype=torch.uint8, device="cuda")
            b_buf = torch.empty(payload, dtype=torch.uint8, device="cuda")
            for src_fmt, fname in ((0, "bgra8"), (1, "rgb10a2")):
                for layout, lname in ((api.TENSOR_PLANAR, "chw"), (api.TENSOR_INTERLEAVED, "hwc")):
                    d = api.tensor_desc(dtype, layout, w * es * (1 if layout == api.TENSOR_PLANAR else 3), w * h * es, SCALE, BIAS)

                    def run():
                        hr = L.mpcvr_tensor_pass(C.c_void_p(src.data_ptr()), w * 4, src_fmt, w, h, C.byref(d), C.c_void_p(dst.data_ptr()), sp)
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
                    ratios["%dx%d %s %s %s" % (w, h, fname, dname, lname)] = mc / mp
                    lines.append("%-10s %-8s %-5s %-4s %14.1f %10.1f %9.0f (%.0f..%.0f) %12.1f %9.0f (%.0f..%.0f) %12.2f"
                                 % ("%dx%d" % (w, h), fname, dname, lname, payload * 1e-6, mp * 1e6, g(mp), g(max(tp)), g(min(tp)), mc * 1e6, g(mc), g(max(tc)), g(min(tc)),
                                    mc / mp))
            del dst, a_buf, b_buf
        del src
        torch.cuda.empty_cache()
    r = list(ratios.values())
    lines.append("# pass / copy (rate for the same payload): %.2f .. %.2f over the %d cases, median %.2f; below 1.0: %s"
                 % (min(r), max(r), len(r), float(np.median(r)), ", ".join(k for k, v in ratios.items() if v < 1.0) or "none"))

    # ---- 2. the batch call ----
    n = a.batch
    ring = n + 16
    lines += ["#", "# 2. mpcvr_process_batch_tensor (fp16 C,H,W, ImageNet mean / std) against what it replaces; %d frames per call, %d calls per window after %d warm-up calls,"
              % (n, a.steps, a.batch_warmup),
              "# median of %d alternating windows (min .. max)" % a.repeats,
              "# a = mpcvr_process_batch + %d x mpcvr_tensor_pass on a caller's stream (the bar); t = mpcvr_process_batch + torch (unpack, permute, cast, normalise);" % n,
              "# b = the new call on a caller's stream; c = the new call on a context that owns its stream (batch lanes)",
              "# workload  contender  chunks  launches  lanes    ms_per_call (min..max)        frames_per_s   vs_a"]
    caller = torch.cuda.Stream()
    legacy = torch.cuda.default_stream()
    for name in a.workloads.split(","):
        wl = dict(bench.WORKLOADS[name])
        w, h, s = wl["w"], wl["h"], wl["scale"]
        dw, dh = wl.get("dst", (w * s, h * s))
        extfmt = api.make_extfmt(**wl["ext"])
        settings = api.default_settings(iUpscaling=wl["iUpscaling"], iDownscaling=wl.get("iDownscaling", 2), output_format=0, bUseDither=wl.get("bUseDither", 1))

        def context(own):
            if own:
                vp = api.VideoProcessor(settings, use_torch_stream=False)
            else:
                with torch.cuda.stream(caller):
                    vp = api.VideoProcessor(settings)
            vp.InitMediaType(wl["cformat"], w, h, extfmt=extfmt)
            vp.SetWindowRect((0, 0, dw, dh))
            vp.SetVideoRect((0, 0, dw, dh))
            return vp

        vp_a, vp_t, vp_b, vp_c = context(False), context(False), context(False), context(True)
        nbytes, pitch = vp_a.GetFrameBytes()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0x4D50)
        srcs = [bench.noise_frame_gpu(torch, wl, nbytes, pitch, gen) for _ in range(ring)]
        rgb = torch.empty((n, dh, dw, 4), dtype=torch.uint8, device="cuda")
        # two sets of tensors, taken in turn call by call (a model still reads one while the next is written): consecutive calls of c write
        # different memory, so the lanes may run them side by side
        outs = [torch.empty((n, 3, dh, dw), dtype=torch.float16, device="cuda") for _ in range(2)]
        arr = C.c_void_p * n
        frame_bytes = 3 * dh * dw * 2
        da = [arr(*[o.data_ptr() + i * frame_bytes for i in range(n)]) for o in outs]
        sa = {k: arr(*[srcs[(k + j) % ring].data_ptr() for j in range(n)]) for k in range(0, ring, 16)}
        batches = {k: vp_a.PrepareBatch([srcs[(k + j) % ring] for j in range(n)], [rgb[i] for i in range(n)]) for k in sa}
        d = api.tensor_desc(api.TENSOR_F16, api.TENSOR_PLANAR, dw * 2, dw * dh * 2, SCALE, BIAS)
        pass_args = [[(C.c_void_p(rgb[i].data_ptr()), dw * 4, 0, dw, dh, C.byref(d), C.c_void_p(outs[k].data_ptr() + i * frame_bytes), C.c_void_p(caller.cuda_stream))
                      for i in range(n)] for k in range(2)]
        with torch.cuda.stream(caller):
            scale_t = torch.tensor(SCALE, dtype=torch.float16, device="cuda").view(1, 3, 1, 1)
            bias_t = torch.tensor(BIAS, dtype=torch.float16, device="cuda").view(1, 3, 1, 1)

        def call_a(i):
            vp_a.ProcessBatch(batches[(i * 16) % ring], None, dw * 4)
            for args in pass_args[i & 1]:
                assert L.mpcvr_tensor_pass(*args) == 0

        def call_t(i):
            vp_t.ProcessBatch(batches[(i * 16) % ring], None, dw * 4)
            x = rgb[..., [2, 1, 0]]                                     # unpack: R, G, B of B8G8R8A8
            x = x.permute(0, 3, 1, 2).to(torch.float16)                 # permute, cast
            torch.add(x.mul_(scale_t), bias_t, out=outs[i & 1])         # normalise

        def call_tensor(vp):
            def call(i):
                hr = L.mpcvr_process_batch_tensor(vp._ctx, n, sa[(i * 16) % ring], C.byref(d), da[i & 1])
                assert hr == 0, (hr, L.mpcvr_last_error(vp._ctx))
            return call

        def bwindow(fn, vp, stream):
            with torch.cuda.stream(stream):
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

        contenders = [("a", call_a, vp_a, caller), ("t", call_t, vp_t, caller), ("b", call_tensor(vp_b), vp_b, caller), ("c", call_tensor(vp_c), vp_c, legacy)]
        times = {c[0]: [] for c in contenders}
        infos = {}
        for _ in range(a.repeats):
            for cname, fn, vp, stream in contenders:
                times[cname].append(bwindow(fn, vp, stream))
                infos[cname] = vp.GetLastBatchInfo()
        base = float(np.median(times["a"]))
        for cname, _, _, _ in contenders:
            t = times[cname]
            m = float(np.median(t))
            info = infos[cname]
            launches = "%d" % (info["launches"] + n) if cname == "a" else "%d+torch" % info["launches"] if cname == "t" else "%d" % info["launches"]
            lanes = ",".join(str(x) for x in sorted(set(info.get("tensor_lanes", [info["lane"]]))))
            lines.append("%-9s %-10s %6s %9s  %-7s %9.3f (%.3f..%.3f) %14.0f %6.3f"
                         % (name, cname, info.get("tensor_chunks", "-"), launches, lanes, m * 1e3, min(t) * 1e3, max(t) * 1e3, n / m, base / m))
        for vp in (vp_a, vp_t, vp_b, vp_c):
            vp.close()
        del srcs, rgb, outs, batches
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
