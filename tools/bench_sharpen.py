"""tools/bench_sharpen.py — what the sharpen extension sustains on resident surfaces, in one process.

    python tools/bench_sharpen.py [--launches 50] [--warmup 5] [--repeats 3] [--steps 6] [--batch-warmup 2] [--batch 32] [--sections 1,2,3] [--out FILE]

1. mpcvr_sharpen_pass (k_sharpen) at 1920x1080, 3840x2160 and 7680x4320, every radius, both modes and the four format pairs, on a smooth
   frame with a code or two of noise (every branch of the definition is taken), beside a device-to-device hipMemcpyAsync of the same
   number of bytes — the method of tools/bench_deband.py: device events around `launches` back-to-back launches after `warmup` launches,
   `repeats` windows with the pass and the copy alternating, the median window and the spread.  Payload = the surface read + the surface
   written (8 bytes per texel); the copy reads AND writes that many bytes, so its own traffic is twice the pass's: the ratio compares time
   for the same payload.  The buffers stay resident between launches, so the last-level cache serves part of the traffic of the smaller
   frames for the pass and the copy alike (the 1080p pair is 16.6 MB).  A second yardstick per size, in the same windows: mpcvr_deband_pass
   at one iteration and R = 8 with its taps from LDS, rgb10a2 -> bgra8 (the row of profiles/r19/deband_pass.txt).
2. Design choices made by measurement: the staging of the tile with 16-byte loads against guarded dword loads (MPCVR_SHARPEN_STAGING=dword,
   read per launch), radius 1 and 3, both modes, rgb10a2 -> bgra8, every size.
3. mpcvr_process_batch_sharpen, 32 frames per call, a 10-bit context (output_format RGB10A2, dither off) into BGRA8 targets with the default
   parameters, for bench.py's up1440 (1080p -> 1440p) and c3hdr (4K P010 PQ -> 8K), alternating window by window:
       a   mpcvr_process_batch into 32 RGB targets, then 32 mpcvr_sharpen_pass calls, on a caller's stream — the bar
       b   mpcvr_process_batch_sharpen on a caller's stream (everything in stream order)
       c   mpcvr_process_batch_sharpen on a context that owns its stream (chunks on the two batch lanes)
Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FMT = {0: "bgra8", 1: "rgb10a2"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--batch-warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--workloads", default="up1440,c3hdr")
    ap.add_argument("--sizes", default="1920x1080,3840x2160,7680x4320")
    ap.add_argument("--sections", default="1,2,3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sections = set(a.sections.split(","))
    import torch
    import bench
    from videorenderer_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("bench_sharpen: no GPU visible")
    L = api.load_library()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lines = ["# device: %s; library: %s" % (torch.cuda.get_device_name(0), os.environ.get("MPCVR_LIB", "this build"))]
    stream = torch.cuda.current_stream().cuda_stream
    sp = C.c_void_p(stream) if stream else None
    os.environ.pop("MPCVR_DEBAND_TAPS", None)
    os.environ.pop("MPCVR_SHARPEN_STAGING", None)

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

    def smooth(w, h, fmt):
        """two slow ramps and their sum in the three channels plus noise of a code or two, quantised to the format: cored texels, sharpened
        texels and texels the limiter stops, side by side"""
        m = 1023 if fmt else 255
        x = torch.arange(w, device="cuda", dtype=torch.int64)[None, :].expand(h, w)
        y = torch.arange(h, device="cuda", dtype=torch.int64)[:, None].expand(h, w)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0x5348)
        r, g, b = ((v + torch.randint(-2, 3, (h, w), device="cuda", generator=gen)).clamp(0, m) for v in (x * m // w, y * m // h, (x + y) * m // (w + h)))
        word = (r | g << 10 | b << 20 | 0xc0000000) if fmt else (b | g << 8 | r << 16 | 0xff000000)
        return (word - 2 ** 32).to(torch.int32).contiguous()      # (the A / X bits are set: the word as a negative int32)

    def pass_fn(src, fmt, w, h, P, dst, dfmt):
        p = api.SharpenParams(*P)
        args = (C.c_void_p(src.data_ptr()), w * 4, fmt, w, h, C.byref(p), 1, C.c_void_p(dst.data_ptr()), w * 4, dfmt, sp)

        def run(_keep=p):
            hr = L.mpcvr_sharpen_pass(*args)
            assert hr == 0, hr
        return run

    def deband_fn(src, w, h, dst):
        p = api.DebandParams(8, 1, 16, 1)
        args = (C.c_void_p(src.data_ptr()), w * 4, 1, w, h, C.byref(p), 1, C.c_void_p(dst.data_ptr()), w * 4, 0, sp)

        def run(_keep=p):
            hr = L.mpcvr_deband_pass(*args)
            assert hr == 0, hr
        return run

    def params_for(fmt, radius, mode):
        """the defaults of the format at the radius and mode of the row"""
        d = api.sharpen_params_default(fmt)
        return (radius, d.amount, d.threshold, d.overshoot, mode, d.dither)

    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    if "1" in sections:
        lines += ["# 1. mpcvr_sharpen_pass vs hipMemcpyAsync(device to device) of the same payload; %d launches per window after %d warm-up, median of %d alternating"
                  % (a.launches, a.warmup, a.repeats),
                  "# windows (min .. max).  payload = surface read + surface written (8 B/texel); the copy reads AND writes that many bytes; resident buffers: the",
                  "# last-level cache serves part of the traffic of the smaller frames, for the pass and the copy alike.  Default amount, threshold, overshoot and dither",
                  "# of the source format.  pass/copy = copy time / pass time.  deband = mpcvr_deband_pass, 1 iteration, R = 8, taps from LDS, rgb10a2 -> bgra8, same windows",
                  "# size       src      dst      r  mode  pass_us (min..max)      copy_us  pass/copy"]
        ratios = []
        for w, h in sizes:
            payload = 8 * w * h
            a_buf = torch.empty(payload, dtype=torch.uint8, device="cuda")
            b_buf = torch.empty(payload, dtype=torch.uint8, device="cuda")
            dst = torch.empty((h, w), dtype=torch.int32, device="cuda")

            def cpy():
                rc = hip.hipMemcpyAsync(C.c_void_p(b_buf.data_ptr()), C.c_void_p(a_buf.data_ptr()), payload, 3, sp)
                assert rc == 0, rc

            frames = {fmt: smooth(w, h, fmt) for fmt in (1, 0)}
            for fmt in (1, 0):
                for dfmt in (0, 1):
                    for radius in (1, 2, 3):
                        for mode in (0, 1):
                            run = pass_fn(frames[fmt], fmt, w, h, params_for(fmt, radius, mode), dst, dfmt)
                            t, tc = [], []
                            for _ in range(a.repeats):          # alternating: both see the same neighbours on a shared machine
                                t.append(window(run))
                                tc.append(window(cpy))
                            m, mc = float(np.median(t)), float(np.median(tc))
                            ratios.append(mc / m)
                            lines.append("%-10s %-8s %-8s %-2d %-5s %8.1f (%.1f..%.1f) %11.1f %10.2f"
                                         % ("%dx%d" % (w, h), FMT[fmt], FMT[dfmt], radius, "luma" if mode else "rgb", m * 1e6, min(t) * 1e6, max(t) * 1e6, mc * 1e6, mc / m))
            run = deband_fn(frames[1], w, h, dst)
            t, tc = [], []
            for _ in range(a.repeats):
                t.append(window(run))
                tc.append(window(cpy))
            m, mc = float(np.median(t)), float(np.median(tc))
            lines.append("%-10s %-8s %-8s %-2s %-5s %8.1f (%.1f..%.1f) %11.1f %10.2f" % ("%dx%d" % (w, h), FMT[1], FMT[0], "-", "deband", m * 1e6, min(t) * 1e6, max(t) * 1e6, mc * 1e6, mc / m))
            del frames, a_buf, b_buf, dst
            torch.cuda.empty_cache()
        lines.append("# pass / copy (rate for the same payload): %.2f .. %.2f over the %d sharpen cases, median %.2f" % (min(ratios), max(ratios), len(ratios), float(np.median(ratios))))

    if "2" in sections:
        lines += ["#", "# 2. design choice: the tile staged with 16-byte loads (the build's rule where surface and pitch allow) against guarded dword loads",
                  "# (MPCVR_SHARPEN_STAGING=dword), rgb10a2 -> bgra8, alternating windows as in table 1",
                  "# size       r  mode  b128_us (min..max)      dword_us (min..max)     dword/b128"]
        for w, h in sizes:
            src, dst = smooth(w, h, 1), torch.empty((h, w), dtype=torch.int32, device="cuda")
            for radius in (1, 3):
                for mode in (0, 1):
                    run = pass_fn(src, 1, w, h, params_for(1, radius, mode), dst, 0)
                    t = {"b128": [], "dword": []}
                    for _ in range(a.repeats):
                        for k in t:
                            if k == "dword":
                                os.environ["MPCVR_SHARPEN_STAGING"] = "dword"
                            t[k].append(window(run))
                            os.environ.pop("MPCVR_SHARPEN_STAGING", None)
                    mb, md = float(np.median(t["b128"])), float(np.median(t["dword"]))
                    lines.append("%-10s %-2d %-5s %8.1f (%.1f..%.1f) %12.1f (%.1f..%.1f) %10.2f" % ("%dx%d" % (w, h), radius, "luma" if mode else "rgb", mb * 1e6, min(t["b128"]) * 1e6,
                                                                                              max(t["b128"]) * 1e6, md * 1e6, min(t["dword"]) * 1e6, max(t["dword"]) * 1e6, md / mb))
            del src, dst
            torch.cuda.empty_cache()

    if "3" in sections:
        n = a.batch
        ring = n + 16
        dp = api.sharpen_params_default(1)
        lines += ["#", "# 3. mpcvr_process_batch_sharpen (context output rgb10a2 with the dither off, targets bgra8, default parameters) against what it replaces; %d frames per call,"
                  % n, "# %d calls per window after %d warm-up calls, median of %d alternating windows (min .. max)" % (a.steps, a.batch_warmup, a.repeats),
                  "# a = mpcvr_process_batch + %d x mpcvr_sharpen_pass on a caller's stream (the bar); b = the new call on a caller's stream;" % n,
                  "# c = the new call on a context that owns its stream (batch lanes)",
                  "# workload  contender  chunks  launches  lanes    ms_per_call (min..max)        frames_per_s   vs_a"]
        caller = torch.cuda.Stream()
        legacy = torch.cuda.default_stream()
        for name in a.workloads.split(","):
            wl = dict(bench.WORKLOADS[name])
            w, h, s = wl["w"], wl["h"], wl["scale"]
            dw, dh = wl.get("dst", (w * s, h * s))
            extfmt = api.make_extfmt(**wl["ext"])
            settings = api.default_settings(iUpscaling=wl["iUpscaling"], iDownscaling=wl.get("iDownscaling", 2), output_format=1, bUseDither=0)

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

            vp_a, vp_b, vp_c = context(False), context(False), context(True)
            nbytes, pitch = vp_a.GetFrameBytes()
            gen = torch.Generator(device="cuda")
            gen.manual_seed(0x4D50)
            srcs = [bench.noise_frame_gpu(torch, wl, nbytes, pitch, gen) for _ in range(ring)]
            rgb = torch.empty((n, dh, dw, 4), dtype=torch.uint8, device="cuda")
            # two sets of targets, taken in turn call by call: consecutive calls of c write different memory, so the lanes may run them side by side
            outs = [torch.empty((n, dh, dw, 4), dtype=torch.uint8, device="cuda") for _ in range(2)]
            arr = C.c_void_p * n
            fb = dh * dw * 4
            da = [arr(*[o.data_ptr() + i * fb for i in range(n)]) for o in outs]
            sa = {k: arr(*[srcs[(k + j) % ring].data_ptr() for j in range(n)]) for k in range(0, ring, 16)}
            batches = {k: vp_a.PrepareBatch([srcs[(k + j) % ring] for j in range(n)], [rgb[i] for i in range(n)]) for k in sa}
            pass_args = [[(C.c_void_p(rgb[i].data_ptr()), dw * 4, 1, dw, dh, C.byref(dp), 7 + i, C.c_void_p(outs[k].data_ptr() + i * fb), dw * 4, 0,
                           C.c_void_p(caller.cuda_stream)) for i in range(n)] for k in range(2)]

            def call_a(i):
                vp_a.ProcessBatch(batches[(i * 16) % ring], None, dw * 4)
                for args in pass_args[i & 1]:
                    assert L.mpcvr_sharpen_pass(*args) == 0

            def call_new(vp):
                def call(i):
                    hr = L.mpcvr_process_batch_sharpen(vp._ctx, n, sa[(i * 16) % ring], C.byref(dp), 7, da[i & 1], dw * 4, 0)
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

            contenders = [("a", call_a, vp_a, caller), ("b", call_new(vp_b), vp_b, caller), ("c", call_new(vp_c), vp_c, legacy)]
            times = {c[0]: [] for c in contenders}
            infos = {}
            for _ in range(a.repeats):
                for cname, fn, vp, st in contenders:
                    times[cname].append(bwindow(fn, vp, st))
                    infos[cname] = vp.GetLastBatchInfo()
            base = float(np.median(times["a"]))
            for cname, _, _, _ in contenders:
                t = times[cname]
                m = float(np.median(t))
                info = infos[cname]
                launches = "%d" % (info["launches"] + n) if cname == "a" else "%d" % info["launches"]
                lanes = ",".join(str(x) for x in sorted(set(info.get("sharpen_lanes", [info["lane"]]))))
                lines.append("%-9s %-10s %6s %9s  %-7s %9.3f (%.3f..%.3f) %14.0f %6.3f"
                             % (name, cname, info.get("sharpen_chunks", "-"), launches, lanes, m * 1e3,
                                min(t) * 1e3, max(t) * 1e3, n / m, base / m))
            for vp in (vp_a, vp_b, vp_c):
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
