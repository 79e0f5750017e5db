"""tools/bench_lut3d.py — what the 3D LUT extension sustains on resident surfaces, in one process.

    python tools/bench_lut3d.py [--launches 200] [--warmup 20] [--repeats 5] [--steps 8] [--batch-warmup 3] [--batch 32] [--sections 1,2,3] [--out FILE]

1. mpcvr_lut3d_pass (k_lut3d) at 1920x1080, 3840x2160 and 7680x4320, n = 17, 33, 65, all four format pairs, on a noise frame (every texel
   in another cell of the table: the worst locality a table can see) and on a rendered test frame (neighbouring texels in the same or
   neighbouring cells), beside a device-to-device hipMemcpyAsync of the same number of bytes — the method of tools/bench_tensor.py: device
   events around `launches` back-to-back launches after `warmup` launches, `repeats` windows with the copy alternating, the median window
   and the spread.  Payload = the surface read + the surface written (8 bytes per texel); the copy reads AND writes that many bytes, so
   its own traffic is twice the pass's: the ratio compares time for the same payload.  The buffers stay resident between launches, so the
   last-level cache serves part of the traffic of the smaller frames for the pass and the copy alike (the 1080p pair is 16.6 MB).
2. The table in LDS against the table read from global memory, on the same table and frame, for the sizes that fit LDS (n = 9, 17, 21,
   27): MPCVR_LUT3D_TABLE=lds / global overrides the dispatcher's rule per launch.  This is the comparison behind the rule in vp_lut3d.h.
3. mpcvr_process_batch_lut3d, 32 frames per call, a 10-bit context (output_format RGB10A2) into BGRA8 targets through n = 33, for
   bench.py's up1440 (1080p -> 1440p) and c3hdr (4K P010 PQ -> 8K), alternating window by window:
       a   mpcvr_process_batch into 32 RGB targets, then 32 mpcvr_lut3d_pass calls, on a caller's stream — the bar
       b   mpcvr_process_batch_lut3d on a caller's stream (everything in stream order)
       c   mpcvr_process_batch_lut3d on a context that owns its stream (chunks on the two batch lanes)
Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FMT = {0: "bgra8", 1: "rgb10a2"}


def smooth_table(n):
    """a table with some colour in it: a gamma and a channel mix, nothing the pass could shortcut"""
    g = np.linspace(0.0, 1.0, n)
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")
    rgb = np.stack([0.8 * r ** 0.8 + 0.2 * gg, 0.9 * gg ** 1.1 + 0.1 * b, 0.7 * b ** 0.9 + 0.3 * r], axis=-1).reshape(-1, 3)
    return rgb.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--batch-warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--workloads", default="up1440,c3hdr")
    ap.add_argument("--sections", default="1,2,3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sections = set(a.sections.split(","))
    import torch
    import bench
    from videorenderer_amd import api, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_lut3d: no GPU visible")
    L = api.load_library()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lines = ["# device: %s; library: %s" % (torch.cuda.get_device_name(0), os.environ.get("MPCVR_LIB", "this build"))]
    stream = torch.cuda.current_stream().cuda_stream
    sp = C.c_void_p(stream) if stream else None
    tables = {n: torch.from_numpy(api.plan_lut3d_entries(smooth_table(n), n).view(np.int16)).cuda() for n in (9, 17, 21, 27, 33, 65)}

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

    def rendered(w, h, fmt):
        """a 1920x1080 NV12 test picture drawn into a w x h window of the format: what the pass meets behind mpcvr_render"""
        frame, pitch = synth.make_frame(1, 1920, 1080, "structure", seed=77)
        vp = api.VideoProcessor(api.default_settings(iUpscaling=2, output_format=fmt))
        vp.InitMediaType(1, 1920, 1080, extfmt=api.make_extfmt(matrix=1))
        vp.SetWindowRect((0, 0, w, h))
        vp.SetVideoRect((0, 0, w, h))
        out = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        vp.CopySample(torch.from_numpy(frame).cuda(), pitch)
        vp.Process(out, w * 4)
        vp.Synchronize()
        vp.close()
        return out

    def pass_fn(src, fmt, w, h, n, dst, dfmt):
        args = (C.c_void_p(src.data_ptr()), w * 4, fmt, w, h, C.c_void_p(tables[n].data_ptr()), n, C.c_void_p(dst.data_ptr()), w * 4, dfmt, sp)

        def run():
            hr = L.mpcvr_lut3d_pass(*args)
            assert hr == 0, hr
        return run

    sizes = ((1920, 1080), (3840, 2160), (7680, 4320))
    if "1" in sections:
        lines += ["# 1. mpcvr_lut3d_pass vs hipMemcpyAsync(device to device) of the same payload; %d launches per window after %d warm-up, median of %d windows (min .. max)"
                  % (a.launches, a.warmup, a.repeats),
                  "# payload = surface read + surface written (8 B/texel); the copy reads AND writes that many bytes; resident buffers: the last-level cache serves part of",
                  "# the traffic of the smaller frames, for the pass and the copy alike",
                  "# case                                        payload_MB    pass_us    pass_GBps (min..max)      copy_us  copy_GBps (min..max)        pass/copy"]
        ratios = {}
        for w, h in sizes:
            payload = 8 * w * h
            a_buf = torch.empty(payload, dtype=torch.uint8, device="cuda")
            b_buf = torch.empty(payload, dtype=torch.uint8, device="cuda")
            dst = torch.empty((h, w), dtype=torch.int32, device="cuda")

            def cpy():
                rc = hip.hipMemcpyAsync(C.c_void_p(b_buf.data_ptr()), C.c_void_p(a_buf.data_ptr()), payload, 3, sp)
                assert rc == 0, rc

            for fmt in (0, 1):
                frames = {"noise": torch.randint(-2 ** 31, 2 ** 31 - 1, (h, w), dtype=torch.int32, device="cuda"), "rendered": rendered(w, h, fmt)}
                for content, src in frames.items():
                    for n in (17, 33, 65):
                        for dfmt in (0, 1):
                            run = pass_fn(src, fmt, w, h, n, dst, dfmt)
                            tp, tc = [], []
                            for _ in range(a.repeats):          # alternating: both see the same neighbours on a shared machine
                                tp.append(window(run))
                                tc.append(window(cpy))
                            g = lambda t: payload / t * 1e-9
                            mp, mc = float(np.median(tp)), float(np.median(tc))
                            key = "%dx%d %s->%s n=%d %s" % (w, h, FMT[fmt], FMT[dfmt], n, content)
                            ratios[key] = mc / mp
                            lines.append("%-10s %-8s %-8s n=%-3d %-9s %12.1f %10.1f %9.0f (%.0f..%.0f) %12.1f %9.0f (%.0f..%.0f) %12.2f"
                                         % ("%dx%d" % (w, h), FMT[fmt], FMT[dfmt], n, content, payload * 1e-6, mp * 1e6, g(mp), g(max(tp)), g(min(tp)), mc * 1e6, g(mc),
                                            g(max(tc)), g(min(tc)), mc / mp))
                del frames
            del a_buf, b_buf, dst
            torch.cuda.empty_cache()
        for content in ("noise", "rendered"):
            r = [v for k, v in ratios.items() if k.endswith(content)]
            lines.append("# pass / copy (rate for the same payload), %s: %.2f .. %.2f over the %d cases, median %.2f" % (content, min(r), max(r), len(r), float(np.median(r))))

    if "2" in sections:
        lines += ["#", "# 2. the table in LDS against the table read from global memory (MPCVR_LUT3D_TABLE overrides the dispatcher's rule), rgb10a2 -> bgra8;",
                  "# %d launches per window after %d warm-up, median of %d alternating windows" % (a.launches, a.warmup, a.repeats),
                  "# case                               lds_us (min..max)        global_us (min..max)      global/lds"]
        for w, h in sizes:
            dst = torch.empty((h, w), dtype=torch.int32, device="cuda")
            for content, src in (("noise", torch.randint(-2 ** 31, 2 ** 31 - 1, (h, w), dtype=torch.int32, device="cuda")), ("rendered", rendered(w, h, 1))):
                for n in (9, 17, 21, 27):
                    run = pass_fn(src, 1, w, h, n, dst, 0)
                    t = {"lds": [], "global": []}
                    for _ in range(a.repeats):
                        for place in ("lds", "global"):
                            os.environ["MPCVR_LUT3D_TABLE"] = place
                            t[place].append(window(run))
                    os.environ.pop("MPCVR_LUT3D_TABLE", None)
                    ml, mg = float(np.median(t["lds"])), float(np.median(t["global"]))
                    lines.append("%-10s n=%-3d %-9s %12.1f (%.1f..%.1f) %14.1f (%.1f..%.1f) %12.2f"
                                 % ("%dx%d" % (w, h), n, content, ml * 1e6, min(t["lds"]) * 1e6, max(t["lds"]) * 1e6, mg * 1e6, min(t["global"]) * 1e6,
                                    max(t["global"]) * 1e6, mg / ml))
            del dst
            torch.cuda.empty_cache()

    if "3" in sections:
        n = a.batch
        ring = n + 16
        lut_n = 33
        lines += ["#", "# 3. mpcvr_process_batch_lut3d (context output rgb10a2, targets bgra8, n = %d) against what it replaces; %d frames per call, %d calls per window after %d"
                  % (lut_n, n, a.steps, a.batch_warmup),
                  "# warm-up calls, median of %d alternating windows (min .. max)" % a.repeats,
                  "# a = mpcvr_process_batch + %d x mpcvr_lut3d_pass on a caller's stream (the bar); b = the new call on a caller's stream;" % n,
                  "# c = the new call on a context that owns its stream (batch lanes)",
                  "# workload  contender  chunks  launches  lanes    ms_per_call (min..max)        frames_per_s   vs_a"]
        caller = torch.cuda.Stream()
        legacy = torch.cuda.default_stream()
        lut = tables[lut_n]
        for name in a.workloads.split(","):
            wl = dict(bench.WORKLOADS[name])
            w, h, s = wl["w"], wl["h"], wl["scale"]
            dw, dh = wl.get("dst", (w * s, h * s))
            extfmt = api.make_extfmt(**wl["ext"])
            settings = api.default_settings(iUpscaling=wl["iUpscaling"], iDownscaling=wl.get("iDownscaling", 2), output_format=1, bUseDither=wl.get("bUseDither", 1))

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
            pass_args = [[(C.c_void_p(rgb[i].data_ptr()), dw * 4, 1, dw, dh, C.c_void_p(lut.data_ptr()), lut_n, C.c_void_p(outs[k].data_ptr() + i * fb), dw * 4, 0,
                           C.c_void_p(caller.cuda_stream)) for i in range(n)] for k in range(2)]

            def call_a(i):
                vp_a.ProcessBatch(batches[(i * 16) % ring], None, dw * 4)
                for args in pass_args[i & 1]:
                    assert L.mpcvr_lut3d_pass(*args) == 0

            def call_new(vp):
                def call(i):
                    hr = L.mpcvr_process_batch_lut3d(vp._ctx, n, sa[(i * 16) % ring], C.c_void_p(lut.data_ptr()), lut_n, da[i & 1], dw * 4, 0)
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
                lanes = ",".join(str(x) for x in sorted(set(info.get("lut3d_lanes", [info["lane"]]))))
                lines.append("%-9s %-10s %6s %9s  %-7s %9.3f (%.3f..%.3f) %14.0f %6.3f"
                             % (name, cname, info.get("lut3d_chunks", "-"), launches, lanes, m * 1e3, min(t) * 1e3, max(t) * 1e3, n / m, base / m))
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
