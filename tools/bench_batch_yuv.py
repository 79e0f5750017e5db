"""tools/bench_batch_yuv.py — what a batch written as NV12 / P010 sustains (mpcvr_process_batch_yuv), beside what a host had to do before it
existed, in one process on resident samples.

    python tools/bench_batch_yuv.py [--steps 8] [--warmup 3] [--repeats 5] [--workloads c3hdr,up1440] [--out FILE]

Workloads are bench.py's own (c3hdr: 4K P010 PQ -> 8K; up1440: 1080p -> 1440p), 32 frames per call, BGRA8 -> NV12 and RGB10A2 -> P010, the
samples cycled through bench.py's ring (batch + 16 frames, beyond the 256 MiB cache), the planes through two sets taken in turn.  Contenders, alternating window by window:
    a          mpcvr_process_batch into 32 RGB targets, then 32 mpcvr_encode_pass calls on the same (caller's) stream — the bar
    b@<budget> mpcvr_process_batch_yuv on a caller's stream (everything in stream order), surface budget 256 MiB / 1 GiB / 4 GiB
    c@<budget> mpcvr_process_batch_yuv on a context that owns its stream (chunks on the two batch lanes), the same budgets
A window is `steps` calls after `warmup` calls, between two device events, ending in a synchronise; the median of `repeats` windows is
reported with the spread (min .. max).  The events of a and b are recorded on the caller's stream; those of c on the legacy default stream,
which the context's own (blocking) stream and its lanes order themselves against.  Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BUDGETS = (("256M", 256 << 20), ("1G", 1 << 30), ("4G", 4 << 30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--workloads", default="c3hdr,up1440")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from videorenderer_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("bench_batch_yuv: no GPU visible")
    L = api.load_library()
    n = a.batch
    ring = n + 16
    MPEG2, TV, M709, M2020 = 5, 2, 1, 4
    ext = lambda matrix: (MPEG2 << 8) | (TV << 12) | (matrix << 15)
    lines = ["# mpcvr_process_batch_yuv against mpcvr_process_batch + %d x mpcvr_encode_pass; %d frames per call, %d calls per window after %d warm-up calls,"
             % (n, n, a.steps, a.warmup),
             "# median of %d alternating windows (min .. max); device: %s" % (a.repeats, torch.cuda.get_device_name(0)),
             "# a = the composition on a caller's stream (the bar); b = the new call on a caller's stream; c = the new call on a context that owns its stream (batch lanes)",
             "# workload  formats         contender  chunks  launches  lanes    ms_per_call (min..max)        frames_per_s   vs_a"]
    caller = torch.cuda.Stream()
    legacy = torch.cuda.default_stream()
    for name in a.workloads.split(","):
        wl = dict(bench.WORKLOADS[name])
        w, h, s = wl["w"], wl["h"], wl["scale"]
        dw, dh = wl.get("dst", (w * s, h * s))
        extfmt = api.make_extfmt(**wl["ext"])
        for src_fmt, cf, fname in ((0, 1, "bgra8->nv12"), (1, 2, "rgb10a2->p010")):
            bpc = 2 if cf == 2 else 1
            desc = ext(M709 if cf == 1 else M2020)
            settings = api.default_settings(iUpscaling=wl["iUpscaling"], iDownscaling=wl.get("iDownscaling", 2), output_format=src_fmt, bUseDither=wl.get("bUseDither", 1))

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
            assert ring * nbytes > (256 << 20), "the ring of samples fits the cache"
            rgb = [torch.empty((dh, dw, 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
            # two sets of planes, taken in turn call by call (an encoder still reads one set while the next is written): consecutive calls
            # of c write different memory, so the lanes may run them side by side
            ys = [[torch.empty((dh, dw * bpc), dtype=torch.uint8, device="cuda") for _ in range(n)] for _ in range(2)]
            uvs = [[torch.empty((dh // 2, dw * bpc), dtype=torch.uint8, device="cuda") for _ in range(n)] for _ in range(2)]
            arr = C.c_void_p * n
            ya, uva = [arr(*[t.data_ptr() for t in s]) for s in ys], [arr(*[t.data_ptr() for t in s]) for s in uvs]
            sa = {k: arr(*[srcs[(k + j) % ring].data_ptr() for j in range(n)]) for k in range(0, ring, 16)}
            batches = {k: vp_a.PrepareBatch([srcs[(k + j) % ring] for j in range(n)], rgb) for k in sa}
            enc_args = [[(C.c_void_p(rgb[i].data_ptr()), dw * 4, src_fmt, dw, dh, cf, desc, C.c_void_p(ys[k][i].data_ptr()), dw * bpc,
                          C.c_void_p(uvs[k][i].data_ptr()), dw * bpc, C.c_void_p(caller.cuda_stream)) for i in range(n)] for k in range(2)]

            def call_a(i):
                vp_a.ProcessBatch(batches[(i * 16) % ring], None, dw * 4)
                for args in enc_args[i & 1]:
                    assert L.mpcvr_encode_pass(*args) == 0

            def call_yuv(vp):
                def call(i):
                    hr = L.mpcvr_process_batch_yuv(vp._ctx, n, sa[(i * 16) % ring], cf, desc, ya[i & 1], dw * bpc, uva[i & 1], dw * bpc)
                    assert hr == 0, (hr, L.mpcvr_last_error(vp._ctx))
                return call

            def window(fn, vp, stream):
                with torch.cuda.stream(stream):
                    for i in range(a.warmup):
                        fn(i)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for i in range(a.steps):
                        fn(a.warmup + i)
                    e1.record()
                    vp.Synchronize()
                    e1.synchronize()
                return e0.elapsed_time(e1) * 1e-3 / a.steps

            contenders = [("a", call_a, vp_a, caller, None)]
            for bname, budget in BUDGETS:
                contenders.append(("b@" + bname, call_yuv(vp_b), vp_b, caller, budget))
                contenders.append(("c@" + bname, call_yuv(vp_c), vp_c, legacy, budget))
            times = {c[0]: [] for c in contenders}
            infos = {}
            for _ in range(a.repeats):
                for cname, fn, vp, stream, budget in contenders:
                    if budget is not None:
                        vp.SetBatchYuvBudget(budget)
                    times[cname].append(window(fn, vp, stream))
                    infos[cname] = vp.GetLastBatchInfo()
            base = float(np.median(times["a"]))
            for cname, _, _, _, _ in contenders:
                t = times[cname]
                m = float(np.median(t))
                info = infos[cname]
                launches = info["launches"] + (n if cname == "a" else 0)
                lanes = ",".join(str(x) for x in sorted(set(info.get("yuv_lanes", [info["lane"]]))))
                lines.append("%-9s %-15s %-10s %6s %9d  %-7s %9.3f (%.3f..%.3f) %14.0f %6.3f"
                             % (name, fname, cname, info.get("yuv_chunks", "-"), launches, lanes, m * 1e3, min(t) * 1e3, max(t) * 1e3, n / m, base / m))
            for vp in (vp_a, vp_b, vp_c):
                vp.close()
            del srcs, rgb, ys, uvs, batches
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
