"""tools/bench_measure.py — what mpcvr_measure_pass (k_measure_maxrgb: the histogram of max(R, G, B) of a rendered RGB surface) sustains on
resident surfaces, and what the histograms cost a batch (mpcvr_process_batch_yuv_stats).

    python tools/bench_measure.py [--sections pass,sweep,batch] [--launches 200] [--warmup 20] [--repeats 5] [--out FILE]
                                  [--steps 6] [--batch-warmup 2] [--batch-repeats 3] [--workloads c3hdr,up1440] [--contenders s,p,h,sl,pl]

pass   3840x2160 and 7680x4320, BGRA8 and RGB10A2, four contents: uniform noise, ONE flat code (every lane of every wavefront adds to one
       bin: the contention worst case), a horizontal gradient, a frame the library rendered from bench.py's noise samples.  Payload = the
       surface's bytes read once.  Beside it, in the same process and alternating window by window: a device-to-device hipMemcpyAsync of
       that many bytes (it reads AND writes them) and mpcvr_encode_pass on the same surface (it reads the same bytes and writes 3/8 or
       3/4 as many on top).  A window is `launches` back-to-back calls between two device events after `warmup` calls; the median of
       `repeats` windows is reported with the spread (min .. max).
sweep  the noise and flat cases under MPCVR_MEASURE_WG_COLS = 256 / 512 / 1024 (the columns one workgroup walks; read once per process,
       so each value runs in a child process): the measurement behind the launcher's choice.
batch  bench.py's workloads, 32 frames per call: s = mpcvr_process_batch_yuv_stats, p = mpcvr_process_batch_yuv (both on a caller's
       stream), h = what a host had to do before (mpcvr_process_batch + n mpcvr_encode_pass + n mpcvr_measure_pass), sl / pl = s / p on a
       context that owns its stream (batch lanes).  With MPCVR_LIB naming an older library only the contenders it has run (p, pl): the
       parent's numbers, process by process.
Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BINS = 1024


def contents(torch, api, bench, w, h, src_fmt, quick):
    """name -> (h, w) int32 device surface"""
    bits = 10 if src_fmt else 8
    top = (1 << bits) - 1
    out = {}
    out["noise"] = torch.randint(-2 ** 31, 2 ** 31 - 1, (h, w), dtype=torch.int32, device="cuda")
    flat = 600 if src_fmt else 150
    out["flat"] = torch.full((h, w), flat | flat << bits | flat << (2 * bits), dtype=torch.int32, device="cuda")
    if quick:
        return out
    ramp = (torch.arange(w, dtype=torch.int64, device="cuda") * (top + 1) // w).to(torch.int32)
    out["gradient"] = (ramp | ramp << bits | ramp << (2 * bits)).repeat(h, 1).contiguous()
    # a frame rendered by the library from bench.py's noise samples: c3hdr (4K -> 8K) or up2160 (720p -> 4K)
    wl = dict(bench.WORKLOADS["c3hdr" if w == 7680 else "up2160"])
    s = wl["scale"]
    dw, dh = wl.get("dst", (wl["w"] * s, wl["h"] * s))
    assert (dw, dh) == (w, h)
    vp = api.VideoProcessor(api.default_settings(iUpscaling=wl["iUpscaling"], iDownscaling=wl.get("iDownscaling", 2), output_format=src_fmt,
                                                 bUseDither=wl.get("bUseDither", 1)))
    vp.InitMediaType(wl["cformat"], wl["w"], wl["h"], extfmt=api.make_extfmt(**wl["ext"]))
    vp.SetWindowRect((0, 0, w, h))
    vp.SetVideoRect((0, 0, w, h))
    nbytes, pitch = vp.GetFrameBytes()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x4D50)
    sample = bench.noise_frame_gpu(torch, wl, nbytes, pitch, gen)
    vp.CopySample(sample, pitch)
    rendered = torch.empty((h, w), dtype=torch.int32, device="cuda")
    vp.Process(rendered, w * 4)
    vp.Synchronize()
    vp.close()
    out["rendered"] = rendered
    return out


def section_pass(a, torch, api, bench, quick=False):
    L = api.load_library()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream
    sp = C.c_void_p(stream) if stream else None
    forced = os.environ.get("MPCVR_MEASURE_WG_COLS")
    lines = ["# mpcvr_measure_pass vs hipMemcpyAsync(device to device) of the same payload and mpcvr_encode_pass on the same surface; %d calls per window after %d warm-up,"
             % (a.launches, a.warmup),
             "# median of %d alternating windows (min .. max); payload = the surface read once (4 B/px); the copy reads AND writes that many bytes, the encode writes 3/8 (NV12) or 3/4 (P010) on top"
             % a.repeats,
             "# device: %s%s" % (torch.cuda.get_device_name(0), "; MPCVR_MEASURE_WG_COLS=" + forced if forced else ""),
             "# case                          content   payload_MB  measure_us  measure_GBps (min..max)     copy_us  copy_GBps   encode_us  encode_GBps  measure/copy  measure/encode"]

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

    hist = torch.zeros(BINS, dtype=torch.int32, device="cuda")
    ext = (5 << 8) | (2 << 12)                             # MPEG-2 siting, limited range
    rates = {}
    for w, h in ((3840, 2160), (7680, 4320)):
        for src_fmt, name in ((0, "bgra8"), (1, "rgb10a2")):
            payload = w * h * 4
            cf, bpc = (2, 2) if src_fmt else (1, 1)
            e = ext | ((4 if src_fmt else 1) << 15)
            y = torch.empty((h, w * bpc), dtype=torch.uint8, device="cuda")
            uv = torch.empty((h // 2, w * bpc), dtype=torch.uint8, device="cuda")
            b_buf = torch.empty(payload, dtype=torch.uint8, device="cuda")
            for cname, src in contents(torch, api, bench, w, h, src_fmt, quick).items():
                def mea():
                    hr = L.mpcvr_measure_pass(C.c_void_p(src.data_ptr()), w * 4, src_fmt, w, h, None, C.c_void_p(hist.data_ptr()), sp)
                    assert hr == 0, hr

                def cpy():
                    rc = hip.hipMemcpyAsync(C.c_void_p(b_buf.data_ptr()), C.c_void_p(src.data_ptr()), payload, 3, sp)
                    assert rc == 0, rc

                def enc():
                    hr = L.mpcvr_encode_pass(C.c_void_p(src.data_ptr()), w * 4, src_fmt, w, h, cf, e, C.c_void_p(y.data_ptr()), w * bpc,
                                             C.c_void_p(uv.data_ptr()), w * bpc, sp)
                    assert hr == 0, hr

                tm, tc, te = [], [], []
                for _ in range(a.repeats):          # alternating: all see the same neighbours on a shared machine
                    tm.append(window(mea))
                    if not quick:
                        tc.append(window(cpy))
                        te.append(window(enc))
                torch.cuda.synchronize()
                assert int(hist.to(torch.int64).sum()) == w * h, "the histogram does not hold every texel"
                g = lambda t: payload / t * 1e-9
                mm = float(np.median(tm))
                rates[(w, name, cname)] = mm
                if quick:
                    lines.append("%-10s %-8s %-9s %10.1f %10.1f %9.0f (%.0f..%.0f)" % ("%dx%d" % (w, h), name, cname, payload * 1e-6, mm * 1e6, g(mm), g(max(tm)), g(min(tm))))
                    continue
                mc, me = float(np.median(tc)), float(np.median(te))
                lines.append("%-10s %-8s %-9s %10.1f %10.1f %9.0f (%.0f..%.0f) %12.1f %9.0f %12.1f %9.0f %12.2f %12.2f"
                             % ("%dx%d" % (w, h), name, cname, payload * 1e-6, mm * 1e6, g(mm), g(max(tm)), g(min(tm)), mc * 1e6, g(mc), me * 1e6, g(me), mc / mm, me / mm))
    for (w, name, cname), t in sorted(rates.items()):
        if cname == "flat":
            lines.append("# contention, %d wide %s: flat takes %.2f x the time of noise" % (w, name, t / rates[(w, name, "noise")]))
    return lines


def section_sweep(a):
    lines = ["# the columns one workgroup walks (MPCVR_MEASURE_WG_COLS), one child process per value; the band is the header's kMeasureBandRows rows"]
    for cols in (256, 512, 1024):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sections", "quick", "--launches", str(a.launches), "--warmup", str(a.warmup),
                            "--repeats", str(a.repeats)], env=dict(os.environ, MPCVR_MEASURE_WG_COLS=str(cols)), capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit("bench_measure: the sweep's child for %d columns failed (%d):\n%s" % (cols, r.returncode, r.stderr[-2000:]))
        lines.append("## wg_cols = %d" % cols)
        lines += [l for l in r.stdout.splitlines() if l and not l.startswith("# mpcvr") and not l.startswith("# median") and not l.startswith("# case")]
    return lines


def section_batch(a, torch, api, bench):
    L = api.load_library()
    n = 32
    ring = n + 16
    have_stats = hasattr(L, "mpcvr_process_batch_yuv_stats") and hasattr(L, "mpcvr_measure_pass")
    wanted = [c for c in a.contenders.split(",") if have_stats or c in ("p", "pl")]
    lib = os.environ.get("MPCVR_LIB")
    lines = ["# the cost of statistics in a batch: %d frames per call, %d calls per window after %d warm-up calls, median of %d alternating windows (min .. max)"
             % (n, a.steps, a.batch_warmup, a.batch_repeats),
             "# s = mpcvr_process_batch_yuv_stats, p = mpcvr_process_batch_yuv (a caller's stream); h = mpcvr_process_batch + n mpcvr_encode_pass + n mpcvr_measure_pass;"
             " sl / pl = s / p on a context that owns its stream (batch lanes)",
             "# device: %s; library: %s" % (torch.cuda.get_device_name(0), "MPCVR_LIB (an older build: p / pl only)" if lib else "this build"),
             "# workload  formats         contender  chunks  launches    ms_per_call (min..max)        frames_per_s"]
    caller = torch.cuda.Stream()
    legacy = torch.cuda.default_stream()
    ext = lambda matrix: (5 << 8) | (2 << 12) | (matrix << 15)
    for name in a.workloads.split(","):
        wl = dict(bench.WORKLOADS[name])
        w, h, s = wl["w"], wl["h"], wl["scale"]
        dw, dh = wl.get("dst", (w * s, h * s))
        extfmt = api.make_extfmt(**wl["ext"])
        for src_fmt, cf, fname in ((0, 1, "bgra8->nv12"), (1, 2, "rgb10a2->p010")):
            bpc = 2 if cf == 2 else 1
            desc = ext(1 if cf == 1 else 4)
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

            ctx = {c: context(c in ("sl", "pl")) for c in wanted}
            any_vp = next(iter(ctx.values()))
            nbytes, pitch = any_vp.GetFrameBytes()
            gen = torch.Generator(device="cuda")
            gen.manual_seed(0x4D50)
            srcs = [bench.noise_frame_gpu(torch, wl, nbytes, pitch, gen) for _ in range(ring)]
            ys = [[torch.empty((dh, dw * bpc), dtype=torch.uint8, device="cuda") for _ in range(n)] for _ in range(2)]
            uvs = [[torch.empty((dh // 2, dw * bpc), dtype=torch.uint8, device="cuda") for _ in range(n)] for _ in range(2)]
            rows = [torch.zeros((n, BINS), dtype=torch.int32, device="cuda") for _ in range(2)]
            arr = C.c_void_p * n
            ya, uva = [arr(*[t.data_ptr() for t in s_]) for s_ in ys], [arr(*[t.data_ptr() for t in s_]) for s_ in uvs]
            sa = {k: arr(*[srcs[(k + j) % ring].data_ptr() for j in range(n)]) for k in range(0, ring, 16)}
            calls = {}
            if "h" in ctx:
                rgb = [torch.empty((dh, dw, 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
                batches = {k: ctx["h"].PrepareBatch([srcs[(k + j) % ring] for j in range(n)], rgb) for k in sa}
                cs = C.c_void_p(caller.cuda_stream)
                enc_args = [[(C.c_void_p(rgb[i].data_ptr()), dw * 4, src_fmt, dw, dh, cf, desc, C.c_void_p(ys[k][i].data_ptr()), dw * bpc,
                              C.c_void_p(uvs[k][i].data_ptr()), dw * bpc, cs) for i in range(n)] for k in range(2)]
                mea_args = [[(C.c_void_p(rgb[i].data_ptr()), dw * 4, src_fmt, dw, dh, None, C.c_void_p(rows[k][i].data_ptr()), cs) for i in range(n)] for k in range(2)]

                def call_h(i):
                    ctx["h"].ProcessBatch(batches[(i * 16) % ring], None, dw * 4)
                    for e_, m_ in zip(enc_args[i & 1], mea_args[i & 1]):
                        assert L.mpcvr_encode_pass(*e_) == 0 and L.mpcvr_measure_pass(*m_) == 0
                calls["h"] = call_h

            def plain(vp):
                def call(i):
                    hr = L.mpcvr_process_batch_yuv(vp._ctx, n, sa[(i * 16) % ring], cf, desc, ya[i & 1], dw * bpc, uva[i & 1], dw * bpc)
                    assert hr == 0, (hr, L.mpcvr_last_error(vp._ctx))
                return call

            def stats(vp):
                def call(i):
                    hr = L.mpcvr_process_batch_yuv_stats(vp._ctx, n, sa[(i * 16) % ring], cf, desc, ya[i & 1], dw * bpc, uva[i & 1], dw * bpc,
                                                         C.c_void_p(rows[i & 1].data_ptr()))
                    assert hr == 0, (hr, L.mpcvr_last_error(vp._ctx))
                return call

            for c in ctx:
                if c in ("p", "pl"):
                    calls[c] = plain(ctx[c])
                elif c in ("s", "sl"):
                    calls[c] = stats(ctx[c])

            def window(fn, vp, stream):
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

            times = {c: [] for c in ctx}
            infos = {}
            for _ in range(a.batch_repeats):
                for c in ctx:
                    times[c].append(window(calls[c], ctx[c], legacy if c in ("sl", "pl") else caller))
                    infos[c] = ctx[c].GetLastBatchInfo()
            torch.cuda.synchronize()
            if have_stats and ("s" in ctx or "sl" in ctx):
                assert bool((rows[0].to(torch.int64).sum(1) == dw * dh).all()), "a row of the batch does not hold every texel"
            for c in ctx:
                t = times[c]
                m = float(np.median(t))
                info = infos[c]
                launches = info["launches"] + (2 * n if c == "h" else 0)
                lines.append("%-9s %-15s %-10s %6s %9d %12.3f (%.3f..%.3f) %14.0f"
                             % (name, fname, c, info.get("yuv_chunks", "-"), launches, m * 1e3, min(t) * 1e3, max(t) * 1e3, n / m))
            for vp in ctx.values():
                vp.close()
            del srcs, ys, uvs, calls
            torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="pass,sweep,batch")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--batch-warmup", type=int, default=2)
    ap.add_argument("--batch-repeats", type=int, default=3)
    ap.add_argument("--workloads", default="c3hdr,up1440")
    ap.add_argument("--contenders", default="s,p,h,sl,pl")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from videorenderer_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("bench_measure: no GPU visible")
    lines = []
    for section in a.sections.split(","):
        if section == "pass":
            lines += section_pass(a, torch, api, bench)
        elif section == "quick":                            # (the sweep's children: noise and flat, the measure pass alone)
            lines += section_pass(a, torch, api, bench, quick=True)
        elif section == "sweep":
            lines += section_sweep(a)
        elif section == "batch":
            lines += section_batch(a, torch, api, bench)
        else:
            raise SystemExit("bench_measure: unknown section " + section)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
