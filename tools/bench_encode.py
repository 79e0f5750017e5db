"""tools/bench_encode.py — what mpcvr_encode_pass (k_encode420: a rendered RGB surface written as NV12 / P010) sustains on resident surfaces,
beside a device-to-device hipMemcpyAsync of the same number of bytes in the same process.

    python tools/bench_encode.py [--launches 200] [--warmup 20] [--repeats 5] [--out FILE]

Per case (3840x2160 and 7680x4320; BGRA8 -> NV12 and RGB10A2 -> P010; centre and left siting): device events around `launches`
back-to-back launches after `warmup` launches, repeated `repeats` times with the copy alternating; the median window is reported and the
spread (min .. max) beside it.  Bytes moved = the surface read once (4 bytes per pixel) + both planes written (1.5 or 3 bytes per pixel);
the copy moves that many bytes (it reads and writes each, so its own traffic is twice that: the ratio compares time for the same payload,
not bus traffic — stated in the output).  Needs a GPU: there is no CPU fallback."""
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from videorenderer_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("bench_encode: no GPU visible")
    L = api.load_library()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream
    sp = C.c_void_p(stream) if stream else None
    MPEG1, MPEG2, TV, M709, M2020 = 1, 5, 2, 1, 4
    ext = lambda chroma, matrix: (chroma << 8) | (TV << 12) | (matrix << 15)
    lines = ["# mpcvr_encode_pass vs hipMemcpyAsync(device to device) of the same payload; %d launches per window after %d warm-up, median of %d windows (min .. max)"
             % (a.launches, a.warmup, a.repeats),
             "# device: %s" % torch.cuda.get_device_name(0),
             "# payload = surface read (4 B/px) + planes written (1.5 B/px NV12, 3 B/px P010); the copy reads AND writes that many bytes",
             "# case                              payload_MB  encode_us  encode_GBps (min..max)      copy_us  copy_GBps (min..max)      encode/copy"]

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

    ratios = []
    for w, h in ((3840, 2160), (7680, 4320)):
        for src_fmt, cf, name in ((0, 1, "bgra8->nv12"), (1, 2, "rgb10a2->p010")):
            bpc = 2 if cf == 2 else 1
            src = torch.randint(0, 2 ** 31 - 1, (h, w), dtype=torch.int32, device="cuda")
            y = torch.empty((h, w * bpc), dtype=torch.uint8, device="cuda")
            uv = torch.empty((h // 2, w * bpc), dtype=torch.uint8, device="cuda")
            payload = w * h * 4 + w * h * bpc * 3 // 2
            a_buf = torch.empty(payload, dtype=torch.uint8, device="cuda")
            b_buf = torch.empty(payload, dtype=torch.uint8, device="cuda")
            for chroma, sname in ((MPEG1, "centre"), (MPEG2, "left")):
                e = ext(chroma, M709 if cf == 1 else M2020)

                def enc():
                    hr = L.mpcvr_encode_pass(C.c_void_p(src.data_ptr()), w * 4, src_fmt, w, h, cf, e, C.c_void_p(y.data_ptr()), w * bpc,
                                             C.c_void_p(uv.data_ptr()), w * bpc, sp)
                    assert hr == 0, hr

                def cpy():
                    rc = hip.hipMemcpyAsync(C.c_void_p(b_buf.data_ptr()), C.c_void_p(a_buf.data_ptr()), payload, 3, sp)
                    assert rc == 0, rc

                te, tc = [], []
                for _ in range(a.repeats):          # alternating: both see the same neighbours on a shared machine
                    te.append(window(enc))
                    tc.append(window(cpy))
                g = lambda t: payload / t * 1e-9
                me, mc = float(np.median(te)), float(np.median(tc))
                ratios.append(mc / me)
                lines.append("%-12s %-14s %-7s %10.1f %10.1f %9.0f (%.0f..%.0f) %12.1f %9.0f (%.0f..%.0f) %10.2f"
                             % ("%dx%d" % (w, h), name, sname, payload * 1e-6, me * 1e6, g(me), g(max(te)), g(min(te)), mc * 1e6, g(mc), g(max(tc)), g(min(tc)),
                                mc / me))
    lines.append("# encode / copy (rate for the same payload): %.2f .. %.2f over the cases, median %.2f" % (min(ratios), max(ratios), float(np.median(ratios))))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
