"""How the exact-2x fused kernel (k_fused_up2x) gets its read-only inputs: the table image baked per plan and the frame table by value.

  * the image mpcvr_get_fused_tables hands out equals, bit for bit, what the kernel's own staging loops compute from the dither table
    (videorenderer_amd/data/dither32x32float16.bin) and the context's tone-map table:
        D[i]  = the fp16 bits,   Di[i] = (uint32_t)(half(d) * 1024.0f + 0.5f) << 14,   T[i] = {lut[i], lut[min(i + 1, 4095)] - lut[i]}
  * a P010 PQ frame, 256 columns (three 120-column strips, the last one 16 columns wide), drawn as single frames and as batches of 1, 2,
    32 and 33 frames: batches of up to 32 carry their frame table in the kernel arguments (GetLastBatchInfo: uploads=0), 33 frames take
    the uploaded table (uploads=1); every draw of a frame holds the same bytes;
  * the same at 128 rows with MPCVR_FUSED_SEG=24 (six segments, the last one 8 rows), and with MPCVR_FUSED_NO_BAKED=1 (the kernel's own
    staging loops): both are read once per process, so a child process draws and the bytes are compared here.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.golden.cases import HDR10, HLG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG = 7
LUT_N = 4096
W = 256


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def make_vp(api, h, extfmt=HDR10):
    vp = api.VideoProcessor(api.default_settings(iUpscaling=4), device=0)
    vp.InitMediaType(2, W, h, extfmt=extfmt)
    vp.SetWindowRect((0, 0, 2 * W, 2 * h))
    vp.SetVideoRect((0, 0, 2 * W, 2 * h))
    return vp


def expected_image(dither_bits, lut):
    d = np.asarray(dither_bits, dtype=np.uint16)
    x = d.view(np.float16).astype(np.float32) * np.float32(1024.0) + np.float32(0.5)
    di = x.astype(np.uint32) << np.uint32(14)
    t = np.zeros((LUT_N, 2), dtype=np.float32)
    if lut is not None:
        lut = np.asarray(lut, dtype=np.float32)
        t[:, 0] = lut
        t[:, 1] = lut[np.minimum(np.arange(LUT_N) + 1, LUT_N - 1)] - lut
    return d.tobytes() + di.astype("<u4").tobytes() + t.tobytes()


@pytest.mark.gpu
def test_baked_image_is_what_the_staging_loops_compute(mpcvr, torch_cuda):
    from videorenderer_amd import api
    dither = np.fromfile(os.path.join(ROOT, "videorenderer_amd", "data", "dither32x32float16.bin"), dtype="<u2")
    assert dither.size == 1024
    # PQ -> SDR: the table the context broadcasts in its parameter blob (its last 4096 floats, behind the dither table)
    vp = make_vp(api, 64)
    blob = vp.GetParamBlob()
    lut = np.frombuffer(blob[-4 * LUT_N:], dtype="<f4")
    assert np.array_equal(np.frombuffer(blob[-4 * LUT_N - 2048:-4 * LUT_N], dtype="<u2"), dither)
    assert lut.min() >= 0.0 and lut.max() > 0.5          # a tone curve, not zeros
    img = vp.GetFusedTables()
    vp.close()
    assert len(img) == 2048 + 4096 + 8 * LUT_N
    assert img == expected_image(dither, lut)
    # no tone-map table in the plan (SDR): dither parts alone, zeros behind them
    vp = make_vp(api, 64, extfmt=0)
    sdr = vp.GetFusedTables()
    vp.close()
    assert sdr == expected_image(dither, None)
    # HLG -> SDR: the table is not handed out anywhere else; its image must still be {value, next - value} pairs of one curve
    vp = make_vp(api, 64, extfmt=HLG)
    hlg = vp.GetFusedTables()
    vp.close()
    assert hlg[:6144] == img[:6144]
    t = np.frombuffer(hlg[6144:], dtype="<f4").reshape(LUT_N, 2)
    assert t[:, 0].max() > 0.5
    assert hlg == expected_image(dither, t[:, 0])


def draw_every_way(api, torch, h):
    """Two noise frames of W x h, each drawn alone (the first one twice), then as batches of 1, 2, 32 and 33 frames that alternate between
    them.  Every target must hold its frame's single draw.  Returns the first frame's bytes."""
    from videorenderer_amd import synth
    vp = make_vp(api, h)
    frames = []
    for i in range(2):
        f, pitch = synth.make_frame(2, W, h, "noise", seed=8100 + i)
        frames.append(torch.from_numpy(np.ascontiguousarray(f)).cuda())
    ww, wh = 2 * W, 2 * h

    def target():
        return torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")

    singles = []
    for f in (frames[0], frames[1], frames[0]):
        dst = target()
        vp.CopySample(f, pitch)
        vp.Process(dst, ww * 4)
        vp.Synchronize()
        singles.append(dst)
    assert vp.GetVPInfo() == "fused_up2x"
    assert torch.equal(singles[0], singles[2])
    assert not torch.equal(singles[0], singles[1])
    assert not bool((singles[0][:, :, :3] == BG).all())
    for n in (1, 2, 32, 33):
        dsts = [target() for _ in range(n)]
        vp.ProcessBatch([frames[i % 2] for i in range(n)], dsts, ww * 4)
        vp.Synchronize()
        info = vp.GetLastBatchInfo()
        assert info["frames"] == n and (n == 1 or info["launches"] == 1), (n, info)
        assert info["uploads"] == (1 if n > 32 else 0), (n, info)
        for i in range(n):
            assert torch.equal(dsts[i], singles[i % 2]), f"{W}x{h}: frame {i} of a batch of {n} differs from its single draw [{info}]"
    out = singles[0].cpu().numpy()
    vp.close()
    return out


@pytest.fixture(scope="module")
def rows128(mpcvr, torch_cuda):
    from videorenderer_amd import api
    out = draw_every_way(api, torch_cuda, 128)
    out.setflags(write=False)
    return out


def draw_in_child(tmp_path, h, env):
    out = os.path.join(str(tmp_path), "child.npy")
    code = ("import os, sys\nsys.path.insert(0, os.getcwd())\nimport numpy as np\nimport torch\nfrom videorenderer_amd import api\nimport tests.test_up2x_entry as t\n"
            f"np.save({out!r}, t.draw_every_way(api, torch, {h}))\nprint('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    return np.load(out)


@pytest.mark.gpu
def test_single_frames_and_batches_hold_the_same_bytes(mpcvr, torch_cuda):
    from videorenderer_amd import api
    draw_every_way(api, torch_cuda, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"MPCVR_FUSED_SEG": "24"}, {"MPCVR_FUSED_NO_BAKED": "1"}], ids=["seg24", "own_staging_loops"])
def test_segments_and_staging_do_not_change_the_bytes(mpcvr, rows128, tmp_path, env):
    """128 rows: six 24-row segments (the last one 8 rows) against the launcher's own choice, the baked image against the kernel's loops."""
    there = draw_in_child(tmp_path, 128, env)
    assert np.array_equal(rows128, there), env
