"""How the same-size convert route (BatchRoute::DirectConvert, LaunchConvertBlocks) gets a batch's frame table: in the kernel arguments up
to the rows the kernel that takes the launch carries, through the table ring past that.

  * NV12 at a 16-byte-aligned pitch, samples and targets on 16-byte boundaries: the streaming kernel (k_convert_stream, 128 rows by value)
    takes the launch — batches of 1, 2, 32, 33, 128 and 129 frames;
  * YV12 (three 8-bit planes, 4:2:0): the block kernel (k_convert_blocks, 32 rows by value) — batches of 1, 2, 32 and 33 frames;
  * frames of 32 x 8 into a 32 x 8 window, two noise frames alternating; every target holds its frame's single Process draw, bit for bit;
  * launches and uploads of GetLastBatchInfo are literals: what the library reported for this very test before the launchers took their
    frames as one value (LaunchFrames) — one launch per batch, no table copy up to the kernel's rows and one past them.

MPCVR_NO_STREAM_CONVERT is read once per process and stays unset here: the format chooses the kernel.
"""
import numpy as np
import pytest

BG = 7
W, H = 32, 8
CF_NV12, CF_YV12 = 1, 14

# {case: {frames of the batch: (launches, uploads)}}
EXPECTED = {
    "nv12_streams": {1: (1, 0), 2: (1, 0), 32: (1, 0), 33: (1, 0), 128: (1, 0), 129: (1, 1)},
    "planar8_blocks": {1: (1, 0), 2: (1, 0), 32: (1, 0), 33: (1, 1)},
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.mark.gpu
@pytest.mark.parametrize("case,cformat", [("nv12_streams", CF_NV12), ("planar8_blocks", CF_YV12)], ids=["nv12_streams", "planar8_blocks"])
def test_batches_hold_their_single_draws_and_count_their_uploads(mpcvr, torch_cuda, case, cformat):
    from videorenderer_amd import api, synth
    torch = torch_cuda
    vp = api.VideoProcessor(api.default_settings(), device=0)
    vp.InitMediaType(cformat, W, H)
    vp.SetWindowRect((0, 0, W, H))
    vp.SetVideoRect((0, 0, W, H))
    frames = []
    for i in range(2):
        f, pitch = synth.make_frame(cformat, W, H, "noise", seed=8300 + i)
        frames.append(torch.from_numpy(np.ascontiguousarray(f)).cuda())
    assert pitch % 16 == 0 and all(f.data_ptr() % 16 == 0 for f in frames)

    def target():
        return torch.full((H, W, 4), BG, dtype=torch.uint8, device="cuda")

    singles = []
    for f in frames:
        dst = target()
        vp.CopySample(f, pitch)
        vp.Process(dst, W * 4)
        vp.Synchronize()
        singles.append(dst)
    assert vp.GetVPInfo().startswith("direct:convert"), vp.GetVPInfo()
    assert not torch.equal(singles[0], singles[1])
    assert not bool((singles[0][:, :, :3] == BG).all())
    for n, (launches, uploads) in EXPECTED[case].items():
        dsts = [target() for _ in range(n)]
        assert all(d.data_ptr() % 16 == 0 for d in dsts)
        vp.ProcessBatch([frames[i % 2] for i in range(n)], dsts, W * 4)
        vp.Synchronize()
        info = vp.GetLastBatchInfo()
        print(f"{case}: batch of {n}: {info}")
        assert vp.GetVPInfo().startswith("direct:convert"), vp.GetVPInfo()
        assert info["frames"] == n and info["launches"] == launches and info["uploads"] == uploads, (case, n, info)
        got = torch.stack(dsts)
        want = torch.stack([singles[i % 2] for i in range(n)])
        bad = (got != want).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, f"{case}: frames {bad[:8]} of a batch of {n} differ from their single draws [{info}]"
    vp.close()
