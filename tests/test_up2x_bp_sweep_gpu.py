"""k_fused_up2x_bp at every launch its gate admits (the table of tests/up2x_bp_cases.py, which tests/test_up2x_bp_cases.py checks on the CPU).

Every `bp` row: the twin and the generic kernel (MPCVR_UP2X_NO_BP=1) report their forms and leave the same bytes — the rows and columns of
a first difference locate a lane or a seam — and the twin's frame is within the bars of tests/test_up2x_bp_gpu.py::against_oracle (8-bit
targets <= 1 code, 10-bit targets the limits of compare_rgb10).  Those bars carry a floor of 0.99 identical channels that was set on frames
of 40,000 channels and more: rows of 64 x 40 source pixels and more are held to it frame by frame, smaller ones to the code limit frame by
frame and to the floor POOLED per test (identical channels over all channels of the test's frames; the per-channel minimum on 10-bit
targets, as compare_rgb10 takes it).  The generic kernel's bytes are the same, so the pooled share is a property of the route, not of the
twin.  MPCVR_UP2X_BP_SWEEP_LOG=<file> appends every test's pool (profiles/r22/up2x_bp_sweep.txt).

Every `generic` / None row: the reported form and route, then the same bars.  Batches: frame i equals the single-frame draw of its
sample, twin == generic for all frames, and frames 32 and 33 — the first two past the by-value frame table — are compared by name.
"""
import os

import numpy as np
import pytest

from tests import up2x_bp_cases as T
from tests.golden.cases import case_frame, oracle_params
from tests.test_parity_gpu import BG, compare, compare_rgb10, has_tail, internal_is_8bit
from tests.test_up2x_bp_gpu import draw, twin_equals_generic

FLOOR = 0.99
DISTINCT = 3          # samples a batch cycles through


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


class Pool:
    """identical / all channels over the frames of one test"""

    def __init__(self, label):
        self.label, self.same, self.total, self.frames, self.small = label, np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64), 0, 0

    def add(self, oracle, c, got, what, seed_shift=0):
        """the frame against the oracle: the code limit (and, from 64 x 40 source pixels on, the floor) now, its channels into the pool"""
        cc = dict(c, seed=c["seed"] + seed_shift)
        frame, pitch = case_frame(cc)
        po = oracle_params(oracle, cc)
        want = oracle.process(po, frame, pitch, dst=np.full((po.window_h, po.window_w, 4), BG, dtype=np.uint8))
        floor = 0.0 if T.is_small(c) else FLOOR
        self.frames += 1
        self.small += T.is_small(c)
        if c.get("output_format", 0) == 1:
            compare_rgb10(got, want, what, tail=has_tail(c), internal8=internal_is_8bit(c), min_same=floor)
            g, w = got.view(np.uint32)[..., 0], want.view(np.uint32)[..., 0]
            for i, sh in enumerate((0, 10, 20)):
                self.same[i] += int((((g >> sh) & 1023) == ((w >> sh) & 1023)).sum())
                self.total[i] += g.size
        else:
            compare(got, want, what, min_same=floor)
            self.same[0] += int((got == want).sum())
            self.total[0] += got.size

    def close(self):
        used = self.total > 0
        assert used.any(), self.label
        share = float((self.same[used] / self.total[used]).min())
        line = f"{self.label}: frames {self.frames} ({self.small} below 64x40), channels {int(self.total.sum())}, pooled identical share {share:.5f}"
        print(line)
        if os.environ.get("MPCVR_UP2X_BP_SWEEP_LOG"):
            with open(os.environ["MPCVR_UP2X_BP_SWEEP_LOG"], "a") as f:
                f.write(line + "\n")
        assert share >= FLOOR, f"{self.label}: only {share:.5f} of the channels of the test's frames identical to the oracle's"


def layout_of(c):
    return {k: c[k] for k in ("sample_off", "target_off") if k in c}


def check_row(mpcvr, oracle, torch, c, pool):
    what = f"{c['name']} ({c['why']})"
    if c["form"] == "bp":
        twin = twin_equals_generic(mpcvr, torch, c, what, **layout_of(c))
        pool.add(oracle, c, twin[0], what + " [twin]")
        return
    (got,), info, form = draw(mpcvr, torch, c, False, **layout_of(c))
    assert form == c["form"], (c["name"], info, form)
    assert all(frag in info for frag in c["route"]) and not any(frag in info for frag in c["no_route"]), (c["name"], info, c["route"], c["no_route"])
    assert (info == "fused_up2x") == (c["form"] is not None), (c["name"], info, form)
    pool.add(oracle, c, got, f"{what} [{info}, {form}]")


def run_rows(mpcvr, oracle, torch, label, rows):
    pool = Pool(label)
    for c in rows:
        check_row(mpcvr, oracle, torch, c, pool)
    pool.close()


WIDTH_CHUNKS = [ch for g in T.GROUPS if g.startswith("widths_") for ch in T.chunks(g, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("label,rows", WIDTH_CHUNKS, ids=[l for l, _ in WIDTH_CHUNKS])
def test_widths(mpcvr, oracle, torch_cuda, label, rows):
    """H = 24 (one segment, 15 iterations): every lane 2 .. 63 owning the last block, lanes 62 / 63 in front of a 2- and a 4-column last strip,
    one to five strips; the headline widths at H = 8."""
    run_rows(mpcvr, oracle, torch_cuda, label, rows)


HEIGHT_CHUNKS = [ch for w in T.HEIGHT_WIDTHS for ch in T.chunks(f"heights_{w}", 13)]


@pytest.mark.gpu
@pytest.mark.parametrize("label,rows", HEIGHT_CHUNKS, ids=[l for l, _ in HEIGHT_CHUNKS])
def test_heights(mpcvr, oracle, torch_cuda, label, rows):
    """seams at rows 24 and 48, last segments of 2, 4, 6 .. 24 rows; H = 6 is refused"""
    run_rows(mpcvr, oracle, torch_cuda, label, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["rects", "settings", "refusals"])
def test_rects_settings_and_refusals(mpcvr, oracle, torch_cuda, group):
    run_rows(mpcvr, oracle, torch_cuda, group, T.rows_of(group))


_SINGLES = {}


def single_frames(mpcvr, torch, c):
    """the twin's single-frame draws of the batch samples of a geometry — computed once, shared by the batch rows, read-only"""
    key = (c["w"], c["h"], c["seed"])
    if key not in _SINGLES:
        outs = []
        for k in range(DISTINCT):
            (got,), info, form = draw(mpcvr, torch, dict(c, seed=c["seed"] + 1000 * k), False)
            assert info == "fused_up2x" and form == "bp", (c["name"], k, info, form)
            got.setflags(write=False)
            outs.append(got)
        assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2]) and not np.array_equal(outs[0], outs[2])
        _SINGLES[key] = outs
    return _SINGLES[key]


BATCH_ROWS = T.rows_of("batches")


@pytest.mark.gpu
@pytest.mark.parametrize("c", BATCH_ROWS, ids=[c["name"] for c in BATCH_ROWS])
def test_batches(mpcvr, oracle, torch_cuda, c):
    n = c["batch"]          # (the 33- and the 34-frame batch draw the same three samples: their single-frame draws are shared)
    what = f"{c['name']} ({c['why']})"
    twin = twin_equals_generic(mpcvr, torch_cuda, c, what, batch=n, distinct=DISTINCT)
    assert len(twin) == n
    singles = single_frames(mpcvr, torch_cuda, c)
    for i in range(n):
        assert np.array_equal(twin[i], singles[i % DISTINCT]), f"{what}: frame {i} of the batch differs from the single-frame draw of sample {i % DISTINCT}"
    if n > 32:            # by name: the frames past the 32 rows of the by-value table (a stale or zero table row would draw another sample, or nothing)
        assert np.array_equal(twin[32], singles[32 % DISTINCT]) and not np.array_equal(twin[32], twin[31]), what
        if n > 33:
            assert np.array_equal(twin[33], singles[33 % DISTINCT]) and not np.array_equal(twin[33], twin[32]), what
    pool = Pool(c["name"])
    for k in range(DISTINCT):
        pool.add(oracle, c, singles[k], f"{what} sample {k} [twin]", seed_shift=1000 * k)
    pool.close()
