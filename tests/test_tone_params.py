"""The arguments of the tone curves, CPU half (tests/tone_params.py holds the table and the frame; tests/test_tone_params_gpu.py draws them).

  * the frame is what the module says it is, and the table means what it says: for every row and operator, branches() over the oracle's
    operator-off texture and the constants mpcvr_plan_hdr10_params sanitises lands on the row's labels, and every reachable branch of the
    HDR10 tone-mapping step is entered by some row with at least 64 pixels (channels for the saturate of operators 1 .. 4);
  * the two branches no row enters: ST 2094-10's MaxFALL alternative is unreachable behind the sanitiser whatever a caller passes; BT.2390's KS
    clamp needs a content peak beyond what a 16-bit HDR10 field carries (an assumption about callers, stated with its limit);
  * the oracle equals the reference's own shader text BIT FOR BIT (B, G, R of the render target) on every HDR10 / Dolby Vision row x six
    operators, same size (the step reads the convert output) and at 384 x 48 (it reads the post-scale surface), and on every SDR_NITS value x
    {PQ, HLG} -> SDR through the convert shader, same size and 2x: against the sha256 pins of tests/golden/tone_params_pins.json everywhere,
    and live where oracle/_ref/libref_hlsl.so is built;
  * mpcvr_create refuses 24 and 401 nits and does not refuse 25 and 400 (the settings are validated in front of the device; Configure on a
    live context, which must stay usable, is in tests/test_tone_params_gpu.py).

The operator-off texture of this frame holds 139 black pixels, 833 distinct grey codes and a largest code of 1023 (asserted); 204 pinned
cases, the oracle bit-identical to the reference text on all of them.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_hlsl"))

from tests import tone_params as T  # noqa: E402
from tests.golden.cases import oracle_params  # noqa: E402
from tests.golden.make_ref_hlsl_golden import rgb_channels  # noqa: E402

with open(os.path.join(HERE, "golden", "tone_params_pins.json")) as _f:
    _DOC = json.load(_f)
PINS = _DOC["cases"]
CASES = T.pin_cases()
FRAME, PITCH = T.frame()
MIN_POPULATION = 64


def sha(ch):
    return hashlib.sha256(ch.astype(np.uint16).tobytes()).hexdigest()


def oracle_rgb(oracle, c):
    a = oracle.process(oracle_params(oracle, c), FRAME, PITCH)
    if c.get("output_format", 0) == 1:
        a = a.view(np.uint32).reshape(a.shape[0], a.shape[1])
    return rgb_channels(a)


_TEX = {}


def texture(oracle, row):
    """the 10-bit texture the step reads on a same-size frame of the row: the oracle's frame with the operator off"""
    key = row["name"] if "dovi" in row else "hdr10"
    if key not in _TEX:
        _TEX[key] = T.texture_codes(oracle.process(oracle_params(oracle, T.hdr_case(row, 0)), FRAME, PITCH))
        _TEX[key].setflags(write=False)
    return _TEX[key]


def sanitised(mpcvr, meta, display, op):
    from videorenderer_amd import api
    out = (C.c_uint32 * 6)()
    assert api.load_library().mpcvr_plan_hdr10_params(*[float(x) for x in meta], float(display), int(op), out) == 0
    return T.constants(out)


# ---- the frame ----------------------------------------------------------------------------------------------------------------------
def test_frame_is_what_the_module_says(oracle):
    assert FRAME.size == T.PITCH * T.H * 3 // 2 and _DOC["frame_sha256"] == hashlib.sha256(FRAME.tobytes()).hexdigest()
    y = FRAME[:T.PITCH * T.H].view("<u2").reshape(T.H, T.W)
    uv = FRAME[T.PITCH * T.H:].view("<u2").reshape(T.H // 2, T.W // 2, 2)
    assert not (y & 63).any() and not (uv & 63).any()                            # P010: the code in the top ten bits
    y, uv = y >> 6, uv >> 6
    assert np.array_equal(np.bincount(y[:8].ravel(), minlength=1024), np.full(1024, 2)) and (uv[:4] == 512).all()
    corners = {(int(uv[r, x, 0]), int(uv[r, x, 1])) for r in range(4, 8) for x in (0, 63, 64, 127)}
    assert corners == set(T.CORNERS) and len(corners) == 8
    assert y[8:16].min() == 64 and y[8:16].max() == 940
    assert y[16:].min() <= 3 and y[16:].max() >= 1020 and uv[8:].min() <= 3 and uv[8:].max() >= 1020
    t = texture(oracle, T.HDR10_ROWS[0])
    black, grey, top = int((t.max(-1) == 0).sum()), len(np.unique(t[:8, :, 1])), int(t.max())
    print(f"TONE frame: operator-off texture has {black} black pixels, {grey} distinct grey codes, a largest code of {top}")
    # (luma codes 0 .. 64 twice = 130 black pixels, nine more in the noise rows; the convert maps the 1024 luma codes onto 833 grey codes)
    assert (black, grey, top) == (139, 833, 1023)


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def test_rows_enter_the_branches_they_are_labelled_with(oracle, mpcvr):
    reached = {}

    def note(branch, n):
        reached[branch] = max(reached.get(branch, 0), int(n))

    most = None
    for row in T.HDR10_ROWS:
        tex = texture(oracle, row)
        k = sanitised(mpcvr, row["meta"], row["display"], 5)
        b5 = T.branches(tex, k, 5)
        assert not b5["ks_clamped"], row["name"]
        assert tuple(n for n in ("inactive", "black", "below", "above") if b5[n]) == row["op5"], (row["name"], b5)
        for n in ("inactive", "black", "below", "above"):
            note("op5 " + n, b5[n])
        b6 = T.branches(tex, sanitised(mpcvr, row["meta"], row["display"], 6), 6)
        assert not b6["fall_alternative"], row["name"]
        assert ("inactive" if b6["inactive"] else "mapped") == row["op6"] and (b6["src"], b6["dst"]) == (row["src"], row["dst"]), (row["name"], b6)
        note("op6 inactive", b6["inactive"]); note("op6 zero", b6["zero"]); note("op6 mapped", b6["mapped"])
        if b6["mapped"]:
            note("op6 source knee " + b6["src"], b6["mapped"]); note("op6 destination knee " + b6["dst"], b6["mapped"])
        for op in (1, 2, 3, 4):
            b = T.branches(tex, sanitised(mpcvr, row["meta"], row["display"], op), op)
            assert b["eff"] == row["eff"] and abs(b["fall"] - row["fall"]) < 1e-6, (row["name"], op, b)
            assert (b["clipped"] == 0) == (row["clipped"] == "none"), (row["name"], op, b)
            note("op1-4 eff = " + b["eff"], b["unclipped"]); note("op1-4 fall " + ("< 1" if b["fall"] < 1 else "= 1"), b["unclipped"])
            note("op1-4 clipped", b["clipped"]); note("op1-4 unclipped", b["unclipped"])
            if most is None or b["clipped"] > most[1]:
                most = (row["name"], b["clipped"])
        print(f"TONE {row['name']:26s} op5 {b5}  op6 {b6}  op1-4 {b}")
    assert most[0] == next(r["name"] for r in T.HDR10_ROWS if r["clipped"] == "most"), most
    # a display peak outside 100 .. 10000 is drawn as 1000, every metadata fallback as labelled
    assert sanitised(mpcvr, T.ROWS_BY_NAME["display_out_of_range_50"]["meta"], 50.0, 5)["display"] == 1000.0
    k = sanitised(mpcvr, (0, 0, 0, 0), 100.0, 6)
    assert (k["min"], k["max"], k["cll"], k["fall"]) == (0.0, 1000.0, 1000.0, 1000.0)
    k = sanitised(mpcvr, T.ROWS_BY_NAME["no_cll_4000"]["meta"], 400.0, 6)
    assert (k["cll"], k["fall"]) == (4000.0, 4000.0)
    want = {"op5 inactive", "op5 black", "op5 below", "op5 above", "op6 inactive", "op6 zero", "op6 mapped", "op6 source knee low", "op6 source knee free",
            "op6 source knee high", "op6 destination knee free", "op6 destination knee high", "op1-4 eff = base", "op1-4 eff = cll", "op1-4 fall < 1",
            "op1-4 fall = 1", "op1-4 clipped", "op1-4 unclipped"}
    assert want <= set(reached), sorted(want - set(reached))
    thin = {b: n for b, n in reached.items() if b in want and n < MIN_POPULATION}
    assert not thin, thin


def test_dolby_vision_rows_reach_the_step_as_labelled(oracle, mpcvr):
    from videorenderer_amd import api, synth
    for row in T.DOVI_ROWS:
        pd = api.plan_dovi(synth.dovi_metadata(**row["dovi"]), int(row["display"]))
        assert bool(pd["l1_present"]) == row["l1"] and bool(pd["l2_enabled"]) == row["l2"], (row["name"], pd["l1_present"], pd["l2_enabled"])
        meta = row["meta"]
        if row["l1"]:                  # L1 min, max, max, avg in place of the HDR10 metadata; operator 5 becomes 6
            l1 = [float(x) for x in pd["l1_nits"]]
            meta = (l1[0], l1[1], l1[1], l1[2])
        tex = texture(oracle, row)
        b6 = T.branches(tex, sanitised(mpcvr, meta, row["display"], 6), 6)
        b5 = T.branches(tex, sanitised(mpcvr, meta, row["display"], 5), 5)
        print(f"TONE {row['name']}: metadata {meta}, op5 {b5}  op6 {b6}")
        assert b6["mapped"] >= MIN_POPULATION and b6["zero"] + b6["mapped"] == T.W * T.H, (row["name"], b6)
        assert b5["below"] >= MIN_POPULATION and b5["above"] >= MIN_POPULATION, (row["name"], b5)
        if row["l1"]:                  # the oracle's operator 5 IS its operator 6 on this row
            a, b = (oracle_rgb(oracle, T.hdr_case(row, op)) for op in (5, 6))
            assert np.array_equal(a, b)
            other = oracle_rgb(oracle, T.hdr_case(dict(row, dovi=dict(row["dovi"], l1=False)), 6))
            assert not np.array_equal(b, other), "level 1 does not reach the step"
        if row["l2"]:
            other = oracle_rgb(oracle, T.hdr_case(dict(row, dovi=dict(row["dovi"], l2=())), 6))
            assert not np.array_equal(oracle_rgb(oracle, T.hdr_case(row, 6)), other), "the level-2 trims do not reach the step"


def test_ks_clamp_needs_a_content_peak_no_hdr10_field_carries():
    """BT.2390's KS = max(0, 1.5 PQ(display) - 0.5 PQ(content)) stays positive for every sanitised display peak (100 .. 10000) and every content
    peak up to 65535 nits, the most a 16-bit MaxCLL / mastering field carries.  An assumption about callers, not something the library
    enforces: mpcvr_set_hdr_metadata takes floats and the sanitiser has no upper clamp, and the last lines show where the clamp does begin."""
    d = np.linspace(100.0, 10000.0, 2000)
    assert (np.diff(T.nits_to_pq(d)) > 0).all() and (np.diff(T.nits_to_pq(np.linspace(10.0, 65535.0, 2000))) > 0).all()      # PQ is increasing
    assert 1.5 * T.nits_to_pq(100.0) - 0.5 * T.nits_to_pq(65535.0) > 0.15
    assert (1.5 * T.nits_to_pq(d) - 0.5 * T.nits_to_pq(65535.0) > 0).all()
    assert 1.5 * T.nits_to_pq(100.0) - 0.5 * T.nits_to_pq(1e6) > 0 > 1.5 * T.nits_to_pq(100.0) - 0.5 * T.nits_to_pq(1e7)
    tex = np.full((1, 1, 3), 500)
    assert not T.branches(tex, dict(min=0.0, max=1000.0, cll=65535.0, fall=400.0, display=100.0), 5)["ks_clamped"]
    assert T.branches(tex, dict(min=0.0, max=1000.0, cll=1e7, fall=400.0, display=100.0), 5)["ks_clamped"]


def test_sanitised_constants_stay_in_their_ranges(mpcvr):
    """through mpcvr_plan_hdr10_params: no metadata leaves MaxFALL at or below 1 (ST 2094-10's `maxFALL > 0 ? ... :` alternative is unreachable
    whatever a caller passes), MaxCLL or the mastering peak at or below 10, the display outside 100 .. 10000 or the mastering black below 0;
    there is no upper clamp on the content peak, and with peaks a 16-bit field carries KS stays positive"""
    for meta in ((0, 0, 0, 0), (-1, -1, -1, -1), (0.005, 10, 10, 1), (5, 11, 10.5, 1.0000001), (0.005, 65535, 65535, 65535), (0, 5, 4000, 0.5),
                 (0, 0, 0, -1e9), (0, 0, 1e-30, 1e-30), (0, 1e7, 1e7, 0)):
        for display in (-1.0, 0.0, 50.0, 99.99, 100.0, 10000.0, 10000.5, 1e9):
            k = sanitised(mpcvr, meta, display, 6)
            assert k["fall"] > 1.0 and k["cll"] > 10.0 and k["max"] > 10.0 and 100.0 <= k["display"] <= 10000.0 and k["min"] >= 0.0, (meta, display, k)
            assert not T.branches(np.full((1, 1, 3), 500), k, 6)["fall_alternative"]
            if max(meta) <= 65535:
                assert not T.branches(np.full((1, 1, 3), 500), k, 5)["ks_clamped"], (meta, display)
    assert sanitised(mpcvr, (0, 1e7, 1e7, 0), 100.0, 5)["cll"] == 1e7            # (no upper clamp: the caller's to keep sane)


# ---- the oracle against the reference's shader text ----------------------------------------------------------------------------------
def test_every_case_is_pinned():
    """one pin per case, holding a hash and the case's settings and nothing else"""
    assert set(PINS) == set(CASES) and len(PINS) == (len(T.HDR10_ROWS) + len(T.DOVI_ROWS)) * 6 * 2 + len(T.SDR_NITS) * 2 * 2
    for key, p in PINS.items():
        assert set(p) == {"rgb_sha256", "case"} and p["case"] == json.loads(json.dumps(T.describe(CASES[key]))), key


def _groups():
    """(id, [keys]): the six operators of a row and geometry in one test; the nine nits values of a tail and geometry in one"""
    g = {}
    for key in CASES:
        part = key.split("/")
        g.setdefault("/".join(p for i, p in enumerate(part) if i != 2), []).append(key)
    return sorted(g.items())


@pytest.mark.parametrize("keys", [v for _, v in _groups()], ids=[k for k, _ in _groups()])
def test_oracle_against_recorded_reference_hlsl(oracle, keys):
    for key in keys:
        assert sha(oracle_rgb(oracle, CASES[key])) == PINS[key]["rgb_sha256"], f"{key}: the oracle is no longer bit-identical to the reference shader text"


def _live():
    import ref_hlsl
    if not ref_hlsl.available():
        pytest.skip("oracle/_ref/libref_hlsl.so not built (no reference tree here)")
    import ref_pipeline
    return ref_pipeline


@pytest.mark.parametrize("keys", [v for _, v in _groups()], ids=[k for k, _ in _groups()])
def test_oracle_against_live_reference_hlsl(oracle, keys):
    RP = _live()
    for key in keys:
        c = CASES[key]
        try:
            ref = rgb_channels(RP.process(oracle_params(oracle, c), FRAME, PITCH))
        except RuntimeError as e:
            if "is not built" in str(e):          # binaries that travelled without the reference tree: only the convert shaders built with them exist
                pytest.skip(str(e))
            raise
        assert sha(ref) == PINS[key]["rgb_sha256"], f"{key}: the reference-text result changed: regenerate tests/golden/tone_params_pins.json"
        d = np.abs(oracle_rgb(oracle, c) - ref)
        assert int(d.max()) == 0, (key, int(d.max()), int((d > 0).sum()))


def test_the_nits_and_the_rows_change_the_frame(mpcvr):
    """The pins are not copies of one frame.  Every nits value has a hash of its own; two rows share a frame through an operator exactly where the
    sanitised constants THAT operator reads are the same: operators 1 .. 4 read eff = min(max(display, mastering), MaxCLL), fall and the
    display; operator 5 the content peak and the display, or nothing behind its early return; operator 6 min, MaxCLL, MaxFALL and the display,
    or nothing."""
    for tail in T.SDR_TAILS:
        for geo in T.PIN_GEOMETRIES_SDR:
            assert len({PINS[f"sdr/{tail}/{n}nits/{geo}"]["rgb_sha256"] for n in T.SDR_NITS}) == len(T.SDR_NITS), (tail, geo)

    def reads(k, op):
        if op == 5:
            return "early return" if k["display"] >= k["cll"] else (k["cll"], k["display"])
        if op == 6:
            return "early return" if k["display"] >= k["cll"] else (k["min"], k["cll"], k["fall"], k["display"])
        base = max(k["display"], k["max"])
        return (min(base, k["cll"]), min(base / k["fall"], 1.0), k["display"])
    for op in T.OPERATORS:
        for geo in T.PIN_GEOMETRIES_HDR:
            by_key, by_hash = {}, {}
            for r in T.HDR10_ROWS:
                by_key.setdefault(reads(sanitised(mpcvr, r["meta"], r["display"], op), op), set()).add(r["name"])
                by_hash.setdefault(PINS[f"hdr10/{r['name']}/op{op}/{geo}"]["rgb_sha256"], set()).add(r["name"])
            assert sorted(map(sorted, by_key.values())) == sorted(map(sorted, by_hash.values())), (op, geo, by_key, by_hash)
    # the early return leaves the step a PQ round trip: the same frame through operators 5 and 6
    for r in T.HDR10_ROWS:
        if r["op6"] == "inactive":
            assert PINS[f"hdr10/{r['name']}/op5/same"]["rgb_sha256"] == PINS[f"hdr10/{r['name']}/op6/same"]["rgb_sha256"]


# ---- range refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nits,ok", [(24, False), (25, True), (400, True), (401, False)])
def test_create_refuses_nits_outside_25_to_400(mpcvr, nits, ok):
    """mpcvr_create validates the settings in front of the device: 24 and 401 are E_INVALIDARG with or without a GPU; 25 and 400 are not
    (without a GPU the call then fails for lack of a device, which is another code)."""
    from videorenderer_amd import api
    L = api.load_library()
    ctx = C.c_void_p()
    st = api.default_settings(iSDRDisplayNits=nits)
    hr = L.mpcvr_create(C.byref(st), 0, C.byref(ctx))
    if ctx.value:
        L.mpcvr_destroy(ctx)
    assert (hr != api.E_INVALIDARG) == ok, (nits, hex(hr & 0xffffffff))
    assert ok or not ctx.value
