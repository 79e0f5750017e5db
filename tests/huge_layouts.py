"""Frames whose rows span 2 GiB and 4 GiB: the guards of the fused kernels restated, pitches on either side of them, and one big device buffer
to lay tiny pictures out in (no GPU needed to import; tests/test_huge_layouts.py checks the arithmetic, tests/test_huge_layouts_gpu.py draws).

The fused kernels (load_raw, k_convert_stream, k_fused_up2x, k_fused_jinc2x, k_fused_strip, k_fused_period, k_convert_blocks) address a row as
base + (uint32_t)row * (uint32_t)pitch and carry the chroma plane offsets as uint32_t.  The host keeps them away from larger frames:

    G1  pitch[0] * (rect_t + out_h + 2) >= 2^32                       the sample's luma rows
    G2  plane_off[1] >= 2^31 or plane_off[2] >= 2^31                  the sample's chroma planes
    G3  dst_pitch * (max(off_y, 0) + out_h) >= 2^32                   the destination's rows (StoreRowsFit32, csrc/vp_params.h)
    G4  surf.pitch * surf.h >= 2^32                                   a context-owned surface: cannot be made large with a small picture

The library forms plane_off[1] = pitch * height for one-plane formats too (FillFusedParams), and rect_t + out_h <= height, so
pitch * (rect_t + out_h + 2) >= 2^32 implies pitch * height >= 2^32 * height / (height + 2) >= 2^31 for every height >= 2: for every sample
the API accepts G2 fires before G1, and the boundary a sample can be put on either side of is G2's 2^31 — reached first by plane_off[2], which
is formed for every format and is the larger sum (g2_pitches below).
"""
from tests.golden.cases import HDR10
from tests.sample_layouts import frame_bytes, row_bytes, sample_bytes
from tests.test_sample_layout_gpu import SDR, chroma_layout
from videorenderer_amd import synth

B31, B32 = 1 << 31, 1 << 32
LEAD = 1 << 31              # bytes of the allocation in front of the frame: a truncated 32-bit offset lands lower, a sign-extended one up to 2 GiB in front
LIMIT = 10 << 30            # no test holds more: the allocation and what assert_rest_intact needs beside it
CHECK_WORDS = 1 << 27       # 8-byte words assert_rest_intact compares at a time ...
CHECK_TEMP = CHECK_WORDS    # ... and the bytes their comparison's result takes (one per word)
INT32_MAX = (1 << 31) - 1


# ---- the guards, restated ------------------------------------------------------------------------------------------------------------
def g1(pitch, rect_t, out_h):
    return pitch * (rect_t + out_h + 2) >= B32


def g2(cformat, h, pitch):
    _, off1, off2 = chroma_layout(cformat, h, pitch)
    return off1 >= B31 or off2 >= B31


def g3(dst_pitch, off_y, out_h):
    return dst_pitch * (max(off_y, 0) + out_h) >= B32


def sample_excluded(c, pitch):
    """do G1 / G2 keep the fused kernels from a sample of case `c` at `pitch`?"""
    r = c.get("src_rect", (0, 0, c["w"], c["h"]))
    return g1(pitch, r[1], r[3] - r[1]) or g2(c["cformat"], c["h"], pitch)


def target_rows(c):
    """(rows G3 multiplies the pitch by, rows of the window that are drawn = the last row written + 1, rows of the window)"""
    w2, h2 = c["dst"]
    ww, wh = c.get("window", (w2, h2))
    oy = c.get("offset", (0, 0))[1]
    return max(oy, 0) + h2, min(oy + h2, wh), wh


# ---- pitches --------------------------------------------------------------------------------------------------------------------------
def legal_pitch(cformat, w, pitch):
    """the pitch rules of mpcvr_set_input (include/mpcvr.h)"""
    b = sample_bytes(cformat)
    ok = row_bytes(cformat, w) <= pitch <= INT32_MAX and pitch % {1: 1, 2: 2, 4: 4}[b] == 0
    if cformat in synth.FORMATS and synth.FORMATS[cformat][:2] == (3, 2):
        ok = ok and (pitch // synth.FORMATS[cformat][2]) % 2 == 0
    return ok


def _up16(v):
    return (v + 15) // 16 * 16


def _no_power_of_two(p):
    return p + 16 if p & (p - 1) == 0 else p


def pitch_under(rows, B):
    """the largest multiple of 16 with pitch * rows < B"""
    return (B - 1) // rows // 16 * 16


def pitch_at(rows, B):
    """the smallest multiple of 16 with pitch * rows >= B"""
    return _up16(-(-B // rows))


def pitch_over(rows, B, drawn=None):
    """about 1.25 x `at`, and large enough that at least 8 of the `drawn` rows (default: all of `rows`) start at or beyond B; no power of two, so
    a wrapped row lands in padding or in another row, never on itself"""
    drawn = rows if drawn is None else drawn
    assert drawn > 8
    p = _no_power_of_two(_up16(max(pitch_at(rows, B) * 5 // 4, -(-B // (drawn - 8)))))
    while not wrapped_rows_clear(p, drawn, B):
        p += 16
    return p


CLEAR = 4096        # bytes at either end of a row that a wrapped row keeps clear of: the pictures here are at most 3 x 1 KiB wide (BATCH_BASES)


def wrapped_rows_clear(pitch, drawn, B):
    """would every row of 0 .. drawn - 1 that starts at or beyond B, addressed modulo B, start in the padding of another row — at least CLEAR
    bytes behind that row's start and in front of the next one's?"""
    return all(CLEAR <= (r * pitch - B) % pitch <= pitch - CLEAR for r in range(drawn) if r * pitch >= B) and pitch & (pitch - 1) != 0


def pitch_beyond(height):
    """the sample side only: pitch * height about 1.1 x 2^32"""
    return _no_power_of_two(_up16(B32 * 11 // 10 // height))


def rows_beyond(pitch, drawn, B):
    """how many of the rows 0 .. drawn - 1 start at or beyond B"""
    return max(0, drawn - -(-B // pitch))


def pitch_of_class(cls, rows, B, drawn=None):
    return {"under": pitch_under(rows, B), "at": pitch_at(rows, B), "over": pitch_over(rows, B, drawn), "beyond": pitch_beyond(rows)}[cls]


def g2_pitches(cformat, h):
    """(the largest multiple of 16 G2 lets through, the smallest it stops): plane_off[2] = plane_off[1] + chroma pitch * chroma rows is formed for
    every format — the interleaved UV plane's end for two planes, twice pitch * height for one — and is the larger sum, so G2's SECOND clause is
    the effective boundary of every format: at the smallest pitch it stops, plane_off[1] is still below 2^31"""
    lo, hi = 0, pitch_at(h, B31) // 16          # (in units of 16 bytes; off2 grows with the pitch)
    assert not g2(cformat, h, 0) and g2(cformat, h, hi * 16)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if g2(cformat, h, mid * 16) else (mid, hi)
    return lo * 16, hi * 16


def sample_alloc(cformat, w, h, pitch):
    return LEAD + frame_bytes(cformat, w, h, pitch) + CHECK_TEMP


def target_alloc(pitch, window_rows, base=0):
    return LEAD + base + pitch * window_rows + CHECK_TEMP


# ---- the cases the GPU tests draw (tests/test_huge_layouts.py checks every (case, class) of these tables on the CPU) ---------------------------
def case(cformat, w, h, dst, seed, exfmt=SDR, **kw):
    return dict(cformat=cformat, w=w, h=h, kind="noise", seed=seed, dst=dst, exfmt=exfmt, **kw)


TARGET_CLASSES = ("under", "at", "over")
# name: (case, what GetVPInfo of the default tier names below the limit, does G3 exclude that kernel at and beyond it).  Not guarded: "direct:convert"
# names the per-pixel kernel too; in front of the HDR10 tone-mapping step and of the error-diffusion pass the fused kernels draw into a surface of
# the context's, and k_hdr10_tonemap / k_errdiff write the target through size_t.
TARGETS = {
    "up2x_lanczos3": (case(2, 64, 32, (128, 64), 1100, HDR10, iUpscaling=4), "fused_up2x", True),
    "up2x_mitchell": (case(2, 64, 32, (128, 64), 1101, HDR10, iUpscaling=1), "fused_up2x", True),
    "jinc2x": (case(2, 64, 32, (128, 64), 1102, SDR, iUpscaling=5), "fused_jinc2x", True),
    "period_3_2": (case(2, 64, 32, (96, 48), 1103, SDR, iUpscaling=4), "kernel=fused_period(", True),
    "strip_5_4": (case(2, 64, 32, (80, 40), 1104, SDR, iUpscaling=2), "kernel=fused_strip(", True),
    "direct_nv12_stream": (case(1, 64, 32, (64, 32), 1105), "direct:convert", False),            # 64 % 4 == 0: k_convert_stream (direct_kernel)
    "direct_nv12_blocks": (case(1, 70, 32, (70, 32), 1106), "direct:convert", False),            # 70 % 4 != 0: k_convert_blocks
    "direct_p010_pq_final": (case(2, 64, 32, (64, 32), 1107, HDR10), "direct:convert+final", False),
    "hdr_tonemap": (case(2, 64, 32, (96, 48), 1108, HDR10, iUpscaling=2, output_format=1, hdr_output=1, hdr_tonemap=2, hdr_display=800.0,
                         hdr_meta=(0.0, 4000.0, 2000.0, 300.0)), "kernel=fused_strip(", False),
    "errdiff": (case(2, 64, 32, (128, 64), 1109, HDR10, iUpscaling=1, bUseDither=2), "fused_up2x", False),
    # off_y counts in the product and lowers the pitch at which it bites
    "up2x_offset": (case(2, 64, 32, (128, 64), 1110, HDR10, iUpscaling=1, window=(140, 88), offset=(4, 20)), "fused_up2x", True),
    # rows above the window are never stored; the guard multiplies by max(off_y, 0) + out_h all the same, 51 rows are drawn
    "up2x_clipped": (case(1, 64, 32, (128, 64), 1111, SDR, iUpscaling=2, window=(90, 56), offset=(-20, -13)), "kernel=fused_strip(", True),
}
BATCH_ROUTES = ("up2x_lanczos3", "strip_5_4")
BATCH_CLASSES = ("under", "over")
BATCH_BASES = (0, 1024, 2048)                   # three targets side by side in the same huge-pitch rows
FAR_BASES = (0, B32 + 65536, 65536)             # ... and three tight targets more than 4 GiB apart in one allocation


def target_pitch(c, cls):
    rows, drawn, _ = target_rows(c)
    return pitch_of_class(cls, rows, B32, drawn)


# under / at: either side of the effective boundary (G2's second clause, g2_pitches); over: pitch * height about 1.25 x 2^31, plane_off[1] beyond
# 2^31 as well and 8 luma rows starting beyond it; beyond: pitch * height about 1.1 x 2^32
SAMPLE_CLASSES = ("under", "at", "over", "beyond")
# name: (case, what GetVPInfo of the default tier names below the limit, classes)
SAMPLES = {}
for _src, _cf, _ex in (("nv12", 1, SDR), ("p010", 2, HDR10)):
    SAMPLES[f"{_src}_up2x"] = (case(_cf, 64, 32, (128, 64), 1200 + _cf, _ex, iUpscaling=4), "fused_up2x", SAMPLE_CLASSES)
    SAMPLES[f"{_src}_period_3_2"] = (case(_cf, 64, 32, (96, 48), 1210 + _cf, _ex, iUpscaling=4), "kernel=fused_period(", SAMPLE_CLASSES)
    SAMPLES[f"{_src}_strip_5_4"] = (case(_cf, 64, 32, (80, 40), 1220 + _cf, _ex, iUpscaling=2), "kernel=fused_strip(", SAMPLE_CLASSES)
    SAMPLES[f"{_src}_same_size"] = (case(_cf, 64, 32, (64, 32), 1230 + _cf, _ex), "direct:convert", SAMPLE_CLASSES)
SAMPLES.update({
    "yuv420p10_third_plane": (case(20, 64, 32, (128, 64), 1240, SDR, iUpscaling=2), "fused_up2x", ("under", "at")),
    "yuy2_one_plane": (case(4, 64, 32, (128, 64), 1241, SDR, iUpscaling=2), "fused_up2x", ("under", "at")),
    "y410_one_plane": (case(12, 64, 32, (128, 64), 1242, SDR, iUpscaling=2), "fused_up2x", ("under", "at")),
    "p010_crop": (case(2, 64, 64, (128, 64), 1243, HDR10, iUpscaling=4, src_rect=(0, 32, 64, 64)), "fused_up2x", ("under", "at", "over")),
    # the repacks read the sample through size_t: both tiers against the oracle
    "rgb32_beyond": (case(30, 64, 32, (96, 48), 1244, 0, iUpscaling=2), "", ("beyond",)),
    "v210_beyond": (case(10, 64, 32, (128, 64), 1245, SDR, iUpscaling=2), "", ("beyond",)),
})


def sample_pitch(c, cls):
    if cls in ("under", "at"):
        return g2_pitches(c["cformat"], c["h"])[cls == "at"]
    return pitch_of_class(cls, c["h"], B31)


# standalone passes: a 64 x 16 surface of 32-bit texels whose rows span more than 4 GiB
PASS_W, PASS_H, PASS_PITCH = 64, 16, (1 << 28) + 64


# ---- the buffer ------------------------------------------------------------------------------------------------------------------------
class HugeBuffer:
    """One device allocation of LEAD + nbytes_frame bytes holding one byte value; the frame starts LEAD bytes in, on a 256-byte boundary.  Rows
    are written and read through as_strided views, so only the picture's bytes ever move between host and device."""

    def __init__(self, torch, nbytes_frame, fill):
        self.torch = torch
        self.total = LEAD + (nbytes_frame + 7) // 8 * 8
        assert self.total + CHECK_TEMP <= LIMIT, self.total
        torch.cuda.empty_cache()            # (nothing of an earlier test's stays cached beside it)
        self.buf = torch.empty(self.total, dtype=torch.uint8, device="cuda")
        assert (self.buf.data_ptr() + LEAD) % 256 == 0
        self.ptr = self.buf.data_ptr() + LEAD
        self.refill(fill)

    def refill(self, fill):
        self.fill = int(fill)
        self.buf.fill_(self.fill)

    def rows(self, offset, n_rows, n_bytes, pitch):
        """n_rows x n_bytes bytes, `pitch` apart, the first `offset` bytes behind the frame's start (a view)"""
        assert 0 <= offset and LEAD + offset + (n_rows - 1) * pitch + n_bytes <= self.total
        return self.buf.as_strided((n_rows, n_bytes), (pitch, 1), LEAD + offset)

    def read(self, view):
        return view.contiguous().cpu().numpy()

    def assert_rest_intact(self, views, what, pitch=None):
        """every byte outside the given row views still holds the fill value (the views are refilled first: read them before).  A reduction
        over an int64 view of the allocation — no second buffer of its size."""
        torch = self.torch
        for v in views:
            v.fill_(self.fill)
        K = int.from_bytes(bytes([self.fill]) * 8, "little", signed=True)
        words = self.buf.view(torch.int64)
        step = CHECK_WORDS
        # (in pieces of 1 GiB, so the comparison's result never takes more than CHECK_TEMP bytes beside the allocation; one read-back at the end)
        written = torch.zeros((), dtype=torch.bool, device="cuda")
        for s in range(0, words.numel(), step):
            written |= (words[s: s + step] != K).any()
        if not bool(written):
            return
        # name what was written (piece by piece: an index tensor of the whole allocation would be as large as it)
        found, n_bad = [], 0
        for s in range(0, words.numel(), step):
            bad = words[s: s + step] != K
            k = int(bad.sum())
            if k:
                n_bad += k
                if len(found) < 65536:
                    found += [(int(i) + s) * 8 - LEAD for i in torch.nonzero(bad).flatten()[:65536 - len(found)]]
            del bad
        # the first written word of every row of `pitch` bytes (or the first words, without a pitch)
        firsts = {}
        for off in found:
            firsts.setdefault(off // pitch if pitch and off >= 0 else off, off)
        where = [f"{-off} bytes in front of the frame" if off < 0 else f"row {off // pitch} from byte {off % pitch} of the row" if pitch else f"byte {off}"
                 for off in list(firsts.values())[:16]]
        rows = sorted(k for k, off in firsts.items() if pitch and off >= 0)
        if len(rows) == len(firsts) > 1 and rows == list(range(rows[0], rows[-1] + 1)) and len({off % pitch for off in firsts.values()}) == 1:
            where = [f"rows {rows[0]} .. {rows[-1]}, each from byte {found[0] % pitch} of the row"]
        raise AssertionError(f"{what}: {n_bad} 8-byte word(s) outside the picture's rows were written (pitch {pitch}), in {len(firsts)} place(s): " + "; ".join(where))

    def free(self):
        self.buf = None
        self.torch.cuda.empty_cache()
