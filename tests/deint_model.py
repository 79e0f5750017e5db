"""The numpy twin of the deinterlacing pass (include/mpcvr.h: mpcvr_deint_pass): the text of the header executed line by line in int64.

deint_plane      one plane (lines x comps unsigned integers) -> the plane, optionally with the side outputs the tests assert on
deint_sample     a whole sample (bytes) through the plane table of api.plan_deint_planes
field_parity     keep, first of a field of a frame (mpcvr_copy_sample_fields)
"""
import numpy as np


def deint_plane(prev, cur, nxt, keep, first, mode, cs=1, mask=None, info=None):
    """prev, cur, nxt: 2-D integer arrays (lines x comps).  keep: parity of the kept lines.  first: the kept field is the temporally first
    field of cur.  mode 0: with the interlacing check, 1: without.  cs: the horizontal neighbour step.  mask: applied on load.
    info (a dict, optional) collects over calls: 'dir' the count of missing components per chosen direction -2 .. 2; 'band_lo' / 'band_hi'
    the components the temporal band raised / lowered to its edge; 'check_raised' those whose diff the interlacing check raised."""
    P, C, N = (np.asarray(a).astype(np.int64) for a in (prev, cur, nxt))
    if mask is not None:
        P, C, N = P & mask, C & mask, N & mask
    L, W = C.shape
    assert L >= 2 and W >= cs and W % cs == 0
    out = C.copy()
    A, B = (P, C) if first else (C, N)          # the frames holding the missing-parity field before / after the shown field
    xs = np.arange(W)
    lo, hi = xs % cs, W - cs + xs % cs

    def col(row, k):
        return row[np.clip(xs + k * cs, lo, hi)]

    for y in range(L):
        if (y & 1) == keep:
            continue
        ym = y - 1 if y - 1 >= 0 else y + 1
        yp = y + 1 if y + 1 < L else y - 1
        up, dn = C[ym], C[yp]
        c, e = up, dn
        d = (A[y] + B[y]) >> 1
        t0 = np.abs(A[y] - B[y])
        t1 = (np.abs(P[ym] - c) + np.abs(P[yp] - e)) >> 1
        t2 = (np.abs(N[ym] - c) + np.abs(N[yp] - e)) >> 1
        diff = np.maximum(np.maximum(t0 >> 1, t1), t2)

        def score(j):
            return sum(np.abs(col(up, k + j) - col(dn, k - j)) for k in (-1, 0, 1))

        def pred(j):
            return (col(up, j) + col(dn, -j)) >> 1

        best, sp = score(0) - 1, pred(0)
        chosen = np.zeros(W, dtype=np.int64)
        for s in (-1, 1):
            s1 = score(s)
            ok1 = s1 < best
            best, sp, chosen = np.where(ok1, s1, best), np.where(ok1, pred(s), sp), np.where(ok1, s, chosen)
            s2 = score(2 * s)
            ok2 = ok1 & (s2 < best)
            best, sp, chosen = np.where(ok2, s2, best), np.where(ok2, pred(2 * s), sp), np.where(ok2, 2 * s, chosen)
        raised = np.zeros(W, dtype=bool)
        if mode == 0 and y - 2 >= 0 and y + 2 < L:
            b = (A[y - 2] + B[y - 2]) >> 1
            f = (A[y + 2] + B[y + 2]) >> 1
            mx = np.maximum(np.maximum(d - e, d - c), np.minimum(b - c, f - e))
            mn = np.minimum(np.minimum(d - e, d - c), np.maximum(b - c, f - e))
            wider = np.maximum(np.maximum(diff, mn), -mx)
            raised = wider > diff
            diff = wider
        assert (diff >= 0).all()
        out[y] = np.minimum(np.maximum(sp, d - diff), d + diff)
        if info is not None:
            dirs = info.setdefault("dir", {j: 0 for j in (-2, -1, 0, 1, 2)})
            for j in dirs:
                dirs[j] += int((chosen == j).sum())
            info["band_lo"] = info.get("band_lo", 0) + int((sp < d - diff).sum())
            info["band_hi"] = info.get("band_hi", 0) + int((sp > d + diff).sum())
            info["check_raised"] = info.get("check_raised", 0) + int(raised.sum())
    return out


def noise(lines, comps, nbytes, seed):
    """three planes of noise whose neighbouring lines and frames are correlated enough for every branch of the filter to be taken: a random
    base picture, a random per-frame change on a third of the components, per-line combing on another third"""
    rng = np.random.default_rng(seed)
    mx = 255 if nbytes == 1 else 65535
    base = rng.integers(0, mx + 1, size=(1, lines, comps))
    base = np.where(rng.random((1, lines, comps)) < 0.5, base, np.repeat(rng.integers(0, mx + 1, size=(1, 1, comps)), lines, axis=1))
    f = np.repeat(base, 3, axis=0)
    change = rng.random((3, lines, comps))
    f = np.where(change < 0.33, rng.integers(0, mx + 1, size=(3, lines, comps)), f)
    f = np.where(change > 0.8, np.clip(f + rng.integers(-mx // 8, mx // 8 + 1, size=(3, lines, comps)), 0, mx), f)
    return f.astype(np.uint8 if nbytes == 1 else np.uint16)


def plane_view(sample, pl):
    """The components of plane `pl` (a dict of api.plan_deint_planes) of a sample held as a 1-D uint8 array: lines x comps, a view."""
    dt = np.uint8 if pl["bytes"] == 1 else np.dtype("<u2")
    rows = np.lib.stride_tricks.as_strided(sample[pl["offset"]:], shape=(pl["lines"], pl["comps"] * pl["bytes"]), strides=(pl["pitch"], 1), writeable=False)
    return np.ascontiguousarray(rows).view(dt)


def deint_sample(planes, prev, cur, nxt, keep, first, mode, dst, dst_planes=None):
    """prev, cur, nxt: samples as 1-D uint8 arrays laid out by `planes` (api.plan_deint_planes).  Writes the pixels of the result into the
    1-D uint8 array dst laid out by dst_planes (default: planes) and leaves every other byte of dst alone.  Returns dst."""
    dst_planes = dst_planes or planes
    for pl, dp in zip(planes, dst_planes):
        o = deint_plane(plane_view(prev, pl), plane_view(cur, pl), plane_view(nxt, pl), keep, first, mode, pl["cs"], pl["mask"])
        o = o.astype(np.uint8 if pl["bytes"] == 1 else np.dtype("<u2"))
        rowb = pl["comps"] * pl["bytes"]
        for y in range(pl["lines"]):
            at = dp["offset"] + y * dp["pitch"]
            dst[at:at + rowb] = o[y].view(np.uint8)
    return dst


def sample_size(planes):
    """bytes of a sample laid out by `planes`: up to the end of the last row's pitch (pitch * lines of the input, as the context counts it)"""
    return max(p["offset"] + p["lines"] * p["pitch"] for p in planes)


def noise_samples(planes, n, seed, poison=0xee):
    """n samples (1-D uint8 arrays of sample_size) whose pixels are `noise` — consecutive triples are correlated frames — and whose every
    other byte is `poison`.  Words of a masked (10-bit planar) plane carry random bits above the mask: the pass must not see them."""
    size = sample_size(planes)
    out = [np.full(size, poison, dtype=np.uint8) for _ in range(n)]
    rng = np.random.default_rng(seed + 7)
    for k, pl in enumerate(planes):
        groups = [noise(pl["lines"], pl["comps"], pl["bytes"], seed + 31 * k + 1000 * g) for g in range((n + 2) // 3)]
        rowb = pl["comps"] * pl["bytes"]
        for i in range(n):
            f = groups[i // 3][i % 3]
            if pl["bytes"] == 2 and pl["mask"] != 0xffff:
                f = (f & pl["mask"]) | (rng.integers(0, 1 << 16, size=f.shape).astype(np.uint16) & np.uint16(0xffff ^ pl["mask"]))
            b = np.ascontiguousarray(f).view(np.uint8).reshape(pl["lines"], rowb)
            for y in range(pl["lines"]):
                at = pl["offset"] + y * pl["pitch"]
                out[i][at:at + rowb] = b[y]
    return out


def field_parity(field_order, field):
    """keep, first of field `field` (0 the first, 1 the second) of a frame of field_order 1 (top field first) / 2 (bottom field first)"""
    return (field if field_order == 1 else 1 - field), int(field == 0)
