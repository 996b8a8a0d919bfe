"""numpy model of the picture import (include/hmgpu.h "picture import"), written from the header's text and the lines of HM it cites
(TVideoIOYuv::read, readPlane, scalePlane); it never calls the library.  Planes are integer arrays; a picture is [Y, Cb, Cr] of int16
at the coding depths (Y alone for 4:0:0), which is what Context.download returns."""
import math

import numpy as np

PLANAR, SEMIPLANAR, RGB = 0, 1, 2
UINT, F16, BF16, F32 = 0, 1, 2, 3
DROP, LINEAR = 0, 1
KR_KB = {1: (0.2126, 0.0722), 5: (0.299, 0.114), 6: (0.299, 0.114), 9: (0.2627, 0.0593)}
# where R, G, B stand in a packed pixel, and its elements: RGB BGR RGBA BGRA ARGB ABGR
PIXEL_POS = {0: ((0, 1, 2), 3), 1: ((2, 1, 0), 3), 2: ((0, 1, 2), 4), 3: ((2, 1, 0), 4), 4: ((1, 2, 3), 4), 5: ((3, 2, 1), 4)}


def shifts(fmt):
    """(csx, csy) of a format with chroma"""
    return (0 if fmt == 3 else 1), (1 if fmt == 1 else 0)


# ---------------------------------------------------------------------------------------------------- elements -> integers at depth D
def uint_codes(raw, depth, msb_aligned=False):
    """unsigned elements: shifted right by 16 - D when msb_aligned; an element above 2^D - 1 is read as 2^D - 1"""
    v = np.asarray(raw).astype(np.int64)
    if msb_aligned:
        v = v >> (16 - depth)
    return np.minimum(v, (1 << depth) - 1)


def float_codes(x, scale, bias, depth):
    """float elements (given as float32, which holds every float16 and bfloat16 exactly):
    clip(rint(fl(fl(x * scale) + bias)), 0, 2^D - 1), NaN -> 0"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        m = np.multiply(np.asarray(x, np.float32), np.float32(scale), dtype=np.float32)
        t = np.rint(np.add(m, np.float32(bias), dtype=np.float32))
        t = np.clip(t, np.float32(0), np.float32((1 << depth) - 1))
    return np.where(np.isnan(t), 0, t).astype(np.int64)


def depth_rule(v, depth, coding):
    """scalePlane, CLIP_TO_709_RANGE 0 (TVideoIOYuv.cpp:70-87)"""
    v = np.asarray(v).astype(np.int64)
    s = coding - depth
    if s >= 0:
        return v << s
    return np.clip((v + (1 << (-s - 1))) >> -s, 0, (1 << coding) - 1)


# ---------------------------------------------------------------------------------------------------- chroma: format, padding
def axis_taps(n_src, change, linear, site):
    """per converted index j: [(source index, weight)], indices clamped to the source plane.  change: 0 same, +1 the picture has more
    samples on the axis, -1 fewer; site: "co-sited", "centred" or "bottom" """
    def clamp(i):
        return min(n_src - 1, max(0, i))

    if change == 0:
        return [[(j, 4)] for j in range(n_src)]
    if change > 0:
        return [[(clamp(j >> 1), 4)] for j in range(2 * n_src)]               # readPlane :324
    out = []
    for j in range(n_src // 2):
        if not linear:
            t = [(2 * j, 4)]                                                  # readPlane :307, :286 / :297
        elif site == "co-sited":
            t = [(2 * j - 1, 1), (2 * j, 2), (2 * j + 1, 1)]
        elif site == "centred":
            t = [(2 * j, 2), (2 * j + 1, 2)]
        else:
            t = [(2 * j, 1), (2 * j + 1, 2), (2 * j + 2, 1)]
        out.append([(clamp(i), w) for i, w in t])
    return out


def convert_chroma(c, ssx, ssy, psx, psy, pic_fmt, down, loc):
    """one chroma plane of the source (subsampling ssx, ssy) to the picture's (psx, psy): (sum + 8) >> 4 over the taps of both axes"""
    c = np.asarray(c).astype(np.int64)
    hs = "centred" if pic_fmt == 1 and (loc & 1) else "co-sited"
    vs = ("centred", "co-sited", "bottom")[loc >> 1]
    ty = axis_taps(c.shape[0], ssy - psy, down == LINEAR, vs)
    tx = axis_taps(c.shape[1], ssx - psx, down == LINEAR, hs)
    my, mx = np.zeros((len(ty), c.shape[0]), np.int64), np.zeros((len(tx), c.shape[1]), np.int64)
    for m, t in ((my, ty), (mx, tx)):
        for j, taps in enumerate(t):
            for i, w in taps:
                m[j, i] += w
    return (my @ c @ mx.T + 8) >> 4


def pad(plane, w, h):
    """readPlane :333-345: the last column repeated, then the last row"""
    p = np.asarray(plane)
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")


def import_yuv(planes, src_fmt, pic_fmt, depth, coding, size, down=DROP, loc=0):
    """planes: [Y, Cb, Cr] integers at the source depths `depth` = (luma, chroma), Y alone for a 4:0:0 source; size: the coded (w, h).
    Returns the picture's planes, int16"""
    w, h = size
    y = np.asarray(planes[0])
    out = [pad(depth_rule(y, depth[0], coding[0]), w, h).astype(np.int16)]
    if pic_fmt == 0:
        return out
    psx, psy = shifts(pic_fmt)
    for k in (1, 2):
        if src_fmt == 0:
            c = np.full((y.shape[0] >> psy, y.shape[1] >> psx), 1 << (depth[1] - 1), np.int64)       # readPlane :263
        else:
            ssx, ssy = shifts(src_fmt)
            c = convert_chroma(planes[k], ssx, ssy, psx, psy, pic_fmt, down, loc)
        out.append(pad(depth_rule(c, depth[1], coding[1]), w >> psx, h >> psy).astype(np.int16))
    return out


# ---------------------------------------------------------------------------------------------------- RGB
def rnd(v):
    """round half away from zero"""
    return -int(math.floor(-v + 0.5)) if v < 0 else int(math.floor(v + 0.5))


def rgb_rows(depth, coding, matrix, full_range, s):
    """the nine coefficients of the header's formula at shift s, the offsets yo, co and the scales ys, cs"""
    kr, kb = KR_KB[matrix]
    bdy, bdc = coding
    m = float((1 << depth) - 1)
    ys = float((1 << bdy) - 1) if full_range else float(219 << (bdy - 8))
    cs = float((1 << bdc) - 1) if full_range else float(224 << (bdc - 8))
    q = float(1 << s)
    yr, yb = rnd(kr * ys / m * q), rnd(kb * ys / m * q)
    yg = rnd(ys / m * q) - yr - yb
    bb, br = rnd(cs / (2 * m) * q), rnd(-kr / (1 - kb) * cs / (2 * m) * q)
    rr, rb = rnd(cs / (2 * m) * q), rnd(-kb / (1 - kr) * cs / (2 * m) * q)
    return [yr, yg, yb, br, -(br + bb), bb, rr, -(rr + rb), rb], (0 if full_range else 16 << (bdy - 8)), 1 << (bdc - 1), ys, cs


def overflow_bound(rows, depth, s):
    """the largest magnitude a sum of the formula can reach, the rounding term included, for R, G, B in 0 .. 2^D - 1"""
    m = (1 << depth) - 1
    worst = 0
    for r in range(3):
        pos = sum(c for c in rows[3 * r:3 * r + 3] if c > 0)
        neg = -sum(c for c in rows[3 * r:3 * r + 3] if c < 0)
        worst = max(worst, max(pos, neg) * m + (1 << (s - 1)))
    return worst


def rgb_coef(depth, coding, matrix, full_range):
    """hmgpu_import_plan.coef by the header's rule: the largest shift <= 30 whose sums stay inside int32"""
    coef = [0] * 16
    coef[13] = (1 << depth) - 1
    if matrix == 0:
        coef[14] = 1
        return coef
    for s in range(30, 0, -1):
        rows, yo, co, _, _ = rgb_rows(depth, coding, matrix, full_range, s)
        if overflow_bound(rows, depth, s) <= 2 ** 31 - 1:
            coef[0], coef[1], coef[2], coef[3] = s, 1 << (s - 1), yo, co
            coef[4:13] = rows
            return coef
    raise ValueError("no shift fits")


def rgb_to_ycc(r, g, b, coef, depth, coding):
    """Y, Cb, Cr at every pixel, at the coding depths"""
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    if coef[14]:
        return depth_rule(g, depth, coding[0]), depth_rule(b, depth, coding[1]), depth_rule(r, depth, coding[1])
    s, half = coef[0], coef[1]
    out = []
    for row, off, bd in ((coef[4:7], coef[2], coding[0]), (coef[7:10], coef[3], coding[1]), (coef[10:13], coef[3], coding[1])):
        t = row[0] * r + row[1] * g + row[2] * b + half
        assert np.abs(t).max() <= 2 ** 31 - 1
        out.append(np.clip((t >> s) + off, 0, (1 << bd) - 1))
    return out


def import_rgb(r, g, b, pic_fmt, depth, coding, size, matrix=1, full_range=0, down=DROP, loc=0, coef=None):
    """R, G, B integers at the source depth -> the picture's planes, int16; coef: the published integers (None: this model's own)"""
    w, h = size
    coef = rgb_coef(depth, coding, matrix, full_range) if coef is None else coef
    y, cb, cr = rgb_to_ycc(r, g, b, coef, depth, coding)
    out = [pad(y, w, h).astype(np.int16)]
    if pic_fmt == 0:
        return out
    psx, psy = shifts(pic_fmt)
    for c in (cb, cr):
        out.append(pad(convert_chroma(c, 0, 0, psx, psy, pic_fmt, down, loc), w >> psx, h >> psy).astype(np.int16))
    return out


def unpack_pixels(px, order):
    """[H, W, C] packed pixels -> R, G, B planes; the A element is read over"""
    pos, nch = PIXEL_POS[order]
    assert px.shape[-1] == nch
    return [px[..., pos[k]] for k in range(3)]
