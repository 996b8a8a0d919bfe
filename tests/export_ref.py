"""numpy restatement of the device export (include/hmgpu.h "device export", k_export.hip): what the kernel must write, sample for
sample, given HM's int16 planes and the integers hmgpu_export_plan_for publishes."""
import numpy as np

PLANAR, SEMIPLANAR, RGB = 0, 1, 2
KR_KB = {1: (0.2126, 0.0722), 5: (0.299, 0.114), 6: (0.299, 0.114), 9: (0.2627, 0.0593)}


def chroma_shift(fmt):
    return (0 if fmt == 3 else 1), (1 if fmt in (0, 1) else 0)


def depth_conv(v, in_bd, out_bd):
    """TVideoIOYuv::write's rule (HM 16.0, CLIP_TO_709_RANGE 0)"""
    v = v.astype(np.int64)
    s = out_bd - in_bd
    if s >= 0:
        return v << s
    return np.clip((v + (1 << (-s - 1))) >> -s, 0, (1 << out_bd) - 1)


def crop_planes(planes, fmt, crop):
    l, r, t, b = crop
    sx, sy = chroma_shift(fmt)
    out = [planes[0][t:planes[0].shape[0] - b, l:planes[0].shape[1] - r]]
    if fmt != 0:
        for c in (1, 2):
            p = planes[c]
            out.append(p[t >> sy:p.shape[0] - (b >> sy), l >> sx:p.shape[1] - (r >> sx)])
    return out


def export_yuv(planes, fmt, bd, out_bd, layout, crop=(0, 0, 0, 0), msb=False):
    """planar: [Y, Cb, Cr] (Y only for 4:0:0); semi-planar: [Y, CbCr as H x W x 2]; values as the container holds them"""
    cp = crop_planes(planes, fmt, crop)
    out = [depth_conv(cp[0], bd[0], out_bd[0]) << (16 - out_bd[0] if msb else 0)]
    if fmt != 0:
        cc = [depth_conv(p, bd[1], out_bd[1]) << (16 - out_bd[1] if msb else 0) for p in cp[1:]]
        out += cc if layout == PLANAR else [np.stack(cc, axis=-1)]
    return out


def export_rgb(planes, fmt, bd, out_bd, coef, crop=(0, 0, 0, 0), msb=False):
    """[3, H, W] R, G, B with the published integers (coef: hmgpu_export_plan.coef)"""
    cp = crop_planes(planes, fmt, crop)
    y = cp[0].astype(np.int64)
    H, W = y.shape
    sx, sy = chroma_shift(fmt)
    if fmt == 0:
        u = np.full((H, W), 1 << (bd[1] - 1), dtype=np.int64)
        v = u.copy()
    else:
        ry, rx = np.arange(H) >> sy, np.arange(W) >> sx
        u = cp[1].astype(np.int64)[ry][:, rx]
        v = cp[2].astype(np.int64)[ry][:, rx]
    sh = 16 - out_bd if msb else 0
    if coef[10]:
        return np.stack([depth_conv(v, bd[1], out_bd), depth_conv(y, bd[0], out_bd), depth_conv(u, bd[1], out_bd)]) << sh
    S, rnd, yo, co, cy, crv, cgu, cgv, cbu, M = coef[:10]
    t = cy * (y - yo) + rnd
    cu, cv = u - co, v - co
    R = np.clip((t + crv * cv) >> S, 0, M)
    G = np.clip((t + cgu * cu + cgv * cv) >> S, 0, M)
    B = np.clip((t + cbu * cu) >> S, 0, M)
    return np.stack([R, G, B]) << sh


def rgb_float(y, u, v, bd_y, bd_c, out_bd, matrix, full_range):
    """H.273's equations in floating point: R'G'B' in [0, 1] scaled to 2^out_bd - 1 (no rounding, no clipping)"""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    y, u, v = (np.asarray(a, dtype=np.float64) for a in (y, u, v))
    if full_range:
        ey = y / ((1 << bd_y) - 1)
        eu, ev = (u - (1 << (bd_c - 1))) / ((1 << bd_c) - 1), (v - (1 << (bd_c - 1))) / ((1 << bd_c) - 1)
    else:
        ey = (y - (16 << (bd_y - 8))) / (219 << (bd_y - 8))
        eu, ev = (u - (1 << (bd_c - 1))) / (224 << (bd_c - 8)), (v - (1 << (bd_c - 1))) / (224 << (bd_c - 8))
    r = ey + 2 * (1 - kr) * ev
    b = ey + 2 * (1 - kb) * eu
    g = ey - 2 * kb * (1 - kb) / kg * eu - 2 * kr * (1 - kr) / kg * ev
    m = (1 << out_bd) - 1
    return np.stack([r * m, g * m, b * m])


def rgb_int(y, u, v, coef):
    """the kernel's integer RGB for flat arrays of samples (before clipping too: returns (clipped, sums))"""
    S, rnd, yo, co, cy, crv, cgu, cgv, cbu, M = [int(c) for c in coef[:10]]
    y, u, v = (np.asarray(a, dtype=np.int64) for a in (y, u, v))
    t = cy * (y - yo) + rnd
    cu, cv = u - co, v - co
    sums = np.stack([t + crv * cv, t + cgu * cu + cgv * cv, t + cbu * cu])
    return np.clip(sums >> S, 0, M), sums
