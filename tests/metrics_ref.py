"""numpy model of hmgpu_metrics_result (include/hmgpu.h "picture metrics"): every field in int64, the SSIM value in float64 exactly as
the header states it.  a, b: 2-d integer arrays of one cropped component plane."""
import math

import numpy as np

FIELDS = ("samples", "sse", "sad", "differing", "first_diff", "ssim_q32", "ssim_windows", "max_abs")
NO_DIFF = -1                       # UINT64_MAX as the int64 the result tensors hold


def chroma_shifts(fmt):
    return (0 if fmt == 3 else 1), (1 if fmt in (0, 1) else 0)


def ssim_constants(bit_depth):
    maxv = float((1 << bit_depth) - 1)
    return int(.01 * .01 * maxv * maxv * 64 + .5), int(.03 * .03 * maxv * maxv * 64 * 63 + .5)


def windows(w, h):
    return ((w >> 2) - 1) * ((h >> 2) - 1) if w >= 8 and h >= 8 else 0


def ssim_q32(a, b, bit_depth):
    """(sum over the windows of llrint(ssim * 2^32), windows)"""
    h, w = a.shape
    n = windows(w, h)
    if not n:
        return 0, 0
    a = a.astype(np.int64)
    b = b.astype(np.int64)
    nx, ny = (w >> 2) - 1, (h >> 2) - 1

    def box(v):                        # sums over the 8x8 windows at (4i, 4j), from 4x4 block sums
        blk = v[:4 * (ny + 1), :4 * (nx + 1)].reshape(ny + 1, 4, nx + 1, 4).sum(axis=(1, 3))
        return blk[:-1, :-1] + blk[:-1, 1:] + blk[1:, :-1] + blk[1:, 1:]
    s1, s2, ss, s12 = box(a), box(b), box(a * a + b * b), box(a * b)
    var = 64 * ss - s1 * s1 - s2 * s2
    covar = 64 * s12 - s1 * s2
    c1, c2 = ssim_constants(bit_depth)
    num = (2 * s1 * s2 + c1).astype(np.float64) * (2 * covar + c2).astype(np.float64)
    den = (s1 * s1 + s2 * s2 + c1).astype(np.float64) * (var + c2).astype(np.float64)
    q = np.rint((num / den) * 4294967296.0).astype(np.int64)
    return int(q.sum()), n


def plane(a, b, bit_depth, ssim=True):
    """the record of one component as a dict of Python ints"""
    a = np.asarray(a).astype(np.int64)
    b = np.asarray(b).astype(np.int64)
    assert a.shape == b.shape and a.ndim == 2
    d = np.abs(a - b)
    nz = np.flatnonzero(d.reshape(-1))
    q, n = ssim_q32(a, b, bit_depth) if ssim else (0, 0)
    return {"samples": int(a.size), "sse": int((d * d).sum()), "sad": int(d.sum()), "differing": int(nz.size),
            "first_diff": int(nz[0]) if nz.size else NO_DIFF, "ssim_q32": q, "ssim_windows": n, "max_abs": int(d.max()) if a.size else 0}


ZERO = {f: 0 for f in FIELDS}


def crop_planes(planes, crop, fmt):
    """the cropped component planes of a picture's three planes; crop (left, right, top, bottom) in luma samples"""
    l, r, t, b = crop
    csx, csy = chroma_shifts(fmt)
    out = []
    for k, p in enumerate(planes):
        sx, sy = (csx, csy) if k else (0, 0)
        out.append(p[t >> sy:p.shape[0] - (b >> sy), l >> sx:p.shape[1] - (r >> sx)])
    return out


def picture(a_planes, b_planes, fmt, bit_depths, components=(0, 1, 2), ssim=True, crop=(0, 0, 0, 0)):
    """the three records of one picture: a_planes / b_planes the uncropped planes (b_planes: already cropped when crop is None)"""
    a = crop_planes(a_planes, crop, fmt)
    b = crop_planes(b_planes, crop, fmt)
    out = []
    for k in range(3):
        if k not in components or (k and fmt == 0):
            out.append(dict(ZERO))
        else:
            out.append(plane(a[k], b[k], bit_depths[1 if k else 0], ssim))
    return out


def psnr(samples, sse, bit_depth):
    maxval = 255 << (bit_depth - 8)
    return 999.99 if sse == 0 else 10.0 * math.log10(float(maxval) * maxval * float(samples) / float(sse))


def tolerance(ssim_windows):
    """|delta| allowed on ssim_q32: the model and the device evaluate the same binary64 expression on exactly representable factors
    (every integer factor is below 2^53), so a window's quotient can differ by a contraction or a last-place rounding only: a
    relative 1e-16 against the llrint quantum of 2^-32 = 2.3e-10, which moves llrint by one unit only at a rounding boundary --
    about one window in a million.  1 + windows / 1024 allows a thousand times that; one misplaced window moves the sum by ~1e7."""
    return 1 + ssim_windows // 1024
