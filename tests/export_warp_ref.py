"""include/hmgpu.h "affine warp export" restated in numpy int64: the output of one slot from S, the slot's window as [3, Hs, Ws]
integers 0 .. M -- what the unscaled export writes for that window before the colour stage, the container shift, the float map, the
mirror and the packing.  S comes from the existing references, or on the GPU from the existing unscaled export of the same picture."""
import numpy as np

IDENTITY = (65536, 0, 0, 0, 65536, 0)


def taps(S, x, y, border, fill):
    """S[:, y, x] for int64 index arrays of one shape, each tap decided on its own: clamped (edge), or fill[c] outside (fill)"""
    S = np.asarray(S, np.int64)
    hs, ws = S.shape[1:]
    v = S[:, np.clip(y, 0, hs - 1), np.clip(x, 0, ws - 1)]
    if border == "fill":
        outside = (x < 0) | (x >= ws) | (y < 0) | (y >= hs)
        v = np.where(outside[None], np.asarray(fill, np.int64).reshape(3, 1, 1), v)
    return v


def warp(S, m, out_size, filter="bilinear", border="edge", fill=(0, 0, 0)):
    """[3, H, W] int64: the v of every output pixel; m: six Q16 ints; out_size: (height, width)"""
    h, w = out_size
    m = [int(v) for v in m]
    oy, ox = np.mgrid[0:h, 0:w].astype(np.int64)
    rnd = 128 if filter == "bilinear" else 32768
    X = m[0] * ox + m[1] * oy + m[2] + rnd
    Y = m[3] * ox + m[4] * oy + m[5] + rnd
    ix, iy = X >> 16, Y >> 16
    if filter == "nearest":
        return taps(S, ix, iy, border, fill)
    fx, fy = (X >> 8) & 255, (Y >> 8) & 255
    acc = ((256 - fx) * (256 - fy) * taps(S, ix, iy, border, fill) + fx * (256 - fy) * taps(S, ix + 1, iy, border, fill) +
           (256 - fx) * fy * taps(S, ix, iy + 1, border, fill) + fx * fy * taps(S, ix + 1, iy + 1, border, fill) + 32768)
    assert int(acc.max()) < 1 << 32
    return acc >> 16
