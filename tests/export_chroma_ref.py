"""numpy restatement of the chroma stage of the RGB exports (include/hmgpu.h "chroma export"): one chroma plane of the decoded
picture, its subsampling and the chroma_sample_loc_type in; the plane on the luma grid out.  Written from the table of taps, one
axis at a time, with none of the kernels' shortcuts."""
import numpy as np

NONE, COSITED, CENTRED, BOTTOM = "none", "co-sited", "centred", "bottom"


def phases(csx, csy, loc):
    """(horizontal, vertical) phase of a format and a chroma_sample_loc_type (H.265 figure E.1); 4:2:2 ignores loc"""
    if not 0 <= loc <= 5:
        raise ValueError("chroma_sample_loc_type 0 .. 5")
    if not csy:
        return (COSITED if csx else NONE), NONE
    return (CENTRED if loc & 1 else COSITED), (CENTRED, COSITED, BOTTOM)[loc >> 1]


def taps(phase, n_luma, n_chroma):
    """per luma coordinate 0 .. n_luma - 1: (i0, i1, w0, w1), the two clamped tap indices and their weights in quarters"""
    x = np.arange(n_luma)
    if phase == NONE:
        i0, w0 = x, np.full(n_luma, 4)
    else:
        j, odd = x >> 1, (x & 1) == 1
        if phase == COSITED:
            i0, w0 = j, np.where(odd, 2, 4)
        elif phase == CENTRED:
            i0, w0 = np.where(odd, j, j - 1), np.where(odd, 3, 1)
        elif phase == BOTTOM:
            i0, w0 = np.where(odd, j, j - 1), np.where(odd, 4, 2)
        else:
            raise ValueError(phase)
    return np.clip(i0, 0, n_chroma - 1), np.clip(i0 + 1, 0, n_chroma - 1), w0, 4 - w0


def upsample(plane, csx, csy, loc):
    """plane [Hc, Wc] of the whole decoded picture -> [Hc << csy, Wc << csx]: c' = (sum wx * wy * C[iy][ix] + 8) >> 4"""
    c = np.asarray(plane).astype(np.int64)
    hc, wc = c.shape
    ph, pv = phases(csx, csy, loc)
    x0, x1, wx0, wx1 = taps(ph, wc << csx, wc)
    y0, y1, wy0, wy1 = taps(pv, hc << csy, hc)
    total = (wy0[:, None] * wx0[None, :]) * c[y0][:, x0] + (wy0[:, None] * wx1[None, :]) * c[y0][:, x1] + \
            (wy1[:, None] * wx0[None, :]) * c[y1][:, x0] + (wy1[:, None] * wx1[None, :]) * c[y1][:, x1]
    return (total + 8) >> 4


def upsample_planes(planes, fmt, loc):
    """[Y, Cb, Cr] of chroma format fmt -> the 4:4:4 planes the linear export works on (4:0:0 and 4:4:4: unchanged)"""
    if fmt in (0, 3):
        return list(planes)
    csx, csy = 1, 1 if fmt == 1 else 0
    return [planes[0]] + [upsample(p, csx, csy, loc).astype(np.asarray(p).dtype) for p in planes[1:]]
