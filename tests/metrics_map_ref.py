"""numpy model of the picture metric maps (include/hmgpu.h "picture metric maps"): the six fields per block in int64.  The window
value, its constants and the cropping are those of tests/metrics_ref.py: window_values() is its ssim_q32 before the sum (the same
float64 expression on the same integers), which tests/test_metrics_map_cpu.py holds against it."""
import numpy as np

from tests import metrics_ref as mref

FIELDS = ("sse", "sad", "differing", "max_abs", "ssim_q32", "ssim_windows")


def grid(width, height, block):
    """(blocks_x, blocks_y) of a cropped luma plane of width x height"""
    return -(-width // block), -(-height // block)


def block_size(fmt, block, k):
    """(bw, bh) of component k in its own samples"""
    csx, csy = mref.chroma_shifts(fmt)
    return (block >> csx, block >> csy) if k else (block, block)


def window_values(a, b, bit_depth):
    """llrint(ssim * 2^32) of every window of the plane: an int64 array [ny, nx], window (j, i) with its top-left at (4i, 4j)"""
    h, w = a.shape
    if not mref.windows(w, h):
        return np.zeros((0, 0), np.int64)
    a = a.astype(np.int64)
    b = b.astype(np.int64)
    nx, ny = (w >> 2) - 1, (h >> 2) - 1

    def box(v):
        blk = v[:4 * (ny + 1), :4 * (nx + 1)].reshape(ny + 1, 4, nx + 1, 4).sum(axis=(1, 3))
        return blk[:-1, :-1] + blk[:-1, 1:] + blk[1:, :-1] + blk[1:, 1:]
    s1, s2, ss, s12 = box(a), box(b), box(a * a + b * b), box(a * b)
    var = 64 * ss - s1 * s1 - s2 * s2
    covar = 64 * s12 - s1 * s2
    c1, c2 = mref.ssim_constants(bit_depth)
    num = (2 * s1 * s2 + c1).astype(np.float64) * (2 * covar + c2).astype(np.float64)
    den = (s1 * s1 + s2 * s2 + c1).astype(np.float64) * (var + c2).astype(np.float64)
    return np.rint((num / den) * 4294967296.0).astype(np.int64)


def _per_block(v, bw, bh, nbx, nby, reduce):
    """v [h, w] reduced over blocks of bw x bh from the top-left, the last ones partial: [nby, nbx]"""
    full = np.zeros((nby * bh, nbx * bw), np.int64)
    full[:v.shape[0], :v.shape[1]] = v
    return reduce(full.reshape(nby, bh, nbx, bw), axis=(1, 3))


def plane(a, b, bit_depth, bw, bh, nbx, nby, ssim=True):
    """the map of one cropped component plane: an int64 array [6 or 4, nby, nbx]"""
    a = np.asarray(a).astype(np.int64)
    b = np.asarray(b).astype(np.int64)
    assert a.shape == b.shape and a.ndim == 2
    assert -(-a.shape[1] // bw) == nbx and -(-a.shape[0] // bh) == nby, (a.shape, bw, bh, nbx, nby)
    d = np.abs(a - b)
    out = np.zeros((6 if ssim else 4, nby, nbx), np.int64)
    out[0] = _per_block(d * d, bw, bh, nbx, nby, np.sum)
    out[1] = _per_block(d, bw, bh, nbx, nby, np.sum)
    out[2] = _per_block((d != 0).astype(np.int64), bw, bh, nbx, nby, np.sum)
    out[3] = _per_block(d, bw, bh, nbx, nby, np.max)
    if ssim:
        q = window_values(a, b, bit_depth)
        if q.size:
            ny, nx = q.shape
            by = (4 * np.arange(ny) // bh)[:, None].repeat(nx, 1)
            bx = (4 * np.arange(nx) // bw)[None, :].repeat(ny, 0)
            np.add.at(out[4], (by, bx), q)
            np.add.at(out[5], (by, bx), 1)
    return out


def picture(a_planes, b_planes, fmt, bit_depths, block, components=(0, 1, 2), ssim=True, crop=(0, 0, 0, 0)):
    """the maps of one picture, [3, F, nby, nbx]: a_planes / b_planes the uncropped planes; the slices of a component that is not
    compared are zero"""
    a = mref.crop_planes(a_planes, crop, fmt)
    b = mref.crop_planes(b_planes, crop, fmt)
    return cropped(a, b, fmt, bit_depths, block, a_planes[0].shape[1] - crop[0] - crop[1], a_planes[0].shape[0] - crop[2] - crop[3], components, ssim)


def cropped(a, b, fmt, bit_depths, block, width, height, components=(0, 1, 2), ssim=True):
    """the same from planes that are cropped already; width x height: the cropped luma size (a[0] may be absent: None)"""
    nbx, nby = grid(width, height, block)
    out = np.zeros((3, 6 if ssim else 4, nby, nbx), np.int64)
    for k in range(3):
        if k in components and not (k and fmt == 0):
            bw, bh = block_size(fmt, block, k)
            out[k] = plane(a[k], b[k], bit_depths[1 if k else 0], bw, bh, nbx, nby, ssim)
    return out


def samples(width, height, fmt, block, k):
    """samples of component k per block, [nby, nbx]"""
    csx, csy = mref.chroma_shifts(fmt)
    w, h = (width >> csx, height >> csy) if k else (width, height)
    nbx, nby = grid(width, height, block)
    bw, bh = block_size(fmt, block, k)
    return _per_block(np.ones((h, w), np.int64), bw, bh, nbx, nby, np.sum)


def block_tolerance(out):
    """per element of ssim_q32: metrics_ref.tolerance of the windows in the block"""
    return 1 + out[..., 5, :, :] // 1024
