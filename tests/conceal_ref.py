"""numpy model of error concealment (include/hmgpu.h "error concealment", hmgpu_pictures_conceal).  It restates the rules of the
header and nothing else; all arithmetic on vectors and coordinates is done in Python integers.

planes: [Y, Cb, Cr] as HM keeps them (int16 [h_c, w_c]); a 4:0:0 context carries 4:2:0-shaped chroma planes that are never written.
grid: tests/motion_ref.grid of the source picture (used / mv / ref_poc per 4x4 block), or None: a source without side information."""
import numpy as np

COPY, MOTION = 0, 1


def clip3(lo, hi, v):
    return lo if v < lo else hi if v > hi else v


def tdiv(a, b):
    """C's integer division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def scale_mv(mv, src_poc, ref_poc, dst_poc):
    """one coordinate of H.265 8.5.3.2.7: the vector that points from src (POC src_poc) to POC ref_poc, stretched to the distance from
    dst to src"""
    td = clip3(-128, 127, src_poc - ref_poc)
    tb = clip3(-128, 127, dst_poc - src_poc)
    if td == 0:
        return 0
    tx = tdiv(16384 + abs(td) // 2, td)
    ds = clip3(-4096, 4095, (tb * tx + 32) >> 6)
    m = ds * mv
    r = (abs(m) + 127) >> 8
    return clip3(-32768, 32767, -r if m < 0 else r)


def scale_mv_spec(mv, td, tb):
    """the same written as the standard prints it, from td and tb (the brute-force side of the scaling test)"""
    if td == 0:
        return 0
    tx = int((16384 + (abs(td) >> 1)) / td)                  # "/": division with truncation towards zero
    ds = min(4095, max(-4096, (tb * tx + 32) >> 6))
    p = ds * mv
    sign = (p > 0) - (p < 0)
    return min(32767, max(-32768, sign * ((abs(p) + 127) >> 8)))


def block_displacement(grid, bx4, by4, src_poc, dst_poc):
    """(dx, dy) in whole luma samples of the 8x8 block whose top-left 4x4 block is (bx4, by4)"""
    if grid is None:
        return 0, 0
    for l in range(2):
        if grid["used"][l][by4, bx4]:
            ref_poc = int(grid["ref_poc"][l][by4, bx4])
            v = [scale_mv(int(grid["mv"][l][k][by4, bx4]), src_poc, ref_poc, dst_poc) for k in range(2)]
            return (v[0] + 2) >> 2, (v[1] + 2) >> 2
    return 0, 0


def displacements(grid, width, height, src_poc, dst_poc):
    """(dx, dy) of every 8x8 luma block, each int [height / 8 rounded up, width / 8 rounded up]"""
    bh, bw = (height + 7) // 8, (width + 7) // 8
    dx, dy = np.zeros((bh, bw), np.int64), np.zeros((bh, bw), np.int64)
    for j in range(bh):
        for i in range(bw):
            dx[j, i], dy[j, i] = block_displacement(grid, 2 * i, 2 * j, src_poc, dst_poc)
    return dx, dy


def chroma_shifts(chroma_format):
    return (0 if chroma_format == 3 else 1, 1 if chroma_format in (0, 1) else 0)


def mask_bits(mask, num_ctus):
    """truth values per CTU from None (all), truth values, or the packed bytes"""
    if mask is None:
        return np.ones(num_ctus, bool)
    mask = np.asarray(mask)
    if mask.dtype == np.uint8 and mask.size == (num_ctus + 7) // 8 and mask.size != num_ctus:
        return np.unpackbits(mask, bitorder="little")[:num_ctus].astype(bool)
    return mask.astype(bool).reshape(num_ctus)


def conceal(dst, src, mask, mode, log2_ctu, chroma_format, bit_depth, dst_poc=0, src_poc=0, fill=(-1, -1, -1), grid=None, reads=None):
    """the planes of dst after one job.  src: planes, or None (fill); bit_depth: (luma, chroma); reads: a list that receives every
    (component, y, x) the model reads from src (the clamping test)"""
    out = [np.array(p, dtype=np.int16, copy=True) for p in dst]
    h, w = out[0].shape
    S = 1 << log2_ctu
    ctus_w, ctus_h = (w + S - 1) // S, (h + S - 1) // S
    bits = mask_bits(mask, ctus_w * ctus_h)
    csx, csy = chroma_shifts(chroma_format)
    comps = [0] if chroma_format == 0 else [0, 1, 2]
    for a in np.flatnonzero(bits):
        cx, cy = int(a) % ctus_w, int(a) // ctus_w
        for by in range(cy * S, min(cy * S + S, h), 8):
            for bx in range(cx * S, min(cx * S + S, w), 8):
                dx, dy = (0, 0)
                if src is not None and mode == MOTION:
                    dx, dy = block_displacement(grid, bx >> 2, by >> 2, src_poc, dst_poc)
                for c in comps:
                    sx, sy = (csx, csy) if c else (0, 0)
                    wc, hc = w >> sx, h >> sy
                    x0, y0 = bx >> sx, by >> sy
                    x1, y1 = min((bx + 8) >> sx, wc), min((by + 8) >> sy, hc)
                    if src is None:
                        out[c][y0:y1, x0:x1] = fill[c] if fill[c] >= 0 else 1 << (bit_depth[1 if c else 0] - 1)
                        continue
                    ddx, ddy = dx >> sx, dy >> sy
                    if ddx == 0 and ddy == 0 and reads is None:
                        out[c][y0:y1, x0:x1] = src[c][y0:y1, x0:x1]
                        continue
                    for y in range(y0, y1):
                        yy = clip3(0, hc - 1, y + ddy)
                        for x in range(x0, x1):
                            xx = clip3(0, wc - 1, x + ddx)
                            if reads is not None:
                                reads.append((c, yy, xx))
                            out[c][y, x] = src[c][yy, xx]
    return out
