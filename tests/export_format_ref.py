"""numpy restatement of the format export (include/hmgpu.h "format export"), unscaled, integers only: one chroma plane of the whole
decoded picture at the source format in, the plane at the output format out.  Written from the rule one axis at a time -- a list of
(index, weight) taps per output sample, weights in quarters that sum to 4 -- with none of the kernel's shortcuts.

Per axis, comparing the subsampling of the source with the output's:
  same                the sample itself
  gain, "replicate"   sample j >> 1
  gain, "linear"      the two taps of the table of "chroma export" for the luma coordinate j, by the siting of the axis
  loss, "drop"        sample 2j
  loss, "linear"      co-sited (2j - 1: 1, 2j: 2, 2j + 1: 1); centred (2j: 2, 2j + 1: 2); bottom (2j: 1, 2j + 1: 2, 2j + 2: 1)
Siting (loc = chroma_sample_loc_type of the 4:2:0 side): horizontally co-sited for loc 0, 2, 4 and for every 4:2:2 side, centred
for 1, 3, 5; vertically centred for loc 0, 1, co-sited for 2, 3, bottom for 4, 5.  Tap indices are clamped to the plane;
c = (sum wx * wy * C[iy][ix] + 8) >> 4."""
import numpy as np

REPLICATE, LINEAR = 0, 1            # up
DROP = 0                            # down (LINEAR = 1 as well)
COSITED, CENTRED, BOTTOM = "co-sited", "centred", "bottom"


def shifts(fmt):
    """(csx, csy) of a chroma_format_idc; 4:0:0 as 4:2:0"""
    return (0 if fmt == 3 else 1), (1 if fmt in (0, 1) else 0)


def siting(fmt420_side, loc):
    """(horizontal, vertical) siting of the subsampled side of a conversion: fmt420_side True when that side is 4:2:0"""
    if not 0 <= loc <= 5:
        raise ValueError("chroma_sample_loc_type 0 .. 5")
    if not fmt420_side:
        return COSITED, None
    return (CENTRED if loc & 1 else COSITED), (CENTRED, COSITED, BOTTOM)[loc >> 1]


def axis_taps(n_src, change, mode, site):
    """per output index j of an axis: a list of (source index, weight) with the indices clamped to 0 .. n_src - 1.
    change: 0 same, +1 the axis gains samples (2 * n_src outputs), -1 it loses them (n_src // 2 outputs)"""
    def clamp(i):
        return min(n_src - 1, max(0, i))

    if change == 0:
        return [[(j, 4)] for j in range(n_src)]
    out = []
    if change > 0:
        for x in range(2 * n_src):
            j, odd = x >> 1, x & 1
            if mode == REPLICATE:
                t = [(j, 4)]
            elif site == COSITED:
                t = [(j, 2), (j + 1, 2)] if odd else [(j, 4)]
            elif site == CENTRED:
                t = [(j, 3), (j + 1, 1)] if odd else [(j - 1, 1), (j, 3)]
            elif site == BOTTOM:
                t = [(j, 4)] if odd else [(j - 1, 2), (j, 2)]
            else:
                raise ValueError(site)
            out.append([(clamp(i), w) for i, w in t])
        return out
    for j in range(n_src // 2):
        if mode == DROP:
            t = [(2 * j, 4)]
        elif site == COSITED:
            t = [(2 * j - 1, 1), (2 * j, 2), (2 * j + 1, 1)]
        elif site == CENTRED:
            t = [(2 * j, 2), (2 * j + 1, 2)]
        elif site == BOTTOM:
            t = [(2 * j, 1), (2 * j + 1, 2), (2 * j + 2, 1)]
        else:
            raise ValueError(site)
        out.append([(clamp(i), w) for i, w in t])
    return out


def conversion(src_fmt, out_fmt, up, down, loc):
    """((horizontal change, mode, siting), (vertical ...)) of a conversion between two formats with chroma"""
    ssx, ssy = shifts(src_fmt)
    osx, osy = shifts(out_fmt)
    gx, gy = ssx - osx, ssy - osy
    assert not (gx * gy < 0 or gx * gy > 0 and gx != gy)
    gain = gx > 0 or gy > 0
    hs, vs = siting((src_fmt if gain else out_fmt) == 1, loc)
    mode = up if gain else down
    return (gx, mode, hs), (gy, mode, vs)


def convert_plane(plane, src_fmt, out_fmt, up=REPLICATE, down=DROP, loc=0):
    """one chroma plane of the whole decoded picture at src_fmt -> the plane at out_fmt"""
    c = np.asarray(plane).astype(np.int64)
    hc, wc = c.shape
    (gx, mx, hs), (gy, my, vs) = conversion(src_fmt, out_fmt, up, down, loc)
    tx, ty = axis_taps(wc, gx, mx, hs), axis_taps(hc, gy, my, vs)
    my, mx = np.zeros((len(ty), hc), np.int64), np.zeros((len(tx), wc), np.int64)      # the taps as matrices: two clamped taps may coincide
    for m, t in ((my, ty), (mx, tx)):
        for j, taps in enumerate(t):
            for i, w in taps:
                m[j, i] += w
    return (my @ c @ mx.T + 8) >> 4


def convert_planes(planes, src_fmt, out_fmt, up=REPLICATE, down=DROP, loc=0, depth_chroma=8):
    """[Y, Cb, Cr] (Y alone for 4:0:0) at src_fmt -> the planes at out_fmt, at the coding depth; a 4:0:0 source gives chroma planes of
    1 << (depth_chroma - 1), which is the sample at the chroma OUTPUT depth: the caller applies no depth rule to them"""
    y = np.asarray(planes[0])
    if out_fmt == 0:
        return [y]
    if src_fmt == 0:
        sx, sy = shifts(out_fmt)
        c = np.full((y.shape[0] >> sy, y.shape[1] >> sx), 1 << (depth_chroma - 1), y.dtype)
        return [y, c, c.copy()]
    if src_fmt == out_fmt:
        return [y] + [np.asarray(p) for p in planes[1:]]
    return [y] + [convert_plane(p, src_fmt, out_fmt, up, down, loc).astype(y.dtype) for p in planes[1:]]


def write_plane_indices(src_fmt, out_fmt, w444, h444):
    """a literal transcription of the index arithmetic of TVideoIOYuv::writePlane for a chroma component (TVideoIOYuv.cpp:362-483):
    per written file row the source row, and per file column the source column; None for a 4:0:0 source (the constant), and
    (None, None) for a 4:0:0 file, which gets no chroma of its own.  w444 / h444: the size of the picture in luma samples.
    Literal includes its row pointer: `src += stride_src` runs after the row when (y444 & mask_y_src) == 0, so where the file has
    more rows than the source (4:2:0 -> 4:2:2 / 4:4:4) file row y reads source row (y + 1) >> 1 -- one row late on odd rows, and
    one row below the plane on the last -- where the export's rule is y >> 1.  HM's applications never take that path (every write
    passes NUM_CHROMA_FORMAT); everywhere else the two agree."""
    if out_fmt == 0:
        return None, None
    if src_fmt == 0:
        return None
    csx_file, csy_file = shifts(out_fmt)
    csx_src, csy_src = shifts(src_fmt)
    width_file = w444 >> csx_file
    mask_y_file, mask_y_src = (1 << csy_file) - 1, (1 << csy_src) - 1
    rows, src_row = [], 0
    for y444 in range(h444):
        if (y444 & mask_y_file) == 0:
            rows.append(src_row)
            # one file row: x << sx for a file narrower than the source, x >> sx for a wider one
            if csx_file < csx_src:
                sx = csx_src - csx_file
                cols = [x >> sx for x in range(width_file)]
            else:
                sx = csx_file - csx_src
                cols = [x << sx for x in range(width_file)]
        if (y444 & mask_y_src) == 0:
            src_row += 1
    return rows, cols
