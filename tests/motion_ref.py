"""numpy model of the motion and block export (include/hmgpu.h "motion and block export", hmgpu_pictures_export_motion): both forms
from an hmgpu_ctu_meta-shaped dict of HM's per-partition arrays plus the slice parameters.  It restates the rules of the header and
nothing else: the z-scan map, which list is used, the values of unused lists, the nearest-exact sampling of the dense form and its
one binary32 product per value.

meta: dict with depth, part_size, pred_mode, qp, ref_idx0, ref_idx1 as [num_ctus, parts], mv0 / mv1 as [num_ctus, parts, 2] (or
[num_ctus, 2 * parts]) and slice_idx [num_ctus] (absent: all 0).  slices: a list of abi.SliceParams, or of (slice_type, ref_poc)
with ref_poc[list][index]."""
import numpy as np

from libhm_amd import abi
from tests import export_batch_ref as bref

NO_REF = abi.MOTION_NO_REF


def zscan(bx, by, s):
    """z-index inside the CTU: the low s bits of bx on the even, of by on the odd bit positions"""
    bx, by = np.asarray(bx, np.int64), np.asarray(by, np.int64)
    z = np.zeros(np.broadcast(bx, by).shape, np.int64)
    for b in range(s):
        z |= ((bx >> b) & 1) << (2 * b)
        z |= ((by >> b) & 1) << (2 * b + 1)
    return z


def block_index(width, height, log2_ctu):
    """(ctu, z) of every block of the W4 x H4 grid, each [H4, W4]"""
    s = log2_ctu - 2
    ctus_w = (width + (1 << log2_ctu) - 1) >> log2_ctu
    by, bx = np.mgrid[0:height // 4, 0:width // 4]
    return (by >> s) * ctus_w + (bx >> s), zscan(bx & ((1 << s) - 1), by & ((1 << s) - 1), s)


def _slice_table(slices):
    types, pocs = [], []
    for sl in slices:
        if isinstance(sl, abi.SliceParams):
            types.append(int(sl.slice_type))
            pocs.append([[int(sl.ref_poc[l][i]) for i in range(abi.MAX_REF)] for l in range(2)])
        else:
            types.append(int(sl[0]))
            pocs.append([list(sl[1][l]) + [0] * (abi.MAX_REF - len(sl[1][l])) for l in range(2)])
    return np.array(types, np.int64), np.array(pocs, np.int64)          # [S], [S, 2, 16]


def grid(meta, slices, width, height, log2_ctu):
    """the whole source grid: dict of mv [2, 2, H4, W4] (list, hor / ver), ref_poc [2, H4, W4], used [2, H4, W4], block [4, H4, W4]"""
    ctu, z = block_index(width, height, log2_ctu)
    n = np.asarray(meta["depth"]).shape[0]

    def take(name):
        return np.asarray(meta[name]).reshape(n, -1)[ctu, z].astype(np.int64)
    part_size, pred_mode, depth, qp = take("part_size"), take("pred_mode"), take("depth"), take("qp")
    slice_idx = np.asarray(meta["slice_idx"]).astype(np.int64)[ctu] if meta.get("slice_idx") is not None else np.zeros_like(ctu)
    types, pocs = _slice_table(slices)
    stype = types[slice_idx]
    decoded = part_size != abi.SIZE_NONE
    inter = decoded & (pred_mode == abi.MODE_INTER)
    mv = np.zeros((2, 2) + ctu.shape, np.int64)
    ref_poc = np.full((2,) + ctu.shape, NO_REF, np.int64)
    used = np.zeros((2,) + ctu.shape, bool)
    for l in range(2):
        ref_idx = take("ref_idx%d" % l)
        by_type = (stype == abi.B_SLICE) | ((stype == abi.P_SLICE) if l == 0 else False)
        used[l] = inter & by_type & (ref_idx >= 0)
        vec = np.asarray(meta["mv%d" % l]).reshape(n, -1, 2)[ctu, z].astype(np.int64)       # [H4, W4, 2]
        mv[l, 0] = np.where(used[l], vec[..., 0], 0)
        mv[l, 1] = np.where(used[l], vec[..., 1], 0)
        ref_poc[l] = np.where(used[l], pocs[slice_idx, l, np.where(used[l], ref_idx, 0)], NO_REF)
    mode = np.where(~decoded, -1, np.where(pred_mode == abi.MODE_INTER, 0, np.where(pred_mode == abi.MODE_INTRA, 1, -1)))
    block = np.stack([mode, log2_ctu - depth, np.where(decoded, part_size, -1), qp])
    return dict(mv=mv, ref_poc=ref_poc, used=used, block=block)


def _lists(mask):
    return [l for l in range(2) if (mask >> l) & 1]


def blocks(meta, slices, width, height, log2_ctu, lists=3, crop=(0, 0, 0, 0)):
    """HMGPU_MOTION_BLOCKS of one picture: mv int16 [L, 2, h4, w4], ref_poc int32 [L, h4, w4], block int8 [4, h4, w4]"""
    assert all(v % 4 == 0 for v in crop)
    g = grid(meta, slices, width, height, log2_ctu)
    l, r, t, b = (v // 4 for v in crop)
    sl = (slice(t, height // 4 - b), slice(l, width // 4 - r))
    sel = _lists(lists)
    return dict(mv=g["mv"][sel][(slice(None), slice(None)) + sl].astype(np.int16),
                ref_poc=g["ref_poc"][sel][(slice(None),) + sl].astype(np.int32),
                block=g["block"][(slice(None),) + sl].astype(np.int8))


def nearest_index(out, size):
    """source index of every output index: min(floor((2 i + 1) * size / (2 * out)), size - 1), in integers"""
    i = np.arange(out, dtype=np.int64)
    return np.minimum(((2 * i + 1) * size) // (2 * out), size - 1)


def dense(meta, slices, width, height, log2_ctu, window, out_size=None, flip=False, sample_type=abi.SAMPLE_F32, lists=3):
    """HMGPU_MOTION_DENSE of one slot.  window (x, y, w, h) in luma samples; out_size (H, W) or None (the window's size).  Returns
    flow0 / flow1 (selected lists) as bit patterns [2, H, W] (uint16 / uint32, tests/export_batch_ref.cast_bits), ref_poc int32
    [L, H, W], block int8 [4, H, W], and the index tables sx [W], sy [H] (luma positions inside the window, before the mirror)."""
    x, y, w, h = window
    H, W = (h, w) if out_size is None else out_size
    g = grid(meta, slices, width, height, log2_ctu)
    sx, sy = nearest_index(W, w), nearest_index(H, h)
    bx, by = (x + sx) >> 2, (y + sy) >> 2
    kx = np.float32(float(W) / (4.0 * w))
    ky = np.float32(float(H) / (4.0 * h))
    out = dict(sx=sx, sy=sy)
    pick = np.ix_(by, bx)
    for l in _lists(lists):
        mvx, mvy = g["mv"][l, 0][pick], g["mv"][l, 1][pick]
        if flip:
            mvx = -mvx[:, ::-1]                        # rows reversed, the horizontal component negated (as an integer: 0 stays +0)
            mvy = mvy[:, ::-1]
        dx = np.multiply(mvx.astype(np.float32), kx, dtype=np.float32)
        dy = np.multiply(mvy.astype(np.float32), ky, dtype=np.float32)
        out["flow%d" % l] = np.stack([bref.cast_bits(dx, sample_type), bref.cast_bits(dy, sample_type)])
    ref = np.stack([g["ref_poc"][l][pick] for l in _lists(lists)]).astype(np.int32)
    blk = g["block"][(slice(None),) + pick].astype(np.int8)
    out["ref_poc"] = ref[:, :, ::-1] if flip else ref
    out["block"] = blk[:, :, ::-1] if flip else blk
    return out
