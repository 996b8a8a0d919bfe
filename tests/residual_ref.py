"""The model of the residual export (include/hmgpu.h "residual export") in numpy and the C oracle's own TU function.
Nothing of the code under test is involved.

Semantics restated.  The residual of a sample of component c is what HM adds to the prediction there: the int16 output of xIT /
invRecurTransformNxN for the transform block that covers it -- de-quantisation (scaling lists included), inverse DCT / DST, transform
skip, rotation, RDPCM, and for cu_transquant_bypass CUs the level itself -- and exactly 0 wherever no coded block covers the sample.
Covered: the sample lies in one of the blocks synth.coded_blocks() lists for the picture's arrays (the cbf chain down to the unit's
transform depth; the 4x4 chroma block shared by four 4x4 luma units included).  Zero although listed: PCM CUs; intra CUs of a picture
decoded without intra_dir[] (`intra=False`).  CUs never decoded (part_size NONE) are not listed.  4:0:0 and 4:2:0 only.

planes():  per coded block the oracle's hmo_inverse_transform_tu(_sl) with QpParam from hmoracle.qp_param and the flags HM's rules give
           the block, painted into int16 planes at each component's own resolution.
dense():   one value per output sample of a window export: luma position (left + sx, top + sy) by the integer nearest rule
           sx = min(floor((2 ox + 1) * win_w / (2 W)), win_w - 1); chroma sample ((left + sx) >> 1, (top + sy) >> 1); a flipped slot
           reverses its rows of samples; float value = float32(r) * float32(scale[c]), one product, then the conversion.
"""
import ctypes as C

import numpy as np

from libhm_amd import abi
from oracle import hmoracle
from tests import synth

REXT = {"ROTATION": 1, "IMPLICIT_RDPCM": 2, "EXPLICIT_RDPCM": 4}      # HMGPU_REXT_* (include/hmgpu.h)


def _zxy(parts):
    z = np.arange(parts)
    x = np.zeros(parts, dtype=np.int64)
    y = np.zeros(parts, dtype=np.int64)
    for b in range(8):
        x |= ((z >> (2 * b)) & 1) << b
        y |= ((z >> (2 * b + 1)) & 1) << b
    return x, y


def rotate_rdpcm(r, rotate, rdpcm):
    """the block read back to front, then running sums along rows (1) or columns (2), carried in int16 (invRdpcmNxN)"""
    r = r[::-1, ::-1] if rotate else r
    if rdpcm == 1:
        r = np.cumsum(r.astype(np.int64), axis=1)
    elif rdpcm == 2:
        r = np.cumsum(r.astype(np.int64), axis=0)
    return np.asarray(r).astype(np.int64).astype(np.uint16).view(np.int16) if rdpcm else np.ascontiguousarray(r, dtype=np.int16)


def _arr(meta, key, like):
    a = meta.get(key)
    return np.zeros_like(like) if a is None else np.asarray(a)


def block_list(seq, meta, intra=True):
    """the coded blocks that carry a residual: rows of synth.coded_blocks() minus PCM CUs and (intra=False) intra CUs"""
    log2_ctu = seq.log2_ctu_size
    blocks = synth.coded_blocks(meta, seq.chroma_format, log2_ctu)
    pm = np.asarray(meta["pred_mode"])
    ipcm = _arr(meta, "ipcm", pm)
    keep = []
    for comp, a, off, size in blocks.tolist():
        z = off // 16 if comp == 0 else off // 4
        if ipcm[a, z]:
            continue
        if pm[a, z] == abi.MODE_INTRA and not intra:
            continue
        keep.append((comp, a, off, size, z))
    return keep


def planes(seq, slices, meta, levels, intra=True):
    """[Y, Cb, Cr] int16 (4:0:0: the chroma planes are all zero): the residual of the picture the arrays describe.  meta: dict of HM's
    arrays [num_ctus, parts]; levels: three arrays [num_ctus, elems] in HM's dense layout; slices: the picture's abi.SliceParams"""
    assert seq.chroma_format in (0, 1)
    rx = REXT
    lib = hmoracle.lib()
    f = lib.hmo_inverse_transform_tu_sl
    log2_ctu = seq.log2_ctu_size
    ctu, parts = 1 << log2_ctu, 1 << (2 * log2_ctu - 4)
    w, h = seq.width, seq.height
    cw = (w + ctu - 1) // ctu
    zx, zy = _zxy(parts)
    out = [np.zeros((h, w), dtype=np.int16), np.zeros((h // 2, w // 2), dtype=np.int16), np.zeros((h // 2, w // 2), dtype=np.int16)]
    bd = [seq.bit_depth_luma, seq.bit_depth_chroma, seq.bit_depth_chroma]
    pm, depth, qp = np.asarray(meta["pred_mode"]), np.asarray(meta["depth"]).astype(np.int64), np.asarray(meta["qp"])
    byp = _arr(meta, "bypass", pm)
    ts = [_arr(meta, k, pm) for k in ("ts_y", "ts_u", "ts_v")]
    dir_l, dir_c = _arr(meta, "intra_dir_l", pm), _arr(meta, "intra_dir_c", pm)
    sidx = meta.get("slice_idx")
    sidx = np.zeros(pm.shape[0], dtype=np.int64) if sidx is None else np.asarray(sidx).astype(np.int64)
    levels = [np.asarray(a).reshape(pm.shape[0], -1) for a in levels]
    flags_seq = seq.range_ext_flags
    for comp, a, off, size, z in block_list(seq, meta, intra):
        sl = slices[min(int(sidx[a]), len(slices) - 1)]
        is_intra = pm[a, z] == abi.MODE_INTRA
        cu_z = z & ~((parts >> (2 * int(depth[a, z]))) - 1)
        lev = np.ascontiguousarray(levels[comp][a, off:off + size * size].reshape(size, size), dtype=np.int16)
        t = int(ts[comp][a, z])
        skipped = bool(byp[a, z]) or bool(t & 1)
        if byp[a, z]:
            r = lev.copy()
        else:
            cqo = sl.cb_qp_offset if comp == 1 else sl.cr_qp_offset if comp == 2 else 0
            per, rem = hmoracle.qp_param(int(qp[a, cu_z]), comp, bd[comp], cqo)
            fl = (1 if (comp == 0 and is_intra) else 0) | (2 if t & 1 else 0)
            r = np.zeros((size, size), dtype=np.int16)
            lists = sl.scaling_lists if bool(sl.scaling_lists) else None
            f(lev.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), size, int(size).bit_length() - 1, bd[comp], per, rem, fl, lists,
              (0 if is_intra else 3) + comp)
        if skipped:
            if is_intra:
                mode = int(dir_l[a, z]) if comp == 0 else int(dir_c[a, z])
                if comp and mode == 36:                                   # DM_CHROMA_IDX: the luma mode of the CU's first partition (4:2:0)
                    mode = int(dir_l[a, cu_z])
                rd = (1 if mode == 10 else 2 if mode == 26 else 0) if flags_seq & rx["IMPLICIT_RDPCM"] else 0
                r = rotate_rdpcm(r, bool(flags_seq & rx["ROTATION"]) and size == 4, rd)
            else:
                r = rotate_rdpcm(r, False, (t >> 1) & 3 if flags_seq & rx["EXPLICIT_RDPCM"] else 0)
        x0 = ((a % cw) * ctu + 4 * int(zx[z])) >> (1 if comp else 0)
        y0 = ((a // cw) * ctu + 4 * int(zy[z])) >> (1 if comp else 0)
        ph, pw = out[comp].shape
        hh, ww = min(size, ph - y0), min(size, pw - x0)
        if hh > 0 and ww > 0:
            out[comp][y0:y0 + hh, x0:x0 + ww] = r[:hh, :ww]
    return out


def crop(pl, c):
    """the PLANES form of a crop (left, right, top, bottom in luma samples)"""
    l, r, t, b = c
    h, w = pl[0].shape
    return [pl[0][t:h - b, l:w - r], pl[1][t // 2:(h - b) // 2, l // 2:(w - r) // 2], pl[2][t // 2:(h - b) // 2, l // 2:(w - r) // 2]]


def nearest(n_in, n_out):
    """source index of every output index: min(floor((2 i + 1) * in / (2 * out)), in - 1)"""
    i = np.arange(n_out, dtype=np.int64)
    return np.minimum(((2 * i + 1) * n_in) // (2 * n_out), n_in - 1)


def convert(r, scale, dtype):
    """int16 residuals -> elements of `dtype` ("int16", "float16", "bfloat16", "float32") as integers of the element's width"""
    if dtype == "int16":
        return r.astype(np.int16)
    f = r.astype(np.float32) * np.float32(scale)
    if dtype == "float32":
        return f.view(np.uint32)
    if dtype == "float16":
        return f.astype(np.float16).view(np.uint16)
    u = f.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def dense(pls, window, flip, size, components=(0, 1, 2), dtype="int16", scale=(1.0, 1.0, 1.0)):
    """one slot [C, H, W] of the DENSE form from the planes of planes(): window (left, top, w, h) in luma samples of the coded picture"""
    left, top, ww, wh = window
    H, W = size
    sx, sy = left + nearest(ww, W), top + nearest(wh, H)
    out = []
    for c in components:
        s = 1 if c else 0
        v = pls[c][(sy >> s)[:, None], (sx >> s)[None, :]]
        if flip:
            v = v[:, ::-1]
        out.append(convert(np.ascontiguousarray(v), scale[c], dtype))
    return np.stack(out, axis=0)
