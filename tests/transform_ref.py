"""The model of the transform export (include/hmgpu.h "transform export") in numpy.  Nothing of the code under test is
involved: the blocks come from synth.coded_blocks(), QpParam from the C oracle (hmo_qp_param_fmt), and the de-quantiser is a numpy
restatement of TComTrQuant::xDeQuant written from HM's text (TComTrQuant.cpp:1203-1311), held against the oracle by
tests/test_transform_cpu.py.

Semantics restated.  Element v * size + u of the level block of a coded block of component c with top-left component sample (x0, y0)
goes to plane element (y0 + v, x0 + u); everything no coded block covers is 0, and so is everything under a PCM CU.  LEVELS: the level.
COEFFS: xDeQuant of it -- QpParam from the QP at the CU's first partition, the slice's chroma offsets and the format's chroma table; flat
scaling or the picture's list 3 * inter + component (a transform-skip block only when it is 4x4); cu_transquant_bypass: the level.
Intra CUs are exported with or without intra_dir[].  info_grid(): six int8 channels per 4x4 luma block.
"""
import ctypes as C

import numpy as np

from libhm_amd import abi
from oracle import hmoracle
from tests import synth
from tests.residual_ref import _arr, _zxy, convert          # noqa: F401  (convert: the float conversion of the dense residual form)

INV_QUANT_SCALES = (40, 45, 51, 57, 64, 72)                 # g_invQuantScales, TComRom.cpp


def subsampling(chroma_format):
    """(csx, csy) of a chroma_format_idc (0 as 1)"""
    fmt = 1 if chroma_format == 0 else chroma_format
    return (0 if fmt == 3 else 1), (1 if fmt == 1 else 0)


def qp_param(qp_y, comp, bit_depth, chroma_qp_offset, chroma_format):
    per, rem = C.c_int(), C.c_int()
    hmoracle.lib().hmo_qp_param_fmt(int(qp_y), comp, bit_depth, int(chroma_qp_offset), 1 if chroma_format == 0 else chroma_format,
                                    C.byref(per), C.byref(rem))
    return per.value, rem.value


def list_matrix(lists, size_id, list_id):
    """the factors m of one list as an n x n matrix: xSetScalingListDec / processScalingListDec (TComTrQuant.cpp:2992-3012, 3092-3106) --
    the 8x8 list replicated over ratio x ratio positions for 16x16 / 32x32, with the DC entry at position 0"""
    n = 4 << size_id
    ratio, mn = (n // 8, 8) if n > 8 else (1, n)
    coef = np.array([lists.coef[size_id][list_id][i] for i in range(mn * mn)], dtype=np.int64).reshape(mn, mn)
    m = np.kron(coef, np.ones((ratio, ratio), dtype=np.int64))
    if ratio > 1:
        m[0, 0] = lists.dc[size_id][list_id]
    return m


def dequant(level, log2_size, bit_depth, per, rem, m=None):
    """xDeQuant of a block of levels (any integer array): flat scaling, or with the list factors m (same shape)"""
    lists = m is not None
    transform_shift = 15 - bit_depth - log2_size                         # getTransformShift, maxTrDynamicRange 15
    right_shift = 6 - (transform_shift + per) + (4 if lists else 0)      # IQUANT_SHIFT, LOG2_SCALING_LIST_NEUTRAL_VALUE
    coef_bits = 15 if lists else 7                                       # dequantCoefBits = 1 + 6 + 8; scaleBits = 6 + 1
    target = min(16, 32 + right_shift - coef_bits)
    q = np.clip(np.asarray(level).astype(np.int64), -(1 << (target - 1)), (1 << (target - 1)) - 1)
    p = q * (INV_QUANT_SCALES[rem] * (np.asarray(m, dtype=np.int64) if lists else 1))
    c = (p + (1 << (right_shift - 1))) >> right_shift if right_shift > 0 else p << (-right_shift)
    return np.clip(c, -32768, 32767)


def blocks(seq, meta):
    """the coded blocks whose coefficients the planes hold -- synth.coded_blocks() minus PCM CUs -- as dicts: comp, ctu, off (into the
    CTU's piece of the dense level array), size, z (the block's first partition), zf (the partition its own flags are stored at), x0 / y0
    (component samples in the picture)"""
    fmt = seq.chroma_format
    csx, csy = subsampling(fmt)
    log2_ctu = seq.log2_ctu_size
    ctu, parts = 1 << log2_ctu, 1 << (2 * log2_ctu - 4)
    cw = (seq.width + ctu - 1) // ctu
    zx, zy = _zxy(parts)
    pm = np.asarray(meta["pred_mode"])
    ipcm = _arr(meta, "ipcm", pm)
    out = []
    for comp, a, off, size in synth.coded_blocks(meta, fmt, log2_ctu).tolist():
        second = 0
        if comp == 0 or fmt == 3:
            z = off // 16
        elif fmt == 2:
            second = 1 if off % (2 * size * size) == size * size else 0
            z = (off - second * size * size) // 8
        else:
            z = off // 4
        zf = z + second * size * size // 8                               # half the block's partitions on (a block of 2 size x 2 size luma samples)
        if ipcm[a, z]:
            continue
        sx, sy = (csx, csy) if comp else (0, 0)
        x0 = ((a % cw) * ctu + 4 * int(zx[z])) >> sx
        y0 = (((a // cw) * ctu + 4 * int(zy[z])) >> sy) + second * size
        out.append(dict(comp=comp, ctu=a, off=off, size=size, z=z, zf=zf, x0=x0, y0=y0))
    return out


def _paint(seq, meta, levels, value):
    csx, csy = subsampling(seq.chroma_format)
    w, h = seq.width, seq.height
    out = [np.zeros((h, w), dtype=np.int16), np.zeros((h >> csy, w >> csx), dtype=np.int16), np.zeros((h >> csy, w >> csx), dtype=np.int16)]
    n = np.asarray(meta["pred_mode"]).shape[0]
    levels = [np.asarray(a).reshape(n, -1) for a in levels]
    for b in blocks(seq, meta):
        size = b["size"]
        lev = levels[b["comp"]][b["ctu"], b["off"]:b["off"] + size * size].reshape(size, size)
        r = value(b, lev)
        ph, pw = out[b["comp"]].shape
        hh, ww = min(size, ph - b["y0"]), min(size, pw - b["x0"])
        if hh > 0 and ww > 0:
            out[b["comp"]][b["y0"]:b["y0"] + hh, b["x0"]:b["x0"] + ww] = r[:hh, :ww]
    return out


def levels_planes(seq, meta, levels):
    """[Y, Cb, Cr] int16 (4:0:0: the chroma planes are all zero): the levels of the picture the arrays describe.  meta: dict of HM's
    arrays [num_ctus, parts]; levels: three arrays [num_ctus, elems] in HM's dense layout"""
    return _paint(seq, meta, levels, lambda b, lev: lev)


def coeff_planes(seq, slices, meta, levels):
    """the same with xDeQuant applied to every block that is not lossless; slices: the picture's abi.SliceParams (chroma QP offsets per
    slice; the scaling lists of the picture are those of its last slice, as on the device)"""
    fmt = seq.chroma_format
    parts = 1 << (2 * seq.log2_ctu_size - 4)
    bd = [seq.bit_depth_luma, seq.bit_depth_chroma, seq.bit_depth_chroma]
    pm, depth, qp = np.asarray(meta["pred_mode"]), np.asarray(meta["depth"]).astype(np.int64), np.asarray(meta["qp"])
    byp = _arr(meta, "bypass", pm)
    ts = [_arr(meta, k, pm) for k in ("ts_y", "ts_u", "ts_v")]
    sidx = meta.get("slice_idx")
    sidx = np.zeros(pm.shape[0], dtype=np.int64) if sidx is None else np.asarray(sidx).astype(np.int64)
    lists = slices[-1].scaling_lists.contents if bool(slices[-1].scaling_lists) else None
    mats = {}

    def value(b, lev):
        comp, a, z, size = b["comp"], b["ctu"], b["z"], b["size"]
        if byp[a, z]:
            return lev
        sl = slices[min(int(sidx[a]), len(slices) - 1)]
        cu_z = z & ~((parts >> (2 * int(depth[a, z]))) - 1)
        per, rem = qp_param(int(qp[a, cu_z]), comp, bd[comp], sl.cb_qp_offset if comp == 1 else sl.cr_qp_offset if comp == 2 else 0, fmt)
        log2 = size.bit_length() - 1
        m = None
        if lists is not None and (not (int(ts[comp][a, b["zf"]]) & 1) or size == 4):      # getUseScalingList, TComTrQuant.h:180
            key = (log2 - 2, (0 if pm[a, z] == abi.MODE_INTRA else 3) + comp)
            if key not in mats:
                mats[key] = list_matrix(lists, *key)
            m = mats[key]
        return dequant(lev, log2, bd[comp], per, rem, m).astype(np.int16)
    return _paint(seq, meta, levels, value)


def info_grid(seq, meta, intra_dir=True):
    """int8 [6, H / 4, W / 4]: the info grid of the picture the arrays describe.  The flag group counts when meta holds it (a key that is
    missing or None: not staged); intra_dir: every decompress call of the picture came with the modes"""
    fmt = seq.chroma_format
    csx, csy = subsampling(fmt)
    log2_ctu = seq.log2_ctu_size
    ctu, parts, pw = 1 << log2_ctu, 1 << (2 * log2_ctu - 4), 1 << (log2_ctu - 2)
    w4, h4 = seq.width // 4, seq.height // 4
    cw = (seq.width + ctu - 1) // ctu
    zx, zy = _zxy(parts)
    ps, pm = np.asarray(meta["part_size"]), np.asarray(meta["pred_mode"])
    depth, tr = np.asarray(meta["depth"]).astype(np.int64), np.asarray(meta["tr_idx"]).astype(np.int64)
    n = ps.shape[0]
    z = np.arange(parts)[None, :] + np.zeros((n, 1), dtype=np.int64)
    rows = np.arange(n)[:, None]
    log2tu = log2_ctu - depth - tr
    tup = 1 << (2 * np.clip(log2tu - 2, 0, 4))
    ch = np.full((6, n, parts), -1, dtype=np.int64)
    ch[0], ch[1] = log2tu, tr
    # channel 2: the coded blocks painted on the grid of 4x4 luma blocks
    coded = np.zeros((3, h4, w4), dtype=np.int64)
    for b in blocks(seq, meta):
        sx, sy = (csx, csy) if b["comp"] else (0, 0)
        x0, y0, x1, y1 = (b["x0"] << sx) >> 2, (b["y0"] << sy) >> 2, ((b["x0"] + b["size"]) << sx) >> 2, ((b["y0"] + b["size"]) << sy) >> 2
        coded[b["comp"], y0:y1, x0:x1] = 1
    # channel 3: the flags at the first partition of the covering block
    flags = np.zeros((n, parts), dtype=np.int64)
    for c, key in enumerate(("ts_y", "ts_u", "ts_v")):
        if meta.get(key) is None or (c and fmt == 0):
            continue
        if c == 0 or fmt == 3:
            zf = z - z % tup
        else:
            bp = np.maximum(tup, 4)
            zf = z - z % bp
            if fmt == 2:
                zf = zf + np.where(z - zf >= bp // 2, bp // 2, 0)
        flags |= (np.asarray(meta[key]).astype(np.int64)[rows, zf] & 1) << c
    if meta.get("bypass") is not None:
        flags |= (np.asarray(meta["bypass"]) != 0).astype(np.int64) << 3
    if meta.get("ipcm") is not None:
        flags |= (np.asarray(meta["ipcm"]) != 0).astype(np.int64) << 4
    ch[3] = flags
    is_intra = pm == abi.MODE_INTRA
    if intra_dir and meta.get("intra_dir_l") is not None:
        ch[4] = np.where(is_intra, np.asarray(meta["intra_dir_l"]).astype(np.int64), -1)
        if fmt != 0:
            ch[5] = np.where(is_intra, np.asarray(meta["intra_dir_c"]).astype(np.int64), -1)
    out = np.full((6, h4, w4), -1, dtype=np.int8)
    bx = (np.arange(n)[:, None] % cw) * pw + zx[None, :]
    by = (np.arange(n)[:, None] // cw) * pw + zy[None, :]
    ok = (bx < w4) & (by < h4)
    dec = ok & (ps != abi.SIZE_NONE)
    for k in (0, 1, 3, 4, 5):
        out[k][by[dec], bx[dec]] = ch[k][dec].astype(np.int8)
    mask = coded[0] | (coded[1] << 1) | (coded[2] << 2)
    out[2][by[dec], bx[dec]] = mask[by[dec], bx[dec]].astype(np.int8)
    return out
