"""numpy restatement of the scaled device export (include/hmgpu.h "scaled export", k_export_scale.hip): the unscaled export of
tests/export_ref.py resampled with the tables hmgpu_export_scale_taps publishes, in the documented integer arithmetic."""
import numpy as np

import libhm_amd
from libhm_amd import abi
from tests import export_ref as ref


def tables(seq, desc, scale):
    """{(chroma, axis): (first, count, weights [out, taps])} of every table the export uses"""
    classes = [0] if desc.layout == ref.RGB or seq.chroma_format == 0 else [0, 1]
    return {(k, ax): libhm_amd.export_scale_taps(seq, desc, scale, k, ax) for k in classes for ax in (0, 1)}


def matrix(tab, n_in):
    """the table as an [out, in] integer matrix"""
    first, count, w = tab
    m = np.zeros((len(first), n_in), np.int64)
    for i in range(len(first)):
        m[i, first[i]:first[i] + count[i]] = w[i, :count[i]]
    return m


def resample(plane, tx, ty, depth, e):
    """one plane of code values 0 .. 2^depth - 1: horizontal taps, E fractional bits kept, vertical taps, clip"""
    s = np.asarray(plane, np.int64)
    h = s @ matrix(tx, s.shape[1]).T
    assert np.abs(h).max(initial=0) < 2 ** 31
    t = (h + (1 << (13 - e))) >> (14 - e)
    v = matrix(ty, s.shape[0]) @ t + (1 << (13 + e))
    assert np.abs(v).max(initial=0) < 2 ** 31
    return np.clip(v >> (14 + e), 0, (1 << depth) - 1)


def export_scaled(planes, fmt, bd, desc, plan, tabs):
    """what the scaled export writes, as export_ref's functions give it: RGB [3, H, W]; planar [Y, Cb, Cr]; semi-planar
    [Y, CbCr as H x W x 2] (Y only for 4:0:0); values as the container holds them"""
    e = int(plan.coef[11])
    out_bd = (desc.bit_depth[0] or bd[0], desc.bit_depth[1] or bd[1])
    crop = tuple(desc.crop)
    if desc.layout == ref.RGB:
        d = out_bd[0]
        src = ref.export_rgb(planes, fmt, bd, d, list(plan.coef), crop)
        out = np.stack([resample(p, tabs[(0, 0)], tabs[(0, 1)], d, e) for p in src])
        return out << (16 - d if desc.msb_aligned else 0)
    src = ref.export_yuv(planes, fmt, bd, out_bd, ref.PLANAR, crop)
    out = [resample(src[0], tabs[(0, 0)], tabs[(0, 1)], out_bd[0], e) << (16 - out_bd[0] if desc.msb_aligned else 0)]
    if fmt != 0:
        cc = [resample(p, tabs[(1, 0)], tabs[(1, 1)], out_bd[1], e) << (16 - out_bd[1] if desc.msb_aligned else 0) for p in src[1:]]
        out += cc if desc.layout == ref.PLANAR else [np.stack(cc, axis=-1)]
    return out


def scale_of(size, filt):
    """abi.ExportScale from (height, width)"""
    return abi.make_export_scale(size[1], size[0], filt)
