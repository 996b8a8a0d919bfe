"""numpy restatement of the colour stage of the RGB exports (include/hmgpu.h "colour export", hmgpu_pictures_export_colour): a
per-channel shaper and a 3D lattice with tetrahedral interpolation, applied to the integer planes of the existing restatements
(tests/export_batch_ref.py, which resamples with tests/scale_ref.py) before the container shift, the float map
(tests/export_batch_ref.py), the mirror (tests/export_windows_ref.py) and the packing (tests/export_pixels_ref.py).  Only the LUT
arithmetic is stated here; it is integer arithmetic, so equality is exact.

A LUT is (depth, lattice, shaper): lattice None or [L, L, L, 3] indexed (b, g, r, channel), shaper None or [3, 2^depth]."""
import ctypes as C

import numpy as np

from libhm_amd import abi
from tests import export_batch_ref as bref
from tests import export_pixels_ref as pref
from tests import export_windows_ref as wref
from tests import scale_ref as sref  # noqa: F401  (the resampling under bref.integers; named so that a reader finds it)


def positions(v, depth, shaper):
    """step 1: [3, ...] positions 0 .. 65535 of the code values v [3, ...]"""
    v = np.asarray(v, np.int64)
    if shaper is not None:
        sh = np.asarray(shaper, np.int64)
        return np.stack([sh[c][v[c]] for c in range(3)])
    return (v << (16 - depth)) | (v >> (2 * depth - 16))


def cells(u, size):
    """step 3: (cell index, fraction) per channel"""
    t = u * (size - 1)
    return t >> 16, t & 0xffff


def lut_apply(rgb, depth, lattice, shaper):
    """steps 1 to 4 on the integers rgb [3, ...] (R, G, B): the integers that take their place"""
    rgb = np.asarray(rgb, np.int64)
    assert rgb.min() >= 0 and rgb.max() < (1 << depth)
    u = positions(rgb, depth, shaper)
    if lattice is None:
        return u
    lat = np.asarray(lattice, np.int64)
    size = lat.shape[0]
    i, f = cells(u, size)
    assert i.max() <= size - 2
    order = np.argsort(-f, axis=0, kind="stable")                    # the axes by descending fraction
    fs = np.take_along_axis(f, order, axis=0)
    w = [65536 - fs[0], fs[0] - fs[1], fs[1] - fs[2], fs[2]]
    axes = np.arange(3).reshape((3,) + (1,) * (rgb.ndim - 1))
    idx = i.copy()
    acc = w[0][..., None] * lat[idx[2], idx[1], idx[0]]
    for k in range(3):
        idx = idx + (axes == order[k])                               # one step along the axis of the k-th largest fraction
        acc = acc + w[k + 1][..., None] * lat[idx[2], idx[1], idx[0]]
    acc = acc + 32768
    assert acc.max() < (1 << 32)                                     # unsigned 32-bit arithmetic on the device
    return np.moveaxis(acc >> 16, -1, 0)


def coverage(rgb, depth, size, shaper):
    """what the integers rgb [3, ...] exercise of a lattice of `size` nodes per axis: the strict orderings of the three fractions
    that occur (of 6), whether a two-way and a three-way tie occur, and per axis whether cell 0 and cell size - 2 occur"""
    i, f = cells(positions(np.asarray(rgb, np.int64), depth, shaper), size)
    i, f = i.reshape(3, -1), f.reshape(3, -1)
    distinct = (f[0] != f[1]) & (f[1] != f[2]) & (f[0] != f[2])
    orderings = {tuple(o) for o in np.argsort(-f[:, distinct], axis=0).T}
    three = (f[0] == f[1]) & (f[1] == f[2])
    return {"orderings": len(orderings), "tie2": bool((~distinct & ~three).any()), "tie3": bool(three.any()),
            "cell0": [bool((i[c] == 0).any()) for c in range(3)], "cell_last": [bool((i[c] == size - 2).any()) for c in range(3)]}


def covered(cov):
    return cov["orderings"] == 6 and cov["tie2"] and cov["tie3"] and all(cov["cell0"]) and all(cov["cell_last"])


def identity_lattice(size, depth):
    """node n of every axis: round(n * M / (size - 1)), half away from zero"""
    m = (1 << depth) - 1
    ramp = np.array([(2 * n * m + (size - 1)) // (2 * (size - 1)) for n in range(size)], np.uint16)
    lat = np.zeros((size, size, size, 3), np.uint16)
    lat[..., 0] = ramp[None, None, :]
    lat[..., 1] = ramp[None, :, None]
    lat[..., 2] = ramp[:, None, None]
    return lat


def _plain(desc, crop=None):
    """the descriptor without the container shift (and with another crop): the colour stage sees the integers before it"""
    d = abi.ExportDesc()
    C.memmove(C.byref(d), C.byref(desc), C.sizeof(d))
    d.msb_aligned = 0
    if crop is not None:
        for k in range(4):
            d.crop[k] = crop[k]
    return d


def integers(seq, planes, fmt, bd, desc, scale, window):
    """[3, H, W]: the integers (R, G, B) of a slot before the colour stage, unmirrored"""
    d = _plain(desc, tuple(window.crop) if window is not None else None)
    return np.stack(bref.integers(seq, planes, fmt, bd, d, scale))


def finish(ints, desc, tensor, window, pixel):
    """step 5: the container shift or the float map, the mirror, the packing; planes [3][H, W], or [H, W, C] with `pixel`"""
    depth = desc.bit_depth[0]
    if tensor is None or tensor.sample_type == abi.SAMPLE_UINT:
        out = [np.asarray(p, np.int64) << (16 - depth if desc.msb_aligned else 0) for p in ints]
    else:
        out = bref.tensor_bits(list(ints), tensor)
    if window is not None and window.flip & 1:
        out = wref.mirror(out, abi.EXPORT_RGB)
    return out if pixel is None else pref.pack(out, desc, tensor, pixel, depth)


def export_colour_ref(seq, planes, fmt, bd, desc, scale, tensor, window, pixel, lut):
    """what slot i of hmgpu_pictures_export_colour holds for the picture `planes`; desc.bit_depth[0] is the output depth (not 0);
    window an abi.ExportWindow or None (desc.crop); pixel an abi.ExportPixel or None (planes); lut (depth, lattice, shaper)"""
    depth, lattice, shaper = lut
    assert desc.layout == abi.EXPORT_RGB and depth == desc.bit_depth[0]
    return finish(lut_apply(integers(seq, planes, fmt, bd, desc, scale, window), depth, lattice, shaper), desc, tensor, window, pixel)
