"""numpy restatement of the batched export with a window and a mirror per picture (include/hmgpu.h, hmgpu_pictures_export_windows):
per slot the existing restatement of the batched export (tests/export_batch_ref.py) with the slot's crop, then the rows reversed.
No arithmetic is restated here."""
import ctypes as C

import numpy as np

from libhm_amd import abi
from tests import export_batch_ref as bref


def window_of(seq, xywh, flip=False):
    """the abi.ExportWindow of (x, y, w, h) in a picture of `seq`"""
    x, y, w, h = xywh
    return abi.make_export_window((x, seq.width - x - w, y, seq.height - y - h), flip)


def desc_with_crop(desc, crop):
    d = abi.ExportDesc()
    C.memmove(C.byref(d), C.byref(desc), C.sizeof(d))
    for i in range(4):
        d.crop[i] = crop[i]
    return d


def mirror(planes, layout):
    """every row of every plane reversed; the CbCr plane of the semi-planar layout ([H, W, 2]) pair by pair"""
    return [np.flip(p, axis=-2 if layout == abi.EXPORT_SEMIPLANAR and p.ndim == 3 else -1) for p in planes]


def export_slot_ref(seq, planes, fmt, bd, desc, scale, tensor, window):
    """what slot i of hmgpu_pictures_export_windows holds, per plane, for the picture `planes` and its abi.ExportWindow"""
    out = bref.export_batch_ref(seq, planes, fmt, bd, desc_with_crop(desc, tuple(window.crop)), scale, tensor)
    out = [np.asarray(p) for p in out]
    return mirror(out, desc.layout) if window.flip & 1 else out
