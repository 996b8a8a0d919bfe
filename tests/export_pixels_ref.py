"""numpy restatement of the packed pixel export (include/hmgpu.h, hmgpu_pictures_export_pixels): the planes of a slot from the
existing restatements (tests/export_windows_ref.py with a window, tests/export_batch_ref.py without) stacked in channel order on the
last axis, with the A element inserted.  No arithmetic is restated here."""
import numpy as np

from libhm_amd import abi
from tests import export_batch_ref as bref
from tests import export_windows_ref as wref

# the plane (0 R, 1 G, 2 B; None: A) of every element of a pixel
CHANNELS = {abi.PIXEL_RGB: (0, 1, 2), abi.PIXEL_BGR: (2, 1, 0), abi.PIXEL_RGBA: (0, 1, 2, None), abi.PIXEL_BGRA: (2, 1, 0, None),
            abi.PIXEL_ARGB: (None, 0, 1, 2), abi.PIXEL_ABGR: (None, 2, 1, 0)}


def alpha_bits(desc, tensor, pixel, depth):
    """the A element as stored: the code value in its container, or the bit pattern of the converted alpha_value"""
    if tensor is None or tensor.sample_type == abi.SAMPLE_UINT:
        a = (1 << depth) - 1 if pixel.alpha == -1 else pixel.alpha
        return a << (16 - depth if desc.msb_aligned else 0)
    return int(bref.cast_bits(np.array([np.float32(pixel.alpha_value)], np.float32), tensor.sample_type)[0])


def pack(planes, desc, tensor, pixel, depth):
    """[H, W, C] from the three planes of a slot"""
    a = np.full_like(planes[0], alpha_bits(desc, tensor, pixel, depth))
    return np.stack([a if k is None else planes[k] for k in CHANNELS[pixel.order]], axis=-1)


def export_pixels_ref(seq, planes, fmt, bd, desc, scale, tensor, window, pixel):
    """what slot i of hmgpu_pictures_export_pixels holds for the picture `planes`: window an abi.ExportWindow, or None (desc.crop)"""
    if window is not None:
        p = wref.export_slot_ref(seq, planes, fmt, bd, desc, scale, tensor, window)
    else:
        p = [np.asarray(v) for v in bref.export_batch_ref(seq, planes, fmt, bd, desc, scale, tensor)]
    return pack(p, desc, tensor, pixel, desc.bit_depth[0] or bd[0])
