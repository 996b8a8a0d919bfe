"""Picture import from torch tensors (Context.import_batch / import_picture; include/hmgpu.h "picture import"): the descriptor and the
source pointers, pitches and batch strides of the tensors export_batch returns -- one stacked tensor, a tuple of planes, packed
pixels or a channels-last tensor."""
import numpy as np

from . import abi
from . import export

PIXELS = {"rgb": abi.PIXEL_RGB, "bgr": abi.PIXEL_BGR, "rgba": abi.PIXEL_RGBA, "bgra": abi.PIXEL_BGRA, "argb": abi.PIXEL_ARGB,
          "abgr": abi.PIXEL_ABGR}


def inverse_affine(depth, mean=None, std=None):
    """(scale, bias), float32 triples, that undo export.affine: x = (v / (2^D - 1) - mean_k) / std_k gives back
    v = x * scale_k + bias_k with scale_k = (2^D - 1) * std_k and bias_k = (2^D - 1) * mean_k, each computed in double and rounded
    once.  depth: an int, or one per plane"""
    d = (depth,) * 3 if isinstance(depth, int) else tuple(depth) + (depth[-1],) * (3 - len(depth))
    mean = (0.0,) * 3 if mean is None else tuple(float(m) for m in mean)
    std = (1.0,) * 3 if std is None else tuple(float(v) for v in std)
    scale = tuple(np.float32(float((1 << d[k]) - 1) * std[k]) for k in range(3))
    bias = tuple(np.float32(float((1 << d[k]) - 1) * mean[k]) for k in range(3))
    return scale, bias


def unsqueeze(tensors):
    """the tensors of one picture with a batch dimension of 1 in front"""
    import torch
    if isinstance(tensors, torch.Tensor):
        return tensors.unsqueeze(0)
    return tuple(t.unsqueeze(0) for t in tensors)


def element(dtype):
    """(abi.SAMPLE_*, element bytes) of a torch dtype"""
    import torch
    if dtype == torch.uint8:
        return abi.SAMPLE_UINT, 1
    if dtype in (getattr(torch, "uint16", torch.int16), torch.int16):
        return abi.SAMPLE_UINT, 2
    if dtype in (torch.float16, torch.bfloat16):
        return export.sample_type(dtype), 2
    if dtype == torch.float32:
        return abi.SAMPLE_F32, 4
    raise ValueError("dtype %r: uint8, uint16 / int16, float16, bfloat16 or float32" % (dtype,))


def _plane(t, n, es, what):
    """(pointer, pitch, batch stride, height, width) of a [N, H, W] plane whose rows are dense"""
    if t.dim() != 3 or t.shape[0] != n:
        raise ValueError("%s: a [%d, H, W] tensor" % (what, n))
    if t.shape[2] > 1 and t.stride(2) != 1:
        raise ValueError("%s: the elements of a row must be dense" % what)
    pitch = t.stride(1) * es if t.shape[1] > 1 else t.shape[2] * es
    return t.data_ptr(), pitch, t.stride(0) * es if n > 1 else pitch * t.shape[1], t.shape[1], t.shape[2]


def _pixels(t, n, es, nch, what):
    """(pointer, pitch, batch stride, height, width) of [N, H, W, C] pixels, the elements of a row dense"""
    if t.dim() != 4 or t.shape[0] != n or t.shape[3] != nch:
        raise ValueError("%s: a [%d, H, W, %d] tensor" % (what, n, nch))
    if t.stride(3) != 1 or (t.shape[2] > 1 and t.stride(2) != nch):
        raise ValueError("%s: the elements of a row must be dense" % what)
    pitch = t.stride(1) * es if t.shape[1] > 1 else t.shape[2] * nch * es
    return t.data_ptr(), pitch, t.stride(0) * es if n > 1 else pitch * t.shape[1], t.shape[1], t.shape[2]


def sources(tensors, n, layout, pixel):
    """(order, [(pointer, pitch, batch stride)] per plane, (height, width) of the source, dtype, source has chroma planes)"""
    import torch
    single = isinstance(tensors, torch.Tensor)
    planes = [tensors] if single else list(tensors)
    if not planes or any(not isinstance(t, torch.Tensor) for t in planes):
        raise ValueError("tensors: a torch tensor or a tuple of them")
    dtype = planes[0].dtype
    if any(t.dtype != dtype for t in planes):
        raise ValueError("tensors: one dtype for every plane")
    es = element(dtype)[1]
    order = -1
    if layout == abi.EXPORT_RGB:
        if pixel is not None:
            if pixel not in PIXELS or not single:
                raise ValueError("pixel: one of %s, with one [N, H, W, C] tensor" % sorted(PIXELS))
            order = PIXELS[pixel]
            spans = [_pixels(planes[0], n, es, 3 if order <= abi.PIXEL_BGR else 4, "tensors")]
        elif single:
            t = planes[0]
            if t.dim() != 4 or t.shape[0] != n or t.shape[1] != 3:
                raise ValueError("tensors: one [%d, 3, H, W] tensor" % n)
            if t.stride(1) == 1 and t.stride(3) == 3:      # channels-last: the bytes of pixel="rgb"
                order = abi.PIXEL_RGB
                spans = [_pixels(t.permute(0, 2, 3, 1), n, es, 3, "tensors")]
            else:
                spans = [_plane(t[:, k], n, es, "tensors[:, %d]" % k) for k in range(3)]
        else:
            if len(planes) != 3:
                raise ValueError("tensors: three [N, H, W] planes R, G, B")
            spans = [_plane(t, n, es, "tensors[%d]" % k) for k, t in enumerate(planes)]
    elif layout == abi.EXPORT_PLANAR:
        if single and planes[0].dim() == 4:
            t = planes[0]
            if t.shape[0] != n or t.shape[1] != 3:
                raise ValueError("tensors: one [%d, 3, H, W] tensor (4:4:4), or a tuple of planes" % n)
            spans = [_plane(t[:, k], n, es, "tensors[:, %d]" % k) for k in range(3)]
        else:
            if len(planes) not in (1, 3):
                raise ValueError("tensors: (Y,) or (Y, Cb, Cr)")
            spans = [_plane(t, n, es, "tensors[%d]" % k) for k, t in enumerate(planes)]
    else:
        if len(planes) not in (1, 2):
            raise ValueError("tensors: (Y,) or (Y, CbCr)")
        spans = [_plane(planes[0], n, es, "tensors[0]")]
        if len(planes) == 2:
            spans.append(_pixels(planes[1], n, es, 2, "tensors[1]"))
    return order, [s[:3] for s in spans], (spans[0][3], spans[0][4]), dtype, len(spans) > 1


def on_device(t, device):
    return t.is_cuda and t.device.index == device


def import_yuvpack(ctx, pics, t, yuv, chroma_down, chroma_loc, size, on_stream):
    """Context.import_batch(yuv=): the one tensor of words export_batch(yuv=) returns, [N, H, W, 2 or 4] elements, [N, H, W] int32
    (Y410) or [N, H, P / 4] int32 (V210: rows of P bytes, the width from size=, else all the pixels P has room for)"""
    import torch
    code = abi.yuvpack_code(yuv)
    n, es = len(pics), abi.YUVPACK_ELEMENT[code]
    if not isinstance(t, torch.Tensor) or not on_device(t, ctx.device):
        raise ValueError("tensors: one tensor of words on the context's GPU (cuda:%d)" % ctx.device)
    per = {abi.YUVPACK_UYVY: 2, abi.YUVPACK_YUY2: 2, abi.YUVPACK_Y210: 2, abi.YUVPACK_Y216: 2, abi.YUVPACK_AYUV: 4, abi.YUVPACK_Y416: 4}.get(code)
    if t.element_size() != es or t.is_floating_point() or t.dim() != (4 if per else 3) or t.shape[0] != n or (per and t.shape[3] != per):
        raise ValueError("tensors: the [%d, H, ...] tensor of %d-byte words that export_batch(yuv=%r) returns" % (n, es, yuv))
    st = t.stride()
    if (per and (st[3] != 1 or (t.shape[2] > 1 and st[2] != per))) or (not per and t.shape[2] > 1 and st[2] != 1):
        raise ValueError("tensors: the words of a row must be dense")
    h = t.shape[1]
    w = t.shape[2] * 4 // 16 * 6 if code == abi.YUVPACK_V210 else t.shape[2]
    if size is not None:
        if size[0] > h or size[1] > w:
            raise ValueError("size: at most the tensor's own (%d, %d)" % (h, w))
        h, w = size
    if chroma_down not in abi.DOWN_FILTERS:
        raise ValueError("chroma_down: one of %s" % sorted(abi.DOWN_FILTERS))
    row = t.shape[2] * (per or 1) * es
    pitch = st[1] * es if t.shape[1] > 1 else row
    d = abi.YUVPACK_DEPTH[code]
    desc = abi.make_import_desc(abi.EXPORT_PLANAR, -1, (w, h), (d, d), 1 if d <= 8 else 2, 0, abi.SAMPLE_UINT,
                                chroma_format=abi.YUVPACK_CHROMA[code], down=chroma_down, loc=chroma_loc)
    stream = torch.cuda.current_stream(ctx.device).cuda_stream if on_stream else 0
    ctx.import_yuvpack_into(pics, desc, abi.make_import_yuvpack(code), t.data_ptr(), pitch, st[0] * es if n > 1 else pitch * t.shape[1],
                            1 if on_stream else 0, stream)


def import_tensors(ctx, pics, tensors, layout, pixel, bit_depth, chroma_format, chroma_down, chroma_loc, matrix, full_range, msb_aligned,
                   scale, bias, mean, std, size, on_stream):
    import torch
    seq, n = ctx.seq, len(pics)
    lay = export.layout_code(layout)
    order, spans, (h, w), dtype, has_chroma = sources(tensors, n, lay, pixel)
    for t in ([tensors] if isinstance(tensors, torch.Tensor) else tensors):
        if not on_device(t, ctx.device):
            raise ValueError("tensors: on the context's GPU (cuda:%d)" % ctx.device)
    if size is not None:
        if size[0] > h or size[1] > w:
            raise ValueError("size: at most the tensors' own (%d, %d)" % (h, w))
        h, w = size
    fmt = seq.chroma_format if chroma_format is None else abi.CHROMA_FORMATS.get(chroma_format, chroma_format)
    if lay != abi.EXPORT_RGB and not has_chroma and fmt != 0 and seq.chroma_format != 0:
        raise ValueError("tensors: the chroma planes of a %s source are missing" % chroma_format)
    if chroma_down not in abi.DOWN_FILTERS:
        raise ValueError("chroma_down: one of %s" % sorted(abi.DOWN_FILTERS))
    bd = (0, 0) if bit_depth is None else (bit_depth, bit_depth) if isinstance(bit_depth, int) else tuple(bit_depth)
    depths = (bd[0] or seq.bit_depth_luma, bd[0] or seq.bit_depth_luma) if lay == abi.EXPORT_RGB else \
        (bd[0] or seq.bit_depth_luma, bd[1] or seq.bit_depth_chroma)
    stype, es = element(dtype)
    sc, bi = (1.0,) * 3, (0.0,) * 3
    if stype == abi.SAMPLE_UINT:
        if any(v is not None for v in (mean, std, scale, bias)):
            raise ValueError("mean / std / scale / bias need float tensors")
        nbytes = es
    else:
        if (scale is not None or bias is not None) and (mean is not None or std is not None):
            raise ValueError("either scale= / bias= or mean= / std=")
        sc, bi = inverse_affine(depths, mean, std)
        sc = sc if scale is None else tuple(scale)
        bi = bi if bias is None else tuple(bias)
        looked_at = depths if lay == abi.EXPORT_RGB or seq.chroma_format != 0 else depths[:1]
        nbytes = 2 if max(looked_at) > 8 else 1
    desc = abi.make_import_desc(lay, order, (w, h), bd, nbytes, int(bool(msb_aligned)), stype, sc, bi, fmt, chroma_down, chroma_loc,
                                matrix, full_range)
    stream = torch.cuda.current_stream(ctx.device).cuda_stream if on_stream else 0
    ctx.import_into(pics, desc, [s[0] for s in spans], [s[1] for s in spans], [s[2] for s in spans], 1 if on_stream else 0, stream)
