"""Device export to torch tensors: layout names, output dtypes and the colour policy shared by Context.export and
hmdec.Picture.export.  No compute here: the conversion is k_export.hip behind hmgpu_picture_export.

Colour policy (the one place it is decided): an RGB export takes `matrix` / `full_range` from the caller; where the caller leaves
them None they come from the picture's VUI (matrix_coefficients, video_full_range_flag).  A stream without a colour description
(matrix 2, "unspecified") is treated as BT.709 (matrix 1); without video_signal_type it is limited range (E.3.1's default).  Codes
the kernel does not implement (anything but 0, 1, 5, 6, 9) are refused with HMGPU_EUNSUPPORTED rather than guessed.
"""
from . import abi

LAYOUTS = {"planar": abi.EXPORT_PLANAR, "yuv": abi.EXPORT_PLANAR, "semiplanar": abi.EXPORT_SEMIPLANAR, "nv12": abi.EXPORT_SEMIPLANAR,
           "rgb": abi.EXPORT_RGB}
UNSPECIFIED = 2


def resolve_colour(matrix, full_range, vui_matrix=UNSPECIFIED, vui_full_range=0):
    """(matrix, full_range) for an RGB export: the caller's values, else the VUI's, with 'unspecified' read as BT.709"""
    if matrix is None:
        matrix = 1 if vui_matrix == UNSPECIFIED else vui_matrix
    if full_range is None:
        full_range = int(vui_full_range)
    return int(matrix), int(full_range)


def torch_dtype(bytes_per_sample):
    """uint8, or for 2-byte samples torch.uint16 where this torch has it, else int16 holding the same bits"""
    import torch
    if bytes_per_sample == 1:
        return torch.uint8
    return getattr(torch, "uint16", torch.int16)


def layout_code(layout):
    if isinstance(layout, int):
        return layout
    try:
        return LAYOUTS[layout.lower()]
    except KeyError:
        raise ValueError("unknown export layout %r (one of %s)" % (layout, ", ".join(sorted(LAYOUTS))))


def make_desc(layout, bit_depth, crop, matrix, full_range, msb_aligned=False):
    """bit_depth: an int for every channel type, a (luma, chroma) pair, or None / 0 for the coding bit depths"""
    bd = (0, 0) if bit_depth is None else (bit_depth, bit_depth) if isinstance(bit_depth, int) else tuple(bit_depth)
    nbytes = 2 if msb_aligned or max(bd) > 8 or min(bd) == 0 else 1
    return abi.make_export_desc(layout_code(layout), bd, nbytes, msb_aligned, tuple(crop), matrix, full_range)


def alloc_outputs(plan, desc, device):
    """torch tensors for what `plan` describes: RGB [3, H, W]; planar (Y, Cb, Cr) 2-D; semi-planar (Y [H, W], CbCr [Hc, Wc, 2]).
    Returns (result, per-plane tensors)."""
    import torch
    dt = torch_dtype(desc.bytes_per_sample)
    dev = torch.device("cuda", device)
    if desc.layout == abi.EXPORT_RGB:
        t = torch.empty((3, plan.height[0], plan.width[0]), dtype=dt, device=dev)
        return t, [t[0], t[1], t[2]]
    planes = []
    for k in range(plan.planes):
        if desc.layout == abi.EXPORT_SEMIPLANAR and k == 1:
            planes.append(torch.empty((plan.height[1], plan.width[1], 2), dtype=dt, device=dev))
        else:
            planes.append(torch.empty((plan.height[k], plan.width[k]), dtype=dt, device=dev))
    return tuple(planes), planes


def export_tensors(call, seq, device, layout, bit_depth, crop, matrix, full_range, msb_aligned=False, on_stream=True):
    """allocate with torch on `device` and run `call(desc, ptrs, pitches, stream)` on torch's current stream"""
    import torch
    from . import export_plan
    desc = make_desc(layout, bit_depth, crop, matrix, full_range, msb_aligned)
    plan = export_plan(seq, desc)
    with torch.cuda.device(device):
        out, planes = alloc_outputs(plan, desc, device)
        stream = torch.cuda.current_stream(device).cuda_stream if on_stream else 0
        ptrs = [p.data_ptr() for p in planes]
        pitches = [p.stride(0) * p.element_size() for p in planes]
        call(desc, ptrs, pitches, stream)
    return out
