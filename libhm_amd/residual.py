"""Residual export to torch tensors (hmgpu_pictures_export_residual, k_residual.hip): the argument handling shared by
Context.export_residual, hmdec.export_residual_batch and hmdec.Picture.residual.  No compute here.

form "planes": int16 planes, each component at its own resolution -- {"y": [N, H, W], "cb" / "cr": [N, H / 2, W / 2]} (4:0:0: "y"
only).  form "dense": {"residual": [N, C, H, W]}, one value per output sample of export_batch(windows=, flip=, size=,
filter="nearest"), C the selected components in component order, int16 or a float dtype (value = float32(r) * scale[c], converted).
The residual is what the decoder adds to the prediction; it is 0 wherever no coded transform block covers the sample.
"""
from . import abi
from . import export

FORMS = {"planes": abi.RESIDUAL_PLANES, "dense": abi.RESIDUAL_DENSE}
NAMES = ("y", "cb", "cr")


def components_mask(components):
    """(0, 1, 2) -> 7; an int is taken as the mask"""
    if isinstance(components, int):
        return components
    mask = 0
    for c in components:
        if c not in (0, 1, 2):
            raise ValueError("components: 0, 1 and / or 2")
        mask |= 1 << c
    return mask


def form_code(form):
    try:
        return form if isinstance(form, int) else FORMS[form.lower()]
    except KeyError:
        raise ValueError("unknown residual form %r (planes or dense)" % (form,))


def plan_for(seq, desc, scale=None, windows=None, n=None):
    """what an export with `desc` writes (hmgpu_residual_plan_for: host code, no GPU); windows: abi.ExportWindow per picture (dense)"""
    return export.side_plan("hmgpu_residual_plan_for", abi.ResidualPlan(), seq, desc, scale, windows, n)


def describe(seq, n, form="planes", components=(0, 1, 2), size=None, windows=None, flip=None, dtype=None, scale=None, crop=(0, 0, 0, 0)):
    """(desc, abi.ExportScale or None, windows or None) of a call; dtype: None (int16), a torch float dtype or an abi.SAMPLE_* code"""
    form = form_code(form)
    mask = components_mask(components)
    if form == abi.RESIDUAL_PLANES:
        if size is not None or windows is not None or flip is not None or dtype is not None or scale is not None:
            raise ValueError("export_residual(form='planes') takes crop only: size / windows / flip / dtype / scale belong to form='dense'")
        return abi.make_residual_desc(form, mask, abi.SAMPLE_UINT, crop), None, None
    st = abi.SAMPLE_UINT if dtype is None else dtype if isinstance(dtype, int) else export.sample_type(dtype)
    if scale is not None and st == abi.SAMPLE_UINT:
        raise ValueError("scale needs a float dtype")
    desc = abi.make_residual_desc(form, mask, st, scale=(1.0, 1.0, 1.0) if scale is None else tuple(scale))
    return desc, export.make_scale(size, "nearest"), export.dense_windows(seq, crop, windows, flip, n)


def residual_plan(seq, form="planes", components=(0, 1, 2), size=None, windows=None, flip=None, dtype=None, scale=None, crop=(0, 0, 0, 0),
                  n=None):
    """what Context.export_residual with these arguments writes per picture (hmgpu_residual_plan_for: host code, no GPU): an
    abi.ResidualPlan -- per destination slot the channels, width, height, element size and row bytes.  n: the number of pictures
    (default: one per window, else 1)"""
    count = n if n is not None else (len(list(windows)) if windows is not None else 1)
    desc, sc, win = describe(seq, count, form, components, size, windows, flip, dtype, scale, crop)
    return plan_for(seq, desc, sc, win, count)


def export_residual(call, seq, device, n, form="planes", components=(0, 1, 2), size=None, windows=None, flip=None, dtype=None, scale=None,
                    out=None, crop=(0, 0, 0, 0), enqueue=True):
    """allocate with torch on `device` (or take the tensors of the dict `out`: only its keys are written) and run
    call(desc, scale, windows, ptrs[3], pitches[3], plane_strides[3], batch_strides[3], stream) on torch's current stream."""
    import torch
    desc, sc, win = describe(seq, n, form, components, size, windows, flip, dtype, scale, crop)
    plan = plan_for(seq, desc, sc, win, n)
    planes = desc.form == abi.RESIDUAL_PLANES
    elem = export.side_dtype(desc.sample_type, dtype)
    names = {k: NAMES[k] for k in range(3) if plan.channels[k]} if planes else {0: "residual"}

    def shape(k):
        return (n, plan.height[k], plan.width[k]) if planes else (n, plan.channels[k], plan.height[k], plan.width[k])
    with torch.cuda.device(device):
        out, ptrs, pitches, pstrides, bstrides = export.side_tensors(out, device, names, shape, lambda k: elem, 3)
        if enqueue:
            call(desc, sc, win, ptrs, pitches, pstrides, bstrides, torch.cuda.current_stream(device).cuda_stream)
    return out


def c_args(ptrs, pitches, pstrides, bstrides):
    """the ctypes arguments (dst[3], pitch[3], plane stride[3], batch stride[3]) of the C entry points"""
    return (abi.ptr_array(ptrs), abi.i64_array(pitches), abi.i64_array(pstrides), abi.i64_array(bstrides))
