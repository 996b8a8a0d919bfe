"""Loop-filter export to torch tensors (hmgpu_pictures_export_loopfilter, k_lfinfo.hip): the argument handling shared by
Context.export_loopfilter, hmdec.export_loopfilter_batch and hmdec.Picture.loopfilter.  No compute here but two small helpers.

form "grids": {"edge": int16 [N, 13, H / 4, W / 4], "sao": int8 [N, 3, 6, ctus_h, ctus_w]} -- per 4x4 luma block the boundary strength,
mean QP, tc, beta, chroma tc and exemption flags of the 4-sample edge units on its left ("ver") and top ("hor") border (channels
abi.LF_*; 0 where the block is off the 8x8 grid in that direction or the unit is not filtered), and per CTB and component the SAO type
(-1 off), first band and the four offsets as applied.  grids=("edge",) or ("sao",) selects one; crop (multiples of 8 luma samples) cuts
the edge grid only.  form "dense": {"loopfilter": [N, 3, H, W]}, one value per output sample of export_batch(windows=, flip=, size=,
filter="nearest"): the Bs of the vertical / horizontal edge whose filter can reach the sample and the luma SAO type + 1, uint8 or a float
dtype (value = float32(v) * scale[c], converted).  The SAO grid and the dense form need a filter call on the picture.
"""
from . import abi
from . import export

FORMS = {"grids": abi.LOOPFILTER_GRIDS, "dense": abi.LOOPFILTER_DENSE}
NAMES = ("edge", "sao", "loopfilter")
edge_names = ("bs_ver", "bs_hor", "qp_ver", "qp_hor", "tc_ver", "tc_hor", "beta_ver", "beta_hor", "tc_cb_ver", "tc_cb_hor", "tc_cr_ver",
              "tc_cr_hor", "flags")
sao_names = ("off", "eo_0", "eo_90", "eo_135", "eo_45", "bo")          # by TYPE + 1: what dense channel 2 indexes
sao_channels = ("type", "band", "off0", "off1", "off2", "off3")


def form_code(form):
    try:
        return form if isinstance(form, int) else FORMS[form.lower()]
    except KeyError:
        raise ValueError("unknown loop-filter form %r (grids or dense)" % (form,))


def edge_mask(grid):
    """edge grid [..., 13, H / 4, W / 4] -> bool [..., 2, H / 4, W / 4]: the block's vertical / horizontal unit is filtered (Bs > 0)"""
    return grid[..., abi.LF_BS_VER:abi.LF_BS_HOR + 1, :, :] > 0


def plan_for(seq, desc, scale=None, windows=None, n=None):
    """what an export with `desc` writes (hmgpu_loopfilter_plan_for: host code, no GPU); windows: abi.ExportWindow per picture (dense)"""
    return export.side_plan("hmgpu_loopfilter_plan_for", abi.LoopfilterPlan(), seq, desc, scale, windows, n)


def describe(seq, n, form="grids", size=None, windows=None, flip=None, dtype=None, scale=None, crop=(0, 0, 0, 0)):
    """(desc, abi.ExportScale or None, windows or None) of a call; dtype: None (uint8), a torch float dtype or an abi.SAMPLE_* code"""
    form = form_code(form)
    if form == abi.LOOPFILTER_GRIDS:
        if size is not None or windows is not None or flip is not None or dtype is not None or scale is not None:
            raise ValueError("export_loopfilter(form='grids') takes crop only: size / windows / flip / dtype / scale belong to form='dense'")
        return abi.make_loopfilter_desc(form, abi.SAMPLE_UINT, crop), None, None
    st = abi.SAMPLE_UINT if dtype is None else dtype if isinstance(dtype, int) else export.sample_type(dtype)
    if scale is not None and st == abi.SAMPLE_UINT:
        raise ValueError("scale needs a float dtype")
    desc = abi.make_loopfilter_desc(form, st, scale=(1.0, 1.0, 1.0) if scale is None else tuple(scale))
    return desc, export.make_scale(size, "nearest"), export.dense_windows(seq, crop, windows, flip, n)


def loopfilter_plan(seq, form="grids", size=None, windows=None, flip=None, dtype=None, scale=None, crop=(0, 0, 0, 0), n=None):
    """what Context.export_loopfilter with these arguments writes per picture (hmgpu_loopfilter_plan_for: host code, no GPU): an
    abi.LoopfilterPlan -- per destination slot (edge, sao, dense) the channels, width, height, element size and row bytes"""
    count = n if n is not None else (len(list(windows)) if windows is not None else 1)
    desc, sc, win = describe(seq, count, form, size, windows, flip, dtype, scale, crop)
    return plan_for(seq, desc, sc, win, count)


def export_loopfilter(call, seq, device, n, form="grids", grids=("edge", "sao"), size=None, windows=None, flip=None, dtype=None, scale=None,
                      out=None, crop=(0, 0, 0, 0), enqueue=True):
    """allocate with torch on `device` (or take the tensors of the dict `out`: only its keys are written) and run
    call(desc, scale, windows, ptrs[3], pitches[3], plane_strides[3], batch_strides[3], stream) on torch's current stream."""
    import torch
    desc, sc, win = describe(seq, n, form, size, windows, flip, dtype, scale, crop)
    plan = plan_for(seq, desc, sc, win, n)
    E, S, D = abi.LOOPFILTER_DST_EDGE, abi.LOOPFILTER_DST_SAO, abi.LOOPFILTER_DST_DENSE
    if desc.form == abi.LOOPFILTER_GRIDS:
        for g in grids:
            if g not in ("edge", "sao"):
                raise ValueError("grids: 'edge' and / or 'sao'")
        names = {k: NAMES[k] for k in (E, S) if NAMES[k] in grids}
        if not names:
            raise ValueError("grids: 'edge' and / or 'sao'")
    else:
        names = {D: NAMES[D]}
    elem = torch.uint8 if desc.sample_type == abi.SAMPLE_UINT else export.side_dtype(desc.sample_type, dtype)
    dtypes = {E: torch.int16, S: torch.int8, D: elem}

    def shape(k):
        return (n, plan.channels[k], plan.height[k], plan.width[k])
    with torch.cuda.device(device):
        flat = None
        if out is not None:
            flat = dict(out)
            if "sao" in flat and S in names:
                flat["sao"] = _sao_planes(flat["sao"], shape(S))
        res, ptrs, pitches, pstrides, bstrides = export.side_tensors(flat, device, names, shape, lambda k: dtypes[k], abi.LOOPFILTER_DSTS)
        if enqueue:
            call(desc, sc, win, ptrs, pitches, pstrides, bstrides, torch.cuda.current_stream(device).cuda_stream)
    if out is not None:
        return out
    if "sao" in res:
        res["sao"] = res["sao"].unflatten(1, (3, abi.LOOPFILTER_SAO_CHANNELS))
    return res


def _sao_planes(t, planes):
    """the caller's SAO tensor [N, 3, 6, h, w] as the run of 18 planes it goes down as: its components six planes apart"""
    import torch
    want = (planes[0], 3, abi.LOOPFILTER_SAO_CHANNELS) + tuple(planes[2:])
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != want or t.stride()[1] != abi.LOOPFILTER_SAO_CHANNELS * t.stride()[2]:
        raise ValueError("out['sao']: an int8 tensor of shape %s whose components lie six planes apart" % (want,))
    st = t.stride()
    return t.as_strided(planes, (st[0], st[2], st[3], st[4]), t.storage_offset())


def c_args(ptrs, pitches, pstrides, bstrides):
    """the ctypes arguments (dst[3], pitch[3], plane stride[3], batch stride[3]) of the C entry points"""
    return (abi.ptr_array(ptrs), abi.i64_array(pitches), abi.i64_array(pstrides), abi.i64_array(bstrides))
