"""Scaled device export on the GPU: k_export_scale.hip behind hmgpu_picture_export_scaled / hmdec_picture_export_scaled /
Picture.export(size=...), bit-exact against the numpy restatement (tests/scale_ref.py), against the unscaled export at equal size,
against HM's `TAppDecoder -d N` files, and ordered against torch's streams."""
import itertools

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, hmdec
from tests import export_ref as ref
from tests import golden_util as gu
from tests import scale_ref as sref

pytestmark = pytest.mark.gpu

CANARY = 0xA5
FILTERS = [abi.SCALE_NEAREST, abi.SCALE_BILINEAR, abi.SCALE_BICUBIC, abi.SCALE_AREA]


def _torch():
    import torch
    return torch


def random_planes(w, h, fmt, bd, seed):
    rng = np.random.default_rng(seed)
    sx, sy = ref.chroma_shift(fmt)
    return [rng.integers(0, 1 << bd[0], (h, w)).astype(np.int16)] + \
           [rng.integers(0, 1 << bd[1], (h >> sy, w >> sx)).astype(np.int16) for _ in range(2)]


def export_raw(ctx, pic, desc, scale, plan, pad, on_stream):
    """scaled export into uint8 device buffers whose rows are `pad` bytes longer than needed, canaries first"""
    torch = _torch()
    bufs, pitches = [], []
    for k in range(plan.planes):
        pitch = plan.row_bytes[k] + pad
        bufs.append(torch.full((plan.height[k], pitch), CANARY, dtype=torch.uint8, device="cuda:%d" % ctx.device))
        pitches.append(pitch)
    torch.cuda.current_stream().synchronize()
    ctx.export_into(pic, desc, [b.data_ptr() for b in bufs], pitches, on_stream, torch.cuda.current_stream().cuda_stream if on_stream else 0, scale)
    if on_stream:
        torch.cuda.current_stream().synchronize()
    else:
        ctx.sync()
    out = []
    for k, b in enumerate(bufs):
        a = b.cpu().numpy()
        assert (a[:, plan.row_bytes[k]:] == CANARY).all(), "padding written (plane %d)" % k
        a = a[:, :plan.row_bytes[k]]
        out.append((a.view("<u2") if desc.bytes_per_sample == 2 else a).astype(np.int64))
    return out


def expected(seq, planes, fmt, bd, desc, scale, plan):
    want = sref.export_scaled(planes, fmt, bd, desc, plan, sref.tables(seq, desc, scale))
    return [w.reshape(w.shape[0], -1) for w in want]


def check_cases(seq, planes, fmt, bd, cases, label):
    n = 0
    with libhm_amd.Context(seq) as ctx:
        pic = ctx.acquire()
        ctx.upload(pic, planes)
        for i, (desc, scale) in enumerate(cases):
            plan = libhm_amd.export_scaled_plan(seq, desc, scale)
            want = expected(seq, planes, fmt, bd, desc, scale, plan)
            got = export_raw(ctx, pic, desc, scale, plan, 64 if i % 2 == 0 else 3, i % 3 != 0)
            assert len(got) == len(want)
            for k in range(len(want)):
                assert np.array_equal(got[k], want[k]), (label, desc.layout, list(desc.bit_depth), desc.bytes_per_sample, desc.msb_aligned,
                                                         tuple(desc.crop), scale.width, scale.height, scale.filter, k)
            n += 1
    return n


# (height, width) from a 200 x 72 picture: 2x and 3.7x reductions, 1.5x and 8x enlargements, asymmetric, tiny; with a crop
SIZES = [((36, 100), (0, 0, 0, 0)), ((20, 54), (0, 0, 0, 0)), ((108, 300), (0, 0, 0, 0)), ((576, 1600), (0, 0, 0, 0)),
         ((24, 224), (0, 0, 0, 0)), ((4, 8), (0, 0, 0, 0)), ((30, 50), (4, 8, 2, 6))]
CONTAINERS = [(8, 1, 0), (10, 2, 0), (10, 2, 1), (16, 2, 0)]


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("bd", [(8, 8), (10, 10), (12, 12)])
def test_random_planes_bit_exact(fmt, bd):
    """every layout x filter x size, the containers in turn, against the numpy restatement; canaries in the row padding stay"""
    w, h = 200, 72
    seq = abi.make_seq(w, h, bd[0], bd[1], max_pictures=2)
    seq.chroma_format = fmt
    planes = random_planes(w, h, fmt, bd, seed=fmt * 100 + bd[0])
    cases = []
    for j, (layout, filt, (size, crop)) in enumerate(itertools.product((ref.PLANAR, ref.SEMIPLANAR, ref.RGB), FILTERS, SIZES)):
        out_bd, nbytes, msb = CONTAINERS[j % len(CONTAINERS)]
        if layout == ref.RGB and out_bd == 16:
            out_bd = 12
        mats = (9, 1) if j % 2 else (1, 0)
        cases.append((abi.make_export_desc(layout, out_bd, nbytes, msb, crop, *mats), sref.scale_of(size, filt)))
    if fmt == 3:                                    # the identity matrix (GBR)
        cases.append((abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 0, 0), sref.scale_of((36, 100), abi.SCALE_BICUBIC)))
    cases.append((abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 180, 0, 52), 1, 0), sref.scale_of((1, 1), abi.SCALE_AREA)))   # 20 x 20 -> 1 x 1
    for layout in (ref.PLANAR, ref.SEMIPLANAR):     # luma and chroma at different output depths: one E, each plane its own clip
        cases.append((abi.make_export_desc(layout, (12, 9), 2, 1, (0, 0, 0, 0), 1, 0), sref.scale_of((36, 100), abi.SCALE_BICUBIC)))
        cases.append((abi.make_export_desc(layout, (8, 10), 2, 0, (4, 8, 2, 6), 1, 0), sref.scale_of((108, 300), abi.SCALE_BILINEAR)))
    assert check_cases(seq, planes, fmt, bd, cases, "random") == len(cases)


@pytest.mark.parametrize("fmt", [0, 1])
def test_large_reductions(fmt):
    """a 1920 x 1080 picture to 60 x 34 (32x) with every filter, and to 224 x 224, RGB and planar"""
    w, h, bd = 1920, 1080, (10, 10)
    seq = abi.make_seq(w, h, bd[0], bd[1], max_pictures=2)
    seq.chroma_format = fmt
    planes = random_planes(w, h, fmt, bd, seed=7 + fmt)
    cases = []
    for filt, layout in itertools.product(FILTERS, (ref.PLANAR, ref.RGB)):
        cases.append((abi.make_export_desc(layout, 8, 1, 0, (0, 0, 0, 0), 1, 0), sref.scale_of((34, 60), filt)))
        cases.append((abi.make_export_desc(layout, 10, 2, 1, (0, 0, 0, 0), 1, 0), sref.scale_of((224, 224), filt)))
    assert check_cases(seq, planes, fmt, bd, cases, "large") == len(cases)


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_equal_size_equals_unscaled(fmt):
    """at the crop's own size every filter gives what hmgpu_picture_export gives, bit for bit"""
    torch = _torch()
    w, h, bd = 200, 72, (10, 10)
    seq = abi.make_seq(w, h, bd[0], bd[1], max_pictures=2)
    seq.chroma_format = fmt
    planes = random_planes(w, h, fmt, bd, seed=40 + fmt)
    with libhm_amd.Context(seq) as ctx:
        pic = ctx.acquire()
        ctx.upload(pic, planes)
        for layout, crop, filt in itertools.product(("planar", "nv12", "rgb"), ((0, 0, 0, 0), (4, 8, 2, 6)), FILTERS):
            cw, ch = w - crop[0] - crop[1], h - crop[2] - crop[3]
            name = {0: "nearest", 1: "bilinear", 2: "bicubic", 3: "area"}[filt]
            a = ctx.export(pic, layout, 10, crop, 1, 0)
            b = ctx.export(pic, layout, 10, crop, 1, 0, size=(ch, cw), filter=name)
            torch.cuda.synchronize()
            for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
                assert torch.equal(x, y), (layout, crop, name)


# ------------------------------------------------------------------------------------------------ libhmdec
HM_D = ["d8_ldp_main10_208x120", "d10_ldb_main12_208x120", "d16_ldp_main8_416x240", "d8_ldb_422_main10_208x120",
        "d8_intra_444_ccp_main10_208x120", "d10_ldp_crop_main8_204x116", "d8_ldb_mono_wp_crop_main10_204x116"]


def _as_np(t):
    torch = _torch()
    if t.dtype == torch.int16 or t.dtype == getattr(torch, "uint16", None):
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


@pytest.mark.parametrize("name", HM_D)
def test_decoder_equal_size_equals_hm_d(name):
    g = gu.load("export_" + name)
    w, h, fmt, frames, out_bd = (int(v) for v in g["geom"])
    src = gu.load(str(g["source"]))
    with hmdec.Decoder(threads=2, device_output=True) as d:
        n = 0
        for poc, planes in d.frames(src["bitstream"], layout="planar", bit_depth=out_bd, size=(h, w), filter="bicubic"):
            for c, p in enumerate(planes):
                assert np.array_equal(_as_np(p), g["poc%02d_%d" % (poc, c)]), (name, poc, c)
            n += 1
        assert n == frames
        assert d.download_bytes == 0 and d.hash_mismatches == 0


LITE = ["ldp_crop_main8_204x116", "ldb_422_main12_208x120", "ldb_444_ccp_main12_208x120", "ldb_mono_wp_crop_main10_204x116",
        "ldp_bd10_8_208x120", "export_vui_bt2020_main10_208x120"]


def _lite(name):
    z = gu.load(name if name.startswith("export_") else "lite_" + name)
    w, h = (int(v) for v in z["geom"][:2])
    bd_y = int(z["geom"][3])
    bd = (10, 8) if "bd10_8" in name else (bd_y, bd_y)
    if "poc00_1" not in z:
        fmt = 0
    else:
        cy, cx = z["poc00_1"].shape
        fmt = 3 if cx == w else 2 if cy == h else 1
    return z, w, h, fmt, bd


@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("name", LITE)
def test_decoder_scaled_rgb_equals_reference(name, devices):
    """Decoder(device_output=True).frames(size=..., layout="rgb") == scale_ref on the golden reconstructions; nothing downloaded"""
    z, w, h, fmt, bd = _lite(name)
    matrix, full = (9, 1) if "bt2020" in name else (1, 0)
    seq = abi.make_seq(w, h, bd[0], bd[1])
    seq.chroma_format = fmt
    size = (45, 77)
    desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), matrix, full)
    scale = sref.scale_of(size, abi.SCALE_BILINEAR)
    plan = libhm_amd.export_scaled_plan(seq, desc, scale)
    tabs = sref.tables(seq, desc, scale)
    n = 0
    with hmdec.Decoder(threads=1 if devices else 2, device_output=True, devices=devices) as d:
        for poc, t in d.frames(z["bitstream"], layout="rgb", size=size):
            assert t.shape == (3,) + size
            planes = [z["poc%02d_%d" % (poc, c)] for c in range(1 if fmt == 0 else 3)]
            if fmt == 0:
                planes += [None, None]
            want = sref.export_scaled(planes, fmt, bd, desc, plan, tabs)
            assert np.array_equal(t.cpu().numpy().astype(np.int64), want), (name, poc)
            n += 1
        assert d.download_bytes == 0
    assert n == int(z["geom"][2])


# ------------------------------------------------------------------------------------------------ ordering, out=
def test_allocator_reuse_on_a_side_stream():
    """scaled exports into fresh tensors allocated and freed on a side stream, other work reusing the blocks in between"""
    torch = _torch()
    w, h = 416, 240
    seq = abi.make_seq(w, h, 10, 10, max_pictures=4)
    planes = [random_planes(w, h, 1, (10, 10), seed=s) for s in range(4)]
    desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    size = (120, 160)
    scale = sref.scale_of(size, abi.SCALE_BICUBIC)
    plan = libhm_amd.export_scaled_plan(seq, desc, scale)
    tabs = sref.tables(seq, desc, scale)
    side = torch.cuda.Stream()
    with libhm_amd.Context(seq) as ctx:
        pics = [ctx.acquire() for _ in range(4)]
        for p, pl in zip(pics, planes):
            ctx.upload(p, pl)
        want = [torch.from_numpy(sref.export_scaled(pl, 1, (10, 10), desc, plan, tabs).astype(np.uint8)).cuda() for pl in planes]
        ok = []
        with torch.cuda.stream(side):
            for i in range(50):
                t = ctx.export(pics[i % 4], "rgb", 8, size=size, filter="bicubic")
                ok.append(torch.equal(t, want[i % 4]))
                del t
                junk = torch.empty((3,) + size, dtype=torch.uint8, device="cuda")
                junk.fill_(7)
                del junk
        side.synchronize()
        assert all(ok), ok


def test_alternating_shapes_without_synchronisation():
    """many exports of more shapes than the context caches tables for, enqueued back to back, checked afterwards"""
    torch = _torch()
    w, h = 416, 240
    seq = abi.make_seq(w, h, 8, 8, max_pictures=2)
    planes = random_planes(w, h, 1, (8, 8), seed=3)
    shapes = [((60 + 4 * i, 100 + 6 * i), FILTERS[i % 4]) for i in range(11)]
    names = {0: "nearest", 1: "bilinear", 2: "bicubic", 3: "area"}
    desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    outs = []
    with libhm_amd.Context(seq) as ctx:
        pic = ctx.acquire()
        ctx.upload(pic, planes)
        torch.cuda.synchronize()
        for i in range(60):
            size, filt = shapes[(i * 7) % len(shapes)] if i % 3 else shapes[i % 3]
            outs.append((size, filt, ctx.export(pic, "rgb", 8, size=size, filter=names[filt], on_stream=i % 2 == 0)))
        ctx.sync()
        torch.cuda.synchronize()
    for size, filt, t in outs:
        scale = sref.scale_of(size, filt)
        plan = libhm_amd.export_scaled_plan(seq, desc, scale)
        want = sref.export_scaled(planes, 1, (8, 8), desc, plan, sref.tables(seq, desc, scale))
        assert np.array_equal(t.cpu().numpy().astype(np.int64), want), (size, filt)


def test_out_views_of_a_batch():
    """out=batch[i] (rows of the batch's pitch) and out=(planes) views equal separately allocated results; a wrong out is refused"""
    torch = _torch()
    w, h = 208, 120
    seq = abi.make_seq(w, h, 10, 10, max_pictures=4)
    with libhm_amd.Context(seq) as ctx:
        pics = [ctx.acquire() for _ in range(3)]
        for i, p in enumerate(pics):
            ctx.upload(p, random_planes(w, h, 1, (10, 10), seed=20 + i))
        batch = torch.zeros((3, 3, 64, 100), dtype=torch.uint8, device="cuda")[:, :, :, :96]     # rows 100 bytes apart
        for i, p in enumerate(pics):
            r = ctx.export(p, "rgb", 8, size=(64, 96), filter="area", out=batch[i])
            assert r.data_ptr() == batch[i].data_ptr()
        yb = torch.zeros((3, 60, 110), dtype=torch.int16, device="cuda")[:, :, :104]
        cb = torch.zeros((3, 30, 56), dtype=torch.int16, device="cuda")[:, :, :52]
        cr = torch.zeros((3, 30, 56), dtype=torch.int16, device="cuda")[:, :, :52]
        for i, p in enumerate(pics):
            ctx.export(p, "planar", 10, size=(60, 104), filter="bicubic", out=(yb[i], cb[i], cr[i]))
        unscaled = torch.zeros((3, 3, h, w + 8), dtype=torch.uint8, device="cuda")[..., :w]
        for i, p in enumerate(pics):
            ctx.export(p, "rgb", 8, out=unscaled[i])
        for i, p in enumerate(pics):
            assert torch.equal(batch[i], ctx.export(p, "rgb", 8, size=(64, 96), filter="area"))
            y, u, v = ctx.export(p, "planar", 10, size=(60, 104), filter="bicubic")
            assert torch.equal(yb[i], y.view(torch.int16)) and torch.equal(cb[i], u.view(torch.int16)) and torch.equal(cr[i], v.view(torch.int16))
            assert torch.equal(unscaled[i], ctx.export(p, "rgb", 8))
        for bad in (torch.zeros((3, 64, 95), dtype=torch.uint8, device="cuda"), torch.zeros((3, 64, 96), dtype=torch.int16, device="cuda"),
                    torch.zeros((3, 64, 96), dtype=torch.uint8), torch.zeros((3, 96, 64), dtype=torch.uint8, device="cuda").transpose(1, 2)):
            with pytest.raises(ValueError):
                ctx.export(pics[0], "rgb", 8, size=(64, 96), out=bad)
