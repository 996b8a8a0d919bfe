"""The picture import on the GPU: hmgpu_pictures_import behind Context.import_batch / import_picture / import_into.  Everything
it does is integer arithmetic (and one float rule) that include/hmgpu.h states in full, so every comparison is an equality of bit
patterns, read back through Context.download.  The yardsticks: tests/import_ref.py (numpy, never calls the library), the existing
exports for the round trips, and the oracle for pictures predicted from an imported reference."""
import ctypes as C
import itertools

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi
from libhm_amd import imports as himports
from tests import geometry_cases as gc
from tests import import_ref as iref
from tests import synth
from tests.test_gpu_export_batch import _hip
from tests.test_gpu_export_format import planted_planes
from tests.test_gpu_formats_fullsize import _oracle_chain, _same

pytestmark = pytest.mark.gpu

W, H = 72, 40                  # the coded picture
SIZES = [(72, 40), (70, 38)]   # the source: chroma groups of 4 with an odd count and a partial last group; two padded columns and rows
FORMATS = (0, 1, 2, 3)
NAMES = {0: "400", 1: "420", 2: "422", 3: "444"}
PAIRS = [(s, p) for s in FORMATS for p in FORMATS]
EINVAL = abi.HMGPU_EINVAL


def _torch():
    import torch
    return torch


def seq_of(fmt, bd, max_pictures=4, w=W, h=H, log2_ctu=6):
    seq = abi.make_seq(w, h, bd[0], bd[1], log2_ctu=log2_ctu, max_pictures=max_pictures)
    seq.chroma_format = fmt
    return seq


def dev(a, nbytes=None):
    """integers as a device tensor of unsigned elements of `nbytes` (2: int16 storage of the same bits)"""
    torch = _torch()
    a = np.ascontiguousarray(a)
    nbytes = nbytes or a.dtype.itemsize
    if nbytes == 1:
        return torch.from_numpy(a.astype(np.uint8)).cuda()
    return torch.from_numpy(a.astype(np.uint16).view(np.int16)).cuda()


def download_full(ctx, pic, fmt):
    """Context.download, without the dummy chroma planes of a 4:0:0 context"""
    p = ctx.download(pic)
    return p if fmt else p[:1]


def assert_planes(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w_) in enumerate(zip(got, want)):
        if not np.array_equal(g, w_):
            bad = np.argwhere(np.asarray(g) != np.asarray(w_))
            raise AssertionError("%s, plane %d: %d samples differ, first at (y, x) = %s: %d for %d" %
                                 (what, k, len(bad), tuple(bad[0]), g[tuple(bad[0])], w_[tuple(bad[0])]))


def source_planes(fmt, w, h, depth, seed):
    """planes of a source at its own depths (luma, chroma), up to 16 bits, planted as planted_planes of
    tests/test_gpu_export_format.py plants them: in chroma the first and the last two columns and rows alternate between the extremes
    and a checkerboard of 0 and the maximum lies in the middle"""
    rng = np.random.default_rng(seed)
    p = [rng.integers(0, 1 << depth[0], (h, w))]
    if fmt == 0:
        return p
    sx, sy = iref.shifts(fmt)
    m = (1 << depth[1]) - 1
    for k in range(2):
        c = rng.integers(0, m + 1, (h >> sy, w >> sx))
        lo, hi = (0, m) if k == 0 else (m, 0)
        c[:, 0], c[:, 1], c[:, -1], c[:, -2] = lo, hi, hi, lo
        c[0, :], c[1, :], c[-1, :], c[-2, :] = hi, lo, lo, hi
        c[0, 0], c[0, -1], c[-1, 0], c[-1, -1] = lo, lo, hi, hi
        yy, xx = np.mgrid[6:14, 8:24]
        c[6:14, 8:24] = np.where((yy + xx + k) & 1, m, 0)
        p.append(c)
    return p


# ------------------------------------------------------------------------------------------------ 1. each source form against the model
# (coding depths, source depths, element bytes, msb_aligned)
YUV_CONFIGS = [((8, 8), (8, 8), 1, False), ((10, 10), (10, 10), 2, False), ((12, 12), (16, 16), 2, True), ((10, 8), (10, 10), 2, True),
               ((8, 8), (10, 10), 2, False), ((10, 10), (8, 8), 1, False), ((12, 12), (8, 8), 2, True)]
DOWNS = [("drop", 0), ("linear", 0), ("linear", 1), ("linear", 2), ("linear", 4)]


@pytest.mark.parametrize("src_fmt,pic_fmt", PAIRS, ids=["%s-to-%s" % (NAMES[s], NAMES[p]) for s, p in PAIRS])
def test_yuv_sources_match_the_model(src_fmt, pic_fmt):
    ssx, ssy = iref.shifts(src_fmt) if src_fmt else (0, 0)
    psx, psy = iref.shifts(pic_fmt) if pic_fmt else (0, 0)
    loses = src_fmt and pic_fmt and (psx > ssx or psy > ssy)
    contexts = {}
    try:
        for ci, (coding, depth, nbytes, msb) in enumerate(YUV_CONFIGS):
            if coding not in contexts:
                ctx = libhm_amd.Context(seq_of(pic_fmt, coding))
                contexts[coding] = (ctx, ctx.acquire())
            ctx, pic = contexts[coding]
            for (sw, sh), layout in itertools.product(SIZES, ("planar", "semiplanar")):
                src = source_planes(src_fmt, sw, sh, depth, 100 * ci + 10 * src_fmt + pic_fmt)
                stored = [v << (16 - depth[1 if k else 0]) if msb else v for k, v in enumerate(src)]
                t = [dev(v, nbytes) for v in stored]
                if layout == "semiplanar" and src_fmt:
                    t = [t[0], _torch().stack(t[1:], dim=-1).contiguous()]
                for down, loc in (DOWNS if loses else DOWNS[:1]):
                    want = iref.import_yuv(src, src_fmt, pic_fmt, depth, coding, (W, H), iref.LINEAR if down == "linear" else iref.DROP, loc)
                    ctx.import_picture(pic, tuple(t), layout=layout, bit_depth=depth, chroma_format=NAMES[src_fmt], chroma_down=down,
                                       chroma_loc=loc, msb_aligned=msb)
                    assert_planes(download_full(ctx, pic, pic_fmt), want,
                                  "%s %dx%d depth %s -> %s, %s loc %d, msb %d" % (layout, sw, sh, depth, coding, down, loc, msb))
    finally:
        for ctx, _ in contexts.values():
            ctx.close()


def float_source(rng, shape, depth, dtype):
    """float elements around code / (2^D - 1) with ties, values outside the range, NaN, infinities and a denormal planted; returns
    (device tensor, the elements as float32 on the host)"""
    torch = _torch()
    m = (1 << depth) - 1
    x = (rng.integers(-3, m + 4, shape) + rng.choice([0.0, 0.5, 0.25, -0.5, 0.4999], shape)) / m
    x = x.astype(np.float32)
    flat = x.reshape(-1)
    flat[:8] = [np.nan, np.inf, -np.inf, 1e-45, 0.5 / m, 1.5 / m, 2.5 / m, 1e30]
    t = torch.from_numpy(x).to(dtype).cuda()
    return t, t.float().cpu().numpy()


ELEMENTS = ["uint8", "uint16", "float16", "bfloat16", "float32"]


@pytest.mark.parametrize("elem", ELEMENTS)
def test_rgb_sources_match_the_model(elem):
    torch = _torch()
    rng = np.random.default_rng(ELEMENTS.index(elem))
    depth = {"uint8": 8, "uint16": 12, "float16": 8, "bfloat16": 8, "float32": 16}[elem]
    coding = {"uint8": (8, 8), "uint16": (10, 10), "float16": (8, 8), "bfloat16": (10, 8), "float32": (12, 12)}[elem]
    m = (1 << depth) - 1
    orders = [None, "rgb", "bgr", "rgba", "bgra", "argb", "abgr"]
    colours = [(mx, fr) for mx in (1, 6, 9) for fr in (0, 1)]
    contexts = {f: libhm_amd.Context(seq_of(f, coding)) for f in FORMATS}
    try:
        pics = {f: c.acquire() for f, c in contexts.items()}
        case = 0
        for order, (matrix, full_range), (sw, sh) in itertools.product(orders, colours + [(0, 0)], SIZES):
            case += 1
            pic_fmt = 3 if matrix == 0 else (1, 1, 2, 3, 0, 1)[case % 6]
            down, loc = DOWNS[case % 5]
            nch = 3 if order is None else len(order)
            if elem.startswith("uint"):
                codes = rng.integers(0, m + 1, (sh, sw, nch))
                codes[:2, :, :3], codes[-2:, :, :3], codes[:, :2, :3], codes[:, -2:, :3] = 0, m, m, 0
                codes[6:14, 8:24, :3] = np.where(np.add.outer(np.arange(8), np.arange(16)) & 1, m, 0)[..., None] ^ (np.arange(3) & 1) * m
                px = dev(codes, 1 if elem == "uint8" else 2)
                kw = {}
            else:
                px, vals = float_source(rng, (sh, sw, nch), depth, getattr(torch, elem))
                sc, bi = (float(m), float(m) * 0.5, float(m) * 2), (0.0, 0.25, -3.0)
                kw = dict(scale=sc, bias=bi)
            pos = iref.PIXEL_POS[himports.PIXELS[order]][0] if order else (0, 1, 2)
            if elem.startswith("uint"):
                rgb = [codes[..., pos[k]] for k in range(3)]
            else:
                rgb = [iref.float_codes(vals[..., pos[k]], sc[k], bi[k], depth) for k in range(3)]
            want = iref.import_rgb(*rgb, pic_fmt, depth, coding, (W, H), matrix, full_range, iref.LINEAR if down == "linear" else iref.DROP, loc)
            if order is None:
                src = px.permute(2, 0, 1).contiguous()                       # one [3, H, W] tensor
                if case % 2:
                    src = tuple(src[k].clone() for k in range(3))            # ... or three planes
                contexts[pic_fmt].import_picture(pics[pic_fmt], src, layout="rgb", bit_depth=depth, matrix=matrix, full_range=full_range,
                                                 chroma_down=down, chroma_loc=loc, **kw)
            else:
                contexts[pic_fmt].import_picture(pics[pic_fmt], px, layout="rgb", pixel=order, bit_depth=depth, matrix=matrix,
                                                 full_range=full_range, chroma_down=down, chroma_loc=loc, **kw)
            assert_planes(download_full(contexts[pic_fmt], pics[pic_fmt], pic_fmt), want,
                          "%s %s %dx%d matrix %d range %d -> %s %s loc %d" % (elem, order, sw, sh, matrix, full_range, NAMES[pic_fmt], down, loc))
    finally:
        for c in contexts.values():
            c.close()


@pytest.mark.parametrize("elem", ["float16", "bfloat16", "float32"])
def test_planar_float_sources_match_the_model(elem):
    torch = _torch()
    rng = np.random.default_rng(40 + ELEMENTS.index(elem))
    depth, coding = (10, 9), (10, 8)
    sc, bi = (1023.0, 511.0, 300.0), (0.0, 0.5, 100.0)
    for src_fmt, pic_fmt, (sw, sh) in ((1, 1, SIZES[0]), (1, 1, SIZES[1]), (3, 1, SIZES[1]), (1, 3, SIZES[0]), (0, 2, SIZES[1])):
        ssx, ssy = iref.shifts(src_fmt) if src_fmt else (0, 0)
        shapes = [(sh, sw)] + ([(sh >> ssy, sw >> ssx)] * 2 if src_fmt else [])
        t, codes = [], []
        for k, shape in enumerate(shapes):
            a, vals = float_source(rng, shape, depth[1 if k else 0], getattr(torch, elem))
            t.append(a)
            codes.append(iref.float_codes(vals, sc[k], bi[k], depth[1 if k else 0]))
        want = iref.import_yuv(codes, src_fmt, pic_fmt, depth, coding, (W, H), iref.LINEAR, 3)
        with libhm_amd.Context(seq_of(pic_fmt, coding)) as ctx:
            pic = ctx.acquire()
            ctx.import_picture(pic, tuple(t), layout="planar", bit_depth=depth, chroma_format=src_fmt, chroma_down="linear", chroma_loc=3,
                               scale=sc, bias=bi)
            assert_planes(ctx.download(pic), want, "%s planar %s -> %s" % (elem, NAMES[src_fmt], NAMES[pic_fmt]))
        if sw != W:
            with pytest.raises(libhm_amd.HmgpuError) as e:                      # semi-planar floats
                with libhm_amd.Context(seq_of(pic_fmt, coding)) as ctx:
                    ctx.import_picture(ctx.acquire(), (t[0], torch.zeros(sh >> 1, sw >> 1, 2, dtype=t[0].dtype, device="cuda")),
                                       layout="semiplanar", bit_depth=depth)
            assert e.value.status == abi.HMGPU_EUNSUPPORTED


@pytest.mark.parametrize("n", [1, 3, 16])
def test_batches(n):
    """n pictures in one call: RGB and 4:4:4 planar from ONE [N, 3, H, W] tensor, 4:2:0 from a tuple of [N, h, w] planes, packed
    pixels from one [N, H, W, C] tensor and from a channels-last tensor"""
    torch = _torch()
    rng = np.random.default_rng(n)
    with libhm_amd.Context(seq_of(1, (8, 8), max_pictures=16)) as ctx:
        pics = [ctx.acquire() for _ in range(n)][::-1]                           # (not in handle order)
        rgb = rng.integers(0, 256, (n, 3, H, W))
        want = [iref.import_rgb(*rgb[i], 1, 8, (8, 8), (W, H), 6, 1) for i in range(n)]
        ctx.import_batch(pics, dev(rgb, 1), layout="rgb", bit_depth=8, matrix=6, full_range=1)
        for i in range(n):
            assert_planes(ctx.download(pics[i]), want[i], "RGB tensor, slot %d" % i)
        cl = dev(rgb[:, ::-1].copy(), 1).contiguous(memory_format=torch.channels_last)                # (other contents: the channels reversed)
        want_cl = [iref.import_rgb(*rgb[i, ::-1], 1, 8, (8, 8), (W, H), 6, 1) for i in range(n)]
        ctx.import_batch(pics, cl, layout="rgb", bit_depth=8, matrix=6, full_range=1)
        for i in range(n):
            assert_planes(ctx.download(pics[i]), want_cl[i], "channels-last tensor, slot %d" % i)
        px = rng.integers(0, 256, (n, H, W, 4))
        ctx.import_batch(pics, dev(px, 1), layout="rgb", pixel="abgr", bit_depth=8, matrix=1, full_range=0)
        for i in range(n):
            assert_planes(ctx.download(pics[i]), iref.import_rgb(px[i, ..., 3], px[i, ..., 2], px[i, ..., 1], 1, 8, (8, 8), (W, H), 1, 0),
                          "ABGR pixels, slot %d" % i)
        yuv = [rng.integers(0, 256, (n, H, W)), rng.integers(0, 256, (n, H // 2, W // 2)), rng.integers(0, 256, (n, H // 2, W // 2))]
        ctx.import_batch(pics, tuple(dev(v, 1) for v in yuv), layout="planar", bit_depth=8)
        for i in range(n):
            assert_planes(ctx.download(pics[i]), [v[i].astype(np.int16) for v in yuv], "planar tuple, slot %d" % i)
        y444 = rng.integers(0, 256, (n, 3, H, W))
        ctx.import_batch(pics, dev(y444, 1), layout="planar", bit_depth=8, chroma_format="444", chroma_down="linear", chroma_loc=1)
        for i in range(n):
            assert_planes(ctx.download(pics[i]), iref.import_yuv(list(y444[i]), 3, 1, (8, 8), (8, 8), (W, H), iref.LINEAR, 1),
                          "4:4:4 tensor, slot %d" % i)


@pytest.mark.parametrize("elem", ["uint8", "uint16", "float16"])
def test_unaligned_sources_take_the_element_path(elem):
    """planes 2 and 6 bytes into their allocation with a pitch that is no multiple of 16: no run of eight elements is aligned"""
    torch = _torch()
    rng = np.random.default_rng(77)
    es = 1 if elem == "uint8" else 2
    depth = 8 if elem != "uint16" else 10
    m = (1 << depth) - 1
    kw = dict(scale=(float(m),) * 3, bias=(0.0,) * 3) if elem == "float16" else {}
    with libhm_amd.Context(seq_of(1, (10, 10))) as ctx:
        pic = ctx.acquire()
        for (sw, sh), form in itertools.product(SIZES, ("planar", "semiplanar", "rgb")):
            if form == "semiplanar" and elem == "float16":
                continue
            shapes = {"planar": [(sh, sw), (sh // 2, sw // 2), (sh // 2, sw // 2)], "semiplanar": [(sh, sw), (sh // 2, sw)], "rgb": [(sh, sw)] * 3}[form]
            codes, views = [], []
            for k, (h_, w_) in enumerate(shapes):
                c = rng.integers(0, m + 1, (h_, w_))
                pitch = w_ + (5 if es == 1 else 3)                               # elements: 77 / 75 / 40 ... bytes never a multiple of 16
                assert (pitch * es) % 16
                off = (2, 6, 6)[k] // es
                buf = torch.zeros(off + pitch * h_ + 64, dtype={"uint8": torch.uint8, "uint16": torch.int16, "float16": torch.float16}[elem],
                                  device="cuda")
                v = torch.as_strided(buf, (1, h_, w_), (pitch * h_, pitch, 1), off)
                if elem == "float16":
                    v.copy_(torch.from_numpy((c / m).astype(np.float16)).cuda())
                    c = iref.float_codes(v[0].float().cpu().numpy(), float(m), 0.0, depth)
                else:
                    v.copy_(dev(c, es))
                assert v.data_ptr() % 16 == (2, 6, 6)[k]
                codes.append(c)
                views.append(v)
            if form == "rgb":
                want = iref.import_rgb(*codes, 1, depth, (10, 10), (W, H), 9, 0)
                ctx.import_batch([pic], tuple(views), layout="rgb", bit_depth=depth, matrix=9, **kw)
            elif form == "planar":
                want = iref.import_yuv(codes, 1, 1, (depth, depth), (10, 10), (W, H))
                ctx.import_batch([pic], tuple(views), layout="planar", bit_depth=depth, **kw)
            else:
                want = iref.import_yuv([codes[0], codes[1][:, 0::2], codes[1][:, 1::2]], 1, 1, (depth, depth), (10, 10), (W, H))
                cbcr = torch.as_strided(views[1], (1, sh // 2, sw // 2, 2), (views[1].stride(0), views[1].stride(1), 2, 1), views[1].storage_offset())
                ctx.import_batch([pic], (views[0], cbcr), layout="semiplanar", bit_depth=depth)
            assert_planes(ctx.download(pic), want, "%s %s %dx%d" % (elem, form, sw, sh))


# ------------------------------------------------------------------------------------------------ 2. round trips through the exports
@pytest.mark.parametrize("fmt", (1, 2, 3))
def test_round_trips_through_the_exports(fmt):
    for bd in ((8, 8), (10, 10)):
        planes = [planted_planes(fmt, W, H, bd[0], 7 * fmt + i + bd[0]) for i in range(3)]
        with libhm_amd.Context(seq_of(fmt, bd, max_pictures=8)) as ctx:
            src = [ctx.acquire() for _ in range(3)]
            dst = [ctx.acquire() for _ in range(3)]
            for p, pl in zip(src, planes):
                ctx.upload(p, pl)
            forms = [("planar", dict(layout="planar", bit_depth=bd[0]), dict(layout="planar", bit_depth=bd[0])),
                     ("planar, 16 bits", dict(layout="planar", bit_depth=16), dict(layout="planar", bit_depth=16)),
                     ("4:4:4 replicated, dropped", dict(layout="planar", bit_depth=bd[0], chroma_format="444"),
                      dict(layout="planar", bit_depth=bd[0], chroma_format="444", chroma_down="drop"))]
            if bd[0] == 8:
                forms.append(("NV12 / NV16 / NV24", dict(layout="semiplanar", bit_depth=8), dict(layout="semiplanar", bit_depth=8)))
            else:
                forms.append(("P010 / P210 / P410", dict(layout="semiplanar", bit_depth=10, msb_aligned=True),
                              dict(layout="semiplanar", bit_depth=10, msb_aligned=True)))
            for name, ekw, ikw in forms:
                for p in dst:
                    ctx.upload(p, [np.zeros_like(v) for v in planes[0]])
                t = ctx.export_batch(src, **ekw)
                ctx.import_batch(dst, t, **ikw)
                for i, p in enumerate(dst):
                    assert_planes(ctx.download(p), planes[i], "%s, %s bits, slot %d" % (name, bd, i))


# ------------------------------------------------------------------------------------------------ 3. an imported picture is a reference
def _int16(planes):
    torch = _torch()
    return tuple(torch.from_numpy(np.ascontiguousarray(v, np.int16)).cuda() for v in planes)


@pytest.mark.parametrize("fmt", (1, 2, 3))
def test_an_imported_picture_is_a_reference(oracle, fmt):
    """A's final planes, from the oracle, imported; B's prediction units lie in A's margins in all eight regions of luma and chroma.
    Then the same into a handle that holds a decoded, SAO-filtered picture: B must read the imported samples"""
    case = (W, H, 4, fmt, 10, 10)
    a_of, bs = gc.margin_pictures(case)
    got = gc.readers_union(bs)
    assert all(got[plane][r] >= 1 for plane in got for r in gc.REGIONS), got
    ref0 = synth.noise_planes(W, H, 10, 3, fmt, 10)
    zero = [np.zeros_like(x) for x in ref0]
    a = a_of["sao"]
    fin = _oracle_chain(oracle, a, zero, [ref0])[2]
    other = synth.noise_planes(W, H, 10, 21, fmt, 10)
    seq = abi.SeqParams.from_buffer_copy(bs[0].seq)
    seq.max_pictures = 3
    with libhm_amd.Context(seq) as ctx:
        h0, ha, hb = ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)

        def check(ref_planes, what):
            for k, b in enumerate(bs):
                sl = abi.clone_slice(b.slice)
                sl.ref_pic[0][0] = ha
                want = [x.copy() for x in zero]
                oracle.decompress_ctus(b.seq, [b.slice], b.meta, b.coeffs, want, [ref_planes])
                ctx.upload(hb, zero)
                ctx.decompress_slice(hb, 0, sl, b.meta, b.coeffs)
                _same(ctx.download(hb), want, "%s: picture B%d" % (what, k))

        ctx.import_picture(ha, _int16(fin), layout="planar", bit_depth=10)
        check(fin, "A imported into a fresh handle")
        ctx.upload(ha, zero)
        ctx.decompress_slice(ha, 0, a.slice, a.meta, a.coeffs)
        ctx.filter_picture(ha, a.pp, a.sao_raw)
        _same(ctx.download(ha), fin, "A decoded and filtered")
        ctx.import_picture(ha, _int16(other), layout="planar", bit_depth=10)
        _same(ctx.download(ha), other, "imported over the filtered picture")
        check(other, "A imported over a decoded, SAO-filtered picture")


# ------------------------------------------------------------------------------------------------ 4. state, 5. handles instead of planes
def _equal_dicts(a, b, what):
    torch = _torch()
    assert a.keys() == b.keys(), what
    for k in a:
        if isinstance(a[k], dict):
            _equal_dicts(a[k], b[k], "%s[%s]" % (what, k))
        else:
            assert torch.equal(a[k], b[k]), "%s[%s]" % (what, k)


def test_state_after_an_import_over_a_decoded_picture(oracle):
    torch = _torch()
    case = (W, H, 4, 1, 10, 10)
    a = gc.margin_pictures(case)[0]["sao"]
    ref0 = synth.noise_planes(W, H, 10, 3, 1, 10)
    zero = [np.zeros_like(x) for x in ref0]
    new = planted_planes(1, W, H, 10, 5)
    seq = abi.SeqParams.from_buffer_copy(a.seq)
    seq.max_pictures = 4
    with libhm_amd.Context(seq) as ctx:
        h0, ha, hn = ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        ctx.upload(ha, zero)
        ctx.upload(hn, new)
        ctx.decompress_slice(ha, 0, a.slice, a.meta, a.coeffs)
        ctx.filter_picture(ha, a.pp, a.sao_raw)
        assert ctx.residual_status([ha]) == abi.HMGPU_OK and ctx.transform_status([ha]) == abi.HMGPU_OK
        assert ctx.loopfilter_status([ha]) == abi.HMGPU_OK
        ctx.export_motion([ha])
        ctx.import_picture(ha, _int16(new), layout="planar", bit_depth=10)
        # the exports, metrics and histograms read the imported samples: what they give for an uploaded picture of the same planes
        for kw in (dict(layout="planar", bit_depth=10), dict(layout="rgb", bit_depth=8), dict(layout="semiplanar", bit_depth=16, msb_aligned=True)):
            got, want = ctx.export_batch([ha], **kw), ctx.export_batch([hn], **kw)
            got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
            assert all(torch.equal(g, w_) for g, w_ in zip(got, want)), kw
        planes_t = [dev(np.asarray(v)[None], 2) for v in new]
        m = ctx.metrics([ha], ref=planes_t)
        for c in ("y", "cb", "cr"):
            assert int(m[c]["sse"][0]) == 0 and int(m[c]["differing"][0]) == 0
        _equal_dicts(ctx.histogram([ha]), ctx.histogram([hn]), "histogram")
        # ... and the side information is gone
        assert ctx.residual_status([ha]) == EINVAL and ctx.transform_status([ha]) == EINVAL
        assert ctx.loopfilter_status([ha]) == EINVAL and ctx.loopfilter_status([ha], need_filter=False) == EINVAL
        with pytest.raises(libhm_amd.HmgpuError) as e:
            ctx.export_motion([ha])
        assert e.value.status == EINVAL
        # 5. imported handles as the reference of the metrics: byte for byte what the same planes give
        refs = [planted_planes(1, W, H, 10, 60 + i) for i in range(2)]
        hr = [ha, ctx.acquire()]
        stacked = [np.stack([r[k] for r in refs]) for k in range(3)]
        ctx.import_batch(hr, _int16(stacked), layout="planar", bit_depth=10)
        tens = [dev(v, 2) for v in stacked]
        _equal_dicts(ctx.metrics([h0, hn], ref_pics=hr), ctx.metrics([h0, hn], ref=tens), "metrics")
        _equal_dicts(ctx.metrics_map([h0, hn], ref_pics=hr, block=8), ctx.metrics_map([h0, hn], ref=tens, block=8), "metrics map")


# ------------------------------------------------------------------------------------------------ 6. neighbours in the slab
def _region_bytes(hip, base, nbytes):
    out = np.zeros(nbytes, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, base, nbytes, 2) == 0
    return out


@pytest.mark.parametrize("fmt", (0, 1, 3))
def test_neighbours_in_the_slab_stay_untouched(fmt):
    """import into handle k of four: handles k - 1 and k + 1 keep every byte, margins included; handle k itself changes exactly where
    an upload of the same planes changes it (its samples: the margins keep the old picture's border until the first use)"""
    torch = _torch()
    hip = _hip()
    bd = (8, 8)
    with libhm_amd.Context(seq_of(fmt, bd, max_pictures=4)) as ctx:
        pics = [ctx.acquire() for _ in range(4)]
        old = [synth.noise_planes(W, H, 8, 30 + i, fmt or 1, 8) for i in range(4)]
        for p, pl in zip(pics, old):
            ctx.upload(p, pl)
        regions = [ctx.device_region(p) for p in pics]                        # (extends every picture's margins)
        ctx.sync()
        before = [_region_bytes(hip, b, n) for b, n in regions]
        for k in (1, 2):
            rgb = np.random.default_rng(k).integers(0, 256, (3, H - 2, W - 2))
            want = iref.import_rgb(*rgb, fmt, 8, bd, (W, H), 1, 0, iref.LINEAR, 2)
            ctx.import_picture(pics[k], dev(rgb, 1), layout="rgb", bit_depth=8, chroma_down="linear", chroma_loc=2)
            ctx.sync()
            torch.cuda.synchronize()
            after = [_region_bytes(hip, b, n) for b, n in regions]
            for j in range(4):
                if j != k:
                    assert np.array_equal(after[j], before[j]), "import into %d changed handle %d" % (k, j)
            full = want if fmt else want + old[k][1:]
            ctx.upload(pics[k], full)
            ctx.sync()
            uploaded = _region_bytes(hip, *regions[k])
            assert np.array_equal(after[k], uploaded), "import into %d wrote outside the samples" % k
            assert not np.array_equal(after[k], before[k])
            before[k] = uploaded


# ------------------------------------------------------------------------------------------------ 7. refusals enqueue nothing
def test_refusals_leave_the_pictures_untouched():
    torch = _torch()
    bd = (10, 10)
    with libhm_amd.Context(seq_of(1, bd, max_pictures=4)) as ctx:
        pics = [ctx.acquire() for _ in range(3)]
        released = ctx.acquire()
        ctx.release(released)
        old = [planted_planes(1, W, H, 10, 80 + i) for i in range(3)]
        for p, pl in zip(pics, old):
            ctx.upload(p, pl)
        desc = abi.make_import_desc(abi.EXPORT_PLANAR, bit_depth=10, bytes_per_sample=2)
        fdesc = abi.make_import_desc(abi.EXPORT_PLANAR, bit_depth=8, bytes_per_sample=1, sample_type=abi.SAMPLE_F32)
        n = 3
        buf = torch.full((n * (W * H + 2 * (W // 2) * (H // 2)) + 64,), 0x0155, dtype=torch.int16, device="cuda")
        fbuf = torch.zeros(n * 2 * W * H + 64, dtype=torch.float32, device="cuda")
        yb, cb = W * H * 2, (W // 2) * (H // 2) * 2
        base = buf.data_ptr()
        ptrs = [base, base + n * yb, base + n * (yb + cb)]
        pitches, bstr = [2 * W, W, W], [yb, cb, cb]
        host = np.zeros(n * W * H * 2, np.int16)
        stream = torch.cuda.current_stream().cuda_stream
        assert ctx.import_source_status(n, desc, ptrs, pitches, bstr) == abi.HMGPU_OK
        hip = _hip()
        raw = C.c_void_p()                                       # an allocation of exactly the luma planes (torch's are parts of larger ones)
        assert hip.hipMalloc(C.byref(raw), n * yb) == 0
        assert ctx.import_source_status(n, desc, [raw.value] + ptrs[1:], pitches, bstr) == abi.HMGPU_OK
        cases = [
            ("a host pointer", pics, desc, [host.ctypes.data] + ptrs[1:], pitches, bstr),
            ("a span that leaves its allocation", pics, desc, [raw.value + 2] + ptrs[1:], pitches, bstr),
            ("a short pitch", pics, desc, ptrs, [2 * W - 2, W, W], bstr),
            ("a short chroma pitch", pics, desc, ptrs, [2 * W, W - 2, W], bstr),
            ("a batch stride inside a plane", pics, desc, ptrs, pitches, [yb - 2, cb, cb]),
            ("a misaligned uint16 source", pics, desc, [base + 1] + ptrs[1:], pitches, bstr),
            ("a misaligned uint16 pitch", pics, desc, ptrs, [2 * W + 1, W, W], bstr),
            ("a misaligned float source", pics, fdesc, [fbuf.data_ptr() + 2, fbuf.data_ptr() + 4 * n * W * H, fbuf.data_ptr() + 4 * n * W * H], [4 * W, 2 * W, 2 * W],
             [4 * W * H, W * H, W * H]),
            ("a missing plane", pics, desc, [ptrs[0], ptrs[1], 0], pitches, bstr),
            ("a repeated handle", [pics[0], pics[1], pics[0]], desc, ptrs, pitches, bstr),
            ("a released handle", [pics[0], released, pics[2]], desc, ptrs, pitches, bstr),
            ("a handle out of range", [pics[0], 99, pics[2]], desc, ptrs, pitches, bstr),
        ]
        for what, hs, d, p, pi, bs_ in cases:
            assert ctx.import_status(hs, d, p, pi, bs_, 1, stream) == EINVAL, what
            if hs is pics:
                assert ctx.import_source_status(n, d, p, pi, bs_) == EINVAL, what
        assert ctx.import_status([], desc, ptrs, pitches, bstr, 1, stream) == EINVAL
        assert ctx.import_status(pics, desc, ptrs, pitches, bstr, 2, stream) == EINVAL
        # the order: a bad descriptor before n, n before the handles, the handles before the source
        bad = abi.make_import_desc(abi.EXPORT_PLANAR, bit_depth=10, bytes_per_sample=2, down=7)
        assert ctx.import_status([99] * 17, bad, [0, 0, 0], pitches, bstr, 1, stream) == abi.HMGPU_EUNSUPPORTED
        assert ctx.import_source_status(17, bad, [0, 0, 0], pitches, bstr) == abi.HMGPU_EUNSUPPORTED
        assert ctx.import_status(pics, None, ptrs, pitches, bstr, 1, stream) == EINVAL
        if torch.cuda.device_count() > 1:
            assert ctx.import_status(pics, desc, ptrs, pitches, bstr, 1, torch.cuda.Stream(device=1).cuda_stream) == EINVAL
        for p, pl in zip(pics, old):
            assert_planes(ctx.download(p), pl, "after the refused calls")
        assert ctx.import_status(pics, desc, ptrs, pitches, bstr, 1, stream) == abi.HMGPU_OK      # the same arguments, whole
        got = ctx.download(pics[0])
        assert (got[0] == 0x0155).all() and (got[1] == 0x0155).all()
        hip.hipFree(raw)


# ------------------------------------------------------------------------------------------------ 8. stream ordering
def test_ordering_without_host_synchronisation(oracle):
    """the import on a side stream: its source written by a kernel enqueued just before on that stream and overwritten just after the
    call; a decode that references the picture follows at once on the context's stream.  And the reverse: an export of the handle's
    old contents, enqueued on the side stream behind a queue of work, still shows them although an import follows at once"""
    torch = _torch()
    case = (W, H, 4, 1, 10, 10)
    _, bs = gc.margin_pictures(case)
    b = bs[0]
    first = synth.noise_planes(W, H, 10, 41, 1, 10)
    second = synth.noise_planes(W, H, 10, 42, 1, 10)
    zero = [np.zeros_like(x) for x in first]
    seq = abi.SeqParams.from_buffer_copy(b.seq)
    seq.max_pictures = 3
    sl = abi.clone_slice(b.slice)
    side = torch.cuda.Stream()
    with libhm_amd.Context(seq) as ctx:
        h0, ha, hb = ctx.acquire(), ctx.acquire(), ctx.acquire()
        assert ha == 1
        sl.ref_pic[0][0] = ha
        want = [x.copy() for x in zero]
        oracle.decompress_ctus(b.seq, [b.slice], b.meta, b.coeffs, want, [first])
        ctx.upload(ha, second)
        ctx.upload(hb, zero)
        staged = _int16(first)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            busy = torch.randn(2048, 2048, device="cuda")
            for _ in range(8):                                   # work ahead of the import on the side stream
                busy = busy @ busy * 1e-3
            src = tuple(t + 0 for t in staged)                   # the source: written by kernels of this stream, just before
            ctx.import_picture(ha, src, layout="planar", bit_depth=10)
            for t in src:
                t.zero_()                                        # ... and overwritten just after
        ctx.decompress_slice(hb, 0, sl, b.meta, b.coeffs)       # at once, on the context's stream: must wait for the import
        _same(ctx.download(hb), want, "B predicted from the picture imported on the side stream")
        _same(ctx.download(ha), first, "the imported picture")
        # the reverse hazard
        with torch.cuda.stream(side):
            for _ in range(8):
                busy = busy @ busy * 1e-3
            t = ctx.export_batch([ha], layout="planar", bit_depth=10)
        ctx.import_picture(ha, _int16(second), layout="planar", bit_depth=10, on_stream=False)     # at once, on the context's stream
        side.synchronize()
        for k in range(3):
            assert np.array_equal(t[k][0].cpu().numpy().view(np.int16), first[k]), k
        _same(ctx.download(ha), second, "the picture imported behind the export")
