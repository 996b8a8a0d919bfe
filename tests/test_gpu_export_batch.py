"""Batched tensor export on the GPU: hmgpu_pictures_export / hmdec_pictures_export behind Context.export_batch, hmdec.export_batch,
Decoder.frames(batch=) and Picture.export(dtype=): integer batches bit for bit the single-picture exports, float elements bit for
bit the numpy restatement (tests/export_batch_ref.py), strides and canaries, refusals, stream ordering."""
import ctypes as C

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, export, hmdec
from tests import export_batch_ref as bref
from tests import export_ref as ref
from tests import golden_util as gu
from tests import scale_ref as sref

pytestmark = pytest.mark.gpu

W, H = 200, 72
CANARY = 0xA5
CONTAINERS = [(8, 0), (10, 0), (10, 1)]                 # (depth, msb_aligned): containers (8, 1, 0), (10, 2, 0), (10, 2, 1)
FILTER_NAMES = {abi.SCALE_NEAREST: "nearest", abi.SCALE_BILINEAR: "bilinear", abi.SCALE_BICUBIC: "bicubic", abi.SCALE_AREA: "area"}
# (size (height, width) or None, filter, crop): unscaled, a 2x bicubic reduction, a 1.5x bilinear enlargement, a crop (both ways)
VARIANTS = [(None, abi.SCALE_BILINEAR, (0, 0, 0, 0)), ((36, 100), abi.SCALE_BICUBIC, (0, 0, 0, 0)), ((108, 300), abi.SCALE_BILINEAR, (0, 0, 0, 0)),
            (None, abi.SCALE_BILINEAR, (4, 8, 2, 6)), ((30, 50), abi.SCALE_AREA, (4, 8, 2, 6))]
DTYPES = {abi.SAMPLE_F16: "float16", abi.SAMPLE_BF16: "bfloat16", abi.SAMPLE_F32: "float32"}


def _torch():
    import torch
    return torch


def random_planes(w, h, fmt, bd, seed):
    rng = np.random.default_rng(seed)
    sx, sy = ref.chroma_shift(fmt)
    return [rng.integers(0, 1 << bd[0], (h, w)).astype(np.int16)] + \
           [rng.integers(0, 1 << bd[1], (h >> sy, w >> sx)).astype(np.int16) for _ in range(2)]


def seq_of(fmt, bd, max_pictures=8, w=W, h=H):
    seq = abi.make_seq(w, h, bd[0], bd[1], max_pictures=max_pictures)
    seq.chroma_format = fmt
    return seq


def bits(t):
    """a tensor's elements as unsigned integers of their own width (bit patterns), on the host"""
    torch = _torch()
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
    a = t.contiguous().view(view).cpu().numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[t.element_size()])


def as_tuple(x):
    return x if isinstance(x, tuple) else (x,)


# ------------------------------------------------------------------------------------------------ 1. batch == singles (integers)
@pytest.mark.parametrize("n", [1, 3, 16])
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_integer_batch_equals_singles(fmt, n):
    """slot i of an integer batch is bit for bit the single-picture export of picture i; the batches name handles twice"""
    torch = _torch()
    bd = (10, 10)
    seq = seq_of(fmt, bd)
    with libhm_amd.Context(seq) as ctx:
        distinct = [ctx.acquire() for _ in range(min(n, 5))]
        for i, p in enumerate(distinct):
            ctx.upload(p, random_planes(W, H, fmt, bd, seed=100 * fmt + i))
        pics = [distinct[(2 * i) % len(distinct)] for i in range(n)] if n > 1 else distinct      # (n = 3: [p0, p2, p1]; 16: repeats)
        if n == 3:
            pics = [distinct[0], distinct[1], distinct[0]]
        j = 0
        for layout in ("planar", "nv12", "rgb"):
            for size, filt, crop in VARIANTS:
                depth, msb = CONTAINERS[j % 3]
                j += 1
                kw = dict(layout=layout, bit_depth=depth, crop=crop, matrix=1, full_range=0, msb_aligned=bool(msb), size=size,
                          filter=FILTER_NAMES[filt])
                got = as_tuple(ctx.export_batch(pics, **kw))
                for i, p in enumerate(pics):
                    one = as_tuple(ctx.export(p, **kw))
                    assert len(one) == len(got)
                    for a, b in zip(got, one):
                        assert a.shape == (n,) + tuple(b.shape) and a.dtype == b.dtype
                        assert torch.equal(a[i], b), (fmt, n, layout, size, crop, depth, msb, i)


# ------------------------------------------------------------------------------------------------ 2. float elements, bit exact
def float_cases(fmt, depth):
    """(layout, matrix, full_range, size, filter, crop, mean, std): RGB limited BT.709 and full BT.2020, planar; unscaled and one size per
    filter; ImageNet constants, and scale 1 / bias 0 (mean None: given explicitly) once per layout"""
    sizes = [(None, abi.SCALE_BILINEAR), ((36, 100), abi.SCALE_NEAREST), ((108, 300), abi.SCALE_BILINEAR), ((20, 54), abi.SCALE_BICUBIC),
             ((24, 224), abi.SCALE_AREA)]
    out = []
    for layout, matrix, full in ((ref.RGB, 1, 0), (ref.RGB, 9, 1), (ref.PLANAR, 1, 0)):
        for k, (size, filt) in enumerate(sizes):
            crop = (4, 8, 2, 6) if k == 3 else (0, 0, 0, 0)
            out.append((layout, matrix, full, size, filt, crop, bref.IMAGENET_MEAN, bref.IMAGENET_STD))
        out.append((layout, matrix, full, None, abi.SCALE_BILINEAR, (0, 0, 0, 0), None, None))
        out.append((layout, matrix, full, (36, 100), abi.SCALE_BICUBIC, (0, 0, 0, 0), None, None))
    return out


def check_float_batch(ctx, seq, pics, planes_of, fmt, bd, depth, st_type, case):
    torch = _torch()
    layout, matrix, full, size, filt, crop, mean, std = case
    desc = abi.make_export_desc(layout, depth, 1 if depth <= 8 else 2, 0, crop, matrix, full)
    scale = None if size is None else sref.scale_of(size, filt)
    if mean is None:
        tensor = abi.make_export_tensor(st_type, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
        kw = dict(scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0))
    else:
        tensor = abi.make_export_tensor(st_type, *export.affine(depth, mean, std))
        kw = dict(mean=mean, std=std)
    dtype = getattr(torch, DTYPES[st_type])
    got = ctx.export_batch(pics, layout={ref.RGB: "rgb", ref.PLANAR: "planar"}[layout], bit_depth=depth, crop=crop, matrix=matrix,
                           full_range=full, size=size, filter=FILTER_NAMES[filt], dtype=dtype, **kw)
    got = as_tuple(got)
    assert all(t.dtype == dtype for t in got)
    cache = {}
    for i, p in enumerate(pics):
        if p not in cache:
            cache[p] = bref.export_batch_ref(seq, planes_of[p], fmt, bd, desc, scale, tensor)
        want = cache[p]
        if layout == ref.RGB:
            assert got[0].shape[:2] == (len(pics), 3)
            assert np.array_equal(bits(got[0][i]), np.stack(want)), (DTYPES[st_type], case, i)
        else:
            assert len(got) == len(want)
            for k in range(len(want)):
                assert np.array_equal(bits(got[k][i]), want[k]), (DTYPES[st_type], case, i, k)


@pytest.mark.parametrize("st_type", [abi.SAMPLE_F16, abi.SAMPLE_BF16, abi.SAMPLE_F32])
@pytest.mark.parametrize("fmt", [1, 3])
@pytest.mark.parametrize("depth", [8, 10])
def test_float_batch_bit_exact(st_type, fmt, depth):
    bd = (10, 10)
    seq = seq_of(fmt, bd)
    with libhm_amd.Context(seq) as ctx:
        a, b = ctx.acquire(), ctx.acquire()
        planes_of = {a: random_planes(W, H, fmt, bd, seed=7 + fmt), b: random_planes(W, H, fmt, bd, seed=70 + fmt)}
        for p, pl in planes_of.items():
            ctx.upload(p, pl)
        for case in float_cases(fmt, depth):
            check_float_batch(ctx, seq, [a, b, a], planes_of, fmt, bd, depth, st_type, case)


def test_float16_overflow_and_subnormals():
    """D = 16 planar, scale 1: 65520 and above give +inf, 65519 gives 65504; scale 2^-20: subnormal results are kept"""
    torch = _torch()
    bd = (12, 12)
    seq = seq_of(1, bd)
    planes = random_planes(W, H, 1, bd, seed=5)
    planes[0][:, 0:100:2] = 4095                         # 4095 << 4 = 65520 next to 4094 << 4 = 65504: an 8x bilinear enlargement
    planes[0][:, 1:100:2] = 4094                         # passes through every sixteenth between them, 65519 among them
    planes[0][10, 100:164] = np.arange(64)               # small samples for the subnormal case
    one = (1.0, 1.0, 1.0)
    with libhm_amd.Context(seq) as ctx:
        p = ctx.acquire()
        ctx.upload(p, planes)
        desc = abi.make_export_desc(ref.PLANAR, 16, 2, 0, (0, 0, 0, 0), 1, 0)
        tensor = abi.make_export_tensor(abi.SAMPLE_F16, one, (0.0,) * 3)
        seen = set()
        for size, filt in ((None, abi.SCALE_BILINEAR), ((H, 8 * W), abi.SCALE_BILINEAR)):
            scale = None if size is None else sref.scale_of(size, filt)
            ints = bref.integers(seq, planes, 1, bd, desc, scale)
            want = bref.tensor_bits(ints, tensor)
            got = ctx.export_batch([p, p], "planar", 16, size=size, filter="bilinear", dtype=torch.float16, scale=one, bias=(0.0,) * 3)
            for k in range(3):
                assert np.array_equal(bits(got[k][0]), want[k]) and np.array_equal(bits(got[k][1]), want[k]), (size, k)
            y, yb = ints[0], bits(got[0][0])
            seen |= set(int(v) for v in np.unique(y[y >= 65504]))
            assert (yb[y >= 65520] == 0x7C00).all() and (yb[y == 65519] == 0x7BFF).all() and (yb[y == 65504] == 0x7BFF).all()
        assert 65519 in seen and 65520 in seen, sorted(seen)
        # subnormals: 12-bit samples 0 .. 63 at D = 12 times 2^-20 are 0 .. 63 * 16 units of 2^-24
        tiny = (2.0 ** -20,) * 3
        desc = abi.make_export_desc(ref.PLANAR, 12, 2, 0, (0, 0, 0, 0), 1, 0)
        got = ctx.export_batch([p], "planar", 12, dtype=torch.float16, scale=tiny, bias=(0.0,) * 3)
        want = bref.tensor_bits(bref.integers(seq, planes, 1, bd, desc), abi.make_export_tensor(abi.SAMPLE_F16, tiny, (0.0,) * 3))
        for k in range(3):
            assert np.array_equal(bits(got[k][0]), want[k])
        assert list(bits(got[0][0])[10, 100:164]) == [16 * v for v in range(64)]          # (all below 0x0400: subnormal)


# ------------------------------------------------------------------------------------------------ 3. strides and canaries
@pytest.mark.parametrize("offset", [1, 4])          # elements: 1 = no vector stores possible, 4 = 16-byte aligned rows
@pytest.mark.parametrize("size", [None, (36, 100)])
def test_strided_out_views_keep_their_canaries(offset, size):
    """out= views into larger canary-filled tensors: rows longer than needed, planes and batch entries apart; every byte outside the
    planned samples keeps its canary and the samples are right (float16 RGB, float32 planar, uint8 semi-planar)"""
    torch = _torch()
    bd, fmt, n = (10, 10), 1, 3
    seq = seq_of(fmt, bd)
    hh, ww = size or (H, W)
    with libhm_amd.Context(seq) as ctx:
        pics = [ctx.acquire() for _ in range(n)]
        for i, p in enumerate(pics):
            ctx.upload(p, random_planes(W, H, fmt, bd, seed=30 + i))
        kw = dict(size=size, filter="bicubic")

        def canary(shape, dtype):
            return torch.full(shape, CANARY, dtype=torch.uint8, device="cuda").view(dtype)

        def check(big, view_of, want):
            """the big tensor equals the canaries with `want` laid into the view"""
            expect = canary(tuple(big.shape[:-1]) + (big.shape[-1] * big.element_size(),), big.dtype)
            view_of(expect).copy_(want)
            assert torch.equal(big.view(torch.uint8), expect.view(torch.uint8))

        # RGB float16: [2n, 4, hh + 3, ww + 16] -> every second batch entry, planes 1 .. 3, rows 1 .. hh, columns offset ..
        rgb_view = lambda t: t[::2, 1:4, 1:hh + 1, offset:offset + ww]
        big = canary((2 * n, 4, hh + 3, 2 * (ww + 16)), torch.float16)
        r = ctx.export_batch(pics, "rgb", 8, out=rgb_view(big), dtype=torch.float16, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD, **kw)
        assert r.data_ptr() == rgb_view(big).data_ptr()
        check(big, rgb_view, ctx.export_batch(pics, "rgb", 8, dtype=torch.float16, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD, **kw))
        # planar float32: a tuple of [n, h, w] views
        # (12 or more columns of padding, so that every plane's rows are a multiple of 16 bytes: offset 4 takes 16-byte stores)
        want = ctx.export_batch(pics, "planar", 10, dtype=torch.float32, **kw)
        pads = [12 + (-w.shape[2]) % 4 for w in want]
        views = [lambda t, pad=pad: t[1:n + 1, 2:t.shape[1] - 3, offset:offset + t.shape[2] - pad] for pad in pads]
        bigs = [canary((n + 2, w.shape[1] + 5, 4 * (w.shape[2] + pad)), torch.float32) for w, pad in zip(want, pads)]
        assert all((b.shape[2] * 4) % 16 == 0 for b in bigs)
        ctx.export_batch(pics, "planar", 10, out=tuple(v(b) for v, b in zip(views, bigs)), dtype=torch.float32, **kw)
        for b, v, w in zip(bigs, views, want):
            check(b, v, w)
        # semi-planar uint8: ([n, h, w], [n, hc, wc, 2])
        want = ctx.export_batch(pics, "nv12", 8, **kw)
        big_y = canary((n + 1, hh + 2, ww + 12), torch.uint8)
        big_c = canary((n + 1, hh // 2 + 2, ww // 2 + 6, 2), torch.uint8)
        y_view = lambda t: t[:n, 1:hh + 1, offset:offset + ww]
        c_view = lambda t: t[1:, :hh // 2, offset // 2 + 1:offset // 2 + 1 + ww // 2]
        ctx.export_batch(pics, "nv12", 8, out=(y_view(big_y), c_view(big_c)), **kw)
        check(big_y, y_view, want[0])
        check(big_c, c_view, want[1])
        with pytest.raises(ValueError):
            ctx.export_batch(pics, "rgb", 8, out=rgb_view(big)[:2], dtype=torch.float16)          # two slots for three pictures
        with pytest.raises(ValueError):
            ctx.export_batch(pics, "rgb", 8, out=rgb_view(big), dtype=torch.float32)              # the wrong dtype


# ------------------------------------------------------------------------------------------------ 4. refusals on the device
def _hip():
    """the HIP runtime this process already runs on"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            L = C.CDLL(line.split()[-1])
            L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            L.hipFree.argtypes = [C.c_void_p]
            L.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
            L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            return L
    raise RuntimeError("no HIP runtime loaded")


def test_refusals_leave_the_destination_untouched():
    torch = _torch()
    bd, fmt = (10, 10), 1
    seq = seq_of(fmt, bd, max_pictures=20)
    desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    tensor = abi.make_export_tensor(abi.SAMPLE_F16, *export.affine(8))
    plane, pitch = 2 * W * H, 2 * W
    E = abi.HMGPU_EINVAL
    with libhm_amd.Context(seq) as ctx:
        pics = [ctx.acquire() for _ in range(17)]
        ctx.upload(pics[0], random_planes(W, H, fmt, bd, seed=1))
        dst = torch.full((17, 3, H, 2 * W), CANARY, dtype=torch.uint8, device="cuda")
        base = dst.data_ptr()
        ptrs, pitches, bstr = [base + k * plane for k in range(3)], [pitch] * 3, [3 * plane] * 3
        stream = torch.cuda.current_stream().cuda_stream

        def refused(pics_, ptrs_=ptrs, bstr_=bstr, on_stream=1, stream_=stream, status=E, desc_=desc, tensor_=tensor):
            with pytest.raises(libhm_amd.HmgpuError) as e:
                ctx.export_batch_into(pics_, desc_, ptrs_, pitches, bstr_, on_stream, stream_, None, tensor_)
            assert e.value.status == status
            torch.cuda.synchronize()
            ctx.sync()
            assert bool((dst == CANARY).all())

        # the destination check on its own (what libhmdec asks before it spreads a batch over several contexts)
        chk = lambda n_, ptrs_=ptrs, bstr_=bstr: ctx.export_destination_status(n_, desc, ptrs_, pitches, bstr_, None, tensor)
        assert chk(16) == abi.HMGPU_OK and chk(0) == E and chk(17) == E and chk(4, bstr_=[plane - 1] * 3) == E
        assert chk(16, ptrs_=[np.zeros(1, np.uint8).ctypes.data] * 3) == E            # not device memory
        assert bool((dst == CANARY).all())
        refused([])                                                     # n = 0
        refused(pics[:17])                                              # n = 17
        refused([pics[0]] * 15 + [63])                                  # an invalid handle as the last of 16
        refused([pics[0]] * 15 + [-1])
        refused(pics[:4], bstr_=[plane - 1] * 3)                        # a batch stride smaller than a plane
        refused(pics[:4], bstr_=[3 * plane, 3 * plane, pitch * (H - 1)])
        host = np.full(16 * 3 * plane, CANARY, np.uint8)                # a destination on the host
        refused(pics[:16], ptrs_=[host.ctypes.data + k * plane for k in range(3)])
        assert (host == CANARY).all()
        refused(pics[:2], status=abi.HMGPU_EUNSUPPORTED, desc_=abi.make_export_desc(ref.SEMIPLANAR, 8, 1, 0, (0, 0, 0, 0), 1, 0))
        bad = abi.make_export_tensor(abi.SAMPLE_F16)
        bad.reserved[4] = 1
        refused(pics[:2], tensor_=bad)
        # a destination one byte too short for the last slot: an allocation of exactly that size
        hip = _hip()
        total = 15 * 3 * plane + 3 * plane
        raw = C.c_void_p()
        assert hip.hipMalloc(C.byref(raw), total - 1) == 0
        try:
            assert hip.hipMemset(raw, CANARY, total - 1) == 0
            refused(pics[:16], ptrs_=[raw.value + k * plane for k in range(3)])
            back = np.zeros(total - 1, np.uint8)
            assert hip.hipMemcpy(back.ctypes.data, raw, total - 1, 2) == 0
            assert (back == CANARY).all()
            ctx.export_batch_into(pics[:15] , desc, [raw.value + k * plane for k in range(3)], pitches, bstr, 1, stream, None, tensor)   # 15 fit
            torch.cuda.synchronize()
        finally:
            hip.hipFree(raw)


def test_stream_of_another_device_is_refused():
    torch = _torch()
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU: no stream of another device")
    seq = seq_of(1, (10, 10))
    desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    other = torch.cuda.Stream(device=1)
    with libhm_amd.Context(seq) as ctx:
        pics = [ctx.acquire() for _ in range(4)]
        dst = torch.full((4, 3, H, W), CANARY, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(libhm_amd.HmgpuError) as e:
            ctx.export_batch_into(pics, desc, [dst.data_ptr() + k * W * H for k in range(3)], [W] * 3, [3 * W * H] * 3, 1, other.cuda_stream)
        assert e.value.status == abi.HMGPU_EINVAL
        torch.cuda.synchronize()
        assert bool((dst == CANARY).all())


# ------------------------------------------------------------------------------------------------ 5. ordering
def test_ordering_without_host_synchronisation():
    """a batch exported on a side stream, then new contents uploaded into the same handles: the tensor holds the first contents
    after synchronising the side stream alone; and an upload followed at once by a batch export gives the uploaded contents"""
    torch = _torch()
    bd, fmt = (10, 10), 1
    w, h = 832, 480
    seq = seq_of(fmt, bd, w=w, h=h)
    first = [random_planes(w, h, fmt, bd, seed=s) for s in range(4)]
    second = [random_planes(w, h, fmt, bd, seed=10 + s) for s in range(4)]
    desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    tensor = abi.make_export_tensor(abi.SAMPLE_F16, *export.affine(8, bref.IMAGENET_MEAN, bref.IMAGENET_STD))
    want = [[np.stack(bref.export_batch_ref(seq, pl, fmt, bd, desc, None, tensor)) for pl in group] for group in (first, second)]
    kw = dict(dtype=torch.float16, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD)
    side = torch.cuda.Stream()
    with libhm_amd.Context(seq) as ctx:
        pics = [ctx.acquire() for _ in range(4)]
        for p, pl in zip(pics, first):
            ctx.upload(p, pl)
        with torch.cuda.stream(side):
            busy = torch.randn(2048, 2048, device="cuda")
            for _ in range(8):                                   # work ahead of the export on the side stream
                busy = busy @ busy * 1e-3
            t = ctx.export_batch(pics, "rgb", 8, **kw)
        for p, pl in zip(pics, second):                          # at once: the context must wait for the export before overwriting
            ctx.upload(p, pl)
        side.synchronize()
        for i in range(4):
            assert np.array_equal(bits(t[i]), want[0][i]), i
        # mirror: the last upload is followed by the export with nothing in between
        with torch.cuda.stream(side):
            for p, pl in zip(pics, first):
                ctx.upload(p, pl)
            t2 = ctx.export_batch(pics, "rgb", 8, **kw)
        side.synchronize()
        for i in range(4):
            assert np.array_equal(bits(t2[i]), want[0][i]), i
        t3 = ctx.export_batch(pics, "rgb", 8, on_stream=False, **kw)          # and on the context's own stream
        ctx.sync()
        for i in range(4):
            assert np.array_equal(bits(t3[i]), want[0][i]), i


# ------------------------------------------------------------------------------------------------ 6. decoder
@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("name,batch", [("ra_notmvp_main8_208x120", 4), ("ldb_444_main10_208x120", 2), ("ra_cra_main8_208x120", 16)])
def test_decoder_frames_batched(name, batch, devices):
    """Decoder.frames(batch=) with float16 ImageNet RGB at 60 x 104 == the per-picture integer exports of a second decode put
    through the restatement; every POC once, in output order, full items first (9 pictures by 4: two; 3 by 2: one; 18 by 16: one),
    the last item the remainder"""
    torch = _torch()
    z = gu.load("lite_" + name)
    frames = int(z["geom"][2])
    size = (60, 104)
    ints = {}
    with hmdec.Decoder(threads=2, device_output=True) as d:
        for poc, t in d.frames(z["bitstream"], layout="rgb", size=size, filter="bicubic"):
            ints[poc] = t.cpu().numpy().astype(np.int64)
    assert len(ints) == frames
    tensor = abi.make_export_tensor(abi.SAMPLE_F16, *export.affine(8, bref.IMAGENET_MEAN, bref.IMAGENET_STD))
    seen, items = [], []
    with hmdec.Decoder(threads=1 if devices else 2, device_output=True, devices=devices) as d:
        for pocs, t in d.frames(z["bitstream"], batch=batch, layout="rgb", dtype=torch.float16, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD,
                                size=size, filter="bicubic"):
            assert t.shape == (len(pocs), 3) + size and t.dtype == torch.float16
            items.append(len(pocs))
            for i, poc in enumerate(pocs):
                assert np.array_equal(bits(t[i]), np.stack(bref.tensor_bits(list(ints[poc]), tensor))), (name, poc)
            seen += pocs
        assert d.download_bytes == 0
    assert seen == sorted(ints)
    assert frames > batch and frames % batch                 # at least one full item, then a remainder
    assert items == [batch] * (frames // batch) + [frames % batch]


def test_hmdec_export_batch_planar_and_refusals():
    """hmdec.export_batch on the pictures fetched after one push: integer planar planes equal Picture.export's; pictures of two
    decoders in one call are refused"""
    torch = _torch()
    z = gu.load("lite_ldp_crop_main8_204x116")
    nals = hmdec.split_nal_units(z["bitstream"])
    with hmdec.Decoder(device_output=True) as d, hmdec.Decoder(device_output=True) as d2:
        def fetched(dec):
            for i, nal in enumerate(nals):
                while True:
                    new_pic, check = dec.push(nal, i == len(nals) - 1)
                    got = []
                    while check:
                        p = dec.get_picture()
                        if p is None:
                            break
                        got.append(p)
                    if got:
                        yield got
                    if not new_pic:
                        break
        other = next(fetched(d2))
        total = 0
        for got in fetched(d):
            batch = hmdec.export_batch(got + got[:1], layout="planar", bit_depth=None)
            for i, p in enumerate(got + got[:1]):
                for a, b in zip(batch, p.export(layout="planar", bit_depth=None)):
                    assert torch.equal(a[i], b)
            total += len(got)
            with pytest.raises(libhm_amd.HmgpuError):
                hmdec.export_batch(got + other[:1], layout="planar", bit_depth=None)
        assert total == int(z["geom"][2])


# ------------------------------------------------------------------------------------------------ 7. one picture, float elements
def test_single_picture_float_export():
    """Picture.export(dtype=torch.float32) and Context.export(dtype=) equal the batch reference for n = 1, without a batch dimension"""
    torch = _torch()
    bd, fmt = (10, 10), 1
    seq = seq_of(fmt, bd)
    planes = random_planes(W, H, fmt, bd, seed=77)
    desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    tensor = abi.make_export_tensor(abi.SAMPLE_F32, *export.affine(8, bref.IMAGENET_MEAN, bref.IMAGENET_STD))
    with libhm_amd.Context(seq) as ctx:
        p = ctx.acquire()
        ctx.upload(p, planes)
        for size, filt in ((None, abi.SCALE_BILINEAR), ((36, 100), abi.SCALE_AREA)):
            scale = None if size is None else sref.scale_of(size, filt)
            t = ctx.export(p, "rgb", 8, size=size, filter=FILTER_NAMES[filt], dtype=torch.float32, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD)
            assert t.dtype == torch.float32 and t.dim() == 3
            assert np.array_equal(bits(t), np.stack(bref.export_batch_ref(seq, planes, fmt, bd, desc, scale, tensor)))
    z = gu.load("lite_ldp_crop_main8_204x116")
    ints = {}
    with hmdec.Decoder(device_output=True) as d:
        for poc, t in d.frames(z["bitstream"], layout="rgb"):
            ints[poc] = t.cpu().numpy().astype(np.int64)
    with hmdec.Decoder(device_output=True) as d:
        for poc, t in d.frames(z["bitstream"], layout="rgb", dtype=torch.float32, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD):
            assert t.dtype == torch.float32 and t.shape == ints[poc].shape
            assert np.array_equal(bits(t), np.stack(bref.tensor_bits(list(ints[poc]), tensor))), poc
