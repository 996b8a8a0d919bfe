"""Device export on the GPU: k_export.hip behind hmgpu_picture_export / hmdec_picture_export / Picture.export, bit-exact against the
numpy restatement (tests/export_ref.py), HM's `TAppDecoder -d N` files and the golden reconstructions; stream ordering against torch."""
import itertools

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, hmdec
from tests import export_ref as ref
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

CANARY = 0xA5


def _torch():
    import torch
    return torch


def random_planes(w, h, fmt, bd, seed):
    rng = np.random.default_rng(seed)
    sx, sy = ref.chroma_shift(fmt)
    return [rng.integers(0, 1 << bd[0], (h, w)).astype(np.int16)] + \
           [rng.integers(0, 1 << bd[1], (h >> sy, w >> sx)).astype(np.int16) for _ in range(2)]


def export_raw(ctx, pic, desc, plan, pad, on_stream, stream):
    """export into uint8 device buffers whose rows are `pad` bytes longer than needed, filled with canary bytes first"""
    torch = _torch()
    bufs, pitches = [], []
    for k in range(plan.planes):
        pitch = plan.row_bytes[k] + pad
        bufs.append(torch.full((plan.height[k], pitch), CANARY, dtype=torch.uint8, device="cuda:%d" % ctx.device))
        pitches.append(pitch)
    torch.cuda.current_stream().synchronize()
    ctx.export_into(pic, desc, [b.data_ptr() for b in bufs], pitches, on_stream, stream)
    if on_stream:
        torch.cuda.current_stream().synchronize()
    else:
        ctx.sync()
    out = []
    for k, b in enumerate(bufs):
        a = b.cpu().numpy()
        assert (a[:, plan.row_bytes[k]:] == CANARY).all(), "padding written (plane %d)" % k
        a = a[:, :plan.row_bytes[k]]
        out.append(a.view("<u2") if desc.bytes_per_sample == 2 else a)
    return out


def expected(planes, fmt, bd, desc, plan):
    out_bd = (desc.bit_depth[0] or bd[0], desc.bit_depth[1] or bd[1])
    if desc.layout == ref.RGB:
        return list(ref.export_rgb(planes, fmt, bd, out_bd[0], list(plan.coef), tuple(desc.crop), desc.msb_aligned))
    got = ref.export_yuv(planes, fmt, bd, out_bd, desc.layout, tuple(desc.crop), desc.msb_aligned)
    return [g.reshape(g.shape[0], -1) for g in got]


BDS = [(8, 8), (10, 10), (12, 12), (10, 8)]


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("bd", BDS)
def test_random_planes_bit_exact(fmt, bd):
    """every layout x output depth x container x crop, against the numpy restatement; canaries in the row padding stay"""
    torch = _torch()
    w, h = 200, 72
    seq = abi.make_seq(w, h, bd[0], bd[1], max_pictures=2)
    seq.chroma_format = fmt
    planes = random_planes(w, h, fmt, bd, seed=fmt * 100 + bd[0] * 10 + bd[1])
    side = torch.cuda.Stream()
    n = 0
    with libhm_amd.Context(seq) as ctx:
        pic = ctx.acquire()
        ctx.upload(pic, planes)
        cases = []
        for layout, out_bd, msb, crop in itertools.product((ref.PLANAR, ref.SEMIPLANAR, ref.RGB), (8, 10, 16), (0, 1), ((0, 0, 0, 0), (4, 8, 2, 6), (2, 6, 0, 2))):
            nbytes = 1 if out_bd == 8 and not msb else 2
            if msb and out_bd == 16:
                continue
            mats = [(1, 0)] if layout != ref.RGB else [(1, 0), (9, 1), (5, 0)] + ([(0, 0)] if fmt == 3 else [])
            for matrix, full in mats:
                cases.append(abi.make_export_desc(layout, out_bd, nbytes, msb, crop, matrix, full))
        for i, desc in enumerate(cases):
            plan = libhm_amd.export_plan(seq, desc)
            want = expected(planes, fmt, bd, desc, plan)
            mode = i % 3                        # context stream / torch side stream / torch's null stream
            pad = 64 if i % 2 == 0 else 3       # (odd padding: unaligned rows take the scalar path)
            if mode == 1:
                with torch.cuda.stream(side):
                    got = export_raw(ctx, pic, desc, plan, pad, 1, side.cuda_stream)
            elif mode == 2:
                got = export_raw(ctx, pic, desc, plan, pad, 1, 0)
            else:
                got = export_raw(ctx, pic, desc, plan, pad, 0, 0)
            assert len(got) == len(want)
            for k in range(len(want)):
                assert np.array_equal(got[k].astype(np.int64), want[k]), (desc.layout, list(desc.bit_depth), desc.msb_aligned, tuple(desc.crop), desc.matrix, k)
            n += 1
    assert n > 50


def test_every_triple_to_rgb():
    """a 4096 x 4096 4:4:4 8-bit picture holding every (Y, Cb, Cr) once: RGB for every matrix and range equals the numpy reference"""
    torch = _torch()
    i = np.arange(1 << 24, dtype=np.int64)
    planes = [(i & 255).reshape(4096, 4096).astype(np.int16), ((i >> 8) & 255).reshape(4096, 4096).astype(np.int16),
              (i >> 16).reshape(4096, 4096).astype(np.int16)]
    seq = abi.make_seq(4096, 4096, 8, 8, max_pictures=1)
    seq.chroma_format = 3
    with libhm_amd.Context(seq) as ctx:
        pic = ctx.acquire()
        ctx.upload(pic, planes)
        for matrix, full in [(1, 0), (1, 1), (5, 0), (5, 1), (9, 0), (9, 1), (0, 0)]:
            t = ctx.export(pic, "rgb", 8, (0, 0, 0, 0), matrix, full)
            torch.cuda.current_stream().synchronize()
            plan = libhm_amd.export_plan(seq, abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), matrix, full))
            want = ref.export_rgb(planes, 3, (8, 8), 8, list(plan.coef))
            assert t.shape == (3, 4096, 4096) and t.dtype == torch.uint8
            assert np.array_equal(t.cpu().numpy(), want), (matrix, full)


# ------------------------------------------------------------------------------------------------ libhmdec
LITE = ["ldp_crop_main8_204x116", "ldb_mono_wp_crop_main10_204x116", "ldb_422_main12_208x120", "ldb_444_main10_208x120", "ldp_bd10_8_208x120"]


def _as_np(t):
    torch = _torch()
    if t.dtype == torch.int16 or t.dtype == getattr(torch, "uint16", None):
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("name", LITE)
def test_decoder_planar_export_equals_golden(name, threads):
    """device output: PLANAR at the coding depth with the conformance crop == the golden reconstruction; nothing downloaded"""
    z = gu.load("lite_" + name)
    frames = int(z["geom"][2])
    seen = []
    with hmdec.Decoder(threads=threads, device_output=True) as d:
        for poc, planes in d.frames(z["bitstream"], layout="planar", bit_depth=None):
            seen.append(poc)
            for c, p in enumerate(planes):
                assert np.array_equal(_as_np(p).astype(np.int64), z["poc%02d_%d" % (poc, c)].astype(np.int64)), (name, poc, c)
            assert len(planes) == (1 if "mono" in name else 3)
        assert d.download_bytes == 0
        assert d.hash_mismatches == 0
    assert seen == list(range(frames))


HM_D = ["d8_ldp_main10_208x120", "d8_ldb_main12_208x120", "d10_ldb_main12_208x120", "d10_ldp_main8_416x240", "d16_ldp_main8_416x240",
        "d8_ldb_422_main10_208x120", "d8_intra_444_ccp_main10_208x120", "d10_ldp_crop_main8_204x116", "d8_ldb_mono_wp_crop_main10_204x116"]


@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("name", HM_D)
def test_decoder_export_equals_hm_d(name, devices):
    g = gu.load("export_" + name)
    w, h, fmt, frames, out_bd = (int(v) for v in g["geom"])
    src = gu.load(str(g["source"]))
    with hmdec.Decoder(threads=1 if devices else 3, device_output=True, devices=devices) as d:
        n = 0
        for poc, planes in d.frames(src["bitstream"], layout="planar", bit_depth=out_bd):
            for c, p in enumerate(planes):
                assert np.array_equal(_as_np(p), g["poc%02d_%d" % (poc, c)]), (name, poc, c)
            n += 1
        assert n == frames
        assert d.download_bytes == 0 and d.hash_mismatches == 0


@pytest.mark.parametrize("name", ["ldp_crop_main8_204x116", "ldb_422_main12_208x120"])
def test_lazy_planes_in_device_output_mode(name):
    """an unmodified libHM client still gets its planes: libHMDEC_get_image_plane downloads on first use"""
    z = gu.load("lite_" + name)
    seen = []
    with hmdec.Decoder(device_output=True) as d:
        def on_output(p):
            before = d.download_bytes
            for c in range(3):
                assert np.array_equal(p.cropped_plane(c), z["poc%02d_%d" % (p.poc, c)])
            seen.append(d.download_bytes - before)
        d.decode_stream(z["bitstream"], on_output=on_output)
    assert len(seen) == int(z["geom"][2]) and all(b > 0 for b in seen)


def test_frames_rgb_matches_host_path():
    """Decoder.frames(layout="rgb"): tensors on the picture's GPU, [3, H, W] uint8, equal to the numpy RGB of the host-path planes
    (the colour policy: this stream has no VUI -> BT.709 limited)"""
    torch = _torch()
    z = gu.load("stream_ldp_main10_208x120")
    host = {}
    with hmdec.Decoder() as d:
        d.decode_stream(z["bitstream"], on_output=lambda p: host.__setitem__(p.poc, [p.plane(c) for c in range(3)]))
    seq = abi.make_seq(208, 120, 10, 10)
    plan = libhm_amd.export_plan(seq, abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0))
    n = 0
    with hmdec.Decoder(device_output=True, threads=2) as d:
        for poc, t in d.frames(z["bitstream"], layout="rgb"):
            assert t.device == torch.device("cuda", 0) and t.dtype == torch.uint8 and t.shape == (3, 120, 208)
            assert np.array_equal(t.cpu().numpy(), ref.export_rgb(host[poc], 1, (10, 10), 8, list(plan.coef)))
            n += 1
        assert d.download_bytes == 0
    assert n == len(host)


def test_vui_stream_exports_with_its_own_matrix():
    """BT.2020 full range from the VUI, against the numpy RGB of the encoder's reconstruction"""
    z = gu.load("export_vui_bt2020_main10_208x120")
    seq = abi.make_seq(208, 120, 10, 10)
    plan = libhm_amd.export_plan(seq, abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 9, 1))
    with hmdec.Decoder(device_output=True) as d:
        for poc, t in d.frames(z["bitstream"], layout="rgb"):
            planes = [z["poc%02d_%d" % (poc, c)] for c in range(3)]
            assert np.array_equal(t.cpu().numpy(), ref.export_rgb(planes, 1, (10, 10), 8, list(plan.coef)))


def test_allocator_reuse_on_a_side_stream():
    """50 exports into fresh tensors allocated and freed on a side stream, with other work reusing the freed blocks in between:
    every export lands after the allocator handed the memory over, and before the next user of the blocks"""
    torch = _torch()
    w, h = 416, 240
    seq = abi.make_seq(w, h, 10, 10, max_pictures=4)
    planes = [random_planes(w, h, 1, (10, 10), seed=s) for s in range(4)]
    plan = libhm_amd.export_plan(seq, abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0))
    side = torch.cuda.Stream()
    with libhm_amd.Context(seq) as ctx:
        pics = [ctx.acquire() for _ in range(4)]
        for p, pl in zip(pics, planes):
            ctx.upload(p, pl)
        want = [torch.from_numpy(ref.export_rgb(pl, 1, (10, 10), 8, list(plan.coef)).astype(np.uint8)).cuda() for pl in planes]
        ok = []
        with torch.cuda.stream(side):
            for i in range(50):
                t = ctx.export(pics[i % 4], "rgb", 8)
                ok.append(torch.equal(t, want[i % 4]))
                del t
                junk = torch.empty((3, h, w), dtype=torch.uint8, device="cuda")
                junk.fill_(7)
                del junk
        side.synchronize()
        assert all(ok), ok
