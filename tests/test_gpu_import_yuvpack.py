"""Packed YUV import on the GPU: hmgpu_pictures_import_yuvpack behind yuv= of Context.import_batch / import_picture.  The call is
defined by the existing one: the words unpacked by include/hmgpu.h's table are a planar source, and the pictures must receive what
hmgpu_pictures_import gives for those planes.  So every check is an equality of downloaded planes: one picture imported from
tests/yuvpack_ref.py's pack() of the planes, one from the planes themselves through the existing planar import (held against numpy by
tests/test_gpu_import.py)."""
import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi
from tests import geometry_cases as gc
from tests import synth
from tests import yuvpack_ref as yref
from tests.test_gpu_formats_fullsize import _oracle_chain, _same
from tests.test_gpu_import import DOWNS, NAMES, assert_planes, dev, download_full, seq_of, source_planes

pytestmark = pytest.mark.gpu

W, H = 72, 40
SIZES = [(72, 40), (70, 38)]
EINVAL, EUNSUPPORTED = abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED


def _torch():
    import torch
    return torch


def garbage(fmt, buf, rng):
    """what an import must read over: A, bits 30-31 of v210 words, the low six bits of y210 elements"""
    buf = buf.copy()
    if fmt == "v210":
        buf[:, 3::4] |= rng.integers(0, 4, buf[:, 3::4].shape).astype(np.uint8) << 6
    elif fmt == "y210":
        buf[:, 0::2] |= rng.integers(0, 64, buf[:, 0::2].shape).astype(np.uint8)
    elif fmt == "ayuv":
        buf[:, 3::4] = rng.integers(0, 256, buf[:, 3::4].shape)
    elif fmt == "y410":
        buf[:, 3::4] |= rng.integers(0, 4, buf[:, 3::4].shape).astype(np.uint8) << 6
    elif fmt == "y416":
        buf[:, 6::8] = rng.integers(0, 256, buf[:, 6::8].shape)
        buf[:, 7::8] = rng.integers(0, 256, buf[:, 7::8].shape)
    return buf


def desc_of(fmt, w, h, down="drop", loc=0):
    d = yref.DEPTH[fmt]
    return abi.make_import_desc(abi.EXPORT_PLANAR, -1, (w, h), (d, d), 1 if d <= 8 else 2, 0, abi.SAMPLE_UINT, chroma_format=yref.CHROMA[fmt],
                                down=down, loc=loc)


def import_words(ctx, pics, fmt, bufs, w, h, down="drop", loc=0, off=0, on_stream=False):
    """the entry itself: one [H, pitch] uint8 array of words per picture, in one device buffer `off` bytes beyond a 256-byte boundary"""
    torch = _torch()
    pitch = bufs[0].shape[1]
    stride = pitch * bufs[0].shape[0] + 2 * yref.ELEMENT[fmt]
    t = torch.empty((512 + off + len(bufs) * stride,), dtype=torch.uint8, device="cuda")
    start = -t.data_ptr() % 256 + off
    host = np.full((t.numel(),), 0x5A, np.uint8)
    for i, b in enumerate(bufs):
        host[start + i * stride:start + i * stride + b.size] = b.reshape(-1)
    t.copy_(torch.from_numpy(host))
    torch.cuda.synchronize()                                     # (the copy is on torch's stream, the import may be on the context's)
    base = t.data_ptr() + start
    stream = torch.cuda.current_stream().cuda_stream if on_stream else 0
    ctx.import_yuvpack_into(pics, desc_of(fmt, w, h, down, loc), abi.make_import_yuvpack(fmt), base, pitch, stride, 1 if on_stream else 0, stream)
    return t


def import_planes(ctx, pic, fmt, planes, down="drop", loc=0):
    """the yardstick: the existing planar import of the same planes"""
    d = yref.DEPTH[fmt]
    ctx.import_picture(pic, tuple(dev(v, 1 if d <= 8 else 2) for v in planes), layout="planar", bit_depth=d, chroma_format=NAMES[yref.CHROMA[fmt]],
                       chroma_down=down, chroma_loc=loc)


# ------------------------------------------------------------------------------------------------ every format into every picture format
@pytest.mark.parametrize("fmt", yref.FORMATS)
def test_words_give_what_their_planes_give(fmt):
    cf, d = yref.CHROMA[fmt], yref.DEPTH[fmt]
    rng = np.random.default_rng(7)
    for pic_fmt in (0, 1, 2, 3):
        loses = pic_fmt and (pic_fmt < cf)
        for bd in (8, 10):
            with libhm_amd.Context(seq_of(pic_fmt, (bd, bd))) as ctx:
                a, b = ctx.acquire(), ctx.acquire()
                for k, (sw, sh) in enumerate(SIZES):
                    src = source_planes(cf, sw, sh, (d, d), 10 * pic_fmt + bd + k)
                    words = garbage(fmt, yref.pack(fmt, *src, alpha=0, pitch=yref.row_bytes(fmt, sw) + 16 * k, canary=0x5A), rng)
                    for down, loc in (DOWNS if loses else DOWNS[:1]):
                        import_planes(ctx, a, fmt, src, down, loc)
                        import_words(ctx, [b], fmt, [words], sw, sh, down, loc, on_stream=bool(k))
                        assert_planes(download_full(ctx, b, pic_fmt), download_full(ctx, a, pic_fmt),
                                      "%s %dx%d into %s at %d bits, %s loc %d" % (fmt, sw, sh, NAMES[pic_fmt], bd, down, loc))


@pytest.mark.parametrize("fmt", yref.FORMATS)
def test_unaligned_sources_and_batches(fmt):
    """sources off 16-, 8- and 4-byte alignment by the format's own element; three pictures a call"""
    cf, d, es = yref.CHROMA[fmt], yref.DEPTH[fmt], yref.ELEMENT[fmt]
    with libhm_amd.Context(seq_of(1, (10, 10), max_pictures=6)) as ctx:
        want = [ctx.acquire() for _ in range(3)]
        got = [ctx.acquire() for _ in range(3)]
        srcs = [source_planes(cf, 70, 38, (d, d), 50 + i) for i in range(3)]
        for i in range(3):
            import_planes(ctx, want[i], fmt, srcs[i], "linear", 2)
        for off in (es, 3 * es, 4, 8):
            if off % es:
                continue
            for g in got:
                ctx.upload(g, [np.zeros((H, W), np.int16), np.zeros((H // 2, W // 2), np.int16), np.zeros((H // 2, W // 2), np.int16)])
            import_words(ctx, got, fmt, [yref.pack(fmt, *s, pitch=yref.row_bytes(fmt, 70) + 4 * es) for s in srcs], 70, 38, "linear", 2, off=off)
            for i in range(3):
                assert_planes(ctx.download(got[i]), ctx.download(want[i]), "%s offset %d picture %d" % (fmt, off, i))


# ------------------------------------------------------------------------------------------------ with the export
@pytest.mark.parametrize("fmt", yref.FORMATS)
def test_export_then_import_is_the_identity(fmt):
    """pictures of the words' own chroma format and depth (16-bit words: 12-bit pictures widened and narrowed again)"""
    cf, d = yref.CHROMA[fmt], yref.DEPTH[fmt]
    bd = min(d, 12)
    with libhm_amd.Context(seq_of(cf, (bd, bd), max_pictures=6)) as ctx:
        pics = [ctx.acquire() for _ in range(3)]
        back = [ctx.acquire() for _ in range(3)]
        planes = [[np.ascontiguousarray(v, np.int16) for v in source_planes(cf, W, H, (bd, bd), 90 + i)] for i in range(3)]
        for p, v in zip(pics, planes):
            ctx.upload(p, v)
        for kw in (dict(), dict(crop=(0, 2, 0, 2))):
            words = ctx.export_batch(pics, yuv=fmt, row_align=128 if fmt == "v210" else 1, **kw)
            size = (38, 70) if kw else ((H, W) if fmt == "v210" else None)
            ctx.import_batch(back, words, yuv=fmt, size=size)
            for i in range(3):
                want = planes[i] if not kw else [np.pad(v[:38 >> (0 if k == 0 or cf != 1 else 1), :70 >> (0 if k == 0 or cf == 3 else 1)],
                                                        ((0, H - 38), (0, (W - 70) >> (0 if k == 0 or cf == 3 else 1))), mode="edge")
                                                 for k, v in enumerate(planes[i])]
                assert_planes(ctx.download(back[i]), want, "%s round trip %s picture %d" % (fmt, sorted(kw), i))
        one = ctx.export(pics[1], yuv=fmt)
        ctx.import_picture(back[0], one, yuv=fmt, size=(H, W) if fmt == "v210" else None)
        assert_planes(ctx.download(back[0]), planes[1], "%s one picture" % fmt)
        with pytest.raises(ValueError):
            ctx.import_batch(back, words, yuv=fmt, bit_depth=8)
        with pytest.raises(ValueError):
            ctx.import_batch(back, words[:2], yuv=fmt)


def test_an_imported_picture_is_a_reference(oracle):
    """A's final planes from the oracle arrive as Y210 words; B's prediction units lie in A's margins"""
    torch = _torch()
    fmt = 2
    case = (W, H, 4, fmt, 10, 10)
    a_of, bs = gc.margin_pictures(case)
    ref0 = synth.noise_planes(W, H, 10, 3, fmt, 10)
    zero = [np.zeros_like(x) for x in ref0]
    fin = _oracle_chain(oracle, a_of["sao"], zero, [ref0])[2]
    seq = abi.SeqParams.from_buffer_copy(bs[0].seq)
    seq.max_pictures = 3
    with libhm_amd.Context(seq) as ctx:
        h0, ha, hb = ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        words = torch.from_numpy(yref.pack("y210", *fin).view(np.int16).reshape(1, H, W, 2)).cuda()
        ctx.import_batch([ha], words, yuv="y210")
        _same(ctx.download(ha), fin, "A imported from Y210")
        for k, b in enumerate(bs):
            sl = abi.clone_slice(b.slice)
            sl.ref_pic[0][0] = ha
            want = [x.copy() for x in zero]
            oracle.decompress_ctus(b.seq, [b.slice], b.meta, b.coeffs, want, [fin])
            ctx.upload(hb, zero)
            ctx.decompress_slice(hb, 0, sl, b.meta, b.coeffs)
            _same(ctx.download(hb), want, "picture B%d" % k)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_pictures_untouched():
    torch = _torch()
    with libhm_amd.Context(seq_of(2, (10, 10), max_pictures=4)) as ctx:
        pics = [ctx.acquire() for _ in range(3)]
        planes = [np.ascontiguousarray(v, np.int16) for v in source_planes(2, W, H, (10, 10), 5)]
        for p in pics:
            ctx.upload(p, planes)
        buf = torch.full((3 * H * W * 8 + 512,), 0x11, dtype=torch.uint8, device="cuda")
        base = buf.data_ptr() + (-buf.data_ptr() % 256)

        def run(fmt, desc="good", pk="good", ptrs=None, pitch=None, bstride=None, handles=None):
            desc = desc_of(fmt, W, H) if desc == "good" else desc
            pk = abi.make_import_yuvpack(fmt) if pk == "good" else pk
            rb = yref.row_bytes(fmt, W)
            pitch = rb if pitch is None else pitch
            bstride = pitch * H if bstride is None else bstride
            ptrs = [base] if ptrs is None else ptrs
            st = ctx.import_yuvpack_status(pics if handles is None else handles, desc, pk, ptrs, [pitch], [bstride])
            if handles is None:
                assert ctx.import_yuvpack_source_status(3, desc, pk, ptrs, [pitch], [bstride]) == st
            return st

        def changed(fmt, **kw):
            d = desc_of(fmt, W, H)
            for k, v in kw.items():
                if k == "bit_depth":
                    d.bit_depth[0], d.bit_depth[1] = v
                elif k == "reserved":
                    d.reserved[v] = 1
                else:
                    setattr(d, k, v)
            return d

        reserved = abi.make_import_yuvpack("uyvy")
        reserved.reserved[6] = 1
        for fmt in yref.FORMATS:
            cf, D, es, rb = yref.CHROMA[fmt], yref.DEPTH[fmt], yref.ELEMENT[fmt], yref.row_bytes(fmt, W)
            assert run(fmt, pk=None) == EINVAL and run(fmt, pk=reserved) == EINVAL
            assert run(fmt, pk=abi.make_import_yuvpack(8)) == EUNSUPPORTED and run(fmt, pk=abi.make_import_yuvpack(-1)) == EUNSUPPORTED
            assert run(fmt, desc=None) == EINVAL
            assert run(fmt, desc=changed(fmt, layout=abi.EXPORT_SEMIPLANAR)) == EINVAL and run(fmt, desc=changed(fmt, layout=abi.EXPORT_RGB)) == EINVAL
            assert run(fmt, desc=changed(fmt, order=0)) == EINVAL and run(fmt, desc=changed(fmt, chroma_format=5 - cf)) == EINVAL
            assert run(fmt, desc=changed(fmt, bit_depth=(D, 12))) == EINVAL and run(fmt, desc=changed(fmt, bit_depth=(9, D))) == EINVAL
            assert run(fmt, desc=changed(fmt, sample_type=abi.SAMPLE_F16)) == EINVAL and run(fmt, desc=changed(fmt, bytes_per_sample=3 - (1 if D <= 8 else 2))) == EINVAL
            if D > 8:
                assert run(fmt, desc=changed(fmt, msb_aligned=1)) == EINVAL
            # the planar import's own steps
            assert run(fmt, desc=changed(fmt, reserved=3)) == EINVAL and run(fmt, desc=changed(fmt, loc=6)) == EINVAL
            assert run(fmt, desc=changed(fmt, width=W + 2)) == EINVAL and run(fmt, desc=changed(fmt, width=35)) == EINVAL
            assert run(fmt, desc=changed(fmt, down=2)) == EUNSUPPORTED
            # the stated order: the format before the descriptor; the descriptor before an unknown `down`
            assert run(fmt, desc=changed(fmt, layout=abi.EXPORT_RGB), pk=abi.make_import_yuvpack(9)) == EUNSUPPORTED
            assert run(fmt, desc=changed(fmt, down=2, order=0)) == EINVAL
            # the source
            assert run(fmt, ptrs=[None]) == EINVAL and run(fmt, ptrs=[base, base]) == EINVAL and run(fmt, ptrs=[base, None, base]) == EINVAL
            assert run(fmt, pitch=rb - es) == EINVAL and run(fmt, bstride=rb * H - es) == EINVAL and run(fmt, bstride=1 << 40) == EINVAL
            if es > 1:
                assert run(fmt, ptrs=[base + es // 2]) == EINVAL and run(fmt, pitch=rb + es // 2) == EINVAL and run(fmt, bstride=rb * H + es // 2) == EINVAL
            assert run(fmt, handles=pics[:2] + [99]) == EINVAL and run(fmt, handles=[pics[0], pics[1], pics[0]]) == EINVAL
        ctx.sync()
        for p in pics:
            assert_planes(ctx.download(p), planes, "after the refusals")
        assert run("y416") == abi.HMGPU_OK
        assert not np.array_equal(ctx.download(pics[0])[0], planes[0])
