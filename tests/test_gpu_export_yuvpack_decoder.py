"""Packed YUV through the decoder: hmdec_pictures_export_yuvpack behind yuv= of Picture.export, hmdec.export_batch and Decoder.frames,
on one 4:2:0 and one 4:2:2 fixture stream.  Every result must be the numpy model of tests/yuvpack_ref.py applied to the same call's
planar format export (chroma_format= of the words' chroma format at their depth), which tests/test_gpu_export_format_decoder.py
holds against a plain context."""
import numpy as np
import pytest

from libhm_amd import hmdec
from tests import golden_util as gu
from tests import yuvpack_ref as yref
from tests.test_gpu_export_format import bits

pytestmark = pytest.mark.gpu

STREAMS = {"420": "export_vui_bt2020_chromaloc2_main10_208x120", "422": "stream_ldb_422_main10_208x120"}


def _torch():
    import torch
    return torch


def rows(t):
    """words [N, H, ...] as numpy bytes [N, H, bytes of a row]"""
    return t.contiguous().view(_torch().uint8).cpu().numpy().reshape(t.shape[0], t.shape[1], -1)


def packed(fmt, planar, n):
    """the model on a planar format export: (Y, Cb, Cr) planes [N, ...], or one [N, 3, H, W] tensor at 4:4:4"""
    p = [bits(planar[:, k]) for k in range(3)] if yref.CHROMA[fmt] == 3 else [bits(t) for t in planar]
    return [yref.pack(fmt, p[0][i], p[1][i], p[2][i]) for i in range(n)]


def planar_kw(fmt, **kw):
    return dict(layout="planar", bit_depth=yref.DEPTH[fmt], chroma_format="422" if yref.CHROMA[fmt] == 2 else "444", **kw)


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_pictures_batches_and_frames(name):
    z = gu.load(STREAMS[name])
    conv = dict(chroma="linear", chroma_down="linear")
    seen, kept = [], {}
    with hmdec.Decoder(threads=1, device_output=True) as d:
        def on_output(p):
            # Picture.export: one picture, no batch dimension
            one = p.export(yuv="v210", **conv)
            want = packed("v210", hmdec.export_batch([p], **planar_kw("v210", **conv)), 1)[0]
            rb = want.shape[1]
            assert one.dim() == 2 and one.dtype == _torch().int32 and np.array_equal(rows(one[None])[0][:, :rb], want), p.poc
            wide = p.export(yuv="v210", row_align=128, **conv)
            assert wide.shape[1] * 4 % 128 == 0 and np.array_equal(rows(wide[None])[0][:, :rb], want)
            # hmdec.export_batch: a batch with a repeated picture, windows and a mirror
            batch = [p, p, p]
            for v in ({}, dict(windows=[(2, 6, 100, 60), (6, 2, 100, 60), (108, 60, 100, 60)], flip=[False, True, True])):
                got = hmdec.export_batch(batch, yuv="uyvy", **conv, **v)
                want3 = packed("uyvy", hmdec.export_batch(batch, **planar_kw("uyvy", **conv, **v)), 3)
                assert got.dim() == 4 and got.shape[3] == 2 and got.dtype == _torch().uint8
                assert all(np.array_equal(rows(got)[i], want3[i]) for i in range(3)), (p.poc, sorted(v))
            got = hmdec.export_batch(batch, yuv="y410", alpha=3, **conv)
            p444 = hmdec.export_batch(batch, **planar_kw("y410", **conv))
            y, cb, cr = (bits(p444[:, k]) for k in range(3))
            assert all(np.array_equal(rows(got)[i], yref.pack("y410", y[i], cb[i], cr[i], 3)) for i in range(3))
            kept[p.poc] = packed("y210", hmdec.export_batch([p], **planar_kw("y210", **conv)), 1)[0]
            seen.append(p.poc)
        d.decode_stream(bytes(z["bitstream"]), on_output=on_output)
        assert d.hash_mismatches == 0 and len(seen) >= 2
    # Decoder.frames: batches of three and single pictures
    with hmdec.Decoder(threads=1, device_output=True) as d:
        got = []
        for pocs, t in d.frames(z["bitstream"], batch=3, yuv="y210", **conv):
            assert t.dim() == 4 and t.shape[3] == 2
            for i, poc in enumerate(pocs):
                assert np.array_equal(rows(t)[i], kept[poc]), poc
            got += pocs
        assert sorted(got) == sorted(seen)
    with hmdec.Decoder(threads=1, device_output=True) as d:
        got = []
        for poc, t in d.frames(z["bitstream"], yuv="y210", **conv):
            assert t.dim() == 3 and np.array_equal(rows(t[None])[0], kept[poc]), poc
            got.append(poc)
        assert sorted(got) == sorted(seen)
