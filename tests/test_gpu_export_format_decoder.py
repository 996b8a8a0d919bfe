"""The format export through the decoder: hmdec_pictures_export_format behind chroma_format= of Picture.export, hmdec.export_batch
and Decoder.frames, with one device context and with two on one GPU.  The first fixture's SPS signals chroma_sample_loc_type 2,
which chroma_loc=None must pick up by itself: every result must equal libhm_amd.Context.export_batch(chroma_format="444",
chroma="linear", chroma_loc=2) on the planes the decoder put out, which tests/test_gpu_export_format.py holds against the numpy
model.  The second is a 4:4:4 stream exported as NV12, held against the model directly."""
import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, hmdec
from tests import export_format_ref as fref
from tests import export_ref as ref
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

STREAM, STREAM444 = "export_vui_bt2020_chromaloc2_main10_208x120", "stream_ldb_444_ccp_main8_208x120"


def _torch():
    import torch
    return torch


class Reference:
    """a plain context of the stream's sequence that takes the decoder's planes"""

    def __init__(self, pic):
        g = pic.geometry()
        self.seq = abi.make_seq(g["width"], g["height"], g["bd_y"], g["bd_c"], log2_ctu=g["log2_ctb"], max_pictures=8)
        self.seq.chroma_format = g["chroma_format"]
        self.crop = pic.conformance_window()
        self.ctx = libhm_amd.Context(self.seq)

    def export(self, planes, layout="planar", **kw):
        pics = [self.ctx.acquire() for _ in planes]
        try:
            for h, p in zip(pics, planes):
                self.ctx.upload(h, [np.ascontiguousarray(c, np.int16) for c in p])
            out = self.ctx.export_batch(pics, layout, crop=self.crop, **kw)
            _torch().cuda.synchronize()
            return out
        finally:
            for h in pics:
                self.ctx.release(h)


def equal(a, b):
    torch = _torch()
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(equal(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_decoder_takes_the_sample_location_from_the_vui(devices):
    torch = _torch()
    z = gu.load(STREAM)
    kw = dict(threads=1, device_output=True, devices=devices)
    lin = dict(chroma_format="444", chroma="linear")
    planes, ref_ = {}, None
    try:
        with hmdec.Decoder(**kw) as d:
            pictures = []

            def on_output(p):
                nonlocal ref_
                assert p.chroma_loc()["top_field"] == 2
                planes[p.poc] = [p.plane(c) for c in range(3)]
                if ref_ is None:
                    ref_ = Reference(p)
                one = p.export("planar", 10, **lin)
                want = ref_.export([planes[p.poc]], bit_depth=10, chroma_loc=2, **lin)[0]
                assert one.dim() == 3 and one.shape[0] == 3 and equal(one, want)
                # chroma_loc= overrides the stream's; the types differ; chroma_format None stays the existing export
                assert equal(p.export("planar", 10, chroma_loc=1, **lin), ref_.export([planes[p.poc]], bit_depth=10, chroma_loc=1, **lin)[0])
                assert not equal(one, p.export("planar", 10, chroma_loc=0, **lin))
                assert equal(p.export("planar", 10), tuple(t[0] for t in ref_.export([planes[p.poc]], bit_depth=10)))
                batch = [p, p, p]
                for v in (dict(bit_depth=10), dict(bit_depth=8, size=(60, 100), filter="bicubic"),
                          dict(bit_depth=10, dtype=torch.float16, windows=[(2, 6, 100, 60), (6, 2, 100, 60), (108, 60, 100, 60)], flip=[False, True, True])):
                    mine = hmdec.export_batch(batch, "planar", **lin, **v)
                    assert mine.dim() == 4 and equal(mine, ref_.export([planes[p.poc]] * 3, chroma_loc=2, **lin, **v)), v.keys()
                # 4:2:2 in pairs (NV16) from the same pictures
                mine = hmdec.export_batch(batch, "semiplanar", 10, chroma_format="422", chroma="linear")
                assert equal(mine, ref_.export([planes[p.poc]] * 3, "semiplanar", bit_depth=10, chroma_format="422", chroma="linear", chroma_loc=2))
                pictures.append(p.poc)
            d.decode_stream(bytes(z["bitstream"]), on_output=on_output)
            assert d.hash_mismatches == 0 and sorted(pictures) == [0, 1]
        with hmdec.Decoder(**kw) as d:
            seen = []
            for pocs, t in d.frames(z["bitstream"], batch=3, layout="planar", bit_depth=10, chroma_format="444", chroma="linear"):
                want = ref_.export([planes[poc] for poc in pocs], bit_depth=10, chroma_loc=2, **lin)
                assert t.dim() == 4 and t.shape[1] == 3 and equal(t[:len(pocs)], want), pocs      # (the last item: its filled slots)
                seen += pocs
            assert sorted(seen) == [0, 1]
        with hmdec.Decoder(**kw) as d:
            seen = []
            for poc, t in d.frames(z["bitstream"], layout="planar", bit_depth=10, chroma_format="444", chroma="linear"):
                assert equal(t, ref_.export([planes[poc]], bit_depth=10, chroma_loc=2, **lin)[0]), poc
                seen.append(poc)
            assert sorted(seen) == [0, 1]
    finally:
        if ref_ is not None:
            ref_.ctx.close()


@pytest.mark.parametrize("down", ["drop", "linear"])
def test_a_444_stream_as_nv12_is_the_model(down):
    z = gu.load(STREAM444)
    seen = []
    with hmdec.Decoder(threads=1, device_output=True) as d:
        def on_output(p):
            g = p.geometry()
            assert g["chroma_format"] == 3
            planes = [p.plane(c) for c in range(3)]
            crop = p.conformance_window()
            y, c = p.export("nv12", 8, chroma_format="420", chroma_down=down)
            model = fref.convert_planes(planes, 3, 1, down=abi.DOWN_FILTERS[down], loc=p.chroma_loc()["top_field"])
            want = ref.export_yuv(model, 1, (g["bd_y"], g["bd_c"]), (8, 8), ref.SEMIPLANAR, tuple(crop))
            assert np.array_equal(y.cpu().numpy(), want[0]) and np.array_equal(c.cpu().numpy(), want[1]), p.poc
            seen.append(p.poc)
        d.decode_stream(bytes(z["bitstream"]), on_output=on_output)
        assert d.hash_mismatches == 0
    assert len(seen) >= 2
