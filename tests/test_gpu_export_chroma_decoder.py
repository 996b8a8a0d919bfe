"""The chroma stage through the decoder: hmdec_pictures_export_chroma behind chroma= of Picture.export, hmdec.export_batch and
Decoder.frames, with one device context and with two on one GPU.  The fixture's SPS signals chroma_sample_loc_type 2 (top-left),
which chroma_loc=None must pick up by itself: every result must equal libhm_amd.Context.export_batch(chroma="linear", chroma_loc=2)
on the planes the decoder put out, which tests/test_gpu_export_chroma.py holds against the numpy restatement.  The planes themselves
must be those of the stream the fixture was rewritten from: the sample location takes no part in reconstruction."""
import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, hmdec
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

STREAM, SOURCE = "export_vui_bt2020_chromaloc2_main10_208x120", "export_vui_bt2020_main10_208x120"


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

    def export(self, planes, **kw):
        pics = [self.ctx.acquire() for _ in planes]
        try:
            for h, p in zip(pics, planes):
                self.ctx.upload(h, [np.ascontiguousarray(c, np.int16) for c in p])
            out = self.ctx.export_batch(pics, "rgb", crop=self.crop, **kw)
            _torch().cuda.synchronize()
            return out
        finally:
            for h in pics:
                self.ctx.release(h)


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_decoder_takes_the_sample_location_from_the_vui(devices):
    torch = _torch()
    z, src = gu.load(STREAM), gu.load(SOURCE)
    kw = dict(threads=1, device_output=True, devices=devices)
    colour = dict(matrix=9, full_range=1)                            # what the VUI says, named for the plain context
    variants = (dict(bit_depth=10), dict(bit_depth=8, size=(60, 100), filter="bicubic", pixel="bgra"),
                dict(bit_depth=10, dtype=torch.float16, windows=True))
    planes, ref = {}, None
    try:
        with hmdec.Decoder(**kw) as d:
            pictures = []

            def on_output(p):
                nonlocal ref
                assert p.chroma_loc() == dict(present=1, top_field=2, bottom_field=2)
                planes[p.poc] = [p.plane(c) for c in range(3)]
                for c in range(3):                                   # bit-exact: the source fixture's pictures
                    assert np.array_equal(planes[p.poc][c], src["poc%02d_%d" % (p.poc, c)]), (p.poc, c)
                if ref is None:
                    ref = Reference(p)
                one = p.export(bit_depth=10, chroma="linear")
                assert torch.equal(one, ref.export([planes[p.poc]], bit_depth=10, chroma="linear", chroma_loc=2, **colour)[0])
                # chroma_loc= overrides the stream's, and the default stays the replicated export
                assert torch.equal(p.export(bit_depth=10, chroma="linear", chroma_loc=1),
                                   ref.export([planes[p.poc]], bit_depth=10, chroma="linear", chroma_loc=1, **colour)[0])
                assert torch.equal(p.export(bit_depth=10), ref.export([planes[p.poc]], bit_depth=10, **colour)[0])
                assert not torch.equal(one, p.export(bit_depth=10))
                batch = [p, p, p]
                for v in variants:
                    v = dict(v)
                    if v.pop("windows", False):
                        v.update(windows=[(2, 6, 100, 60), (6, 2, 100, 60), (108, 60, 100, 60)], flip=[False, True, True])
                    mine = hmdec.export_batch(batch, chroma="linear", **v)
                    assert torch.equal(mine, ref.export([planes[p.poc]] * 3, chroma="linear", chroma_loc=2, **colour, **v)), v.keys()
                pictures.append(p.poc)
            d.decode_stream(bytes(z["bitstream"]), on_output=on_output)
            assert d.hash_mismatches == 0 and sorted(pictures) == [0, 1]
        # Decoder.frames, picture by picture and in batches
        with hmdec.Decoder(**kw) as d:
            seen = []
            for poc, t in d.frames(z["bitstream"], bit_depth=10, chroma="linear", pixel="rgb"):
                assert torch.equal(t, ref.export([planes[poc]], bit_depth=10, chroma="linear", chroma_loc=2, pixel="rgb", **colour)[0]), poc
                seen.append(poc)
            assert sorted(seen) == [0, 1]
        with hmdec.Decoder(**kw) as d:
            seen = []
            for pocs, t in d.frames(z["bitstream"], batch=2, bit_depth=8, chroma="linear", size=(60, 104)):
                want = ref.export([planes[poc] for poc in pocs], bit_depth=8, chroma="linear", chroma_loc=2, size=(60, 104), **colour)
                assert torch.equal(t[:len(pocs)], want), pocs
                seen += pocs
            assert sorted(seen) == [0, 1]
    finally:
        if ref is not None:
            ref.ctx.close()


def test_a_stream_without_the_flag_reads_as_type_0():
    torch = _torch()
    z = gu.load(SOURCE)
    with hmdec.Decoder(threads=1, device_output=True) as d:
        for poc, t in d.frames(z["bitstream"], bit_depth=10, chroma="linear"):
            pass
    with hmdec.Decoder(threads=1, device_output=True) as d:
        def on_output(p):
            assert p.chroma_loc() == dict(present=0, top_field=0, bottom_field=0)
            assert torch.equal(p.export(bit_depth=10, chroma="linear"), p.export(bit_depth=10, chroma="linear", chroma_loc=0))
            assert not torch.equal(p.export(bit_depth=10, chroma="linear"), p.export(bit_depth=10, chroma="linear", chroma_loc=2))
        d.decode_stream(bytes(z["bitstream"]), on_output=on_output)
