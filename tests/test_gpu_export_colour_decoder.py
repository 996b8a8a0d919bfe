"""The colour stage through the decoder: hmdec_colour_lut_create / hmdec_pictures_export_colour behind Decoder.colour_lut and lut= of
hmdec.export_batch, Picture.export and Decoder.frames, with one device context and with two on one GPU (the LUT is created in each
context when an export first needs it there).  Every result must equal libhm_amd.Context.export_batch(lut=) on the planes the decoder
put out, which tests/test_gpu_export_colour.py holds against the numpy restatement."""
import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, hmdec
from tests import export_batch_ref as bref
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

STREAM = "lite_ra_notmvp_main8_208x120"
COLOUR = dict(layout="rgb", matrix=1, full_range=0)


def _torch():
    import torch
    return torch


def fetched(dec, nals):
    """the pictures put out after each push"""
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


def tables(depth, size, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1 << depth, (size, size, size, 3)).astype(np.uint16), rng.integers(0, 65536, (3, 1 << depth)).astype(np.uint16))


class Reference:
    """a plain context of the stream's sequence that takes the decoder's planes"""

    def __init__(self, pic, lattice, shaper, depth):
        g = pic.geometry()
        self.seq = abi.make_seq(g["width"], g["height"], g["bd_y"], g["bd_c"], log2_ctu=g["log2_ctb"], max_pictures=8)
        self.seq.chroma_format = g["chroma_format"]
        self.crop = pic.conformance_window()
        self.ctx = libhm_amd.Context(self.seq)
        self.lut = self.ctx.colour_lut(lattice, shaper, depth)

    def export(self, planes, **kw):
        pics = [self.ctx.acquire() for _ in planes]
        try:
            for h, p in zip(pics, planes):
                self.ctx.upload(h, [np.ascontiguousarray(c, np.int16) for c in p])
            out = self.ctx.export_batch(pics, crop=self.crop, lut=self.lut, **kw)
            _torch().cuda.synchronize()
            return out
        finally:
            for h in pics:
                self.ctx.release(h)

    def close(self):
        self.ctx.close()


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_decoder(devices):
    torch = _torch()
    z = gu.load(STREAM)
    frames = int(z["geom"][2])
    nals = hmdec.split_nal_units(z["bitstream"])
    lattice, shaper = tables(8, 17, 5)
    kw = dict(threads=1, device_output=True, devices=devices)
    variants = (dict(), dict(size=(30, 44), pixel="bgra", alpha=9),
                dict(dtype=torch.float16, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD, memory_format=torch.channels_last))
    planes, ref, total = {}, None, 0
    try:
        # hmdec.export_batch and Picture.export: the pictures fetched after one push, the first of them twice
        with hmdec.Decoder(**kw) as d:
            lut = d.colour_lut(lattice, shaper, 8)
            for got in fetched(d, nals):
                pictures = (got + got[:1])[:4]
                xywh = [(2 * ((3 * i) % 7), 2 * (i % 5), 94, 60) for i in range(len(pictures))]
                flips = [i % 2 == 0 for i in range(len(pictures))]
                mine = [hmdec.export_batch(pictures, windows=xywh, flip=flips, lut=lut, **COLOUR, **v) for v in variants]
                one = got[0].export(lut=lut, **COLOUR)
                for p in got:
                    planes[p.poc] = [p.plane(c) for c in range(3)]
                if ref is None:
                    ref = Reference(got[0], lattice, shaper, 8)
                own = [planes[p.poc] for p in pictures]
                for v, t in zip(variants, mine):
                    assert torch.equal(t, ref.export(own, windows=xywh, flip=flips, **COLOUR, **v)), (devices, v.keys(), [p.poc for p in pictures])
                assert torch.equal(one, ref.export(own[:1], **COLOUR)[0])
                total += len(got)
            # the stream says nothing about its colours: lut="sdr" has no source to start from
            with pytest.raises(ValueError):
                hmdec.export_batch(pictures, lut="sdr", **COLOUR)
            # a handle the decoder does not know, and a LUT of another depth
            with pytest.raises(libhm_amd.HmgpuError) as e:
                hmdec.export_batch(pictures, lut=lut.handle + 100, **COLOUR)
            assert e.value.status == abi.HMGPU_EINVAL
            with d.colour_lut(None, np.zeros((3, 1024), np.uint16), 10) as deep:
                with pytest.raises(libhm_amd.HmgpuError) as e:
                    hmdec.export_batch(pictures, lut=deep, **COLOUR)
                assert e.value.status == abi.HMGPU_EINVAL
            lut.close()
            with pytest.raises(libhm_amd.HmgpuError) as e:
                hmdec.export_batch(pictures, lut=lut, **COLOUR)
            assert d.download_bytes > 0                              # (only the planes this test asked for)
        assert total == frames and len(planes) == frames
        # Decoder.frames, picture by picture and in batches of 4
        with hmdec.Decoder(**kw) as d, d.colour_lut(lattice, shaper, 8) as lut:
            seen = []
            for poc, t in d.frames(z["bitstream"], lut=lut, pixel="rgb", **COLOUR):
                assert torch.equal(t, ref.export([planes[poc]], pixel="rgb", **COLOUR)[0]), poc
                seen.append(poc)
            assert sorted(seen) == sorted(planes) and d.download_bytes == 0
        with hmdec.Decoder(**kw) as d, d.colour_lut(lattice, shaper, 8) as lut:
            seen = []
            for pocs, t in d.frames(z["bitstream"], batch=4, lut=lut, size=(60, 104), filter="bicubic", **COLOUR):
                want = ref.export([planes[poc] for poc in pocs], size=(60, 104), filter="bicubic", **COLOUR)
                assert torch.equal(t[:len(pocs)], want), pocs
                seen += pocs
            assert sorted(seen) == sorted(planes) and d.download_bytes == 0
    finally:
        if ref is not None:
            ref.close()
