"""The affine warp export through the decoder: hmdec_pictures_export_warp behind warp= of Picture.export, hmdec.export_batch and
Decoder.frames, with one device context and with two on one GPU.  Every result must equal tests/export_warp_ref.py applied to the
plain export of the same picture (its conformance crop, or the slot's window), bit for bit."""
import numpy as np
import pytest

from libhm_amd import export, hmdec
from tests import export_warp_ref as wref
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

STREAM = "export_vui_bt2020_main10_208x120"
SIZE = (75, 131)                                     # (height, width): odd, partial tiles


def _torch():
    import torch
    return torch


def ints(t):
    return t.cpu().numpy().astype(np.int64) & 0xffff


def maps_for(n, src, seed):
    torch = _torch()
    return export.random_affine(n, SIZE, src, degrees=30, translate=(0.05, 0.05), scale=(0.7, 1.6), shear=(-8, 8),
                                generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_pictures_and_batches_through_the_decoder(devices):
    z = gu.load(STREAM)
    kw = dict(threads=1, device_output=True, devices=devices)
    S, seen = {}, []
    wins = [(2, 6, 100, 60), (108, 60, 100, 60), (0, 0, 208, 120)]
    with hmdec.Decoder(**kw) as d:
        def on_output(p):
            S[p.poc] = ints(p.export(bit_depth=10))
            src = S[p.poc].shape[1:]
            m = maps_for(3, src, 10 + p.poc)
            for filt, border in (("bilinear", "edge"), ("nearest", "fill")):
                one = p.export(bit_depth=10, warp=m[0], size=SIZE, filter=filt, border=border, fill=(1, 2, 1000))
                assert np.array_equal(ints(one), wref.warp(S[p.poc], m[0], SIZE, filt, border, (1, 2, 1000))), (p.poc, filt)
            # the orientation helper: a quarter turn of the whole picture
            om, osize = export.orientation_map(1, False, False, src)
            assert np.array_equal(ints(p.export(bit_depth=10, warp=om, size=osize)), np.rot90(S[p.poc], 1, (1, 2)))
            # a batch with windows of different sizes, a mirror, packed pixels at 8 bits
            s8 = [ints(p.export(bit_depth=8, crop=None)[:, y:y + h, x:x + w]) for x, y, w, h in wins]
            got = hmdec.export_batch([p, p, p], bit_depth=8, crop=None, warp=m, size=SIZE, windows=wins, flip=[False, True, False], pixel="bgr",
                                     border="fill", fill=(9, 8, 7))
            for i in range(3):
                want = wref.warp(s8[i], m[i], SIZE, "bilinear", "fill", (9, 8, 7))
                want = want[:, :, ::-1] if i == 1 else want
                assert np.array_equal(ints(got[i]), want[::-1].transpose(1, 2, 0)), (p.poc, i)
            seen.append(p.poc)
        d.decode_stream(bytes(z["bitstream"]), on_output=on_output)
        assert d.hash_mismatches == 0 and sorted(seen) == [0, 1]
    src = S[0].shape[1:]
    # Decoder.frames in batches: fn(n) names the maps of each call's pictures
    with hmdec.Decoder(**kw) as d:
        calls, seen = [], []

        def fn(n):
            calls.append(maps_for(n, src, 50 + len(calls)))
            return calls[-1]
        for pocs, t in d.frames(z["bitstream"], batch=4, bit_depth=10, warp=fn, size=SIZE, border="fill", fill=(0, 1023, 0)):
            assert t.shape == (len(pocs), 3) + SIZE
            seen += pocs
            maps = [m for c in calls for m in c]
            for i, poc in enumerate(pocs):
                assert np.array_equal(ints(t[i]), wref.warp(S[poc], maps[i], SIZE, "bilinear", "fill", (0, 1023, 0))), poc
        assert sorted(seen) == [0, 1] and sum(len(c) for c in calls) == 2
    # picture by picture with one map
    with hmdec.Decoder(**kw) as d:
        m = maps_for(1, src, 99)[0]
        for poc, t in d.frames(z["bitstream"], bit_depth=10, warp=m, size=SIZE, filter="nearest"):
            assert np.array_equal(ints(t), wref.warp(S[poc], m, SIZE, "nearest"))
    with hmdec.Decoder(**kw) as d:                   # ... and with the function of the batched form: fn(1) per picture
        given = []

        def one(n):
            given.append(maps_for(n, src, 70 + len(given)))
            return given[-1]
        for k, (poc, t) in enumerate(d.frames(z["bitstream"], bit_depth=10, warp=one, size=SIZE)):
            assert len(given) == k + 1 and np.array_equal(ints(t), wref.warp(S[poc], given[k][0], SIZE))
        assert len(given) == 2
    # the dense side-information forms cannot be aligned with a warp
    for side in (dict(motion=dict(form="dense", dtype=_torch().float32)), dict(residual=dict(form="dense"))):
        with hmdec.Decoder(**kw) as d:
            with pytest.raises(ValueError):
                next(iter(d.frames(z["bitstream"], batch=2, warp=lambda n: [wref.IDENTITY] * n, size=SIZE, **side)))
    with hmdec.Decoder(**kw) as d:
        with pytest.raises(ValueError):
            next(iter(d.frames(z["bitstream"], bit_depth=10, warp=wref.IDENTITY, size=SIZE, filter="bicubic")))
