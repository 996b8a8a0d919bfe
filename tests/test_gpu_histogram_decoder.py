"""The picture histograms through libhmdec (hmdec_pictures_histogram) behind hmdec.histogram_batch and Picture.histogram: fixture
streams decoded with device output on, every picture's counts and records against the model (tests/histogram_ref.py) on the planes a
decoder without device output hands out, cropped to the conformance window -- maxRGB with the matrix and range the VUI resolves to."""
import ctypes as C

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, export, hmdec, histogram
from tests import golden_util as gu
from tests import histogram_ref as href
from tests.test_gpu_metrics_decoder import host_pictures

pytestmark = pytest.mark.gpu

ALL = ("y", "cb", "cr", "maxrgb")


def _torch():
    import torch
    return torch


def compare(out, i, want, where, with_hist=True):
    """picture i of a batch result (i None: a result without the batch dimension) against the model's four channels"""
    for c, name in enumerate(href.NAMES):
        ch = out[name]
        for f in href.FIELDS:
            got = int(ch[f] if i is None else ch[f][i])
            assert got == want[c][f], (where, name, f, got, want[c][f])
        assert ("hist" in ch) == (with_hist and want[c]["samples"] > 0), (where, name)
        if "hist" in ch:
            h = (ch["hist"] if i is None else ch["hist"][i]).cpu().numpy().astype(np.int64)
            assert np.array_equal(h, want[c]["hist"]), (where, name)


@pytest.mark.parametrize("kw", [dict(threads=1), dict(threads=1, devices=[0, 0])], ids=["one_context", "two_contexts"])
@pytest.mark.parametrize("name", ["ra_main10_208x120", "ldb_422_main10_208x120"])
def test_decoded_pictures_against_the_model_on_the_decoders_own_planes(name, kw):
    host = host_pictures(name)
    seen, kept = [], []
    with hmdec.Decoder(device=0, device_output=True, **kw) as d:
        def on_output(pic):
            planes, bds = host[pic.poc]
            g, col, crop = pic.geometry(), pic.colour(), pic.conformance_window()
            fmt = g["chroma_format"]
            seq = abi.make_seq(g["width"], g["height"], g["bd_y"], g["bd_c"], log2_ctu=g["log2_ctb"])
            seq.chroma_format = fmt
            matrix, full_range = export.resolve_colour(None, None, col["matrix"], col["full_range"])
            coef = list(libhm_amd.histogram_plan(seq, ("maxrgb",), crop=crop, matrix=matrix, full_range=full_range).coef)
            want = href.picture(planes, fmt, bds, (0, 1, 2, 3), crop=crop, coef=coef)
            # the pictures fetched since the last push: this one twice and, where the decoder still holds it, the one before
            batch = [pic, pic]
            out = hmdec.histogram_batch(batch, channels=ALL)
            for i in range(2):
                compare(out, i, want, (name, pic.poc, i))
            assert histogram.records(out).shape == (2, 4, 8)
            one = pic.histogram(channels=("y", "maxrgb"), bins=256, histogram=True)
            red = href.picture(planes, fmt, bds, (0, 3), log2_bins=8, crop=crop, coef=coef)
            compare(one, None, red, (name, pic.poc, "one"))
            rec_only = pic.histogram(channels=ALL, histogram=False)
            compare(rec_only, None, want, (name, pic.poc, "records"), with_hist=False)
            # a matrix of the caller's own overrides the VUI's
            other = hmdec.histogram_batch([pic], channels=("maxrgb",), matrix=9, full_range=1, rgb_bit_depth=8)
            coef9 = list(libhm_amd.histogram_plan(seq, ("maxrgb",), crop=crop, matrix=9, full_range=1, rgb_bit_depth=8).coef)
            compare(other, 0, href.picture(planes, fmt, bds, (3,), crop=crop, coef=coef9, rgb_bit_depth=8), (name, pic.poc, "bt2020"))
            seen.append(pic.poc)
            kept.append(int(out["y"]["sum"][0]))
        d.decode_stream(gu.load("stream_" + name)["bitstream"], on_output=on_output)
    assert sorted(seen) == sorted(host)
    assert len(set(kept)) > 1                                            # the pictures of a stream differ


def test_a_decoder_without_device_output_is_refused_with_a_message():
    torch = _torch()
    name = "ra_main10_208x120"
    done = []
    with hmdec.Decoder(device=0) as d:
        def on_output(pic):
            if done:
                return
            L = hmdec.lib()
            rec = torch.full((32,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
            desc = abi.make_histogram_desc(7, 0, 0)
            st = L.hmdec_pictures_histogram(pic.ctx, 1, abi.ptr_array([pic.h], 1), C.byref(desc), None, None, abi.addr(rec.data_ptr()), 256, 1, None)
            assert st == abi.HMGPU_EINVAL
            assert b"hmdec_set_device_output" in L.hmdec_last_error(pic.ctx)
            with pytest.raises(libhm_amd.HmgpuError, match="hmdec_set_device_output"):
                pic.histogram()
            torch.cuda.synchronize()
            assert bool((rec == 0x5A5A5A5A).all())
            done.append(pic.poc)
        d.decode_stream(gu.load("stream_" + name)["bitstream"], on_output=on_output)
    assert done
