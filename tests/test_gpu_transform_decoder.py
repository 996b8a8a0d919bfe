"""The transform export through libhmdec (hmdec_pictures_export_transform) behind hmdec.export_transform_batch and Picture.transform:
eight HM-encoded fixture streams end to end -- all four chroma formats, PCM, scaling lists, lossless CUs, cross-component prediction --
every picture bit for bit against the model (tests/transform_ref.py) applied to a parse-only decoder's arrays."""
import ctypes as C

import numpy as np
import pytest

from libhm_amd import abi, hmdec
from tests import golden_util as gu
from tests import transform_ref as tref
from tests.test_gpu_residual_decoder import KEYS, bits

pytestmark = pytest.mark.gpu

STREAMS = ["ldp_main8_416x240", "ra_main10_208x120", "intra_main10_208x120", "ldp_pcm_main8_208x120", "ldp_sl_main10_208x120",
           "ldp_lossless_main10_208x120", "ldb_422_main10_208x120", "intra_444_ccp_main10_208x120"]
NAMES = ("y", "cb", "cr")
_models = {}


def models(name):
    """POC -> (levels planes, coefficient planes, info grid), from the arrays a parse-only decoder leaves (no device involved);
    computed once per stream"""
    if name in _models:
        return _models[name]
    z = gu.load("stream_" + name)
    out = {}
    with hmdec.Decoder(parse_only=True) as d:
        def on_output(p):
            g = p.geometry()
            n = g["num_ctbs"]
            meta = {mine: p.array(theirs).reshape(n, -1) for theirs, mine in KEYS}
            meta["slice_idx"] = p.array("slice_idx")
            seq = abi.make_seq(g["width"], g["height"], g["bd_y"], g["bd_c"], log2_ctu=g["log2_ctb"], range_ext_flags=g["range_ext"])
            seq.chroma_format = g["chroma_format"]
            slices, keep = [], []
            for i in range(p.num_slices()):
                sp, sl = p.slice_params(i)
                if bool(sp.scaling_lists):
                    sp.scaling_lists = C.pointer(sl)
                    keep.append(sl)
                slices.append(sp)
            levels = [p.array("coeff%d" % k).reshape(n, -1) for k in range(3)]
            out[p.poc] = (tref.levels_planes(seq, meta, levels), tref.coeff_planes(seq, slices, meta, levels), tref.info_grid(seq, meta),
                          1 if g["chroma_format"] == 0 else 3)
        d.decode_stream(z["bitstream"], on_output=on_output)
    _models[name] = out
    return out


@pytest.mark.parametrize("kw", [dict(threads=1), dict(threads=3), dict(threads=1, devices=[0, 0])], ids=["t1", "t3", "two_contexts"])
@pytest.mark.parametrize("name", STREAMS)
def test_every_picture_of_a_stream_matches_the_model(name, kw):
    z = gu.load("stream_" + name)
    want = models(name)
    seen = []
    with hmdec.Decoder(device=0, device_output=True, **kw) as d:
        def on_output(pic):
            lv, co, info, ncomp = want[pic.poc]
            one = pic.transform()
            assert sorted(one) == sorted(list(NAMES[:ncomp]) + ["info"])
            both = hmdec.export_transform_batch([pic, pic], "coeffs")
            for k in range(ncomp):
                assert np.array_equal(bits(one[NAMES[k]]), lv[k]), (name, pic.poc, "levels", k)
                for slot in range(2):
                    assert np.array_equal(bits(both[NAMES[k]][slot]), co[k]), (name, pic.poc, "coeffs", k, slot)
            assert np.array_equal(one["info"].cpu().numpy(), info), (name, pic.poc)
            assert np.array_equal(both["info"][1].cpu().numpy(), info), (name, pic.poc)
            seen.append((pic.poc, bool(lv[0].any()), any(not np.array_equal(a, b) for a, b in zip(lv, co))))
        d.decode_stream(z["bitstream"], on_output=on_output)
        assert d.hash_mismatches == 0
    assert len(seen) == len(want) >= 1 and any(nz for _, nz, _ in seen)
    # (a lossless stream's coefficients are its levels)
    assert any(diff for _, _, diff in seen) or "lossless" in name
