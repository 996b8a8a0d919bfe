"""The residual export through libhmdec (hmdec_pictures_export_residual) behind hmdec.export_residual_batch, Picture.residual and
Decoder.frames(residual=): four HM-encoded fixture streams end to end, every picture bit for bit against the model
(tests/residual_ref.py) applied to the parser's own arrays."""
import ctypes as C

import numpy as np
import pytest

from libhm_amd import abi, hmdec
from tests import golden_util as gu
from tests import residual_ref as rref

pytestmark = pytest.mark.gpu

STREAMS = ["ldp_main8_416x240", "ra_main10_208x120", "intra_main10_208x120", "ldp_pcm_main8_208x120"]
KEYS = [("depth", "depth"), ("part_size", "part_size"), ("pred_mode", "pred_mode"), ("qp", "qp"), ("tr_idx", "tr_idx"),
        ("cbf0", "cbf_y"), ("cbf1", "cbf_u"), ("cbf2", "cbf_v"), ("ts0", "ts_y"), ("ts1", "ts_u"), ("ts2", "ts_v"),
        ("intra_dir0", "intra_dir_l"), ("intra_dir1", "intra_dir_c"), ("bypass", "bypass"), ("ipcm", "ipcm")]
_models = {}


def _torch():
    import torch
    return torch


def bits(t):
    torch = _torch()
    if t.dtype == torch.int16:
        return t.cpu().numpy()
    view = {2: torch.int16, 4: torch.int32}[t.element_size()]
    return t.contiguous().view(view).cpu().numpy().view({2: np.uint16, 4: np.uint32}[t.element_size()])


def models(name):
    """POC -> the model's planes, from the arrays a parse-only decoder leaves (no device involved); computed once per stream"""
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
            out[p.poc] = rref.planes(seq, slices, meta, levels)
        d.decode_stream(z["bitstream"], on_output=on_output)
    _models[name] = out
    return out


@pytest.mark.parametrize("kw", [dict(threads=1), dict(threads=3), dict(threads=1, devices=[0, 0])], ids=["t1", "t3", "two_contexts"])
@pytest.mark.parametrize("name", STREAMS)
def test_frames_yield_the_residual_of_every_picture(name, kw):
    z = gu.load("stream_" + name)
    want = models(name)
    seen = []
    with hmdec.Decoder(device=0, device_output=True, **kw) as d:
        for pocs, rgb, res in d.frames(z["bitstream"], batch=3, residual=True):
            assert sorted(res) == ["cb", "cr", "y"] and rgb.shape[0] == len(pocs)
            for slot, poc in enumerate(pocs):
                for k, key in enumerate(("y", "cb", "cr")):
                    assert res[key].shape[0] == len(pocs)
                    assert np.array_equal(bits(res[key][slot]), want[poc][k]), (name, poc, key)
                seen.append((poc, bool(want[poc][0].any())))
        assert d.hash_mismatches == 0
    assert len(seen) == len(want) >= 1 and any(nz for _, nz in seen)


def test_single_picture_calls_and_the_batch_call_agree():
    name = "ra_main10_208x120"
    z = gu.load("stream_" + name)
    want = models(name)
    torch = _torch()
    with hmdec.Decoder(device=0, device_output=True) as d:
        def on_output(pic):
            got = hmdec.export_residual_batch([pic, pic], components=(0, 2))
            assert sorted(got) == ["cr", "y"]
            one = pic.residual()
            for bad in (dict(flip=True), dict(window=(0, 0, 96, 64)), dict(size=(32, 48))):      # they belong to form="dense"
                with pytest.raises(ValueError):
                    pic.residual(**bad)
            for k, key in enumerate(("y", "cb", "cr")):
                assert np.array_equal(bits(one[key]), want[pic.poc][k]), (pic.poc, key)
            assert torch.equal(got["y"][1], one["y"]) and torch.equal(got["cr"][0], one["cr"])
            dn = pic.residual("dense", size=(32, 48), window=(36, 20, 96, 64), flip=True, dtype=torch.float16, scale=(0.5, 0.25, 0.125))
            assert np.array_equal(bits(dn["residual"]), rref.dense(want[pic.poc], (36, 20, 96, 64), True, (32, 48), dtype="float16", scale=(0.5, 0.25, 0.125)))
        d.decode_stream(z["bitstream"], on_output=on_output)


def test_pixels_and_motion_are_unchanged_with_residual_on():
    """Decoder.frames(batch=4, windows=fn, size=, motion=, residual=): each call's windows and flips apply to pixels, motion and the
    dense residual alike; the pixels and the motion are those of the same run without residual="""
    torch = _torch()
    name = "ra_main10_208x120"
    z = gu.load("stream_" + name)
    want = models(name)

    def run(**extra):
        rng = np.random.RandomState(5)
        calls = []

        def fn(n):
            wins = [(int(2 * rng.randint(0, 40)), int(2 * rng.randint(0, 20)), 96, 64) for _ in range(n)]
            flips = [bool(rng.randint(0, 2)) for _ in range(n)]
            calls.append((wins, flips))
            return wins, flips
        with hmdec.Decoder(device=0, device_output=True) as d:
            items = [(list(it[0]), it[1].clone()) + tuple({k: t.clone() for k, t in side.items()} for side in it[2:])
                     for it in d.frames(z["bitstream"], batch=4, windows=fn, size=(32, 48), filter="nearest", motion=dict(form="dense", dtype=torch.float16),
                                        **extra)]
        return items, [wf for wins, flips in calls for wf in zip(wins, flips)]

    plain, w0 = run()
    both, w1 = run(residual=dict(form="dense", dtype=torch.float32, scale=(0.5, 0.5, 0.5)))
    assert w0 == w1 and len(plain) == len(both)
    i = 0
    for a, b in zip(plain, both):
        assert len(a) == 3 and len(b) == 4 and a[0] == b[0]
        assert torch.equal(a[1], b[1])
        assert sorted(a[2]) == sorted(b[2]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
        assert tuple(b[3]["residual"].shape) == (len(b[0]), 3, 32, 48)
        for slot, poc in enumerate(b[0]):
            win, flip = w1[i]
            i += 1
            assert np.array_equal(bits(b[3]["residual"][slot]), rref.dense(want[poc], win, flip, (32, 48), dtype="float32", scale=(0.5, 0.5, 0.5))), poc
    assert i == len(w1)
    # the checks of the residual dict come before anything is decoded
    with hmdec.Decoder(parse_only=True) as d:
        for bad in (dict(form="dense", windows=[(0, 0, 96, 64)]), dict(flip=[True]), dict(out={}), dict(form="nope")):
            with pytest.raises(ValueError):
                next(d.frames(z["bitstream"], batch=4, size=(32, 48), filter="nearest", residual=bad))
        with pytest.raises(ValueError):
            next(d.frames(z["bitstream"], residual=True))
