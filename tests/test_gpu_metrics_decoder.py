"""The picture metrics through libhmdec (hmdec_pictures_metrics) behind hmdec.metrics_batch and Picture.metrics: fixture streams
decoded with device output on, every picture compared on the device with planes made from the decoder's own host output plus known
noise; the records must equal the model (tests/metrics_ref.py)."""
import ctypes as C

import numpy as np
import pytest

from libhm_amd import abi, hmdec, metrics
from tests import golden_util as gu
from tests import metrics_ref as mref

pytestmark = pytest.mark.gpu

NAMES = ("y", "cb", "cr")
_host = {}


def _torch():
    import torch
    return torch


def host_pictures(name):
    """POC -> (the three planes a decoder without device output hands out, bit depths); decoded once per stream"""
    if name not in _host:
        out = {}
        with hmdec.Decoder(device=0) as d:
            def on_output(p):
                g = p.geometry()
                out[p.poc] = ([p.plane(c).astype(np.int64) for c in range(3)], (g["bd_y"], g["bd_c"]))
            d.decode_stream(gu.load("stream_" + name)["bitstream"], on_output=on_output)
        _host[name] = out
    return _host[name]


def noisy(planes, bds, poc):
    """the planes with noise of a known seed, every fourth picture left as it is"""
    if poc % 4 == 0:
        return [p.copy() for p in planes]
    rng = np.random.RandomState(1000 + poc)
    return [np.clip(p + rng.randint(-9, 10, size=p.shape), 0, (1 << bds[1 if k else 0]) - 1) for k, p in enumerate(planes)]


def tensors(stacks, bds):
    torch = _torch()
    if max(bds) <= 8:
        return [torch.from_numpy(s.astype(np.uint8)).cuda() for s in stacks]
    return [torch.from_numpy(s.astype(np.uint16).view(np.int16)).cuda() for s in stacks]


def compare(rec, want, where):
    for k in range(3):
        for f, name in enumerate(mref.FIELDS):
            got, exp = int(rec[k, f]), want[k][name]
            if name == "ssim_q32":
                assert abs(got - exp) <= mref.tolerance(want[k]["ssim_windows"]), (where, k, got, exp)
            else:
                assert got == exp, (where, k, name, got, exp)


@pytest.mark.parametrize("kw", [dict(threads=1), dict(threads=1, devices=[0, 0])], ids=["one_context", "two_contexts"])
@pytest.mark.parametrize("name", ["ldp_main8_416x240", "ra_main10_208x120"])
def test_decoded_pictures_against_noisy_originals(name, kw):
    host = host_pictures(name)
    seen = []
    with hmdec.Decoder(device=0, device_output=True, **kw) as d:
        def on_output(pic):
            planes, bds = host[pic.poc]
            refs = [noisy(planes, bds, pic.poc), noisy(planes, bds, pic.poc + 1)]
            out = hmdec.metrics_batch([pic, pic], tensors([np.stack([r[k] for r in refs]) for k in range(3)], bds))
            rec = metrics.records(out).cpu().numpy()
            for i in range(2):
                compare(rec[i], [mref.plane(planes[k], refs[i][k], bds[1 if k else 0]) for k in range(3)], (name, pic.poc, i))
            one = pic.metrics(tensors(refs[0], bds), components=(0, 2), ssim=False)
            assert int(one["y"]["sse"]) == int(rec[0, 0, 1]) and int(one["cr"]["sad"]) == int(rec[0, 2, 2])
            assert int(one["cb"]["samples"]) == 0 and int(one["y"]["ssim_windows"]) == 0
            seen.append((pic.poc, int(rec[0, 0, 3])))
        d.decode_stream(gu.load("stream_" + name)["bitstream"], on_output=on_output)
    assert sorted(p for p, _ in seen) == sorted(host)
    assert any(diff == 0 for _, diff in seen) and any(diff > 0 for _, diff in seen)


def test_pictures_as_the_reference_are_refused_with_a_message():
    torch = _torch()
    name = "ra_main10_208x120"
    done = []
    with hmdec.Decoder(device=0, device_output=True) as d:
        def on_output(pic):
            if done:
                return
            L = hmdec.lib()
            res = torch.full((24,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
            desc = abi.make_metrics_desc(abi.METRICS_REF_PICTURES)
            st = L.hmdec_pictures_metrics(pic.ctx, 1, abi.ptr_array([pic.h], 1), C.byref(desc), None, None, None, abi.addr(res.data_ptr()), 192, 1, None)
            assert st == abi.HMGPU_EUNSUPPORTED
            assert b"HMGPU_METRICS_REF_PLANES" in L.hmdec_last_error(pic.ctx)
            torch.cuda.synchronize()
            assert bool((res == 0x5A5A5A5A).all())
            done.append(pic.poc)
        d.decode_stream(gu.load("stream_" + name)["bitstream"], on_output=on_output)
    assert done
