"""The picture metric maps through libhmdec (hmdec_pictures_metrics_map) behind hmdec.metrics_map_batch and Picture.metrics_map: a fixture
stream decoded with device output on, on one context and on two, every picture compared on the device with planes made from the
decoder's own host output plus noise of a known seed in known blocks; the maps must equal the model (tests/metrics_map_ref.py), and
metrics.mismatch_blocks must name exactly the blocks that hold the noise."""
import ctypes as C

import numpy as np
import pytest

from libhm_amd import abi, hmdec, metrics
from tests import golden_util as gu
from tests import metrics_map_ref as mmap
from tests.test_gpu_metrics_decoder import host_pictures, tensors
from tests.test_gpu_metrics_map import compare

pytestmark = pytest.mark.gpu

NAMES = ("y", "cb", "cr")
B = 16


def noisy_blocks(planes, bds, poc, fmt, block):
    """the planes with noise of a known seed inside a few blocks of the luma grid (every fourth picture left as it is), and the set of
    (by, bx) that hold it.  Every noisy sample differs: the noise is 1 .. 9 away from the sample, towards the middle of the range"""
    out = [p.copy() for p in planes]
    if poc % 4 == 0:
        return out, set()
    rng = np.random.RandomState(1000 + poc)
    h, w = planes[0].shape
    nbx, nby = mmap.grid(w, h, block)
    hit = set((int(rng.randint(nby)), int(rng.randint(nbx))) for _ in range(5))
    for by, bx in hit:
        for k in range(3):
            bw, bh = mmap.block_size(fmt, block, k)
            cell = out[k][by * bh:(by + 1) * bh, bx * bw:(bx + 1) * bw]
            step = rng.randint(1, 10, size=cell.shape)
            cell += np.where(cell < (1 << (bds[1 if k else 0] - 1)), step, -step)
    return out, hit


@pytest.mark.parametrize("kw", [dict(threads=1), dict(threads=1, devices=[0, 0])], ids=["one_context", "two_contexts"])
def test_decoded_pictures_against_noisy_originals(kw):
    name = "ra_main10_208x120"
    host = host_pictures(name)
    seen = []
    with hmdec.Decoder(device=0, device_output=True, **kw) as d:
        def on_output(pic):
            planes, bds = host[pic.poc]
            made = [noisy_blocks(planes, bds, pic.poc, 1, B), noisy_blocks(planes, bds, pic.poc + 1, 1, B)]
            refs = [m[0] for m in made]
            out = hmdec.metrics_map_batch([pic, pic], tensors([np.stack([r[k] for r in refs]) for k in range(3)], bds), block=B)
            got = metrics.maps(out).cpu().numpy()
            want = np.stack([mmap.picture(planes, refs[i], 1, bds, B) for i in range(2)])
            compare(got, want, (pic.poc,))
            for i in range(2):
                for k in range(3):
                    idx = metrics.mismatch_blocks(out[NAMES[k]]).cpu().numpy()
                    assert set((int(y), int(x)) for j, y, x in idx if j == i) == made[i][1], (pic.poc, i, k)
            one = pic.metrics_map(tensors(refs[0], bds), block=64, components=(0, 2), ssim=False)
            assert sorted(one["y"]) == ["differing", "max_abs", "sad", "sse"] and one["y"]["sse"].shape == (2, 4)
            assert int(one["y"]["sse"].sum()) == int(got[0, 0, 0].sum()) and int(one["cr"]["sad"].sum()) == int(got[0, 2, 1].sum())
            assert not bool(one["cb"]["sse"].any())
            seen.append((pic.poc, len(made[0][1])))
        d.decode_stream(gu.load("stream_" + name)["bitstream"], on_output=on_output)
    assert sorted(p for p, _ in seen) == sorted(host)
    assert any(k == 0 for _, k in seen) and any(k > 0 for _, k in seen)


def test_pictures_as_the_reference_are_refused_with_a_message():
    import torch
    done = []
    with hmdec.Decoder(device=0, device_output=True) as d:
        def on_output(pic):
            if done:
                return
            L = hmdec.lib()
            buf = torch.full((3, 6, 8, 13), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
            desc, md = abi.make_metrics_desc(abi.METRICS_REF_PICTURES), abi.make_metrics_map_desc(B)
            maps = abi.ptr_array([buf[k].data_ptr() for k in range(3)])
            st = L.hmdec_pictures_metrics_map(pic.ctx, 1, abi.ptr_array([pic.h], 1), C.byref(desc), C.byref(md), None, None, None, maps,
                                              abi.i64_array([13 * 8] * 3), abi.i64_array([8 * 13 * 8] * 3), abi.i64_array([6 * 8 * 13 * 8] * 3), 1, None)
            assert st == abi.HMGPU_EUNSUPPORTED
            assert b"HMGPU_METRICS_REF_PLANES" in L.hmdec_last_error(pic.ctx)
            torch.cuda.synchronize()
            assert bool((buf == 0x5A5A5A5A).all())
            done.append(pic.poc)
        d.decode_stream(gu.load("stream_ra_main10_208x120")["bitstream"], on_output=on_output)
    assert done
