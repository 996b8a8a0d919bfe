"""The walk of the motion-compensation launches (k_mc.hip, launch_mc): a call's CTU range is covered in vertical bands of BAND_W CTU
columns, band after band, and must reach every CTU of the range exactly once -- for pictures narrower than a band, as wide as one,
one column short of and beyond one, with a last band of a single column, for ranges that start in the middle of a CTU row (the parts
of a picture that 8 / n XCDs share, slices) and in both grid modes.  Every case is bit-exact parity with the C oracle through
decompress_pictures + filter_pictures; the target pictures hold a blocky picture beforehand, so a square the walk leaves out shows."""
import functools

import numpy as np
import pytest

from libhm_amd import abi
from tests import synth
from tests.test_gpu_fullsize import _oracle_chain

pytestmark = pytest.mark.gpu

BAND_W = 15                                   # kBandW of k_mc.hip
COLS = [1, BAND_W - 1, BAND_W, BAND_W + 1, 2 * BAND_W + 1]
BD = 10


@functools.lru_cache(maxsize=None)
def _planes(width, height):
    """two reference pictures and what the targets hold before the call; shared by the cases of a size, never written"""
    return synth.noise_planes(width, height, BD, 71), synth.blocky_planes(width, height, BD, 72), synth.blocky_planes(width, height, BD, 73)


def _chain_slices(oracle, p, cur, refs):
    """_oracle_chain for a picture of several slices"""
    rec = [a.copy() for a in cur]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, rec, refs)
    oracle.loop_filter_pic(p.seq, p.slices, p.meta, p.pp, rec, 3)
    prm = oracle.sao_reconstruct_params(p.seq, p.pp, p.meta, p.sao_raw)
    return oracle.sao_process(p.seq, p.slices, p.pp, p.meta, prm, rec)


def _run(oracle, width, height, log2_ctu, n=1, num_slices=1, bi=False):
    import libhm_amd
    ref0, ref1, cur = _planes(width, height)
    pics = [synth.make_picture(width, height, BD, seed=800 + 13 * i + log2_ctu, bi=bi, ref_handles=([0], [1]), mv_range=64, log2_ctu=log2_ctu,
                               num_slices=num_slices) for i in range(n)]
    if num_slices > 1:
        assert all(any(a % p.ctus_w for a, _ in p.slice_ranges) for p in pics)      # a call's range starts inside a CTU row
        want = [_chain_slices(oracle, p, cur, [ref0, ref1]) for p in pics]
    else:
        want = [_oracle_chain(oracle, p, cur, [ref0, ref1])[2] for p in pics]
    with libhm_amd.Context(abi.make_seq(width, height, BD, BD, log2_ctu=log2_ctu, max_pictures=2 + n)) as ctx:
        h0, h1 = ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        ctx.upload(h1, ref1)
        hs = [ctx.acquire() for _ in range(n)]
        for h in hs:
            ctx.upload(h, cur)
        ctx.decompress_pictures([(hs[i], pics[i].slices, pics[i].meta, pics[i].coeffs) for i in range(n)])
        ctx.filter_pictures([(hs[i], pics[i].pp, abi.sao_array_from_raw(pics[i].sao_raw)) for i in range(n)])
        for i in range(n):
            got = ctx.download(hs[i])
            for c in range(3):
                assert np.array_equal(got[c], want[i][c]), "picture %d comp %d" % (i, c)


@pytest.mark.parametrize("log2_ctu", [6, 4])
@pytest.mark.parametrize("cols", COLS)
def test_band_walk_covers_pictures_of_every_width(oracle, cols, log2_ctu):
    """one picture on eight XCDs (eight ranges, most of them starting inside a CTU row), three CTU rows high"""
    _run(oracle, cols << log2_ctu, 3 << log2_ctu, log2_ctu)


def test_band_walk_with_a_partial_last_ctu_column(oracle):
    """976 x 176: 15.25 x 2.75 CTUs of 64 samples -- the last band is one column of 16 samples"""
    _run(oracle, 976, 176, 6)


@pytest.mark.parametrize("n", [2, 4, 8, 3])
def test_band_walk_in_batches(oracle, n):
    """n = 2, 4, 8: 8 / n XCDs per picture (grid mode 1; n = 1 is every other case of this file); n = 3: one grid column per picture (mode 0)"""
    _run(oracle, (BAND_W + 1) * 64, 128, 6, n=n)


def test_band_walk_of_slices_that_start_inside_a_row(oracle):
    _run(oracle, (2 * BAND_W + 1) * 64, 192, 6, num_slices=3)


def test_band_walk_of_a_b_picture(oracle):
    _run(oracle, (BAND_W + 1) * 64, 192, 6, bi=True)
