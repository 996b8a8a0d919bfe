"""Deblocking decisions on pictures whose motion lets them fall both ways: synthetic pictures (tests/synth.py) with coherent motion
(mv_coherence), two references per list in swapped order and smooth references (smooth_planes), so that between inter PUs boundary strength 0,
1 by motion and 1 by references all occur in hundreds of edge units and the luma filter, which finds d >= beta nearly everywhere on pictures
predicted from noise, changes several per cent of the samples.  Bit-exact against the C oracle at every stage."""
import numpy as np
import pytest

from tests import bs_ref
from tests import synth

pytestmark = pytest.mark.gpu

W, H = 520, 328
STAGES = ("reconstruction", "deblocking (stages=3)", "SAO (stages=4)", "all stages in one call")


def motion_picture(fmt, bi):
    """(picture, reference 0, reference 1, start contents): P or B, 10 % intra CUs, few coded blocks, motion that spreads over neighbouring PUs"""
    p = synth.make_picture(W, H, 10, seed=0xC0 + 2 * fmt + int(bi), bi=bi, intra_frac=0.1, cbf_prob=0.2, mv_coherence=0.7, num_refs=2,
                           l1_refs=2 if bi else 1, ref_handles=([0, 1], [1, 0]), chroma_format=fmt)
    return p, synth.smooth_planes(W, H, 10, 71 + fmt, fmt), synth.smooth_planes(W, H, 10, 81 + fmt, fmt), synth.blocky_planes(W, H, 10, 91, fmt)


def oracle_chain(oracle, p, cur, refs):
    rec = [a.copy() for a in cur]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, rec, refs)
    dbk = [a.copy() for a in rec]
    oracle.loop_filter_pic(p.seq, p.slices, p.meta, p.pp, dbk, 3)
    prm = oracle.sao_reconstruct_params(p.seq, p.pp, p.meta, p.sao_raw)
    return rec, dbk, oracle.sao_process(p.seq, p.slices, p.pp, p.meta, prm, dbk)


def check_content(oracle, p, want, bi):
    """the picture holds what the test is about (conditions on the input, counted with the oracle's boundary strengths)"""
    counts = bs_ref.motion_units(p, *oracle.boundary_strengths(p.seq, p.slices, p.meta, p.pp))
    changed = float((want[0][0] != want[1][0]).mean())
    print("inter PU edge units: %s; deblocking changes %.1f %% of luma" % (counts, 100 * changed))
    for k in ("Bs 0", "Bs 1 by motion", "Bs 1 by references") + (("swapped lists", "both vectors from one picture") if bi else ()):
        assert counts[k] >= 100, (k, counts)
    assert changed > 0.05
    return counts, changed


def _same(got, want, what):
    for c in range(3):
        if not np.array_equal(got[c], want[c]):
            bad = np.argwhere(got[c] != want[c])
            raise AssertionError("%s, component %d: %d samples differ, first at (y, x) = %s" % (what, c, len(bad), tuple(bad[0])))


@pytest.mark.parametrize("bi", [False, True])
@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_coherent_motion_matches_oracle(oracle, fmt, bi):
    import libhm_amd
    p, ref0, ref1, cur = motion_picture(fmt, bi)
    want = oracle_chain(oracle, p, cur, [ref0, ref1])
    check_content(oracle, p, want, bi)
    with libhm_amd.Context(p.seq) as ctx:
        h0, h1, hc = ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        ctx.upload(h1, ref1)
        ctx.upload(hc, cur)
        ctx.decompress_slice(hc, 0, p.slice, p.meta, p.coeffs)
        _same(ctx.download(hc), want[0], STAGES[0])
        ctx.filter_picture(hc, p.pp, p.sao_raw, stages=3)
        _same(ctx.download(hc), want[1], STAGES[1])
        ctx.filter_picture(hc, p.pp, p.sao_raw, stages=4)
        _same(ctx.download(hc), want[2], STAGES[2])
        ctx.upload(hc, cur)
        ctx.decompress_pictures([(hc, p.slices, p.meta, p.coeffs)])
        ctx.filter_picture(hc, p.pp, p.sao_raw)
        _same(ctx.download(hc), want[2], STAGES[3])
