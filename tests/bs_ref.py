"""A numpy restatement of the reference / vector test of xGetBoundaryStrengthSingle (TComLoopFilter.cpp:474-532) on the pictures of
tests/synth.py, for the edge units of the 8x8 grid that lie between two inter PUs without coded luma: what the boundary strength of such a
unit is and WHY -- the classes a test wants to see in numbers before it trusts a comparison of filtered pictures.  Coverage only: expected
samples and boundary strengths always come from the oracle (motion_units() asserts that the two agree where both speak)."""
import numpy as np


def _raster(p, a, fill=0):
    """[num_ctus, parts] (or [num_ctus, parts, 2]) in z order -> the picture's grid of 4x4 partitions"""
    a = np.asarray(a)
    out = np.full((p.height // 4, p.width // 4) + a.shape[2:], fill, dtype=np.int64)
    ok = p.inside
    out[p.py[ok] // 4, p.px[ok] // 4] = a[ok]
    return out


def _mvd4(a, b):
    return (np.abs(a - b) >= 4).any(axis=-1)


def motion_units(p, bs_ver, bs_hor):
    """p: a SynthPicture; bs_ver / bs_hor: the oracle's boundary strengths.  Returns counts (dict) over the edge units between different inter
    PUs neither of which has a coded luma block (so that only references and vectors decide): Bs 0, Bs 1 by motion (the same pictures, a vector
    component 4 or more quarter samples apart), Bs 1 by references, units whose sides hold the same two pictures in swapped lists, units whose
    sides both take their two vectors from one picture"""
    m = p.meta_np
    lists = [[int(p.slice.ref_pic[l][i]) for i in range(int(p.slice.num_ref_idx[l]))] + [-1] for l in range(2)]       # (index -1 -> no picture)
    pic = [_raster(p, np.array(lists[l])[np.asarray(m["ref_idx%d" % l])], -1) for l in range(2)]
    mv = [_raster(p, m["mv%d" % l]) for l in range(2)]
    inter = _raster(p, (np.asarray(m["pred_mode"]) == 0) & (np.asarray(m["part_size"]) != 8), 0) == 1
    coded = _raster(p, (np.asarray(m["cbf_y"]) >> np.asarray(m["tr_idx"])) & 1) == 1
    n_pu = int(p.pu_idx.max()) + 1
    pu = _raster(p, np.arange(p.num_ctus)[:, None] * n_pu + p.pu_idx, -1)
    total = {"Bs 0": 0, "Bs 1 by motion": 0, "Bs 1 by references": 0, "swapped lists": 0, "both vectors from one picture": 0}
    for direction, bs_z in (("ver", bs_ver), ("hor", bs_hor)):
        bs = _raster(p, bs_z)
        if direction == "ver":
            P, Q = (slice(None), slice(1, None, 2)), (slice(None), slice(2, None, 2))
        else:
            P, Q = (slice(1, None, 2), slice(None)), (slice(2, None, 2), slice(None))
        k = min(pu[P].shape[0], pu[Q].shape[0]), min(pu[P].shape[1], pu[Q].shape[1])
        cut = lambda a, s: a[s][:k[0], :k[1]]
        sel = cut(inter, P) & cut(inter, Q) & ~cut(coded, P) & ~cut(coded, Q) & (cut(pu, P) != cut(pu, Q))
        p0, p1, q0, q1 = cut(pic[0], P), cut(pic[1], P), cut(pic[0], Q), cut(pic[1], Q)
        pm0, pm1, qm0, qm1 = cut(mv[0], P), cut(mv[1], P), cut(mv[0], Q), cut(mv[1], Q)
        same = ((p0 == q0) & (p1 == q1)) | ((p0 == q1) & (p1 == q0))
        straight = _mvd4(qm0, pm0) | _mvd4(qm1, pm1)
        crossed = _mvd4(qm1, pm0) | _mvd4(qm0, pm1)
        by_motion = np.where(p0 != p1, np.where(p0 == q0, straight, crossed), straight & crossed)
        want = np.where(same, by_motion.astype(np.int64), 1)
        assert np.array_equal(cut(bs, Q)[sel], want[sel]), "the restatement and the oracle disagree on a boundary strength (%s edges)" % direction
        total["Bs 0"] += int((sel & (want == 0)).sum())
        total["Bs 1 by motion"] += int((sel & same & (want == 1)).sum())
        total["Bs 1 by references"] += int((sel & ~same).sum())
        total["swapped lists"] += int((sel & same & (p0 != p1) & (p0 != q0)).sum())
        total["both vectors from one picture"] += int((sel & same & (p0 == p1) & (p0 >= 0)).sum())
    return total
