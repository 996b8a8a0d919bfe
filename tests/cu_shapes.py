"""The pictures of tests/test_gpu_cu_shapes.py -- symmetric and NxN prediction units, intra NxN, transform trees up to three levels deep
(tests/synth.py: part_probs, min_cu_log2, intra_nxn_prob, tr_depth_max) -- as parameter sets, so that tests/test_synth_shapes_cpu.py can hold
exactly these sets to the parser's invariants and count, without a GPU, that the shapes a GPU case is there for are in its picture; and the
closed form of explicit weighted prediction on pictures with whole-sample motion and no residual."""
import numpy as np

from libhm_amd import abi
from tests import synth

SHAPES = dict(part_probs=(0.4, 0.25, 0.25, 0.1), intra_nxn_prob=0.5, tr_depth_max=3, cbf_prob=0.7, mv_coherence=0.5)
CROSSED = dict(bi=True, num_refs=2, l1_refs=2, ref_handles=([0, 1], [1, 0]))
P_REFS = dict(num_refs=2, ref_handles=([0, 1], [1]))
NO_AMP = (0.15, 0.3, 0.3, 0.25, 0.0)
MIN16_PARTS = (0.3, 0.25, 0.25, 0.2)          # inter NxN stands in minimum CUs only: a larger share where those are 16x16

# ---- 1. the shape matrix, 4:2:0: (width, height, keywords).  Every value of picture type, intra share {0, 0.2}, bit depth {8, 10, 12}, CTU
# size {64, 32, 16} and minimum CU size {8, 16} occurs, and each of them in a B picture and in a picture with intra CUs
MATRIX = {
    "P-bd8-ctu64-min8":         (416, 240, dict(P_REFS, bit_depth=8, intra_frac=0.0, log2_ctu=6, min_cu_log2=3)),
    "B-intra-bd10-ctu64-min8":  (832, 480, dict(CROSSED, bit_depth=10, intra_frac=0.2, log2_ctu=6, min_cu_log2=3)),
    "B-intra-bd12-ctu32-min16": (416, 240, dict(CROSSED, bit_depth=12, intra_frac=0.2, log2_ctu=5, min_cu_log2=4, mode_probs=NO_AMP, part_probs=MIN16_PARTS)),
    "P-intra-bd10-ctu16-min8":  (416, 240, dict(P_REFS, bit_depth=10, intra_frac=0.2, log2_ctu=4, min_cu_log2=3)),
    "B-intra-bd8-ctu16-min16":  (416, 240, dict(CROSSED, bit_depth=8, intra_frac=0.2, log2_ctu=4, min_cu_log2=4, mode_probs=NO_AMP, part_probs=MIN16_PARTS)),
    "P-intra-bd12-ctu32-min8":  (832, 480, dict(P_REFS, bit_depth=12, intra_frac=0.2, log2_ctu=5, min_cu_log2=3)),
    "B-bd8-ctu64-min16":        (416, 240, dict(CROSSED, bit_depth=8, intra_frac=0.0, log2_ctu=6, min_cu_log2=4, part_probs=MIN16_PARTS)),
    "B-intra-bd10-1080p":       (1920, 1080, dict(CROSSED, bit_depth=10, intra_frac=0.2, log2_ctu=6, min_cu_log2=3)),
    "all-intra-bd10":           (416, 240, dict(P_REFS, bit_depth=10, intra_frac=1.0, log2_ctu=6, min_cu_log2=3, mode_probs=NO_AMP)),
    "P-intra-five-slices":      (832, 480, dict(P_REFS, bit_depth=10, intra_frac=0.2, log2_ctu=6, min_cu_log2=3, num_slices=5, lf_across_slices=0)),
}

# ---- 2. symmetric PUs only: in 8x8 CUs (every tile is cut: the cells kernels) and in 16 .. 64 CUs (none is: 64x32 .. 16x8 PUs start and end
# the vertical runs of the LDS-staged kernels)
_SYM = dict(part_probs=(0, 0.5, 0.5, 0), tr_depth_max=2, cbf_prob=0.6, mv_coherence=0.3, bit_depth=10)
SYMMETRIC = {
    "P-8x8":   (416, 240, dict(_SYM, **P_REFS, mode_probs=(0, 0, 0, 1, 0))),
    "B-8x8":   (416, 240, dict(_SYM, **CROSSED, mode_probs=(0, 0, 0, 1, 0))),
    "P-large": (448, 256, dict(_SYM, **P_REFS, mode_probs=(0.3, 0.4, 0.3, 0, 0))),          # (whole CTUs: CTUs cut by the border would bring 8x8 CUs)
    "B-large": (832, 512, dict(_SYM, **CROSSED, mode_probs=(0.3, 0.4, 0.3, 0, 0))),
}

# ---- 3. the other chroma formats on the matrix's options: sizes {416x240, 832x480} x {P, B} x depth pairs {8/8, 10/10, 12/10}
FORMATS = {}
for _fmt in (2, 3, 0):
    for _i, ((_w, _h), _bi, (_bd, _bdc), _ctu, _min) in enumerate([((416, 240), False, (8, 8), 6, 3), ((832, 480), True, (10, 10), 6, 3),
                                                                  ((416, 240), True, (12, 10), 5, 4), ((832, 480), False, (12, 10), 4, 3)]):
        if _fmt == 0 and _i == 3:
            continue
        FORMATS["fmt%d-%s-bd%d-%d-ctu%d" % (_fmt, "B" if _bi else "P", _bd, _bdc, 1 << _ctu)] = (_w, _h, dict(
            CROSSED if _bi else P_REFS, chroma_format=_fmt, bit_depth=_bd, bit_depth_chroma=_bdc, intra_frac=0.2 if _min == 3 else 0.35, log2_ctu=_ctu, min_cu_log2=_min,
            ccp_prob=0.4 if _fmt == 3 else 0.0, **(dict(part_probs=MIN16_PARTS) if _min == 4 else {})))

ALL = {"matrix": MATRIX, "symmetric": SYMMETRIC, "formats": FORMATS}


def keywords(group, name):
    kw = ALL[group][name][2]
    return dict(SHAPES, **kw) if group != "symmetric" else dict(kw)


def count_size(group, name):
    """where test_synth_shapes_cpu.py counts a set's shapes: 416x240, or the set's own size where that is none of the three standard ones"""
    w, h, _ = ALL[group][name]
    return (416, 240) if (w, h) in ((416, 240), (832, 480), (1920, 1080)) else (w, h)


def make(group, name, size=None, **over):
    """the picture of one parameter set (size: another (width, height); over: keywords on top)"""
    w, h, _ = ALL[group][name]
    kw = keywords(group, name)
    kw.update(over)
    if size is not None:
        w, h = size
    seed = 0xC5 + sum(ord(ch) for ch in group + name)
    p = synth.make_picture(w, h, seed=seed, **kw)
    if kw.get("intra_frac") == 1.0:
        for sl in p.slices:
            sl.slice_type = abi.I_SLICE
            sl.num_ref_idx[0] = sl.num_ref_idx[1] = 0
    return p


def _chain(cbf, tr):
    c = (1 << (tr + 1)) - 1
    return (cbf & c) == c


def counts(p):
    """members of each shape class in a picture, from its per-partition arrays: CUs, PUs, transform leaves, chroma blocks and nodes"""
    m = {k: np.asarray(v).astype(np.int64) for k, v in p.meta_np.items() if k != "slice_idx"}
    n, parts = m["depth"].shape
    z = np.arange(parts)[None, :]
    dec = p.inside
    ps, tr = m["part_size"], m["tr_idx"]
    cu_log2 = p.log2_ctu - m["depth"]
    cu_parts = parts >> (2 * m["depth"])
    inter = dec & (m["pred_mode"] == abi.MODE_INTER)
    cu_first = dec & (z % cu_parts == 0)
    sym = (ps == abi.SIZE_2NxN) | (ps == abi.SIZE_Nx2N)
    out = {}
    for name, code in (("2NxN", abi.SIZE_2NxN), ("Nx2N", abi.SIZE_Nx2N)):
        out[name + " CUs of 8x8"] = int((cu_first & inter & (ps == code) & (cu_log2 == 3)).sum())
        out[name + " CUs of 16 and more"] = int((cu_first & inter & (ps == code) & (cu_log2 >= 4)).sum())
    key = np.arange(n)[:, None] * 4 * parts + p.pu_idx
    out["8x4 PUs"] = np.unique(key[inter & (ps == abi.SIZE_2NxN) & (cu_log2 == 3)]).size
    out["4x8 PUs"] = np.unique(key[inter & (ps == abi.SIZE_Nx2N) & (cu_log2 == 3)]).size
    out["bi-predicted 2NxN / Nx2N PUs"] = np.unique(key[inter & sym & (m["ref_idx0"] >= 0) & (m["ref_idx1"] >= 0)]).size
    out["inter NxN CUs"] = int((cu_first & inter & (ps == abi.SIZE_NxN)).sum())
    out["intra NxN CUs"] = int((cu_first & ~inter & (ps == abi.SIZE_NxN)).sum())
    leaf_parts = np.maximum(cu_parts >> (2 * tr), 1)
    leaf_first = dec & (z % leaf_parts == 0)
    out["leaves at transform depth 2"] = int((leaf_first & (tr == 2)).sum())
    out["leaves at transform depth 3"] = int((leaf_first & (tr == 3)).sum())
    out["shared 4x4 chroma blocks under CUs above 8x8"] = 0
    out["chroma nodes set without a set child"] = 0
    if p.chroma_format:
        shared = (leaf_parts == 1) & bool(p.csx)
        if p.csx:
            out["shared 4x4 chroma blocks under CUs above 8x8"] = int((dec & shared & (z % 4 == 0) & (cu_log2 > 3) & _chain(m["cbf_u"], tr)).sum())
        own = tr - shared
        for cbf in (m["cbf_u"], m["cbf_v"]):
            for d in range(3):
                node_parts = np.maximum(cu_parts >> (2 * d), 1)
                inner = dec & (own > d)
                child = synth._group_any(inner & (((cbf >> (d + 1)) & 1) != 0), node_parts)
                out["chroma nodes set without a set child"] += int((inner & (z % node_parts == 0) & (((cbf >> d) & 1) != 0) & ~child).sum())
    return out


def possible(kw, width, height):
    """the classes of counts() that a parameter set is there for at a picture size (CTUs cut by the border take 16x16 and minimum CUs).
    tests/test_synth_shapes_cpu.py holds every set to it in both directions -- 20 members and more of each class named here, fewer of every
    other --, so a mistake in this model fails a test instead of dropping an assertion"""
    b, intra, chroma_format = bool(kw.get("bi")), kw.get("intra_frac", 0.0), kw.get("chroma_format", 1)
    min8 = kw.get("min_cu_log2", 3) == 3
    probs = kw.get("part_probs", SHAPES["part_probs"])
    modes = kw.get("mode_probs", (0.1, 0.3, 0.3, 0.2, 0.1))
    ctu = kw.get("log2_ctu", 6)
    cut = bool(width % (1 << ctu) or height % (1 << ctu))
    inter, depth_max = intra < 1.0, kw.get("tr_depth_max", SHAPES["tr_depth_max"])
    small = inter and min8 and (modes[3] > 0 or cut)
    big_cus = sum(modes[:3]) > 0 or not min8                    # CUs of 16 and more all over the picture, not only in cut CTUs
    large = inter and (big_cus or cut)
    min_cus = modes[3] > 0 or cut or (not min8 and (modes[2] > 0 or ctu == 4))
    return {"2NxN CUs of 8x8": small, "Nx2N CUs of 8x8": small, "8x4 PUs": small, "4x8 PUs": small, "2NxN CUs of 16 and more": large,
            "Nx2N CUs of 16 and more": large, "bi-predicted 2NxN / Nx2N PUs": b and large, "inter NxN CUs": inter and not min8 and probs[3] > 0 and min_cus,
            "intra NxN CUs": intra > 0 and kw.get("intra_nxn_prob", 0) > 0 and min_cus,
            "leaves at transform depth 2": (big_cus or cut) and depth_max >= 2, "leaves at transform depth 3": ctu >= 5 and depth_max >= 3 and sum(modes[:2]) > 0,
            "shared 4x4 chroma blocks under CUs above 8x8": big_cus and depth_max >= 2 and chroma_format in (1, 2),
            "chroma nodes set without a set child": chroma_format != 0 and depth_max >= 2 and big_cus}


def wants_cells(p):
    """the host's rule for launching the cells kernels, from the arrays: an inter CU of 8x8 that is not 2Nx2N, or an AMP CU of 16x16"""
    m = p.meta_np
    cu_log2 = p.log2_ctu - m["depth"]
    ps = m["part_size"]
    inter = p.inside & (m["pred_mode"] == abi.MODE_INTER)
    return bool((inter & (((cu_log2 == 3) & (ps != abi.SIZE_2Nx2N)) | ((cu_log2 == 4) & (ps >= abi.SIZE_2NxnU) & (ps <= abi.SIZE_nRx2N)))).any())


# ------------------------------------------------------------------------------------------------ weighted prediction in closed form
def set_weights(p, denoms, seed):
    """explicit weighted prediction on all slices of p: log2 denominators (luma, chroma), weights over (1 << denominator) + [-128, 127], offsets
    over [-128, 127] << (bit depth - 8), per list, reference index and component (the first four entries are the four corners of that range)"""
    rng = np.random.RandomState(seed)
    bds = (p.bit_depth, p.bit_depth_chroma, p.bit_depth_chroma)
    for sl in p.slices:
        sl.weighted_pred = 1
        sl.wp_log2_denom[0], sl.wp_log2_denom[1] = denoms
        k = 0
        for l in range(2):
            for r in range(2):
                for c in range(3):
                    d = denoms[1 if c else 0]
                    dw, o = int(rng.randint(-128, 128)), int(rng.randint(-128, 128))
                    if k < 4:
                        dw, o = ((-128, 127), (127, -128), (-128, -128), (127, 127))[k]
                    elif k % 2 == 0:                                   # every other entry a gain of 0 .. 2, so that not all of the picture clips
                        dw = int(rng.randint(-min(128, 1 << d), min(127, 1 << d) + 1))
                    k += 1
                    sl.wp_weight[l][r][c] = (1 << d) + dw
                    sl.wp_offset[l][r][c] = o << (bds[c] - 8)


def whole_sample_motion(p):
    """p with every vector rounded to an even number of luma samples (whole chroma samples too) -- the picture must have no residual"""
    m = dict(p.meta_np)
    m["mv0"], m["mv1"] = (m["mv0"] >> 3) << 3, (m["mv1"] >> 3) << 3
    assert len(synth.coded_blocks(m, p.chroma_format, p.log2_ctu)) == 0 and not p.intra.any()      # (chroma nodes set with nothing below code nothing)
    p.meta_np, p.meta = m, abi.MetaHolder(m)
    return p


def weighted_closed_form(p, planes_of_handle):
    """the planes of an inter-only picture without residual and with whole-sample motion under explicit weighted prediction, in Python
    integers from TComWeightPrediction's definitions: with s the reference sample, P = s << (14 - bd), shiftNum = max(2, 14 - bd):
      one list:  clip(((w * P + round) >> shift) + o),  shift = denominator + shiftNum, round = 1 << (shift - 1) (0 for shift 0)
      two lists: clip((w0 * P0 + w1 * P1 + round + ((o0 + o1) << (shift - 1))) >> shift),  shift = denominator + 1 + shiftNum, round = 1 << (shift - 1)
    (weightUnidir / weightBidir; P is the interpolation's intermediate plus IF_INTERNAL_OFFS, which both add back).  One slice."""
    m, sl = p.meta_np, p.slice
    ctu, cw = 1 << p.log2_ctu, p.ctus_w
    zx, zy = synth._zxy(m["depth"].shape[1])
    z_of = np.zeros((ctu // 4, ctu // 4), dtype=np.int64)
    z_of[zy, zx] = np.arange(zx.size)
    by, bx = np.mgrid[0:p.height // 4, 0:p.width // 4]
    a, zz = (by * 4 // ctu) * cw + bx * 4 // ctu, z_of[by % (ctu // 4), bx % (ctu // 4)]
    out = []
    for c in range(3):
        sx, sy = (p.csx, p.csy) if c else (0, 0)
        bd = p.bit_depth_chroma if c else p.bit_depth
        if c and p.chroma_format == 0:
            out.append(None)
            continue
        rep_x, rep_y = 4 >> sx, 4 >> sy
        up = lambda v: np.repeat(np.repeat(v, rep_y, axis=0), rep_x, axis=1)
        h, w = p.height >> sy, p.width >> sx
        y, x = np.mgrid[0:h, 0:w]
        shift_num = max(2, 14 - bd)
        denom = int(sl.wp_log2_denom[1 if c else 0])
        P, W, O, use = [], [], [], []
        for l in range(2):
            ridx = up(m["ref_idx%d" % l][a, zz])
            mv = m["mv%d" % l][a, zz]
            dx, dy = up(mv[..., 0]) >> (2 + sx), up(mv[..., 1]) >> (2 + sy)
            yy, xx = np.clip(y + dy, 0, h - 1), np.clip(x + dx, 0, w - 1)
            s = np.zeros((h, w), dtype=np.int64)
            wgt, off = np.zeros((h, w), dtype=np.int64), np.zeros((h, w), dtype=np.int64)
            for r in range(int(sl.num_ref_idx[l])):
                plane = planes_of_handle[int(sl.ref_pic[l][r])][c].astype(np.int64)
                sel = ridx == r
                s[sel] = plane[yy[sel], xx[sel]]
                wgt[sel], off[sel] = int(sl.wp_weight[l][r][c]), int(sl.wp_offset[l][r][c])
            P.append(s << (14 - bd)); W.append(wgt); O.append(off); use.append(ridx >= 0)
        sh1 = denom + shift_num
        rnd1 = (1 << (sh1 - 1)) if sh1 > 0 else 0
        uni = [((W[l] * P[l] + rnd1) >> sh1) + O[l] for l in range(2)]
        sh2 = denom + 1 + shift_num
        both = (W[0] * P[0] + W[1] * P[1] + (1 << (sh2 - 1)) + ((O[0] + O[1]) << (sh2 - 1))) >> sh2
        v = np.where(use[0] & use[1], both, np.where(use[0], uni[0], uni[1]))
        assert (use[0] | use[1]).all()
        out.append(np.clip(v, 0, (1 << bd) - 1).astype(np.int16))
    return out
