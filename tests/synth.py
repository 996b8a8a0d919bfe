"""Synthetic HM-shaped pictures for full-size parity tests and for bench.py.

Produces exactly what HM's parser would leave behind for a picture -- per-CTU TComDataCU arrays in z-scan order,
coefficient levels in HM's layout, raw SAO parameters -- but drawn from a seeded PRNG instead of a bitstream:
  * CTU partitioning drawn from {64x64, 4x32x32, 16x16x16, 64x8x8, AMP at 32x32} with p = {.1,.3,.3,.2,.1}
  * one motion vector per PU: integer part uniform in [-64, 64] luma samples, fraction uniform over the 16 phases
  * transform trees of depth 0/1, cbf with p = 0.5 per TU and component, "typical" levels: top-left 8x8 (4x4)
    Laplacian(b = 12) with P(nonzero) = 0.35
  * QP uniform in [22, 37] per CTU; optional fraction of intra CUs (Bs = 2 edges for the loop filter)
  * SAO per CTU and component: off .3 / BO .2 / EO0-3 .125 each
Everything is numpy-vectorised so that a 3840x2160 picture takes about a second to draw.
"""
import numpy as np

from libhm_amd import abi


def _zxy(parts):
    z = np.arange(parts)
    x = np.zeros(parts, dtype=np.int64)
    y = np.zeros(parts, dtype=np.int64)
    for b in range(8):
        x |= ((z >> (2 * b)) & 1) << b
        y |= ((z >> (2 * b + 1)) & 1) << b
    return x, y


class SynthPicture:
    pass


def make_picture(width, height, bit_depth=10, seed=1, bi=False, intra_frac=0.0, num_refs=1, slice_qp_range=(22, 37),
                 cbf_prob=0.5, sao=True, mode_probs=(0.1, 0.3, 0.3, 0.2, 0.1), ref_handles=None, mv_range=64,
                 coef_dist="typical", tr_split_prob=0.35, intra_modes=True, num_slices=1, lf_across_slices=1,
                 chroma_format=1, log2_ctu=6, bit_depth_chroma=None, ccp_prob=0.0, mv_coherence=0.0, l1_refs=1,
                 part_probs=None, min_cu_log2=3, intra_nxn_prob=0.0, tr_depth_max=1):
    """Returns a SynthPicture with .seq, .slice (abi.SliceParams), .meta (MetaHolder), .coeffs (CoeffHolder),
    .sao_raw [num_ctus,3,35], .pp, .meta_np.  ref_handles: device picture handles of list-0 / list-1 references.
    coef_dist: "typical" (see above), "stress" (every level of a coded TU uniform over the full int16 range) or
    "dense" (every level uniform in -3..3).
    chroma_format 0 / 1 / 2 / 3, log2_ctu 4 / 5 / 6 and bit_depth_chroma (None: the luma depth) select the other shapes of
    include/hmgpu.h (hmgpu_seq_params, hmgpu_ctu_meta, hmgpu_coeffs); with the defaults every array is what it always was, the PRNG
    being consumed in the same order (tests/test_synth_digests_cpu.py).
      * CTUs of 32 / 16 samples: the CU-size modes name the same CU sizes, capped at the CTU (a "64x64" CTU of a 16-sample CTU picture is
        one 16x16 CU); AMP at min(32, CTU size), which gives 4- and 12-sample wide PUs in 16-sample CTUs; QP and SAO stay per CTU
      * 4:4:4: every luma TU has chroma twins of its size (4x4 chroma per 4x4 luma, 32x32 chroma); 4:2:2: the chroma block of a transform
        unit is two squares, the upper one first, each with a flag of its own one transform depth below the unit's bit over the upper /
        lower half of the unit's partitions (TDecSbac::parseQtCbf), the 4x8 block of an 8x8 CU split into 4x4 luma TUs riding with the
        first child; 4:0:0: no coded chroma block
      * ccp_prob (4:4:4 only): probability that a transform unit whose luma block is coded carries a cross-component prediction weight
        from {+-1, +-2, +-4, +-8} per chroma component (meta ccp_u / ccp_v, on all partitions of the unit; intra units only with the
        chroma mode DM, as in HM); 0 = the arrays are absent
    Motion that lets the deblocking filter decide both ways (boundary strength 0 or 1 between inter PUs); both options draw from a second
    generator, so the arrays of a picture made without them stay what they were:
      * mv_coherence: probability that a PU, instead of its own draw, takes the vectors and reference indices of the PU left of it or above
        it (as that PU ends up, so motion spreads over areas), each vector component moved by -5 .. 5 quarter samples: the |difference| >= 4
        test of xGetBoundaryStrengthSingle then falls both ways
      * l1_refs (with bi): number of list-1 references, 1 or 2.  ref_handles=([0, 1], [1, 0]) with num_refs=2, l1_refs=2 gives PUs the same
        two pictures in swapped lists and PUs whose two vectors point into one picture -- the "crossed" and p0 == p1 branches
    The rest of HM's CU syntax; these draw from a third generator, and with all four at their defaults nothing changes:
      * part_probs = (p 2Nx2N, p 2NxN, p Nx2N, p NxN) for the inter CUs of CTU modes 0-3 (mode 4 stays AMP): motion, reference indices
        and the bi-prediction kind per PU, on all partitions of the PU; 8x4 / 4x8 PUs take one list only; inter NxN only in CUs of the
        minimum size when that is above 8 (elsewhere 2Nx2N)
      * min_cu_log2 3 / 4: with 4 the "64x8x8" CTU mode gives 16x16 CUs (width and height multiples of 16)
      * intra_nxn_prob: share of the intra CUs of the minimum size that are SIZE_NxN: tr_idx >= 1, a luma mode per PU, the chroma mode per
        CU (4:4:4: per PU)
      * tr_depth_max 1 .. 3: transform trees drawn node by node with tr_split_prob (_transform_trees); any of the four options switches
        to these trees.  Only they follow rqt_root_cbf: the default pictures, pinned byte for byte, keep tr_idx 1 in inter CUs without any
        coded block, where HM's parser leaves 0 -- the one rule of check_parser_invariants() that default pictures break"""
    assert chroma_format in (0, 1, 2, 3) and log2_ctu in (4, 5, 6) and l1_refs in (1, 2)
    assert min_cu_log2 in (3, 4) and tr_depth_max in (1, 2, 3) and (min_cu_log2 == 3 or (width % 16 == 0 and height % 16 == 0))
    shapes = part_probs is not None or min_cu_log2 != 3 or intra_nxn_prob > 0 or tr_depth_max > 1
    fmt = 1 if chroma_format == 0 else chroma_format                  # 4:0:0 keeps the geometry of 4:2:0
    csx, csy = (0 if fmt == 3 else 1), (1 if fmt == 1 else 0)
    bdc = bit_depth if bit_depth_chroma is None else bit_depth_chroma
    rng = np.random.RandomState(seed)
    ctu, pw, parts = 1 << log2_ctu, 1 << (log2_ctu - 2), 1 << (2 * log2_ctu - 4)
    cw, ch = (width + ctu - 1) // ctu, (height + ctu - 1) // ctu
    n = cw * ch
    zx, zy = _zxy(parts)
    ctu_x = (np.arange(n) % cw) * ctu
    ctu_y = (np.arange(n) // cw) * ctu
    px = ctu_x[:, None] + 4 * zx[None, :]
    py = ctu_y[:, None] + 4 * zy[None, :]
    inside = (px < width) & (py < height)

    # ---- CTU partitioning mode.  CTUs cut by the picture border take the modes whose CUs fit (16x16 / 8x8)
    mode = rng.choice(5, size=n, p=mode_probs)
    partial = (ctu_x + ctu > width) | (ctu_y + ctu > height)
    if width % 16 or height % 16:
        mode[partial] = 3                                          # only 8x8 CUs tile a picture that is not a multiple of 16
    else:
        mode[partial] = np.where(rng.rand(int(partial.sum())) < 0.6, 2, 3)
    cu_log2 = np.minimum(np.array([6, 5, 4, min_cu_log2, 5])[mode], log2_ctu)  # per CTU
    depth = (log2_ctu - cu_log2)[:, None] * np.ones((1, parts), dtype=np.int64)
    cu_parts = (1 << (2 * (cu_log2 - 2)))[:, None]                # partitions per CU
    z = np.arange(parts)[None, :]
    cu_idx = z // cu_parts                                         # CU index inside the CTU (z order)
    child = (z % cu_parts) // np.maximum(cu_parts // 4, 1)         # quadrant inside the CU
    n_cu_max = parts // 4
    n_pu_max = 2 * n_cu_max

    # ---- part size: 2Nx2N except mode 4 (AMP, one of 2NxnU, 2NxnD, nLx2N, nRx2N per CU)
    amp_type = rng.randint(4, 8, size=(n, n_cu_max))
    part_size = np.zeros((n, parts), dtype=np.int64)
    is_amp = (mode == 4)[:, None] & np.ones((1, parts), dtype=bool)
    part_size[is_amp] = np.take_along_axis(amp_type, cu_idx, axis=1)[is_amp]
    # PU index inside the CU (0/1) for AMP CUs: depends on the partition's row/column inside the 32x32 CU (8 partitions wide;
    # 16x16 CUs in 16-sample CTUs: 4 wide)
    amp_w = min(8, pw)
    rel_x = zx[None, :] % amp_w
    rel_y = zy[None, :] % amp_w
    pu_in_cu = np.zeros((n, parts), dtype=np.int64)
    pu_in_cu = np.where(is_amp & (part_size == abi.SIZE_2NxnU), (rel_y >= amp_w // 4).astype(np.int64), pu_in_cu)
    pu_in_cu = np.where(is_amp & (part_size == abi.SIZE_2NxnD), (rel_y >= amp_w - amp_w // 4).astype(np.int64), pu_in_cu)
    pu_in_cu = np.where(is_amp & (part_size == abi.SIZE_nLx2N), (rel_x >= amp_w // 4).astype(np.int64), pu_in_cu)
    pu_in_cu = np.where(is_amp & (part_size == abi.SIZE_nRx2N), (rel_x >= amp_w - amp_w // 4).astype(np.int64), pu_in_cu)
    pu_idx = cu_idx * 2 + pu_in_cu                                 # < 128

    # ---- prediction mode per CU
    intra_cu = rng.rand(n, n_cu_max) < intra_frac
    intra = np.take_along_axis(intra_cu, cu_idx, axis=1)
    intra &= ~is_amp                                               # AMP is inter only
    pred_mode = intra.astype(np.int64)

    # ---- the CU shapes beyond 2Nx2N / AMP (part_probs, min_cu_log2, intra_nxn_prob, tr_depth_max): everything they draw comes from a
    # third generator; a CU then has four PU slots, the first two filled by the pinned generators as before
    rng3 = np.random.RandomState(seed ^ 0x5A9E5)
    slots = 4 if shapes else 2
    small_pu = np.zeros((n, parts), dtype=bool)                    # partitions of 8x4 / 4x8 PUs: one list only (8.5.3.2.2)
    if shapes:
        at_min = (cu_log2 == min(min_cu_log2, log2_ctu))[:, None]
        ps = np.take_along_axis(rng3.choice(4, size=(n, n_cu_max), p=part_probs if part_probs is not None else (1, 0, 0, 0)), cu_idx, axis=1)
        ps = np.where((ps == abi.SIZE_NxN) & ~(at_min & (min_cu_log2 > 3)), abi.SIZE_2Nx2N, ps)      # inter NxN: minimum CUs above 8x8 only
        nxn_intra = np.take_along_axis(rng3.rand(n, n_cu_max) < intra_nxn_prob, cu_idx, axis=1) & at_min
        ps = np.where(intra, np.where(nxn_intra, abi.SIZE_NxN, abi.SIZE_2Nx2N), ps)
        part_size = np.where(is_amp, part_size, ps)
        cu_w = (1 << (cu_log2 - 2))[:, None]                       # CU width in partitions
        hx = ((zx[None, :] % cu_w) >= cu_w // 2).astype(np.int64)
        hy = ((zy[None, :] % cu_w) >= cu_w // 2).astype(np.int64)
        pu_in_cu = np.where(part_size == abi.SIZE_2NxN, hy, np.where(part_size == abi.SIZE_Nx2N, hx, np.where(part_size == abi.SIZE_NxN, 2 * hy + hx, pu_in_cu)))
        pu_idx = cu_idx * 4 + pu_in_cu
        small_pu = (cu_log2 == 3)[:, None] & ((part_size == abi.SIZE_2NxN) | (part_size == abi.SIZE_Nx2N))

    def widen(a, extra):
        """per-PU draws [n, 2 per CU, ...] -> [n, 4 per CU, ...]: slots 2 and 3 from extra()"""
        if slots == 2:
            return a
        a = a.reshape((n, n_cu_max, 2) + a.shape[2:])
        return np.concatenate([a, extra().reshape(a.shape)], axis=2).reshape((n, 4 * n_cu_max) + a.shape[3:])

    # ---- motion per PU
    def draw_mv():
        mvi = rng.randint(-mv_range, mv_range + 1, size=(n, n_pu_max, 2))
        mvf = rng.randint(0, 4, size=(n, n_pu_max, 2))
        return mvi * 4 + mvf
    def draw_mv3():
        return rng3.randint(-mv_range, mv_range + 1, size=(n, n_pu_max, 2)) * 4 + rng3.randint(0, 4, size=(n, n_pu_max, 2))
    mv0_pu = widen(draw_mv(), draw_mv3)
    mv1_pu = widen(draw_mv(), draw_mv3)
    idx3 = np.repeat(pu_idx[:, :, None], 2, axis=2)
    mv0 = np.take_along_axis(mv0_pu, idx3, axis=1)
    mv1 = np.take_along_axis(mv1_pu, idx3, axis=1)
    ref_idx0 = np.zeros((n, parts), dtype=np.int64)
    if num_refs > 1:
        ref_pu = widen(rng.randint(0, num_refs, size=(n, n_pu_max)), lambda: rng3.randint(0, num_refs, size=(n, n_pu_max)))
        ref_idx0 = np.take_along_axis(ref_pu, pu_idx, axis=1)
    ref_idx1 = np.full((n, parts), -1, dtype=np.int64)
    if bi:
        # per PU: 0 = L0 only, 1 = L1 only, 2 = both   (8x4 / 4x8 PUs do not exist here, so bi is legal everywhere)
        kind_pu = widen(rng.choice(3, size=(n, n_pu_max), p=(0.2, 0.1, 0.7)), lambda: rng3.choice(3, size=(n, n_pu_max), p=(0.2, 0.1, 0.7)))
        kind = np.take_along_axis(kind_pu, pu_idx, axis=1)
        if shapes:
            kind = np.where(small_pu & (kind == 2), np.take_along_axis(rng3.randint(0, 2, size=(n, 4 * n_cu_max)), pu_idx, axis=1), kind)
        ref_idx1 = np.where(kind >= 1, 0, -1)
        ref_idx0 = np.where(kind == 1, -1, ref_idx0)
    ref_idx0 = np.where(intra, -1, ref_idx0)
    ref_idx1 = np.where(intra, -1, ref_idx1)
    mv0 = np.where((ref_idx0 < 0)[:, :, None], 0, mv0)
    mv1 = np.where((ref_idx1 < 0)[:, :, None], 0, mv1)

    rng2 = np.random.RandomState(seed ^ 0x5EED2)                 # the later options: never the first generator, whose order is pinned
    if bi and l1_refs > 1:
        ref1_pu = widen(rng2.randint(0, l1_refs, size=(n, n_pu_max)), lambda: rng3.randint(0, l1_refs, size=(n, n_pu_max)))
        ref_idx1 = np.where(ref_idx1 >= 0, np.take_along_axis(ref1_pu, pu_idx, axis=1), -1)
    if mv_coherence > 0:
        # PUs in decoding order (CTU by CTU, z order inside): the PU left of / above a PU's first partition has had its turn
        key = (np.arange(n)[:, None] * (slots * n_cu_max) + pu_idx)[inside & ~intra]
        _, first = np.unique(key, return_index=True)
        a_all, z_all = np.nonzero(inside & ~intra)
        order = np.argsort(first, kind="stable")
        take = rng2.rand(first.size) < mv_coherence
        above = rng2.rand(first.size) < 0.5
        delta = rng2.randint(-5, 6, size=(first.size, 2, 2))
        for i in order:
            if not take[i]:
                continue
            a, zf = a_all[first[i]], z_all[first[i]]
            nx, ny = px[a, zf] - (0 if above[i] else 4), py[a, zf] - (4 if above[i] else 0)
            if nx < 0 or ny < 0:
                continue
            na = (ny // ctu) * cw + nx // ctu
            nz = np.nonzero((zx == (nx % ctu) // 4) & (zy == (ny % ctu) // 4))[0][0]
            if intra[na, nz] or (small_pu[a, zf] and ref_idx0[na, nz] >= 0 and ref_idx1[na, nz] >= 0):
                continue
            mine = (pu_idx[a] == pu_idx[a, zf]) & inside[a] & ~intra[a]
            ref_idx0[a, mine], ref_idx1[a, mine] = ref_idx0[na, nz], ref_idx1[na, nz]
            mv0[a, mine] = mv0[na, nz] + delta[i, 0] if ref_idx0[na, nz] >= 0 else 0
            mv1[a, mine] = mv1[na, nz] + delta[i, 1] if ref_idx1[na, nz] >= 0 else 0

    # ---- transform tree: tr_idx in {0,1} per CU (64x64 CUs and AMP CUs always split once)
    tr_cu = (rng.rand(n, n_cu_max) < tr_split_prob).astype(np.int64)
    tr_idx = np.take_along_axis(tr_cu, cu_idx, axis=1)
    tr_idx = np.where(((cu_log2 == 6) | (mode == 4))[:, None], 1, tr_idx)
    # cbf: per CU one flag for the unsplit TU and four for the children, per component
    cbf = []
    for comp in range(3):
        c0 = rng.rand(n, n_cu_max) < cbf_prob
        c1 = rng.rand(n, n_cu_max, 4) < cbf_prob
        if comp > 0 and csx:
            # 8x8 CUs split once: a single 4x4 chroma TU for the four 4x4 luma TUs; its flag is stored at both depths
            # (4:4:4: every 4x4 luma TU has its own chroma twins)
            one = np.repeat(c1[:, :, :1], 4, axis=2)
            c1 = np.where((mode == 3)[:, None, None], one, c1)
        if comp > 0 and chroma_format == 0:
            c0, c1 = np.zeros_like(c0), np.zeros_like(c1)
        any1 = c1.any(axis=2)
        b0_unsplit = np.take_along_axis(c0, cu_idx, axis=1)
        b0_split = np.take_along_axis(any1, cu_idx, axis=1)
        flat = c1.reshape(n, n_cu_max * 4)
        b1 = np.take_along_axis(flat, cu_idx * 4 + child, axis=1)
        bits = np.where(tr_idx == 0, b0_unsplit.astype(np.int64), b0_split.astype(np.int64) | (b1.astype(np.int64) << 1))
        if comp > 0 and fmt == 2:
            # 4:2:2: which of the block's two squares are coded -- 0 both, 1 the upper one only, 2 the lower one only --, drawn per
            # block like its flag; the squares' flags sit one depth below the block's bit, over the upper / lower half of the block's
            # partitions.  The block of an 8x8 CU split once (4x8) belongs to the CU: halves of the CU, the draw of its first child
            k0 = rng.randint(0, 3, size=(n, n_cu_max))
            k1 = rng.randint(0, 3, size=(n, n_cu_max, 4))
            k1 = np.where((mode == 3)[:, None, None], np.repeat(k1[:, :, :1], 4, axis=2), k1)
            kind = np.where(tr_idx == 0, np.take_along_axis(k0, cu_idx, axis=1),
                            np.take_along_axis(k1.reshape(n, n_cu_max * 4), cu_idx * 4 + child, axis=1))
            blk_parts = np.where((tr_idx == 0) | (cu_parts == 4), cu_parts, np.maximum(cu_parts // 4, 1)) * np.ones((1, parts), dtype=np.int64)
            lower = (z % blk_parts) >= blk_parts // 2
            coded = ((bits >> tr_idx) & 1) != 0
            sub = coded & np.where(lower, kind != 1, kind != 2)
            bits = bits | (sub.astype(np.int64) << (tr_idx + 1))
        cbf.append(bits)
    if shapes:
        tr_idx, cbf = _transform_trees(rng3, n, parts, cu_log2, cu_parts, z, tr_split_prob, tr_depth_max, cbf_prob, chroma_format,
                                       ((cu_log2 == 6) | (mode == 4))[:, None] | (intra & (part_size == abi.SIZE_NxN)), intra)
    # ---- intra prediction modes: one luma mode per CU (2Nx2N), chroma mode from HM's candidate set incl. DM (36)
    luma_mode_cu = rng.randint(0, 35, size=(n, n_cu_max))
    intra_dir_l = np.take_along_axis(luma_mode_cu, cu_idx, axis=1)
    chroma_mode_cu = np.array([0, 1, 10, 26, 34, 36])[rng.randint(0, 6, size=(n, n_cu_max))]
    intra_dir_c = np.take_along_axis(chroma_mode_cu, cu_idx, axis=1)
    if shapes:                                                      # NxN: a luma mode per PU; the chroma mode per CU, in 4:4:4 per PU
        nxn = intra & (part_size == abi.SIZE_NxN)
        slot = cu_idx * 4 + pu_in_cu
        intra_dir_l = np.where(nxn, np.take_along_axis(rng3.randint(0, 35, size=(n, 4 * n_cu_max)), slot, axis=1), intra_dir_l)
        if not csx:
            cm4 = np.array([0, 1, 10, 26, 34, 36])[rng3.randint(0, 6, size=(n, 4 * n_cu_max))]
            intra_dir_c = np.where(nxn, np.take_along_axis(cm4, slot, axis=1), intra_dir_c)
    qp_ctu = rng.randint(slice_qp_range[0], slice_qp_range[1] + 1, size=n)
    qp = np.repeat(qp_ctu[:, None], parts, axis=1)

    # undecoded partitions (outside the picture): HM's initCU defaults
    def outside(a, v):
        return np.where(inside, a, v)
    part_size = outside(part_size, abi.SIZE_NONE)
    depth = outside(depth, 0)
    pred_mode = outside(pred_mode, 0)
    tr_idx = outside(tr_idx, 0)
    cbf = [outside(c, 0) for c in cbf]
    ref_idx0 = outside(ref_idx0, -1)
    ref_idx1 = outside(ref_idx1, -1)
    mv0 = np.where(inside[:, :, None], mv0, 0)
    mv1 = np.where(inside[:, :, None], mv1, 0)

    # ---- coefficient levels in HM's layout
    coef = [np.zeros((n, ctu * ctu), dtype=np.int16), np.zeros((n, ctu * ctu >> (csx + csy)), dtype=np.int16),
            np.zeros((n, ctu * ctu >> (csx + csy)), dtype=np.int16)]
    log2cu_p = (log2_ctu - depth)
    log2tu_p = log2cu_p - tr_idx
    decoded = inside & (part_size != abi.SIZE_NONE)
    for comp in range(3):
        chain = (1 << (tr_idx + 1)) - 1
        has = decoded & ((cbf[comp] & chain) == chain)
        for log2tu_l in range(2, 6):           # luma TU size of the node
            tu_parts = 1 << (2 * max(log2tu_l - 2, 0))
            sel = has & (log2tu_p == log2tu_l)
            if comp == 0 or log2tu_l > 2 or not csx:
                origin = sel & ((np.arange(parts)[None, :] % tu_parts) == 0)
                size = (1 << log2tu_l) >> (csx if comp else 0)
                blk_parts = tu_parts
            else:
                origin = sel & ((np.arange(parts)[None, :] % 4) == 0)      # shared 4x4 chroma TU rides with the first child
                size = 4
                blk_parts = 4
            # the squares of the block: one, or in 4:2:2 chroma two of half the width one above the other, the upper one first; the
            # lower one's flag is that of the first partition of the block's lower half
            squares = [(origin, 0)]
            if comp and fmt == 2:
                sub_bit = (cbf[comp] >> (tr_idx + 1)) & 1
                squares = [(origin & (sub_bit != 0), 0), (origin & (np.roll(sub_bit, -(blk_parts // 2), axis=1) != 0), size * size)]
            for org, sq_off in squares:
                a_idx, z_idx = np.nonzero(org)
                if a_idx.size == 0:
                    continue
                if coef_dist == "stress":
                    k = size
                    lev = rng.randint(-32768, 32768, size=(a_idx.size, k, k)).astype(np.int16)
                elif coef_dist == "dense":       # every position of the TU small and non-zero-ish: all basis functions, few samples reach the final clip
                    k = size
                    lev = rng.randint(-3, 4, size=(a_idx.size, k, k)).astype(np.int16)
                else:
                    k = min(size, 8)
                    lev = np.round(rng.laplace(0, 12, size=(a_idx.size, k, k))) * (rng.rand(a_idx.size, k, k) < 0.35)
                    lev = np.clip(lev, -32768, 32767).astype(np.int16)
                off = ((16 * z_idx) >> ((csx + csy) if comp else 0)) + sq_off
                rr, cc = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
                flat_idx = off[:, None, None] + rr[None] * size + cc[None]
                coef[comp][a_idx[:, None, None], flat_idx] = lev

    # ---- cross-component prediction weights (4:4:4): per transform unit = luma TU, non-zero only where its luma block is coded
    ccp = None
    if fmt == 3 and ccp_prob > 0:
        tu_first = np.arange(parts)[None, :] & ~(np.maximum(1 << (2 * (log2tu_p - 2)), 1) - 1)
        chain = (1 << (tr_idx + 1)) - 1
        luma_coded = decoded & ((cbf[0] & chain) == chain)
        allowed = luma_coded & (~intra | (intra_dir_c == 36))
        ccp = []
        for comp in (1, 2):
            w = np.array([1, 2, 4, 8])[rng.randint(0, 4, size=(n, parts))] * np.where(rng.rand(n, parts) < 0.5, -1, 1)
            w = w * (rng.rand(n, parts) < ccp_prob)
            ccp.append(np.where(allowed, np.take_along_axis(w, tu_first, axis=1), 0))

    # ---- SAO
    sao_raw = np.zeros((n, 3, 35), dtype=np.int32)
    if sao:
        maxo = 7
        for comp in range(3):
            kind = rng.choice(6, size=n, p=(0.3, 0.2, 0.125, 0.125, 0.125, 0.125))     # 0 off, 1 BO, 2.. EO0..3
            sao_raw[:, comp, 0] = np.where(kind == 0, abi.SAO_OFF, abi.SAO_NEW)
            sao_raw[:, comp, 1] = np.where(kind == 1, abi.SAO_BO, np.maximum(kind - 2, 0))
            band = rng.randint(0, 32, size=n)
            sao_raw[:, comp, 2] = np.where(kind == 1, band, 0)
            offs = rng.randint(-maxo, maxo + 1, size=(n, 4))
            for i in range(4):
                bidx = (band + i) % 32
                bo = np.zeros((n, 32), dtype=np.int32)
                bo[np.arange(n), bidx] = offs[:, i]
                sao_raw[:, comp, 3:] += np.where((kind == 1)[:, None], bo, 0)
            eo = np.zeros((n, 32), dtype=np.int32)
            eo[:, 0] = np.abs(offs[:, 0]); eo[:, 1] = np.abs(offs[:, 1]); eo[:, 3] = -np.abs(offs[:, 2]); eo[:, 4] = -np.abs(offs[:, 3])
            sao_raw[:, comp, 3:] += np.where((kind >= 2)[:, None], eo, 0)

    if chroma_format == 0:
        sao_raw[:, 1:, :] = 0               # no chroma syntax in a monochrome stream: the parser leaves SAO_OFF (0)
    p = SynthPicture()
    p.width, p.height, p.bit_depth, p.num_ctus, p.ctus_w = width, height, bit_depth, n, cw
    p.seq = abi.make_seq(width, height, bit_depth, bdc, log2_ctu=log2_ctu, max_pictures=4)
    p.seq.chroma_format = chroma_format
    p.chroma_format, p.log2_ctu, p.bit_depth_chroma, p.csx, p.csy = chroma_format, log2_ctu, bdc, csx, csy
    handles = ref_handles if ref_handles is not None else ([0] * num_refs, [0])
    l0 = list(handles[0])[:max(num_refs, 1)]
    l1 = list(handles[1])[:l1_refs] if bi else []
    p.slice = abi.make_slice(abi.B_SLICE if bi else abi.P_SLICE, (l0, l1), ([100 + i for i in range(len(l0))], [200 + i for i in range(len(l1))]))
    # slices: contiguous CTU ranges starting at seeded CTU addresses (mid-row starts included); slice k may differ in its
    # deblocking offsets and chroma QP offsets, all share the reference lists
    p.slices, p.slice_ranges = [p.slice], [(0, n)]
    slice_idx = np.zeros(n, dtype=np.uint16)
    if num_slices > 1:
        starts = [0] + sorted(int(v) for v in rng.choice(np.arange(1, n), size=num_slices - 1, replace=False))
        p.slices, p.slice_ranges = [], []
        for k, a in enumerate(starts):
            b_ = starts[k + 1] if k + 1 < len(starts) else n
            sl = abi.make_slice(abi.B_SLICE if bi else abi.P_SLICE, (l0, l1), ([100 + i for i in range(len(l0))], [200 + i for i in range(len(l1))]),
                                cb_qp_offset=int(rng.randint(-3, 4)), cr_qp_offset=int(rng.randint(-3, 4)),
                                beta_offset_div2=int(rng.randint(-2, 3)), tc_offset_div2=int(rng.randint(-2, 3)),
                                lf_across_slices=lf_across_slices)
            sl.pps_cb_qp_offset, sl.pps_cr_qp_offset = sl.cb_qp_offset, sl.cr_qp_offset
            p.slices.append(sl)
            p.slice_ranges.append((a, b_ - a))
            slice_idx[a:b_] = k
        p.slice = p.slices[0]
    m = {"depth": depth, "part_size": part_size, "pred_mode": pred_mode, "qp": qp, "tr_idx": tr_idx, "cbf_y": cbf[0], "cbf_u": cbf[1],
         "cbf_v": cbf[2], "mv0": mv0, "mv1": mv1, "ref_idx0": ref_idx0, "ref_idx1": ref_idx1,
         "intra_dir_l": np.where(intra, intra_dir_l, 1), "intra_dir_c": np.where(intra, intra_dir_c, 36)}
    m["slice_idx"] = slice_idx
    if ccp is not None:
        m["ccp_u"], m["ccp_v"] = ccp
    if not intra_modes:                 # the caller leaves intra CUs to somebody else: no modes, nothing reconstructed there
        del m["intra_dir_l"], m["intra_dir_c"]
    p.meta_np = m
    p.meta = abi.MetaHolder(m)
    p.coeffs = abi.CoeffHolder(*coef)
    p.sao_raw = sao_raw
    p.pp = abi.make_pic_params(sao_enabled=1 if sao else 0)
    p.inside = inside
    p.intra = intra & decoded
    p.px, p.py = px, py
    p.pu_idx = pu_idx                     # [num_ctus, parts]: the PU a partition belongs to, numbered inside its CTU
    p.small_pu = small_pu & decoded & ~intra      # partitions of 8x4 / 4x8 PUs
    return p


def _transform_trees(rng3, n, parts, cu_log2, cu_parts, z, split_prob, depth_max, cbf_prob, chroma_format, force, intra):
    """A transform tree per CU and its flags as HM's parser leaves them (TDecEntropy::xDecodeTransform, TDecSbac::parseQtCbf): a node splits
    with split_prob while its luma size is above 4 and its depth below depth_max (force: at depth 0 regardless); tr_idx = depth of a
    partition's leaf; cbf bit d = flag of the depth-d node the partition lies in -- luma: the OR of the node's leaves; chroma: a flag of the
    node's own, set wherever a child's is and now and then without one (the children are then not coded at all); 4x4 luma leaves share the
    chroma block of their 8x8 parent, whose bit they repeat at their own depth (4:4:4: chroma follows luma); 4:2:2: the two squares' flags
    one depth below the block's bit over the halves of its partitions.  An inter CU with no flag set at all has tr_idx 0 (rqt_root_cbf).
    Returns (tr_idx, [cbf_y, cbf_u, cbf_v])."""
    fmt = 1 if chroma_format == 0 else chroma_format
    csx = 0 if fmt == 3 else 1

    def at(a, first):
        return np.take_along_axis(a, first, axis=1)
    tr_idx = np.zeros((n, parts), dtype=np.int64)
    alive = np.ones((n, parts), dtype=bool)
    for d in range(3):
        first = z & ~(np.maximum(cu_parts >> (2 * d), 1) - 1)
        draw = at(rng3.rand(n, parts) < split_prob, first)
        if d == 0:
            draw = draw | force
        alive = alive & draw & ((cu_log2[:, None] - d) > 2) & (d < depth_max)
        tr_idx = tr_idx + alive
    leaf_parts = np.maximum(cu_parts >> (2 * tr_idx), 1)
    cbf = []
    for comp in range(3):
        if comp and chroma_format == 0:
            cbf.append(np.zeros((n, parts), dtype=np.int64))
            continue
        share = bool(comp and csx)
        shared = (leaf_parts == 1) & share
        tc = tr_idx - shared                                       # depth of the node that owns the block
        blk = np.where(shared, 4, leaf_parts)
        leaf = at(rng3.rand(n, parts) < cbf_prob, z & ~(blk - 1))
        # a chroma node now and then set with nothing coded below it: the shallowest such node on a partition's path
        alone = np.full((n, parts), 9, dtype=np.int64)
        for d in range(3):
            pick = at(rng3.rand(n, parts) < 0.25, z & ~(np.maximum(cu_parts >> (2 * d), 1) - 1)) & (tc > d) & (alone == 9) & bool(comp)
            alone = np.where(pick, d, alone)
        leaf = leaf & (alone == 9)
        cur = np.zeros((n, parts), dtype=bool)
        bits = np.zeros((n, parts), dtype=np.int64)
        for d in (3, 2, 1, 0):
            node_parts = np.maximum(cu_parts >> (2 * d), 1)
            inner = _group_any(cur, node_parts) | (alone == d)
            cur = np.where(tc == d, leaf, (tc > d) & inner)
            bits = bits | (cur.astype(np.int64) << d)
        bits = bits | np.where(shared, ((bits >> tc) & 1) << tr_idx, 0)
        if comp and fmt == 2:
            kind = at(rng3.randint(0, 3, size=(n, parts)), z & ~(blk - 1))     # 0 both squares, 1 the upper one only, 2 the lower one only
            lower = (z % blk) >= blk // 2
            sub = (((bits >> tr_idx) & 1) != 0) & np.where(lower, kind != 1, kind != 2)
            bits = bits | (sub.astype(np.int64) << (tr_idx + 1))
        cbf.append(bits)
    empty = ~_group_any((cbf[0] | cbf[1] | cbf[2]) != 0, cu_parts) & ~intra      # no flag anywhere in the CU: nothing to undo but tr_idx
    tr_idx = np.where(empty, 0, tr_idx)
    return tr_idx, cbf


def intra_sample_mask(p, comp):
    """True where a sample belongs to an intra CU (not reconstructed by the device in this round)"""
    cs = 1 if comp else 0
    mask = np.zeros((p.height >> cs, p.width >> cs), dtype=bool)
    a, z = np.nonzero(p.intra)
    if a.size:
        x, y = p.px[a, z] >> cs, p.py[a, z] >> cs
        step = 4 >> cs
        for dy in range(step):
            for dx in range(step):
                mask[y + dy, x + dx] = True
    return mask


def _plane_geometry(chroma_format, bit_depth, bit_depth_chroma):
    """per component (log2 horizontal, log2 vertical subsampling, bit depth); 4:0:0 keeps 4:2:0-shaped chroma planes (hmgpu_seq_params)"""
    csx, csy = (0 if chroma_format == 3 else 1), (1 if chroma_format in (0, 1) else 0)
    bdc = bit_depth if bit_depth_chroma is None else bit_depth_chroma
    return [(0, 0, bit_depth), (csx, csy, bdc), (csx, csy, bdc)]


def noise_planes(width, height, bit_depth, seed, chroma_format=1, bit_depth_chroma=None):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 1 << bd, size=(height >> sy, width >> sx)).astype(np.int16) for sx, sy, bd in _plane_geometry(chroma_format, bit_depth, bit_depth_chroma)]


def smooth_planes(width, height, bit_depth, seed, chroma_format=1, bit_depth_chroma=None):
    """piecewise ramps: every 32x32 region of a plane (the same area in chroma samples) has a level and two slopes of its own, plus noise of
    +-1 -- references on which motion-compensated prediction stays smooth inside a block and steps at block edges, so that the deblocking
    filter finds d < beta on a large part of the edges (on noise_planes it almost never does)"""
    rng = np.random.RandomState(seed)
    out = []
    for sx, sy, bd in _plane_geometry(chroma_format, bit_depth, bit_depth_chroma):
        w, h = width >> sx, height >> sy
        gh, gw = (h + 31) // 32, (w + 31) // 32
        sc = 1 << (bd - 8)
        level = rng.randint(40 * sc, 216 * sc, size=(gh, gw))
        slope = rng.randint(-4 * sc, 4 * sc + 1, size=(2, gh, gw)) / 8.0
        y, x = np.mgrid[0:h, 0:w]
        v = level[y // 32, x // 32] + slope[0][y // 32, x // 32] * (x % 32 - 16) + slope[1][y // 32, x // 32] * (y % 32 - 16) + rng.randint(-1, 2, size=(h, w))
        out.append(np.clip(np.round(v), 0, (1 << bd) - 1).astype(np.int16))
    return out


def blocky_planes(width, height, bit_depth, seed, chroma_format=1, bit_depth_chroma=None):
    """low-pass noise + 8x8 blocking steps: splits the deblocking decisions between off / weak / strong"""
    rng = np.random.RandomState(seed)
    out = []
    for sx, sy, bit_depth in _plane_geometry(chroma_format, bit_depth, bit_depth_chroma):
        w, h = width >> sx, height >> sy
        base = rng.randint(0, 1 << bit_depth, size=((h + 15) // 16 + 1, (w + 15) // 16 + 1)).astype(np.float64)
        up = np.kron(base, np.ones((16, 16)))[:h, :w]
        for _ in range(2):
            up = (up + np.roll(up, 3, 0) + np.roll(up, 3, 1) + np.roll(up, -3, 0) + np.roll(up, -3, 1)) / 5.0
        steps = rng.randint(-6, 7, size=((h + 7) // 8, (w + 7) // 8)) * (1 << (bit_depth - 8))
        up = up * 0.6 + (1 << (bit_depth - 1)) * 0.4 + np.kron(steps, np.ones((8, 8)))[:h, :w] + rng.randint(-2, 3, size=(h, w))
        out.append(np.clip(np.round(up), 0, (1 << bit_depth) - 1).astype(np.int16))
    return out


def coded_blocks(meta, chroma_format, log2_ctu):
    """The coded transform blocks of a picture, from HM's per-partition arrays alone (meta: dict with depth, part_size, tr_idx, cbf_y /
    cbf_u / cbf_v as [num_ctus, parts]): an int64 array [N, 4] of (component, CTU, offset of the block in the CTU's piece of the
    component's level array, size of the square block).  The rules are those of include/hmgpu.h (hmgpu_coeffs): a block is coded iff the
    cbf bits of its transform unit are set down to the unit's transform depth; luma at 16 * z; chroma at (16 * z) >> (csx + csy), half the
    size in 4:2:0 (the four 4x4 luma TUs of an 8x8 node share the 4x4 block at the first of them), the luma size in 4:4:4, and in 4:2:2
    two squares of half the width, the lower one behind the upper one, each coded iff its own flag -- one transform depth below the unit's
    bit, at the first partition of the upper / lower half of the block's partitions -- is set.  make_picture lays its levels out by the same
    rules but in code of its own; tests/test_synth_formats_cpu.py holds this function against HM's own fixtures."""
    fmt = 1 if chroma_format == 0 else chroma_format
    csx, csy = (0 if fmt == 3 else 1), (1 if fmt == 1 else 0)
    depth, tr = np.asarray(meta["depth"]).astype(np.int64), np.asarray(meta["tr_idx"]).astype(np.int64)
    n, parts = depth.shape
    decoded = np.asarray(meta["part_size"]) != abi.SIZE_NONE
    log2tu = log2_ctu - depth - tr
    z = np.arange(parts)[None, :]
    tu_parts = 1 << (2 * np.maximum(log2tu - 2, 0))
    chain = (1 << (tr + 1)) - 1
    out = []
    for comp, key in enumerate(("cbf_y", "cbf_u", "cbf_v")):
        if comp and chroma_format == 0:
            break
        cbf = np.asarray(meta[key]).astype(np.int64)
        coded = decoded & ((cbf & chain) == chain) & (log2tu >= 2) & (log2tu <= 5)
        shared = (log2tu == 2) & (comp > 0) & (csx == 1)           # the chroma block of an 8x8 node with four 4x4 luma TUs
        blk_parts = np.where(shared, 4, tu_parts)
        origin = coded & ((z % blk_parts) == 0)
        size = np.where(shared, 4, (1 << log2tu) >> (csx if comp else 0))
        off = (16 * z[0]) >> ((csx + csy) if comp else 0)
        squares = [(origin, 0)]
        if comp and fmt == 2:
            sub = (cbf >> (tr + 1)) & 1
            a, zz = np.nonzero(origin)
            low = np.zeros_like(origin)
            low[a, zz] = sub[a, zz + blk_parts[a, zz] // 2] != 0
            squares = [(origin & (sub != 0), 0), (low, 1)]
        for org, second in squares:
            a, zz = np.nonzero(org)
            sz = size[a, zz] * np.ones_like(a)
            out.append(np.stack([np.full(a.shape, comp, dtype=np.int64), a, off[zz] + second * sz * sz, sz], axis=1))
    return np.concatenate(out, axis=0) if out else np.zeros((0, 4), dtype=np.int64)


def block_mask(blocks, num_ctus, elems):
    """boolean [3][num_ctus, elems[comp]]: True at the level positions the blocks of coded_blocks() cover"""
    masks = [np.zeros((num_ctus, e), dtype=bool) for e in elems]
    for comp in range(3):
        b = blocks[blocks[:, 0] == comp]
        for sz in np.unique(b[:, 3]):
            s = b[b[:, 3] == sz]
            idx = s[:, 2][:, None] + np.arange(sz * sz)[None, :]
            masks[comp][s[:, 1][:, None], idx] = True
    return masks


def _group_any(flag, group_parts):
    """flag [n, parts] ORed over the aligned z-order group of group_parts[a, z] (a power of four) partitions that holds partition z"""
    n, parts = flag.shape
    out = np.zeros_like(flag)
    v = 1
    while v <= parts:
        sel = group_parts == v
        if sel.any():
            out = np.where(sel, np.repeat(flag.reshape(n, parts // v, v).any(axis=2), v, axis=1), out)
        v *= 4
    return out


def check_parser_invariants(meta, chroma_format, log2_ctu, slice_types):
    """What the standard's syntax (7.3.8, 7.4.9, 8.5.3.2.2) and HM's parser (TDecEntropy::xDecodeTransform, TDecSbac::parseQtCbf) guarantee
    of the per-partition arrays of a picture, whatever the stream; raises AssertionError naming the first rule broken.  meta: dict of
    [num_ctus, parts] arrays as in SynthPicture.meta_np; slice_types: HMGPU slice type per entry of the slice table (meta["slice_idx"]).
      1. depth, part_size, pred_mode, qp are uniform over a CU, which is aligned to its size
      2. motion vectors, reference indices and so the lists in use are uniform over each PU of the part_size geometry (eight shapes);
         intra CUs use no list; P slices use list 0 only, I slices none; an inter PU uses a list
      3. no 8x4 / 4x8 PU uses both lists
      4. AMP in CUs of 16 and more; NxN only in CUs of one size, the smallest in the picture (the minimum CU size), inter NxN only
         when that is above 8; intra CUs are 2Nx2N or NxN, intra NxN has tr_idx >= 1
      5. tr_idx is uniform over its leaf, the leaf lies inside the CU and is 4 .. 32 samples; an inter CU with no flag set has no tree: tr_idx 0, whatever its size
      6. cbf: no bit above tr_idx (4:2:2 chroma: tr_idx + 1); every bit d <= tr_idx is uniform over the depth-d node; bit d + 1 set implies
         bit d; luma bit d = OR over the node of the leaves' bits; chroma bit d is set wherever a deeper one of the node is; 4x4 luma leaves
         under subsampled chroma repeat their parent's chroma bit; 4:2:2: the bit below the block's own is uniform over each half of the
         block and the block's bit is the OR of the halves; 4:0:0 has no chroma flag
      7. chroma modes of intra partitions are planar, DC, horizontal, vertical, 34 or DM (36), and uniform over a CU unless 4:4:4 NxN"""
    fmt = 1 if chroma_format == 0 else chroma_format
    csx = 0 if fmt == 3 else 1
    g = {k: np.asarray(v).astype(np.int64) for k, v in meta.items() if k in (
        "depth", "part_size", "pred_mode", "qp", "tr_idx", "cbf_y", "cbf_u", "cbf_v", "mv0", "mv1", "ref_idx0", "ref_idx1", "intra_dir_l", "intra_dir_c")}
    depth, ps, tr = g["depth"], g["part_size"], g["tr_idx"]
    n, parts = depth.shape
    dec = ps != abi.SIZE_NONE
    z = np.arange(parts)[None, :]
    zx, zy = _zxy(parts)
    z_of = np.zeros((1 << (log2_ctu - 2), 1 << (log2_ctu - 2)), dtype=np.int64)
    z_of[zy, zx] = np.arange(parts)

    def at(a, first):
        return np.take_along_axis(a, first, axis=1)

    def same(a, first, where, what):
        bad = where & (at(a, first) != a) if a.ndim == 2 else where & (np.take_along_axis(a, first[:, :, None], axis=1) != a).any(axis=2)
        assert not bad.any(), "%s: %d partitions, first at CTU %d z %d" % ((what, int(bad.sum())) + tuple(int(v[0]) for v in np.nonzero(bad)))
    # 1
    assert (depth[dec] <= log2_ctu - 3).all(), "CU below 8x8"
    cu_parts = parts >> (2 * depth)
    cu_first = z & ~(cu_parts - 1)
    for k in ("depth", "part_size", "pred_mode", "qp"):
        same(g[k], cu_first, dec, "%s not uniform over the CU" % k)
    assert not (dec & ~at(dec, cu_first)).any()
    cu_log2 = log2_ctu - depth
    intra = dec & (g["pred_mode"] == abi.MODE_INTRA)
    inter = dec & ~intra
    # 2: the PU of every partition: its index and the z index of its first partition
    cu_w = 1 << (cu_log2 - 2)
    rx, ry = zx[None, :] % cu_w, zy[None, :] % cu_w
    q, h = cu_w // 4, cu_w // 2
    zero = np.zeros_like(rx)
    ox = np.select([ps == abi.SIZE_Nx2N, ps == abi.SIZE_NxN, ps == abi.SIZE_nLx2N, ps == abi.SIZE_nRx2N], [h, h, q, cu_w - q], cu_w)
    oy = np.select([ps == abi.SIZE_2NxN, ps == abi.SIZE_NxN, ps == abi.SIZE_2NxnU, ps == abi.SIZE_2NxnD], [h, h, q, cu_w - q], cu_w)
    pux, puy = np.where(rx >= ox, ox, zero), np.where(ry >= oy, oy, zero)      # the PU's origin inside the CU
    pu_first = z_of[(zy[None, :] - ry + puy), (zx[None, :] - rx + pux)]
    for k in ("mv0", "mv1", "ref_idx0", "ref_idx1"):
        same(g[k], pu_first, dec, "%s not uniform over the PU" % k)
    st = np.asarray(slice_types).reshape(-1)[np.asarray(meta["slice_idx"]).astype(np.int64) if "slice_idx" in meta else np.zeros(n, dtype=np.int64)][:, None]
    l0, l1 = g["ref_idx0"] >= 0, g["ref_idx1"] >= 0
    assert not (intra & (l0 | l1)).any(), "an intra CU uses a reference list"
    assert not (inter & ~(l0 | l1)).any(), "an inter PU uses no list"
    assert not (dec & l1 & (st != abi.B_SLICE)).any() and not (dec & (l0 | l1) & (st == abi.I_SLICE)).any(), "list not allowed by the slice type"
    assert not (inter & (st == abi.I_SLICE)).any(), "inter CU in an I slice"
    # 3
    assert not (inter & (cu_log2 == 3) & ((ps == abi.SIZE_2NxN) | (ps == abi.SIZE_Nx2N)) & l0 & l1).any(), "bi-predicted 8x4 / 4x8 PU"
    # 4
    amp = dec & (ps >= abi.SIZE_2NxnU) & (ps <= abi.SIZE_nRx2N)
    assert (cu_log2[amp] >= 4).all(), "AMP in an 8x8 CU"
    nxn = dec & (ps == abi.SIZE_NxN)
    if nxn.any():
        sizes = np.unique(cu_log2[nxn])
        assert sizes.size == 1 and sizes[0] == cu_log2[dec].min(), "NxN outside the minimum CU size"
        assert not (nxn & inter).any() or sizes[0] > 3, "inter NxN in 8x8 CUs"
    assert not (intra & (ps != abi.SIZE_2Nx2N) & ~nxn).any(), "intra CU neither 2Nx2N nor NxN"
    assert (tr[nxn & intra] >= 1).all(), "intra NxN without its transform split"
    # 5
    cbfs = [g["cbf_y"], g["cbf_u"], g["cbf_v"]]
    log2tu = cu_log2 - tr
    assert (log2tu[dec] >= 2).all(), "transform leaf below 4x4"
    leaf_parts = np.maximum(cu_parts >> (2 * tr), 1)
    same(tr, z & ~(leaf_parts - 1), dec, "tr_idx not uniform over its leaf")
    coded_cu = _group_any(dec & ((cbfs[0] | cbfs[1] | cbfs[2]) != 0), cu_parts)
    assert not (dec & coded_cu & (log2tu > 5)).any(), "transform leaf above 32x32"
    assert not (dec & ~coded_cu & ~intra & (tr != 0)).any(), "inter CU without a coded block (rqt_root_cbf 0) with a transform tree"
    # 6
    for comp, cbf in enumerate(cbfs):
        what = "cbf of component %d: " % comp
        if comp and chroma_format == 0:
            assert not cbf[dec].any(), what + "set in 4:0:0"
            continue
        top = tr + (1 if comp and fmt == 2 else 0)
        assert not (dec & ((cbf >> (top + 1)) != 0)).any(), what + "bit above the leaf's depth"
        shared = (leaf_parts == 1) & bool(comp and csx)
        own = tr - shared                                               # depth of the node that carries the block
        bit = [(cbf >> d) & 1 for d in range(6)]
        for d in range(4):
            node_parts = np.maximum(cu_parts >> (2 * d), 1)
            here = dec & (d <= own)
            same(bit[d], z & ~(node_parts - 1), here, what + "bit %d not uniform over its node" % d)
            below = dec & (d < tr)
            assert not (below & (bit[d + 1] > bit[d])).any(), what + "bit %d set under a clear bit %d" % (d + 1, d)
            deeper = _group_any(dec & (d < own) & (bit[d + 1] != 0), node_parts)
            assert not (dec & (d < own) & deeper & (bit[d] == 0)).any(), what + "node at depth %d clear above a set child" % d
            if comp == 0:
                leaves = _group_any(dec & (np.take_along_axis(np.stack(bit, axis=2), tr[:, :, None], axis=2)[:, :, 0] != 0), node_parts)
                assert not (here & (leaves != (bit[d] != 0))).any(), what + "bit %d is not the OR of its node's leaves" % d
        if comp and csx:
            rep = np.take_along_axis(np.stack(bit, axis=2), tr[:, :, None], axis=2)[:, :, 0]
            par = np.take_along_axis(np.stack(bit, axis=2), np.maximum(tr - 1, 0)[:, :, None], axis=2)[:, :, 0]
            assert not (dec & shared & (rep != par)).any(), what + "a 4x4 luma leaf does not repeat its parent's bit"
        if comp and fmt == 2:
            blk = np.where(shared, 4, leaf_parts)
            first = z & ~(blk - 1)
            sub = np.take_along_axis(np.stack(bit, axis=2), (tr + 1)[:, :, None], axis=2)[:, :, 0]
            up, lo = at(sub, first), at(sub, np.minimum(first + blk // 2, parts - 1))
            same(sub, np.where((z - first) >= blk // 2, first + blk // 2, first), dec, what + "square flag not uniform over its half")
            ownbit = np.take_along_axis(np.stack(bit, axis=2), tr[:, :, None], axis=2)[:, :, 0]
            assert not (dec & (ownbit != (up | lo))).any(), what + "block bit is not the OR of its squares' flags"
    # 7
    if "intra_dir_c" in g and chroma_format:
        ok = np.isin(g["intra_dir_c"], (0, 1, 10, 26, 34, 36))
        assert ok[intra].all(), "chroma mode outside HM's candidate set"
        same(g["intra_dir_c"], cu_first, intra & ~(nxn & (fmt == 3)), "chroma mode not uniform over the CU")
        same(g["intra_dir_c"], pu_first, intra, "chroma mode not uniform over the PU")
        same(g["intra_dir_l"], pu_first, intra, "luma mode not uniform over the PU")
        assert (g["intra_dir_l"][intra] <= 34).all()
