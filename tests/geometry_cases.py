"""The case tables and picture builders of tests/test_gpu_geometry.py: parity with the oracle at the extremes of picture, batch and slab
geometry -- pictures of one to a few CTUs, several of them per call, strips past 4096 and 8192 samples, contexts of 64 pictures (handles 32
to 63) and a slab of pictures beyond the reach of 32-bit offsets.  Nothing here needs a GPU: tests/test_geometry_cases_cpu.py holds every
case to what its name says before tests/test_gpu_geometry.py takes it to the device."""
import functools

import numpy as np

from libhm_amd import abi
from tests import synth

REGIONS = ("left", "right", "above", "below", "above left", "above right", "below left", "below right")      # (as tests/test_gpu_filter_margins.py)

# ------------------------------------------------------------------------------------------------ 1. pictures of at most a few CTUs
SMALL_SIZES = [(8, 8), (16, 8), (8, 16), (16, 16), (24, 40), (8, 64), (64, 8), (72, 8), (8, 72), (56, 56), (72, 64)]
DEPTHS = [(8, 8), (10, 10), (12, 12), (10, 8)]
# (width, height, log2_ctu, chroma format, luma depth, chroma depth): every size with every CTU size and chroma format, the depth pair
# rotating with all three
SMALL_CASES = [(w, h, c, f) + DEPTHS[(i + c + f) % 4] for i, (w, h) in enumerate(SMALL_SIZES) for c in (4, 5, 6) for f in (0, 1, 2, 3)]


def case_id(case):
    return "%dx%d-ctu%d-fmt%d-bd%d-%d" % (case[0], case[1], 1 << case[2], case[3], case[4], case[5])


def geometry(case):
    """(CTUs per row, CTU rows, valid columns of the last CTU column, valid rows of the last CTU row)"""
    w, h, c = case[0], case[1], 1 << case[2]
    return (w + c - 1) // c, (h + c - 1) // c, (w - 1) % c + 1, (h - 1) % c + 1


def _kw(case):
    return dict(chroma_format=case[3], log2_ctu=case[2], bit_depth_chroma=case[5])


@functools.lru_cache(maxsize=None)
def small_pictures(case):
    """((label, picture), ...) of one case, read only: a P and a B picture (references at handles 0 and 1) that both hold intra and inter
    CUs -- the first seed from 0 that gives both and, in the B picture, a PU that uses list 1 --; an 8x8 picture is one CU, so there it is one all-inter and one all-intra picture each"""
    w, h, _, _, bd, _ = case
    out = []
    for bi in (False, True):
        name = "B" if bi else "P"
        if (w, h) == (8, 8):
            for intra in (0.0, 1.0):
                out.append(("%s %s" % (name, "intra" if intra else "inter"),
                            synth.make_picture(w, h, bd, seed=3 + int(bi), bi=bi, intra_frac=intra, ref_handles=([0], [1]), **_kw(case))))
            continue
        for seed in range(40):
            p = synth.make_picture(w, h, bd, seed=seed, bi=bi, intra_frac=0.4, ref_handles=([0], [1]), **_kw(case))
            if p.intra.any() and (p.inside & ~p.intra).any() and (not bi or (p.meta_np["ref_idx1"] >= 0).any()):
                break
        out.append((name, p))
    return tuple(out)


def sao_everywhere(p, seed):
    """every CTU component that the drawn parameters leave off gets a band offset: SAO on in every CTU and coded component"""
    rng = np.random.RandomState(seed)
    raw = p.sao_raw
    comps = 1 if p.chroma_format == 0 else 3
    for a in range(raw.shape[0]):
        for comp in range(comps):
            if raw[a, comp, 0] == abi.SAO_OFF:
                band = int(rng.randint(0, 32))
                raw[a, comp, :] = 0
                raw[a, comp, 0], raw[a, comp, 1], raw[a, comp, 2] = abi.SAO_NEW, abi.SAO_BO, band
                for i in range(4):
                    raw[a, comp, 3 + (band + i) % 32] = int(rng.choice([-5, -2, 3, 6]))
    assert (raw[:, :comps, 0] == abi.SAO_NEW).all()
    return p


def with_bypass(p):
    """cu_transquant_bypass on every CU of the picture: no filter touches it (the fused filter's variant for exempt CUs)"""
    m = dict(p.meta_np)
    m["bypass"], m["ipcm"] = np.ones(m["depth"].shape, dtype=np.uint8), np.zeros(m["depth"].shape, dtype=np.uint8)
    p.meta_np, p.meta = m, abi.MetaHolder(m)
    return p


def pu_boxes(p):
    """[(CTU, PU index inside the CTU, x0, y0, x1, y1, CU x, CU y)] of the inter PUs of p: luma samples, x1 / y1 exclusive"""
    m = p.meta_np
    use = p.inside & (m["pred_mode"] == abi.MODE_INTER)
    cu = (1 << p.log2_ctu) >> m["depth"]
    out = []
    for a in range(p.num_ctus):
        for k in np.unique(p.pu_idx[a][use[a]]):
            sel = use[a] & (p.pu_idx[a] == k)
            x, y = p.px[a][sel], p.py[a][sel]
            c = int(cu[a][sel][0])
            out.append((a, int(k), int(x.min()), int(y.min()), int(x.max()) + 4, int(y.max()) + 4, int(x.min()) & ~(c - 1), int(y.min()) & ~(c - 1)))
    return out


def aim_at_margins(p, first_region, seed):
    """list-0 vectors of p set deliberately: PU k (in pu_boxes order) reads margin region (first_region + k) % 8 of its reference -- the
    whole PU lies 4 samples beyond the picture on the region's side(s), which TComDataCU::clipMv allows for every PU (a CU may lie up to
    CTU size + 7 samples before the picture and start up to 7 samples behind it) -- with a random quarter-sample phase.  Returns the
    regions aimed at."""
    rng = np.random.RandomState(seed)
    m = dict(p.meta_np)
    mv = np.array(m["mv0"])
    aimed = []
    for k, (a, pu, x0, y0, x1, y1, _, _) in enumerate(pu_boxes(p)):
        r = REGIONS[(first_region + k) % 8]
        dx = -x1 - 4 if "left" in r else (p.width - x0 + 4 if "right" in r else 0)
        dy = -y1 - 4 if "above" in r else (p.height - y0 + 4 if "below" in r else 0)
        sel = p.inside & (np.arange(p.num_ctus)[:, None] == a) & (p.pu_idx == pu) & (m["ref_idx0"] >= 0)
        mv[sel] = (4 * dx + int(rng.randint(0, 4)), 4 * dy + int(rng.randint(0, 4)))
        aimed.append(r)
    m["mv0"] = mv
    p.meta_np, p.meta = m, abi.MetaHolder(m)
    return aimed


def margin_readers(p):
    """tests/test_gpu_filter_margins.py's margin_readers for any chroma format: {"luma" / "chroma": {region: number of PUs of p whose
    window, after clipMv, holds samples of that margin region of the list-0 reference}} (4:0:0 counts the 4:2:0-shaped planes)"""
    m = p.meta_np
    w, h, ctu = p.width, p.height, 1 << p.log2_ctu
    use = p.inside & (m["pred_mode"] == 0) & (m["ref_idx0"] >= 0)
    cu = ctu >> m["depth"]
    cu_x, cu_y = p.px & ~(cu - 1), p.py & ~(cu - 1)
    mvx = np.minimum((w + 8 - cu_x - 1) << 2, np.maximum((-ctu - 8 - cu_x + 1) * 4, m["mv0"][:, :, 0]))
    mvy = np.minimum((h + 8 - cu_y - 1) << 2, np.maximum((-ctu - 8 - cu_y + 1) * 4, m["mv0"][:, :, 1]))
    pu = np.arange(p.num_ctus)[:, None] * 4096 + p.pu_idx
    out = {}
    for name, sx, sy in (("luma", 0, 0), ("chroma", p.csx, p.csy)):
        pw, ph = w >> sx, h >> sy
        x0, y0 = (p.px >> sx) + (mvx >> (2 + sx)), (p.py >> sy) + (mvy >> (2 + sy))
        x1, y1 = x0 + (4 >> sx) - 1, y0 + (4 >> sy) - 1
        reg = dict.fromkeys(REGIONS, 0)
        for k in np.unique(pu[use]):
            sel = use & (pu == k)
            xa, xb, ya, yb = x0[sel].min(), x1[sel].max(), y0[sel].min(), y1[sel].max()
            le, ri, ab, be = xa < 0, xb >= pw, ya < 0, yb >= ph
            rows_in, cols_in = yb >= 0 and ya < ph, xb >= 0 and xa < pw
            for r, hit in zip(REGIONS, (le and rows_in, ri and rows_in, ab and cols_in, be and cols_in, ab and le, ab and ri, be and le, be and ri)):
                reg[r] += bool(hit)
        out[name] = reg
    return out


def readers_union(pictures):
    """margin_readers summed over pictures"""
    total = {plane: dict.fromkeys(REGIONS, 0) for plane in ("luma", "chroma")}
    for p in pictures:
        for plane, reg in margin_readers(p).items():
            for r in REGIONS:
                total[plane][r] += reg[r]
    return total


MARGIN_VARIANTS = ("sao", "no sao", "bypass")


@functools.lru_cache(maxsize=None)
def margin_pictures(case):
    """({variant: picture A}, (pictures B ...)), read only.  A: a P picture from handle 0 -- with SAO on in every CTU and component (the
    fused filter writes its margins), with SAO off (the extension kernel does) and with cu_transquant_bypass on the whole picture (SAO
    on: the fused filter's variant for exempt CUs).  B: P pictures of inter CUs of 16x16 and 8x8 whose vectors aim_at_margins() has set,
    as many as it takes until every region has had every PU position's turn at least once: eight for a picture of one PU."""
    w, h, _, _, bd, _ = case
    a = {}
    for k, v in enumerate(MARGIN_VARIANTS):
        p = synth.make_picture(w, h, bd, seed=900 + k, ref_handles=([0], [0]), sao=(v != "no sao"), **_kw(case))
        if v != "no sao":
            sao_everywhere(p, 5 + k)
        if v == "bypass":
            with_bypass(p)
        a[v] = p
    bs = []
    first = 0
    while first < 8:
        b = synth.make_picture(w, h, bd, seed=951 + first, ref_handles=([0], [0]), mode_probs=(0, 0, 0.25, 0.75, 0), **_kw(case))
        aimed = aim_at_margins(b, first, 77 + first)
        bs.append(b)
        first += len(aimed)
    return a, tuple(bs)


# ------------------------------------------------------------------------------------------------ 2. several tiny pictures per call
BATCH_SIZES = [(8, 8, 6), (72, 8, 6), (24, 40, 4)]          # (width, height, log2_ctu): 1, 2 and 6 CTUs
BATCH_NS = [1, 2, 3, 5, 8, 16]
BATCH_BD = 10


@functools.lru_cache(maxsize=None)
def batch_pictures(w, h, log2_ctu, n, bi):
    """n pictures for one call, every one with a seed and an intra share of its own, SAO on everywhere (the batch takes the fused filter)"""
    pics = []
    for i in range(n):
        p = synth.make_picture(w, h, BATCH_BD, seed=0xB00 + 31 * i + n + int(bi), bi=bi, intra_frac=(0.0, 0.3, 0.6, 0.15)[i % 4],
                               ref_handles=([0], [1]), log2_ctu=log2_ctu)
        pics.append(sao_everywhere(p, i))
    return tuple(pics)


# ------------------------------------------------------------------------------------------------ 3. strips
# (width, height, log2_ctu, chroma format, luma depth, chroma depth, B picture)
STRIPS = [(8200, 64, 6, 1, 10, 10, False), (64, 4360, 6, 1, 8, 8, False), (16392, 8, 4, 1, 10, 10, True), (8, 8200, 4, 2, 8, 8, False),
          (8200, 72, 5, 3, 10, 10, True)]


def strip_id(s):
    return "%dx%d-ctu%d-fmt%d-%s" % (s[0], s[1], 1 << s[2], s[3], "B" if s[6] else "P")


@functools.lru_cache(maxsize=None)
def strip_pictures(s):
    """(the picture of all four stages, a B picture with vectors of up to 160 samples: beyond the short side of the strip in both
    directions, so into the left and right margins of a tall strip and the margins above and below of a wide one -- and, near the ends of
    the long side, into the other two)"""
    w, h, log2_ctu, fmt, bd, bdc, bi = s
    kw = dict(chroma_format=fmt, log2_ctu=log2_ctu, bit_depth_chroma=bdc, ref_handles=([0], [1]))
    p = synth.make_picture(w, h, bd, seed=0x57 + log2_ctu + fmt, bi=bi, intra_frac=0.3, **kw)
    far = synth.make_picture(w, h, bd, seed=0x58 + log2_ctu + fmt, bi=True, intra_frac=0.0, mv_range=160, **kw)
    return p, far


# ------------------------------------------------------------------------------------------------ 4. sixty-four pictures
DPB_CONTEXTS = [(64, 64, 6, 8), (72, 40, 4, 10)]            # (width, height, log2_ctu, bit depth)
DPB_UPLOADED = (0, 32)                                      # references uploaded: their reconstruction planes are the picture
DPB_DECODED_SAO = (31, 33, 63)                              # decoded from handle 0 and filtered with SAO: the SAO planes are
DPB_DECODED_NO_SAO = (62,)                                  # decoded and filtered in a picture without SAO


def dpb_sao_masks():
    """(low word, high word) of the pictures whose final planes are the SAO planes, as the motion-compensation kernels get them"""
    lo = sum(1 << hnd for hnd in DPB_DECODED_SAO if hnd < 32)
    hi = sum(1 << (hnd - 32) for hnd in DPB_DECODED_SAO if hnd >= 32)
    return lo, hi


@functools.lru_cache(maxsize=None)
def dpb_pictures(w, h, log2_ctu, bd):
    """({handle: picture decoded into it}, ((label, picture predicted from the handles 0, 31, 32, 33, 62, 63), ...))"""
    from tests import cu_shapes as cs
    dec = {}
    for hnd in DPB_DECODED_SAO + DPB_DECODED_NO_SAO:
        sao = hnd in DPB_DECODED_SAO
        p = synth.make_picture(w, h, bd, seed=0xD00 + hnd, intra_frac=0.2, ref_handles=([0], [0]), log2_ctu=log2_ctu, sao=sao)
        dec[hnd] = sao_everywhere(p, hnd) if sao else p
    kw = dict(log2_ctu=log2_ctu, intra_frac=0.15)
    small = dict(cs.SHAPES, mode_probs=(0, 0, 0.3, 0.7, 0))              # 8x8 CUs with 8x4 / 4x8 PUs: the cells kernels
    pics = [("P", synth.make_picture(w, h, bd, seed=0xD50, num_refs=2, ref_handles=([31, 32], [0]), **kw)),
            ("B", synth.make_picture(w, h, bd, seed=0xD51, bi=True, num_refs=2, l1_refs=2, ref_handles=([33, 62], [63, 0]), **kw)),
            ("P cells", synth.make_picture(w, h, bd, seed=0xD52, num_refs=2, ref_handles=([32, 63], [0]), **dict(kw, **small))),
            ("B cells", synth.make_picture(w, h, bd, seed=0xD53, bi=True, num_refs=2, l1_refs=2, ref_handles=([33, 62], [62, 33]), **dict(kw, **small)))]
    wp = synth.make_picture(w, h, bd, seed=0xD54, bi=True, num_refs=2, l1_refs=2, ref_handles=([63, 32], [33, 31]), **kw)
    set_weights(wp, 5)
    pics.append(("B weighted", wp))
    return dec, tuple(pics)


def set_weights(p, seed):
    """explicit weighted prediction per list, reference index and component"""
    sl = p.slice
    sl.weighted_pred = 1
    sl.wp_log2_denom[0], sl.wp_log2_denom[1] = 5, 4
    rng = np.random.RandomState(seed)
    for l in range(2):
        for r in range(2):
            for c in range(3):
                sl.wp_weight[l][r][c] = int((1 << sl.wp_log2_denom[1 if c else 0]) + rng.randint(-12, 13))
                sl.wp_offset[l][r][c] = int(rng.randint(-20, 21))


# ------------------------------------------------------------------------------------------------ 5. the plain-address windows
WIN_LIMIT = 0xffff0000                                      # bytes of a slab of pictures from which the kernels take 64-bit addresses
PLAIN = (4096, 2368, 6, 10)                                 # (width, height, log2_ctu, bit depth), 4:2:0, 64 pictures
PLAIN_PICTURES = 64


def plane_bytes(seq):
    """(bytes of the luma plane, bytes of the plane that holds Cb and Cr in turns) of a device picture: margins of 128 samples beside and
    80 rows above and below the CTU-aligned picture, rows padded to 64 samples plus 64, eight spare rows, each plane padded to 256 bytes"""
    fmt = 1 if seq.chroma_format == 0 else seq.chroma_format
    csx, csy = (0 if fmt == 3 else 1), (1 if fmt == 1 else 0)
    ctu = 1 << seq.log2_ctu_size
    rows = (seq.height + ctu - 1) // ctu * ctu
    up = lambda v, a: (v + a - 1) // a * a
    luma = (up(seq.width, 64) + 2 * 128 + 64) * (rows + 2 * 80 + 8) * 2
    chroma = 2 * (up(seq.width >> csx, 64) + 2 * (128 >> csx) + 64) * ((rows >> csy) + 2 * (80 >> csy) + 8) * 2
    return up(luma, 256), up(chroma, 256)


def plane_set_bytes(seq):
    """bytes of one set of planes of a device picture (include/hmgpu.h, hmgpu_picture_device_region)"""
    return sum(plane_bytes(seq))


def slab_bytes(seq):
    """all pictures of a context: a reconstruction set and, behind it, an SAO set each"""
    return 2 * plane_set_bytes(seq) * seq.max_pictures


def straddling_handle(seq):
    """the handle whose planes hold the byte at offset 4 GiB of the slab"""
    return (1 << 32) // (2 * plane_set_bytes(seq))


def plain_sao_picture(size=None):
    """the picture decoded into the last handle and finished with SAO, so that its final planes are its SAO set -- whose luma plane
    holds the byte at offset 4 GiB of the slab (test_plain_address_geometry_is_the_smallest_past_the_limit)"""
    w, h, log2_ctu, bd = PLAIN
    if size is not None:
        w, h = size
    return synth.make_picture(w, h, bd, seed=0xA9, ref_handles=([0], [0]), log2_ctu=log2_ctu, intra_frac=0.0, cbf_prob=0.2)


def plain_pictures(size=None):
    """((label, picture), ...): P and B with vectors of up to 64 samples, P with explicit weights, P with vectors of up to 160 samples (at
    the borders: into the margins) -- the four variants of each motion-compensation kernel -- predicted from handle 0, the last handle
    that lies wholly below 4 GiB and the last one, which straddles it.  size: another (width, height), for the census"""
    w, h, log2_ctu, bd = PLAIN
    if size is not None:
        w, h = size
    last, below = PLAIN_PICTURES - 1, PLAIN_PICTURES - 2
    kw = dict(log2_ctu=log2_ctu, intra_frac=0.0, cbf_prob=0.3, sao=False)
    pics = [("P", synth.make_picture(w, h, bd, seed=0xA0, num_refs=2, ref_handles=([below, last], [0]), **kw)),
            ("B", synth.make_picture(w, h, bd, seed=0xA1, bi=True, num_refs=2, l1_refs=2, ref_handles=([0, below], [last, below]), **kw)),
            ("P weighted", synth.make_picture(w, h, bd, seed=0xA2, num_refs=2, ref_handles=([last, 0], [0]), **kw)),
            ("P margins", synth.make_picture(w, h, bd, seed=0xA3, num_refs=2, ref_handles=([below, last], [0]), mv_range=160, **kw))]
    set_weights(pics[2][1], 6)
    return tuple(pics)


# ------------------------------------------------------------------------------------------------ 6. exports on sub-CTU pictures
EXPORT_CASES = [(8, 8, 4), (8, 8, 6), (24, 40, 4)]           # (width, height, log2_ctu)


@functools.lru_cache(maxsize=None)
def export_pictures(w, h, log2_ctu, fmt):
    """three B pictures of 10 bits from the references at handles 0 and 1 for the exports: every block coded; all inter, all intra, and
    30 % intra CUs (an 8x8 picture is one CU)"""
    return tuple(synth.make_picture(w, h, 10, seed=0xE0 + i + log2_ctu, bi=True, intra_frac=(0.0, 1.0, 0.3)[i], num_refs=2, cbf_prob=1.0,
                                    ref_handles=([0, 1], [1]), chroma_format=fmt, log2_ctu=log2_ctu) for i in range(3))
