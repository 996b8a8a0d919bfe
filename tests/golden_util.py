"""Load the golden fixtures (tests/golden/*.npz, made by oracle/make_golden.py from the real HM) into the ABI structs."""
import hashlib
import os

import numpy as np

from libhm_amd import abi

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STREAMS = ["ldp_main8_416x240", "ra_main10_208x120", "ldp_main10_208x120", "intra_main10_208x120", "ldp_cip_main10_208x120",
           "ldp_wp_main10_208x120", "ra_wp_main8_208x120", "ldp_sl_main10_208x120", "ldp_sldef_main8_208x120", "ldp_tiles_main10_832x128", "ldp_lossless_main10_208x120", "ldp_pcm_main8_208x120"]
# 4:2:2 / 4:4:4, the latter with cross-component prediction: range-extension configurations, inter and intra
STREAMS_CF = ["ldb_444_ccp_main8_208x120", "intra_444_ccp_main10_208x120", "ldb_422_main10_208x120", "intra_422_main8_208x120"]
# bitstream + encoder reconstruction only (oracle/make_golden.py LITE): syntax HM 16.0's own decoder cannot be run on, or variants
LITE = ["ldp_slices_main8_208x120", "ldp_depslices_main10_208x120", "ldp_wpp_main10_416x240", "ldp_wpp_depslices_main8_416x240",
        "ldp_dqp_main10_208x120", "ra_cra_main8_208x120", "ldp_ctu32_main8_208x120", "ldp_ctu16_main10_208x120", "ldp_crop_main8_204x116",
        "ldp_tileslices_main10_832x128", "ldb_main8_208x120", "ldp_cqp_vui_main10_208x120", "ldp_nosao_main10_208x120",
        "ldp_nodbk_main8_208x120", "ldp_nofilters_main8_208x120", "ra_notmvp_main8_208x120", "ldp_mincu16_main10_208x112",
        "intra_qp12_main8_208x120", "ra_parmrg4_main8_208x120", "ldp_tudepth1_main10_208x120", "ldp_maxtb16_noamp_main8_208x120",
        "ldp_nots_nosdh_main10_208x120", "ldp_ctu32_mincu16_main8_224x128", "ldp_qpneg_main10_208x120", "ldp_qp48_main8_208x120",
        "ldp_slicedbk_main10_208x120", "ldp_qgctu_main8_208x120", "ldp_tilesexp_main10_832x192", "ldp_bd10_8_208x120", "ldp_bd8_10_208x120",
        # sps_range_extension() tools in 4:2:0: rotation, implicit / explicit RDPCM, single significance context, persistent Rice
        "ldb_rext420_main8_208x120", "ldb_rext420_lossless_main8_208x120", "intra_rext420_main8_208x120",
        "intra_rext420_lossless_main8_208x120", "ldb_rext420_mixed_main10_208x120", "ldb_rext420_ts32_nosmooth_main8_208x120",
        "ldb_rext420_wp_hp_main10_208x120", "ldb_rext420_wpp_depslices_main8_416x240", "ldb_rext420_tileslices_main10_832x128",
        # monochrome (4:0:0)
        "ldb_mono_rext_main8_208x120", "ldb_mono_wp_crop_main10_204x116", "intra_mono_main8_208x120"]
# 4:2:2 / 4:4:4 variants: without cross-component prediction, lossless (rotation + RDPCM on full-size chroma), transform skip up to 32x32
# chroma blocks, cross-component prediction between different bit depths, 16- and 32-sample CTUs, weighted prediction, wavefronts + slices,
# scaling lists
LITE_CF = ["ldb_444_main10_208x120", "ldb_444_lossless_main8_208x120", "intra_444_ts32_nosmooth_main8_208x120", "ldb_444_ccp_bd10_8_208x120",
           "ldb_444_ctu16_main8_208x120", "ldb_422_lossless_main8_208x120", "ldb_422_wp_main10_208x120", "ldb_422_wpp_depslices_main8_416x240",
           "intra_422_qp12_main10_208x120", "ldb_422_ctu32_main8_208x120",
           # scaling lists from a file in 4:4:4: coded 32x32 chroma blocks, de-quantised with the lists HM copies from the 16x16 chroma lists
           "ldb_444_sl_main8_208x120"]
# bit depth 12, 4:2:0 (oracle/make_golden.py: CF420 streams)
STREAMS_BD12 = ["ldb_main12_208x120", "intra_main12_208x120"]
LITE_BD12 = ["ldb_ts32_main12_208x120", "ldb_wp_main12_208x120", "ldb_sl_main12_208x120", "intra_qp4_main12_208x120", "ldb_bd12_10_208x120",
             "ldb_444_ccp_main12_208x120", "ldb_422_main12_208x120"]
# directional content made for HM's encoder to pick every luma intra mode at 16x16 and 32x32, with and without strong intra smoothing
# (oracle/make_golden.py STREAMS_INTRA; tests/test_intra_census_cpu.py counts what they hold)
STREAMS_INTRA = ["imodes_large_main8_416x256", "imodes_large_main12_416x256", "imodes_large_a_444_ccp_main10_416x256",
                 "imodes_large_b_444_ccp_main10_416x256", "imodes_large_c_444_ccp_main10_416x256", "imodes_large_a_422_main8_416x256",
                 "imodes_large_b_422_main8_416x256", "imodes_all_main10_416x240", "imodes_cip_ldp_main10_224x128",
                 "imodes_nosmooth_422_main12_224x128"]
STREAMS_INTRA_420 = [n for n in STREAMS_INTRA if "_444" not in n and "_422" not in n]
STREAMS_EXT = STREAMS_CF + STREAMS_BD12          # beyond Main / Main10: other chroma formats, 12 bits
LITE_EXT = LITE_CF + LITE_BD12
# HM-encoded streams rewritten at the bit level (oracle/make_surgery.py) for syntax HM's encoder never writes; expected pictures = HM's own
# DECODER on the rewritten stream: pps_scaling_list_data; long-term reference pictures + ref_pic_list_modification
SURGERY = ["surgery_ppssl_main8_208x120", "surgery_ltr_rplm_main10_208x120"]
_cache = {}


def load(name):
    if name not in _cache:
        _cache[name] = np.load(os.path.join(GOLD, name + ".npz"))
    return _cache[name]


class Picture:
    """One decoded picture of a fixture stream: ABI inputs + HM's planes at the three stages."""

    def __init__(self, z, idx, poc_to_handle):
        k = "pic%02d_" % idx
        info = z[k + "info"]
        (self.width, self.height, self.bd_y, self.bd_c, self.poc, self.slice_type, self.num_ctus, self.ctus_w, self.parts,
         self.ctu_size, self.num_slices, self.use_sao, self.lf_across_tiles) = (int(v) for v in info[:13])
        self.index = idx
        s0 = z[k + "slices"][0]
        self.seq = abi.make_seq(self.width, self.height, self.bd_y, self.bd_c, log2_ctu=int(np.log2(self.ctu_size)), max_pictures=12,
                                strong_intra_smoothing=int(s0[25]) if int(s0[27]) else 1, range_ext_flags=int(s0[28]))
        self.chroma_format = int(info[13])
        self.seq.chroma_format = self.chroma_format
        self.csx, self.csy = (0 if self.chroma_format == 3 else 1), (1 if self.chroma_format in (0, 1) else 0)
        self.slices = []
        self.ref_pocs = set()
        wp_all = z[k + "wp"] if (k + "wp") in z.files else None
        self.scaling_lists = None
        if (k + "scaling_lists") in z.files and int(z[k + "scaling_lists"][0]):
            raw = z[k + "scaling_lists"]
            self.scaling_lists = abi.ScalingLists()
            coef, dc = raw[1:1 + 1536].reshape(4, 6, 64), raw[1 + 1536:].reshape(4, 6)
            for sz in range(4):
                for l in range(6):
                    self.scaling_lists.dc[sz][l] = int(dc[sz, l]) if sz >= 2 else 16
                    for i in range(64):
                        self.scaling_lists.coef[sz][l][i] = int(coef[sz, l, i])
        for si, s in enumerate(z[k + "slices"]):
            refs, pocs = [], []
            for l in range(2):
                p = [int(v) for v in s[32 + 16 * l: 32 + 16 * l + int(s[12 + l])]]
                pocs.append(p)
                refs.append([poc_to_handle[v] for v in p])
                self.ref_pocs.update(p)
            self.slices.append(abi.make_slice(int(s[0]), refs, pocs, cb_qp_offset=int(s[2] + s[4]), cr_qp_offset=int(s[3] + s[5]),
                                              pps_cb=int(s[2]), pps_cr=int(s[3]), deblocking_disable=int(s[6]),
                                              beta_offset_div2=int(s[7]), tc_offset_div2=int(s[8]), lf_across_slices=int(s[9])))
            self.slices[-1].constrained_intra_pred = int(s[26])
            self.slices[-1].lf_across_tiles = self.lf_across_tiles
            if self.scaling_lists is not None:
                import ctypes
                self.slices[-1].scaling_lists = ctypes.pointer(self.scaling_lists)
            if wp_all is not None and wp_all[si][0]:
                wp, sl = wp_all[si], self.slices[-1]
                sl.weighted_pred = 1
                sl.wp_log2_denom[0], sl.wp_log2_denom[1] = int(wp[1]), int(wp[2])
                for l in range(2):
                    for r in range(16):
                        for c in range(3):
                            sl.wp_weight[l][r][c] = int(wp[3 + (l * 16 + r) * 3 + c])
                            sl.wp_offset[l][r][c] = int(wp[99 + (l * 16 + r) * 3 + c])
            else:
                assert s[14] == 0 or int(s[0]) != 1      # weighted_pred_flag on a P slice needs its table
        m = {n: z[k + "meta_" + n] for n in ("depth", "part_size", "pred_mode", "qp", "tr_idx", "cbf_y", "cbf_u", "cbf_v", "ts_y",
                                             "ts_u", "ts_v", "mv0", "mv1", "ref_idx0", "ref_idx1", "intra_dir_l", "intra_dir_c",
                                             "bypass", "ipcm")}
        if (k + "meta_ccp_u") in z.files and int(s0[29]):                 # cross-component prediction weights (4:4:4 streams that use the tool)
            m["ccp_u"], m["ccp_v"] = z[k + "meta_ccp_u"], z[k + "meta_ccp_v"]
        m["slice_idx"] = z[k + "meta_slice_idx"].astype(np.uint16)
        if (k + "tile_idx") in z.files:
            m["tile_idx"] = z[k + "tile_idx"].astype(np.uint16)
        self.meta_np = m
        self.meta = abi.MetaHolder(m)
        pcm = [z[k + "pcm%d" % c] for c in range(3)] if (k + "pcm0") in z.files else None
        self.coeffs = abi.CoeffHolder(z[k + "coeff0"], z[k + "coeff1"], z[k + "coeff2"], pcm)
        if (k + "pcm_info") in z.files:
            pi = z[k + "pcm_info"]
            self.seq.pcm_bit_depth_luma, self.seq.pcm_bit_depth_chroma = int(pi[0]), int(pi[1])
            self.seq.pcm_loop_filter_disable = int(pi[2] and pi[3])
        self.sao_raw = z[k + "sao_raw"]
        self.sao_rec = z[k + "sao_rec"]
        self.pre = [z[k + "pre%d" % c] for c in range(3)]
        self.dbk = [z[k + "dbk%d" % c] for c in range(3)]
        self.fin = [z[k + "fin%d" % c] for c in range(3)]
        self.md5 = bytes(z[k + "md5"])
        self.crc = z[k + "crc"]              # decoded-picture-hash CRC (6 bytes) and checksum (12 bytes), TComPicYuvMD5.cpp
        self.checksum = z[k + "checksum"]
        self.pp = abi.make_pic_params(sao_enabled=self.use_sao, lf_across_tiles=self.lf_across_tiles)

    def inter_mask(self, comp):
        """boolean mask of the plane: True where the sample belongs to an inter-coded, decoded CU"""
        sx, sy = (self.csx, self.csy) if comp else (0, 0)
        mask = np.zeros((self.height >> sy, self.width >> sx), dtype=bool)
        pm = self.meta_np["pred_mode"]
        ps = self.meta_np["part_size"]
        pw = self.ctu_size // 4
        for a in range(self.num_ctus):
            cx, cy = (a % self.ctus_w) * self.ctu_size, (a // self.ctus_w) * self.ctu_size
            for zidx in range(self.parts):
                x = sum(((zidx >> (2 * b)) & 1) << b for b in range(8))
                y = sum(((zidx >> (2 * b + 1)) & 1) << b for b in range(8))
                px, py = cx + 4 * x, cy + 4 * y
                if px >= self.width or py >= self.height:
                    continue
                if pm[a, zidx] == abi.MODE_INTER and ps[a, zidx] != abi.SIZE_NONE:
                    mask[py >> sy:(py >> sy) + (4 >> sy), px >> sx:(px >> sx) + (4 >> sx)] = True
        return mask


def stream_pictures(name):
    z = load("stream_" + name)
    n = int(z["num_pics"][0])
    poc_to_handle = {}
    pics = []
    for i in range(n):
        poc = int(z["pic%02d_info" % i][4])
        p = Picture(z, i, poc_to_handle)
        poc_to_handle[poc] = i          # picture handle == decode index
        pics.append(p)
    return pics


def hm_md5(planes, bit_depths):
    """MD5 per plane the way TComPicYuvMD5.cpp:44-84,183-205 feeds libmd5: raster order, visible area,
    1 byte/sample for bit depth <= 8 else 2 bytes little-endian."""
    out = b""
    for p, bd in zip(planes, bit_depths):
        data = p.astype(np.uint8).tobytes() if bd <= 8 else p.astype("<u2").tobytes()
        out += hashlib.md5(data).digest()
    return out
