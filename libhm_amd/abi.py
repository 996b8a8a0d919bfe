"""ctypes mirror of include/hmgpu.h (the C ABI of libhmgpu.so) + helpers to fill the structs from numpy arrays.

Pure declarations: no compute here.  Field order and types must match include/hmgpu.h exactly
(tests/test_abi.py cross-checks sizes against the compiled library).
"""
import ctypes as C

import numpy as np

HMGPU_OK, HMGPU_EINVAL, HMGPU_EDEVICE, HMGPU_EUNSUPPORTED, HMGPU_ENOMEM = 0, 1, 2, 3, 4
MAX_REF = 16
NO_PIC = -1
B_SLICE, P_SLICE, I_SLICE = 0, 1, 2
MODE_INTER, MODE_INTRA = 0, 1
SIZE_2Nx2N, SIZE_2NxN, SIZE_Nx2N, SIZE_NxN, SIZE_2NxnU, SIZE_2NxnD, SIZE_nLx2N, SIZE_nRx2N, SIZE_NONE = range(9)
SAO_OFF, SAO_NEW, SAO_MERGE = 0, 1, 2
SAO_EO_0, SAO_EO_90, SAO_EO_135, SAO_EO_45, SAO_BO = range(5)
NUM_KERNELS = 13

STAGE_DEBLOCK_VER, STAGE_DEBLOCK_HOR, STAGE_SAO, STAGE_RECON = 1, 2, 4, 8


class SeqParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("bit_depth_luma", C.c_int32), ("bit_depth_chroma", C.c_int32),
                ("chroma_format", C.c_int32), ("log2_ctu_size", C.c_int32), ("max_pictures", C.c_int32),
                ("pcm_loop_filter_disable", C.c_int32), ("strong_intra_smoothing", C.c_int32), ("pcm_bit_depth_luma", C.c_int32), ("pcm_bit_depth_chroma", C.c_int32),
                ("range_ext_flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class ScalingLists(C.Structure):
    _fields_ = [("coef", ((C.c_int32 * 64) * 6) * 4), ("dc", (C.c_int32 * 6) * 4)]


class SliceParams(C.Structure):
    _fields_ = [("slice_type", C.c_int32), ("cb_qp_offset", C.c_int32), ("cr_qp_offset", C.c_int32),
                ("pps_cb_qp_offset", C.c_int32), ("pps_cr_qp_offset", C.c_int32), ("deblocking_disable", C.c_int32),
                ("beta_offset_div2", C.c_int32), ("tc_offset_div2", C.c_int32), ("lf_across_slices", C.c_int32),
                ("weighted_pred", C.c_int32), ("lf_across_tiles", C.c_int32), ("num_ref_idx", C.c_int32 * 2),
                ("ref_pic", (C.c_int32 * MAX_REF) * 2), ("ref_poc", (C.c_int32 * MAX_REF) * 2), ("constrained_intra_pred", C.c_int32), ("reserved", C.c_int32 * 4),
                ("wp_log2_denom", C.c_int32 * 2), ("wp_weight", ((C.c_int16 * 3) * MAX_REF) * 2), ("wp_offset", ((C.c_int16 * 3) * MAX_REF) * 2),
                ("scaling_lists", C.POINTER(ScalingLists))]


class CtuMeta(C.Structure):
    _fields_ = [("depth", C.c_void_p), ("part_size", C.c_void_p), ("pred_mode", C.c_void_p), ("qp", C.c_void_p),
                ("tr_idx", C.c_void_p), ("cbf", C.c_void_p * 3), ("transform_skip", C.c_void_p * 3),
                ("mv", C.c_void_p * 2), ("ref_idx", C.c_void_p * 2), ("intra_dir", C.c_void_p * 2),
                ("transquant_bypass", C.c_void_p), ("ipcm", C.c_void_p), ("slice_idx", C.c_void_p), ("tile_idx", C.c_void_p),
                ("ccp_alpha", C.c_void_p * 2)]


class CtuMetaOut(CtuMeta):
    """hmgpu_ctu_meta_out: hmgpu_ctu_meta's fields, writable (hmgpu_unpack_input); same layout"""


class Coeffs(C.Structure):
    _fields_ = [("level", C.c_void_p * 3), ("pcm_sample", C.c_void_p * 3), ("ctu_level_start", C.c_void_p * 3)]


class SaoParam(C.Structure):
    _fields_ = [("mode_idc", C.c_int32), ("type_idc", C.c_int32), ("type_aux_info", C.c_int32), ("offset", C.c_int32 * 32)]


class PicParams(C.Structure):
    _fields_ = [("lf_across_tiles", C.c_int32), ("sao_enabled", C.c_int32), ("sao_offset_shift_luma", C.c_int32),
                ("sao_offset_shift_chroma", C.c_int32), ("reserved", C.c_int32 * 8)]


class PictureJob(C.Structure):
    _fields_ = [("pic", C.c_int32), ("num_slices", C.c_int32), ("slices", C.POINTER(C.POINTER(SliceParams))),
                ("meta", C.POINTER(CtuMeta)), ("coeffs", C.POINTER(Coeffs))]


class PackedJob(C.Structure):
    _fields_ = [("pic", C.c_int32), ("num_slices", C.c_int32), ("slices", C.POINTER(C.POINTER(SliceParams))),
                ("blob", C.c_void_p), ("bytes", C.c_size_t), ("pcm_sample", C.c_void_p * 3)]


class FilterJob(C.Structure):
    _fields_ = [("pic", C.c_int32), ("pp", C.POINTER(PicParams)), ("sao", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double * NUM_KERNELS), ("kernel_launches", C.c_uint64 * NUM_KERNELS),
                ("intra_partitions", C.c_uint64), ("inter_partitions", C.c_uint64), ("coded_tus", (C.c_uint64 * 3) * 4)]


EXPORT_PLANAR, EXPORT_SEMIPLANAR, EXPORT_RGB = 0, 1, 2


class ExportDesc(C.Structure):
    _fields_ = [("layout", C.c_int32), ("bit_depth", C.c_int32 * 2), ("bytes_per_sample", C.c_int32), ("msb_aligned", C.c_int32),
                ("crop", C.c_int32 * 4), ("matrix", C.c_int32), ("full_range", C.c_int32), ("reserved", C.c_int32 * 6)]


class ExportPlan(C.Structure):
    _fields_ = [("planes", C.c_int32), ("width", C.c_int32 * 3), ("height", C.c_int32 * 3), ("row_bytes", C.c_int32 * 3),
                ("coef", C.c_int32 * 16)]


SCALE_NEAREST, SCALE_BILINEAR, SCALE_BICUBIC, SCALE_AREA = 0, 1, 2, 3


class ExportScale(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("filter", C.c_int32), ("reserved", C.c_int32 * 5)]


def make_export_scale(width, height, filter=SCALE_BILINEAR):
    s = ExportScale()
    s.width, s.height, s.filter = width, height, filter
    return s


SAMPLE_UINT, SAMPLE_F16, SAMPLE_BF16, SAMPLE_F32 = 0, 1, 2, 3
EXPORT_MAX_BATCH = 16


class ExportTensor(C.Structure):
    _fields_ = [("sample_type", C.c_int32), ("scale", C.c_float * 3), ("bias", C.c_float * 3), ("reserved", C.c_int32 * 5)]


def make_export_tensor(sample_type, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
    t = ExportTensor()
    t.sample_type = sample_type
    for k in range(3):
        t.scale[k], t.bias[k] = float(scale[k]), float(bias[k])
    return t


class ExportWindow(C.Structure):
    _fields_ = [("crop", C.c_int32 * 4), ("flip", C.c_int32), ("reserved", C.c_int32 * 3)]


def make_export_window(crop, flip=False):
    """crop: (left, right, top, bottom) luma samples removed from the coded picture; flip: mirror each output row"""
    w = ExportWindow()
    for i in range(4):
        w.crop[i] = int(crop[i])
    w.flip = 1 if flip else 0
    return w


PIXEL_RGB, PIXEL_BGR, PIXEL_RGBA, PIXEL_BGRA, PIXEL_ARGB, PIXEL_ABGR = range(6)


class ExportPixel(C.Structure):
    _fields_ = [("order", C.c_int32), ("alpha", C.c_int32), ("alpha_value", C.c_float), ("reserved", C.c_int32 * 5)]


def make_export_pixel(order, alpha=-1, alpha_value=1.0):
    """order: PIXEL_*; alpha: the A code value of unsigned elements (-1: opaque); alpha_value: the A of float elements"""
    p = ExportPixel()
    p.order, p.alpha, p.alpha_value = int(order), int(alpha), float(alpha_value)
    return p


COLOUR_MAX_LUTS = 8


class ColourLutDesc(C.Structure):
    _fields_ = [("depth", C.c_int32), ("size", C.c_int32), ("has_shaper", C.c_int32), ("reserved", C.c_int32 * 5)]


def make_colour_lut_desc(depth, size, has_shaper):
    """depth: the code values' bits in and out (8 .. 16); size: nodes per axis (0: shaper only, 2 .. 65)"""
    d = ColourLutDesc()
    d.depth, d.size, d.has_shaper = int(depth), int(size), int(bool(has_shaper))
    return d


CHROMA_REPLICATE, CHROMA_LINEAR = 0, 1
CHROMA_FILTERS = {"replicate": CHROMA_REPLICATE, "linear": CHROMA_LINEAR}


class ExportChroma(C.Structure):
    _fields_ = [("filter", C.c_int32), ("loc", C.c_int32), ("reserved", C.c_int32 * 6)]


def make_export_chroma(filter=CHROMA_LINEAR, loc=0):
    """filter: CHROMA_* or its name; loc: chroma_sample_loc_type 0 .. 5 (H.265 figure E.1)"""
    c = ExportChroma()
    c.filter, c.loc = int(CHROMA_FILTERS.get(filter, filter)), int(loc)
    return c


def chroma_stage(chroma, chroma_loc, default_loc=0):
    """chroma= / chroma_loc= of the Python exports: None for "replicate" (the existing entries), else the ExportChroma of the new one;
    chroma_loc None: default_loc"""
    if chroma not in CHROMA_FILTERS:
        raise ValueError("chroma: one of %s" % sorted(CHROMA_FILTERS))
    if chroma == "replicate":
        return None
    return make_export_chroma(chroma, default_loc if chroma_loc is None else chroma_loc)


DOWN_DROP, DOWN_LINEAR = 0, 1
DOWN_FILTERS = {"drop": DOWN_DROP, "linear": DOWN_LINEAR}
CHROMA_FORMATS = {"400": 0, "420": 1, "422": 2, "444": 3}


class ExportFormat(C.Structure):
    _fields_ = [("chroma_format", C.c_int32), ("up", C.c_int32), ("down", C.c_int32), ("loc", C.c_int32), ("reserved", C.c_int32 * 4)]


def make_export_format(chroma_format, up=CHROMA_REPLICATE, down=DOWN_DROP, loc=0):
    """chroma_format: 0 .. 3 or "400" / "420" / "422" / "444"; up: CHROMA_* or its name; down: DOWN_* or its name; loc:
    chroma_sample_loc_type 0 .. 5 of the 4:2:0 side of the conversion"""
    f = ExportFormat()
    f.chroma_format = int(CHROMA_FORMATS.get(chroma_format, chroma_format))
    f.up, f.down, f.loc = int(CHROMA_FILTERS.get(up, up)), int(DOWN_FILTERS.get(down, down)), int(loc)
    return f


def format_stage(chroma_format, chroma, chroma_down, chroma_loc, default_loc=0):
    """chroma_format= / chroma= / chroma_down= / chroma_loc= of the Python exports: None for chroma_format None (the existing
    entries), else the ExportFormat of the format export; chroma_loc None: default_loc"""
    if chroma_format is None:
        if chroma_down != "drop":
            raise ValueError("chroma_down needs chroma_format=")
        return None
    if not isinstance(chroma_format, int) and chroma_format not in CHROMA_FORMATS:
        raise ValueError("chroma_format: None, 0 .. 3 or one of %s" % sorted(CHROMA_FORMATS))
    if chroma not in CHROMA_FILTERS:
        raise ValueError("chroma: one of %s" % sorted(CHROMA_FILTERS))
    if chroma_down not in DOWN_FILTERS:
        raise ValueError("chroma_down: one of %s" % sorted(DOWN_FILTERS))
    return make_export_format(chroma_format, chroma, chroma_down, default_loc if chroma_loc is None else chroma_loc)


# packed YUV (include/hmgpu.h "packed YUV"): per word format its chroma format, depth, bytes per element of the returned tensor and A's range
YUVPACK_UYVY, YUVPACK_YUY2, YUVPACK_Y210, YUVPACK_Y216, YUVPACK_V210, YUVPACK_AYUV, YUVPACK_Y410, YUVPACK_Y416 = range(8)
YUVPACKS = {"uyvy": YUVPACK_UYVY, "yuy2": YUVPACK_YUY2, "y210": YUVPACK_Y210, "y216": YUVPACK_Y216, "v210": YUVPACK_V210,
            "ayuv": YUVPACK_AYUV, "y410": YUVPACK_Y410, "y416": YUVPACK_Y416}
YUVPACK_CHROMA = {YUVPACK_UYVY: 2, YUVPACK_YUY2: 2, YUVPACK_Y210: 2, YUVPACK_Y216: 2, YUVPACK_V210: 2, YUVPACK_AYUV: 3, YUVPACK_Y410: 3,
                  YUVPACK_Y416: 3}
YUVPACK_DEPTH = {YUVPACK_UYVY: 8, YUVPACK_YUY2: 8, YUVPACK_Y210: 10, YUVPACK_Y216: 16, YUVPACK_V210: 10, YUVPACK_AYUV: 8, YUVPACK_Y410: 10,
                 YUVPACK_Y416: 16}
YUVPACK_ELEMENT = {YUVPACK_UYVY: 1, YUVPACK_YUY2: 1, YUVPACK_Y210: 2, YUVPACK_Y216: 2, YUVPACK_V210: 4, YUVPACK_AYUV: 1, YUVPACK_Y410: 4,
                   YUVPACK_Y416: 2}


def yuvpack_code(yuv):
    """HMGPU_YUVPACK_* of a name ("uyvy" ... "y416") or of the code itself"""
    if isinstance(yuv, int):
        return yuv
    if not isinstance(yuv, str) or yuv.lower() not in YUVPACKS:
        raise ValueError("yuv: one of %s" % sorted(YUVPACKS))
    return YUVPACKS[yuv.lower()]


class ExportYuvPack(C.Structure):
    _fields_ = [("format", C.c_int32), ("alpha", C.c_int32), ("reserved", C.c_int32 * 6)]


def make_export_yuvpack(yuv, alpha=0):
    """yuv: YUVPACK_* or its name; alpha: the A of AYUV / Y410 / Y416"""
    p = ExportYuvPack()
    p.format, p.alpha = yuvpack_code(yuv), int(alpha)
    return p


class ImportYuvPack(C.Structure):
    _fields_ = [("format", C.c_int32), ("reserved", C.c_int32 * 7)]


def make_import_yuvpack(yuv):
    """yuv: YUVPACK_* or its name"""
    p = ImportYuvPack()
    p.format = yuvpack_code(yuv)
    return p


class ImportDesc(C.Structure):
    _fields_ = [("layout", C.c_int32), ("order", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("bit_depth", C.c_int32 * 2),
                ("bytes_per_sample", C.c_int32), ("msb_aligned", C.c_int32), ("sample_type", C.c_int32), ("scale", C.c_float * 3),
                ("bias", C.c_float * 3), ("chroma_format", C.c_int32), ("down", C.c_int32), ("loc", C.c_int32), ("matrix", C.c_int32),
                ("full_range", C.c_int32), ("reserved", C.c_int32 * 8)]


class ImportPlan(C.Structure):
    _fields_ = [("planes", C.c_int32), ("width", C.c_int32 * 3), ("height", C.c_int32 * 3), ("row_bytes", C.c_int32 * 3),
                ("coef", C.c_int32 * 16)]


def make_import_desc(layout, order=-1, size=(0, 0), bit_depth=(0, 0), bytes_per_sample=1, msb_aligned=0, sample_type=SAMPLE_UINT,
                     scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0), chroma_format=1, down=DOWN_DROP, loc=0, matrix=1, full_range=0):
    """the source of a picture import (hmgpu_import_desc).  size: (width, height) in luma samples, 0 = the coded size; bit_depth: an
    int or (luma, chroma), 0 = the coding depth; chroma_format: 0 .. 3 or its name; down: DOWN_* or its name"""
    d = ImportDesc()
    d.layout, d.order = int(layout), int(order)
    d.width, d.height = int(size[0]), int(size[1])
    bd = (bit_depth, bit_depth) if isinstance(bit_depth, int) else tuple(bit_depth)
    d.bit_depth[0], d.bit_depth[1] = bd
    d.bytes_per_sample, d.msb_aligned, d.sample_type = int(bytes_per_sample), int(msb_aligned), int(sample_type)
    for k in range(3):
        d.scale[k], d.bias[k] = float(scale[k]), float(bias[k])
    d.chroma_format = int(CHROMA_FORMATS.get(chroma_format, chroma_format))
    d.down, d.loc = int(DOWN_FILTERS.get(down, down)), int(loc)
    d.matrix, d.full_range = int(matrix), int(full_range)
    return d


WARP_NEAREST, WARP_BILINEAR = 0, 1
WARP_EDGE, WARP_FILL = 0, 1
WARP_FILTERS = {"nearest": WARP_NEAREST, "bilinear": WARP_BILINEAR}
WARP_BORDERS = {"edge": WARP_EDGE, "fill": WARP_FILL}


class ExportWarp(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("filter", C.c_int32), ("border", C.c_int32), ("fill", C.c_int32 * 3),
                ("reserved", C.c_int32 * 5)]


class WarpMap(C.Structure):
    _fields_ = [("m", C.c_int32 * 6), ("reserved", C.c_int32 * 2)]


def make_export_warp(width, height, filter=WARP_BILINEAR, border=WARP_EDGE, fill=(0, 0, 0)):
    """filter: WARP_NEAREST / WARP_BILINEAR or its name; border: WARP_EDGE / WARP_FILL or its name; fill: (r, g, b) code values"""
    w = ExportWarp()
    w.width, w.height = int(width), int(height)
    w.filter, w.border = int(WARP_FILTERS.get(filter, filter)), int(WARP_BORDERS.get(border, border))
    for k in range(3):
        w.fill[k] = int(fill[k])
    return w


def warp_map_array(maps):
    """n maps of six Q16 ints (a sequence of sequences or an [n, 6] integer array) as a WarpMap array; None: a null pointer"""
    if maps is None:
        return None
    rows = [[int(v) for v in m] for m in maps]
    if any(len(m) != 6 for m in rows):
        raise ValueError("warp: six ints per map")
    arr = (WarpMap * len(rows))()
    for i, m in enumerate(rows):
        for k in range(6):
            if not -(1 << 31) <= m[k] < (1 << 31):
                raise ValueError("warp: map values are int32 (Q16)")
            arr[i].m[k] = m[k]
    return arr


def warp_stage(warp, size, filter, border, fill, n):
    """warp= / size= / filter= / border= / fill= of the Python exports: None without warp, else (ExportWarp, WarpMap array) of n maps"""
    if warp is None:
        if border != "edge" or fill is not None:
            raise ValueError("border / fill need warp=")
        return None
    if size is None:
        raise ValueError("warp: size=(height, width) is required, the output size")
    if filter not in WARP_FILTERS:
        raise ValueError("warp: filter \"bilinear\" or \"nearest\"")
    if border not in WARP_BORDERS:
        raise ValueError("warp: border \"edge\" or \"fill\"")
    maps = warp_map_array(warp)
    if len(maps) != n:
        raise ValueError("warp: one map per picture (%d pictures, %d maps)" % (n, len(maps)))
    h, w = (int(v) for v in size)
    return make_export_warp(w, h, filter, border, (0, 0, 0) if fill is None else tuple(fill)), maps


MOTION_BLOCKS, MOTION_DENSE = 0, 1
MOTION_NO_REF = -(1 << 31)
MOTION_DST_MV0, MOTION_DST_MV1, MOTION_DST_REF, MOTION_DST_BLOCK, MOTION_DSTS = 0, 1, 2, 3, 4


class MotionDesc(C.Structure):
    _fields_ = [("form", C.c_int32), ("lists", C.c_int32), ("sample_type", C.c_int32), ("crop", C.c_int32 * 4), ("reserved", C.c_int32 * 5)]


class MotionPlan(C.Structure):
    _fields_ = [("lists", C.c_int32), ("channels", C.c_int32 * 4), ("width", C.c_int32 * 4), ("height", C.c_int32 * 4),
                ("elem_bytes", C.c_int32 * 4), ("row_bytes", C.c_int32 * 4), ("reserved", C.c_int32 * 3)]


def make_motion_desc(form, lists=3, sample_type=SAMPLE_UINT, crop=(0, 0, 0, 0)):
    """form: MOTION_BLOCKS / MOTION_DENSE; lists: the mask (bit 0 list 0, bit 1 list 1); crop: (left, right, top, bottom), BLOCKS only"""
    d = MotionDesc()
    d.form, d.lists, d.sample_type = int(form), int(lists), int(sample_type)
    for i in range(4):
        d.crop[i] = int(crop[i])
    return d


RESIDUAL_PLANES, RESIDUAL_DENSE = 0, 1


class ResidualDesc(C.Structure):
    _fields_ = [("form", C.c_int32), ("components", C.c_int32), ("sample_type", C.c_int32), ("crop", C.c_int32 * 4),
                ("scale", C.c_float * 3), ("reserved", C.c_int32 * 6)]


class ResidualPlan(C.Structure):
    _fields_ = [("channels", C.c_int32 * 3), ("width", C.c_int32 * 3), ("height", C.c_int32 * 3), ("elem_bytes", C.c_int32 * 3),
                ("row_bytes", C.c_int32 * 3), ("reserved", C.c_int32 * 1)]


def make_residual_desc(form, components=7, sample_type=SAMPLE_UINT, crop=(0, 0, 0, 0), scale=(1.0, 1.0, 1.0)):
    """form: RESIDUAL_PLANES / RESIDUAL_DENSE; components: the mask (bit c: component c); crop: (left, right, top, bottom), PLANES only;
    scale: per component, the float types of DENSE"""
    d = ResidualDesc()
    d.form, d.components, d.sample_type = int(form), int(components), int(sample_type)
    for i in range(4):
        d.crop[i] = int(crop[i])
    for k in range(3):
        d.scale[k] = float(scale[k])
    return d


TRANSFORM_LEVELS, TRANSFORM_COEFFS = 0, 1
TRANSFORM_DST_INFO, TRANSFORM_DSTS, TRANSFORM_INFO_CHANNELS = 3, 4, 6


class TransformDesc(C.Structure):
    _fields_ = [("value", C.c_int32), ("components", C.c_int32), ("sample_type", C.c_int32), ("scale", C.c_float * 3),
                ("reserved", C.c_int32 * 6)]


class TransformPlan(C.Structure):
    _fields_ = [("channels", C.c_int32 * 4), ("width", C.c_int32 * 4), ("height", C.c_int32 * 4), ("elem_bytes", C.c_int32 * 4),
                ("row_bytes", C.c_int32 * 4), ("reserved", C.c_int32 * 4)]


def make_transform_desc(value=TRANSFORM_LEVELS, components=7, sample_type=SAMPLE_UINT, scale=(1.0, 1.0, 1.0)):
    """value: TRANSFORM_LEVELS / TRANSFORM_COEFFS; components: the mask (bit c: component c); scale: per component, the float types"""
    d = TransformDesc()
    d.value, d.components, d.sample_type = int(value), int(components), int(sample_type)
    for k in range(3):
        d.scale[k] = float(scale[k])
    return d


LOOPFILTER_GRIDS, LOOPFILTER_DENSE = 0, 1
LOOPFILTER_DST_EDGE, LOOPFILTER_DST_SAO, LOOPFILTER_DST_DENSE, LOOPFILTER_DSTS = 0, 1, 2, 3
LOOPFILTER_EDGE_CHANNELS, LOOPFILTER_SAO_CHANNELS = 13, 6
(LF_BS_VER, LF_BS_HOR, LF_QP_VER, LF_QP_HOR, LF_TC_VER, LF_TC_HOR, LF_BETA_VER, LF_BETA_HOR, LF_TC_CB_VER, LF_TC_CB_HOR, LF_TC_CR_VER,
 LF_TC_CR_HOR, LF_FLAGS) = range(13)
LF_SAO_TYPE, LF_SAO_BAND, LF_SAO_OFF0 = 0, 1, 2


class LoopfilterDesc(C.Structure):
    _fields_ = [("form", C.c_int32), ("sample_type", C.c_int32), ("crop", C.c_int32 * 4), ("scale", C.c_float * 3),
                ("reserved", C.c_int32 * 7)]


class LoopfilterPlan(C.Structure):
    _fields_ = [("channels", C.c_int32 * 3), ("width", C.c_int32 * 3), ("height", C.c_int32 * 3), ("elem_bytes", C.c_int32 * 3),
                ("row_bytes", C.c_int32 * 3), ("reserved", C.c_int32 * 1)]


def make_loopfilter_desc(form=LOOPFILTER_GRIDS, sample_type=SAMPLE_UINT, crop=(0, 0, 0, 0), scale=(1.0, 1.0, 1.0)):
    """form: LOOPFILTER_GRIDS / LOOPFILTER_DENSE; crop: (left, right, top, bottom) in multiples of 8, GRIDS only; sample_type and scale
    (per channel): the element of DENSE"""
    d = LoopfilterDesc()
    d.form, d.sample_type = int(form), int(sample_type)
    for i in range(4):
        d.crop[i] = int(crop[i])
    for k in range(3):
        d.scale[k] = float(scale[k])
    return d


METRICS_REF_PICTURES, METRICS_REF_PLANES = 0, 1
METRICS_NO_DIFF = (1 << 64) - 1


class MetricsDesc(C.Structure):
    _fields_ = [("reference", C.c_int32), ("components", C.c_int32), ("ssim", C.c_int32), ("ref_bytes_per_sample", C.c_int32),
                ("crop", C.c_int32 * 4), ("reserved", C.c_int32 * 7)]


class MetricsResult(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("sse", C.c_uint64), ("sad", C.c_uint64), ("differing", C.c_uint64), ("first_diff", C.c_uint64),
                ("ssim_q32", C.c_int64), ("ssim_windows", C.c_uint64), ("max_abs", C.c_uint32), ("reserved", C.c_uint32)]


class MetricsPlan(C.Structure):
    _fields_ = [("channels", C.c_int32 * 3), ("width", C.c_int32 * 3), ("height", C.c_int32 * 3), ("elem_bytes", C.c_int32 * 3),
                ("row_bytes", C.c_int32 * 3), ("result_bytes", C.c_int32), ("ssim_windows", C.c_int64 * 3)]


def make_metrics_desc(reference, components=7, ssim=1, ref_bytes_per_sample=0, crop=(0, 0, 0, 0)):
    """reference: METRICS_REF_*; components: the mask (bit c: component c); ref_bytes_per_sample: 1 / 2 with METRICS_REF_PLANES;
    crop: (left, right, top, bottom) in luma samples"""
    d = MetricsDesc()
    d.reference, d.components, d.ssim, d.ref_bytes_per_sample = int(reference), int(components), int(ssim), int(ref_bytes_per_sample)
    for i in range(4):
        d.crop[i] = int(crop[i])
    return d


METRICS_MAP_SSE, METRICS_MAP_SAD, METRICS_MAP_DIFFERING, METRICS_MAP_MAX_ABS, METRICS_MAP_SSIM_Q32, METRICS_MAP_SSIM_WINDOWS = range(6)
METRICS_MAP_FIELDS = 6


class MetricsMapDesc(C.Structure):
    _fields_ = [("log2_block", C.c_int32), ("reserved", C.c_int32 * 7)]


class MetricsMapPlan(C.Structure):
    _fields_ = [("blocks_x", C.c_int32), ("blocks_y", C.c_int32), ("block_w", C.c_int32 * 3), ("block_h", C.c_int32 * 3),
                ("width", C.c_int32 * 3), ("height", C.c_int32 * 3), ("channels", C.c_int32 * 3), ("fields", C.c_int32),
                ("row_bytes", C.c_int32), ("reserved", C.c_int32 * 5)]


def make_metrics_map_desc(block=16):
    """block: the side of a block in luma samples; the call takes 8, 16, 32 or 64 (log2_block 3 .. 6).  Any other size becomes a
    log2_block the library refuses"""
    d = MetricsMapDesc()
    block = int(block)
    d.log2_block = block.bit_length() - 1 if block > 0 and block & (block - 1) == 0 else -1
    return d


HISTOGRAM_Y, HISTOGRAM_CB, HISTOGRAM_CR, HISTOGRAM_MAXRGB = 0, 1, 2, 3


class HistogramDesc(C.Structure):
    _fields_ = [("channels", C.c_int32), ("log2_bins", C.c_int32), ("histogram", C.c_int32), ("rgb_bit_depth", C.c_int32),
                ("matrix", C.c_int32), ("full_range", C.c_int32), ("crop", C.c_int32 * 4), ("reserved", C.c_int32 * 6)]


class HistogramResult(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("sum", C.c_uint64), ("sum_sq", C.c_uint64), ("min", C.c_uint32), ("max", C.c_uint32),
                ("reserved", C.c_uint32 * 8)]


class HistogramPlan(C.Structure):
    _fields_ = [("channels", C.c_int32 * 4), ("width", C.c_int32 * 4), ("height", C.c_int32 * 4), ("depth", C.c_int32 * 4),
                ("log2_bins", C.c_int32 * 4), ("hist_bytes", C.c_int32 * 4), ("record_bytes", C.c_int32), ("coef", C.c_int32 * 16),
                ("reserved", C.c_int32 * 3)]


def make_histogram_desc(channels=7, log2_bins=0, histogram=1, rgb_bit_depth=0, matrix=1, full_range=0, crop=(0, 0, 0, 0)):
    """channels: the mask (bit c: channel c, HISTOGRAM_*); log2_bins: 0 (one bin per code value) or 4 .. 12; histogram: 0 for the
    records alone; rgb_bit_depth / matrix / full_range: of maxRGB, as in make_export_desc; crop: (left, right, top, bottom) in luma samples"""
    d = HistogramDesc()
    d.channels, d.log2_bins, d.histogram, d.rgb_bit_depth = int(channels), int(log2_bins), int(histogram), int(rgb_bit_depth)
    d.matrix, d.full_range = int(matrix), int(full_range)
    for i in range(4):
        d.crop[i] = int(crop[i])
    return d


def make_export_desc(layout, bit_depth=(0, 0), bytes_per_sample=1, msb_aligned=0, crop=(0, 0, 0, 0), matrix=1, full_range=0):
    d = ExportDesc()
    d.layout = layout
    bd = (bit_depth, bit_depth) if isinstance(bit_depth, int) else tuple(bit_depth)
    d.bit_depth[0], d.bit_depth[1] = bd
    d.bytes_per_sample, d.msb_aligned = bytes_per_sample, int(msb_aligned)
    for i in range(4):
        d.crop[i] = crop[i]
    d.matrix, d.full_range = matrix, int(full_range)
    return d


CONCEAL_COPY, CONCEAL_MOTION = 0, 1


class ConcealJob(C.Structure):
    _fields_ = [("dst", C.c_int32), ("src", C.c_int32), ("mode", C.c_int32), ("dst_poc", C.c_int32), ("src_poc", C.c_int32),
                ("fill", C.c_int32 * 3), ("ctu_mask", C.c_void_p), ("reserved", C.c_int32 * 4)]


def conceal_mask_bytes(mask, num_ctus):
    """the ctu_mask bytes of a sequence of num_ctus truth values (CTU a: bit a & 7 of byte a >> 3); a uint8 array passes as it is"""
    mask = np.asarray(mask)
    if mask.dtype == np.uint8 and mask.ndim == 1 and mask.size == (num_ctus + 7) // 8:
        return np.ascontiguousarray(mask)
    return np.packbits(mask.astype(bool).reshape(num_ctus), bitorder="little")


def conceal_job_array(jobs, num_ctus):
    """the ConcealJob array of a sequence of jobs -- ConcealJob structures, or dicts with dst and, optionally, src (None: fill), mode
    ("copy" / "motion" or CONCEAL_*), dst_poc, src_poc, fill (three values, negative: mid-grey), mask (None: every CTU; truth values per
    CTU, or the packed bytes), reserved -- and the list that keeps the masks alive"""
    jobs = list(jobs)
    arr = (ConcealJob * max(len(jobs), 1))()
    keep = []
    for i, j in enumerate(jobs):
        if isinstance(j, ConcealJob):
            arr[i] = j
            continue
        q = arr[i]
        q.dst = int(j["dst"])
        q.src = NO_PIC if j.get("src") is None else int(j["src"])
        mode = j.get("mode", CONCEAL_COPY)
        q.mode = {"copy": CONCEAL_COPY, "motion": CONCEAL_MOTION}.get(mode, mode)
        q.dst_poc, q.src_poc = int(j.get("dst_poc", 0)), int(j.get("src_poc", 0))
        for k, v in enumerate(j.get("fill", (-1, -1, -1))):
            q.fill[k] = int(v)
        if j.get("mask") is not None:
            m = conceal_mask_bytes(j["mask"], num_ctus)
            keep.append(m)
            q.ctu_mask = m.ctypes.data
        for k, v in enumerate(j.get("reserved", ())):
            q.reserved[k] = int(v)
    return arr, keep


# ------------------------------------------------------------------------------------------------ marshalling of the export calls
def ref(x):
    """an optional struct argument: byref(x), or NULL for None"""
    return C.byref(x) if x is not None else None


def addr(v):
    """a pointer argument (a destination, a stream) from an integer: 0 / None is NULL"""
    return C.c_void_p(v or None)


def window_array(windows):
    """the ExportWindow array of a sequence of windows (never of length 0), or NULL for None"""
    if windows is None:
        return None
    windows = list(windows)
    return (ExportWindow * max(len(windows), 1))(*windows)


def handle_array(pics):
    """the int32 array of a list of picture handles (never of length 0)"""
    return (C.c_int32 * max(len(pics), 1))(*pics)


def ptr_array(ptrs, n=3):
    """n pointers, the missing ones NULL"""
    return (C.c_void_p * n)(*(list(ptrs) + [None] * (n - len(ptrs))))


def i64_array(values, n=3):
    """n int64 (pitches, strides), the missing ones 0"""
    return (C.c_int64 * n)(*(list(values) + [0] * (n - len(values))))


# ------------------------------------------------------------------------------------------------ helpers
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p).value


def make_seq(width, height, bd_luma, bd_chroma=None, log2_ctu=6, max_pictures=8, strong_intra_smoothing=1, range_ext_flags=0):
    s = SeqParams()
    s.width, s.height = width, height
    s.bit_depth_luma = bd_luma
    s.bit_depth_chroma = bd_luma if bd_chroma is None else bd_chroma
    s.chroma_format = 1
    s.log2_ctu_size = log2_ctu
    s.max_pictures = max_pictures
    s.strong_intra_smoothing = strong_intra_smoothing
    s.range_ext_flags = range_ext_flags
    return s


def num_ctus(seq):
    c = 1 << seq.log2_ctu_size
    return ((seq.width + c - 1) // c) * ((seq.height + c - 1) // c)


def parts_per_ctu(seq):
    return 1 << (2 * seq.log2_ctu_size - 4)


META_ARRAYS = [("depth", np.uint8), ("part_size", np.int8), ("pred_mode", np.int8), ("qp", np.int8), ("tr_idx", np.uint8),
               ("cbf_y", np.uint8), ("cbf_u", np.uint8), ("cbf_v", np.uint8), ("ts_y", np.uint8), ("ts_u", np.uint8),
               ("ts_v", np.uint8), ("mv0", np.int16), ("mv1", np.int16), ("ref_idx0", np.int8), ("ref_idx1", np.int8),
               ("intra_dir_l", np.uint8), ("intra_dir_c", np.uint8), ("bypass", np.uint8), ("ipcm", np.uint8),
               ("slice_idx", np.uint16), ("tile_idx", np.uint16), ("ccp_u", np.int8), ("ccp_v", np.int8)]


class MetaHolder:
    """Keeps the numpy arrays alive next to the CtuMeta struct that points into them."""

    def __init__(self, arrays):
        self.arrays = {}
        for name, dt in META_ARRAYS:
            a = arrays.get(name)
            if a is not None:
                a = np.ascontiguousarray(a, dtype=dt)
            self.arrays[name] = a
        g = self.arrays
        m = CtuMeta()
        m.depth, m.part_size, m.pred_mode, m.qp, m.tr_idx = (_ptr(g[k]) for k in ("depth", "part_size", "pred_mode", "qp", "tr_idx"))
        for i, k in enumerate(("cbf_y", "cbf_u", "cbf_v")):
            m.cbf[i] = _ptr(g[k])
        for i, k in enumerate(("ts_y", "ts_u", "ts_v")):
            m.transform_skip[i] = _ptr(g[k])
        m.mv[0], m.mv[1] = _ptr(g["mv0"]), _ptr(g["mv1"])
        m.ref_idx[0], m.ref_idx[1] = _ptr(g["ref_idx0"]), _ptr(g["ref_idx1"])
        m.intra_dir[0], m.intra_dir[1] = _ptr(g["intra_dir_l"]), _ptr(g["intra_dir_c"])
        m.transquant_bypass, m.ipcm = _ptr(g["bypass"]), _ptr(g["ipcm"])
        m.slice_idx, m.tile_idx = _ptr(g["slice_idx"]), _ptr(g["tile_idx"])
        m.ccp_alpha[0], m.ccp_alpha[1] = _ptr(g["ccp_u"]), _ptr(g["ccp_v"])
        self.struct = m


class StagingHolder:
    """numpy views of a staging block (hmgpu_staging_alloc): .arrays[name] / .levels[k] / .starts[k] alias the page-locked memory;
    .struct / .coeffs are the structs to hand to the whole-picture calls.  fill() copies ordinary arrays in, levels in HM's dense
    layout; fill_compact() packs the levels (hmgpu_pack_levels: coded TUs only)."""

    def __init__(self, handle, meta_struct, coeff_struct, num_ctus, parts, ctu, chroma_shift=2):
        """chroma_shift: log2 of the luma samples per chroma sample (csx + csy): 2 for 4:2:0 / 4:0:0, 1 for 4:2:2, 0 for 4:4:4"""
        self.handle, self.struct = handle, meta_struct
        self.num_ctus = num_ctus
        np_ = num_ctus * parts

        def view(addr, dt, n):
            return np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_uint8)), shape=(n * np.dtype(dt).itemsize,)).view(dt)
        m = meta_struct
        addr = {"depth": m.depth, "part_size": m.part_size, "pred_mode": m.pred_mode, "qp": m.qp, "tr_idx": m.tr_idx,
                "cbf_y": m.cbf[0], "cbf_u": m.cbf[1], "cbf_v": m.cbf[2], "ts_y": m.transform_skip[0], "ts_u": m.transform_skip[1],
                "ts_v": m.transform_skip[2], "mv0": m.mv[0], "mv1": m.mv[1], "ref_idx0": m.ref_idx[0], "ref_idx1": m.ref_idx[1],
                "intra_dir_l": m.intra_dir[0], "intra_dir_c": m.intra_dir[1], "bypass": m.transquant_bypass, "ipcm": m.ipcm,
                "slice_idx": m.slice_idx, "tile_idx": m.tile_idx}
        self.arrays = {}
        for name, dt in META_ARRAYS:
            if name not in addr:
                continue                                    # (arrays a staging block does not hold: cross-component prediction weights)
            n = num_ctus if name in ("slice_idx", "tile_idx") else (2 * np_ if name in ("mv0", "mv1") else np_)
            self.arrays[name] = view(addr[name], dt, n)
        self.levels = [view(coeff_struct.level[k], np.int16, num_ctus * ctu * ctu >> (chroma_shift if k else 0)) for k in range(3)]
        self.starts = [view(coeff_struct.ctu_level_start[k], np.uint32, num_ctus + 1) for k in range(3)]
        self._all = {"intra": (m.intra_dir[0], m.intra_dir[1]), "ts": tuple(m.transform_skip[k] for k in range(3)),
                     "bypass": m.transquant_bypass, "ipcm": m.ipcm}
        self._compact = coeff_struct
        self._dense = Coeffs()
        for k in range(3):
            self._dense.level[k] = coeff_struct.level[k]
        self.coeffs = self._dense

    def _fill_meta(self, meta):
        for name, _ in META_ARRAYS:
            if name not in self.arrays:
                continue
            src = meta.arrays.get(name)
            if src is not None:
                self.arrays[name][:] = src.reshape(-1)
            elif name in ("ref_idx0", "ref_idx1"):
                self.arrays[name][:] = -1
            else:
                self.arrays[name][:] = 0

    def set_groups(self, intra=True, flags=True):
        """leave optional groups of the block out of the copy: the intra modes (a picture without intra CUs), the transform-skip /
        lossless / PCM flags (a picture that uses none of them)"""
        m = self.struct
        m.intra_dir[0], m.intra_dir[1] = self._all["intra"] if intra else (None, None)
        for k in range(3):
            m.transform_skip[k] = self._all["ts"][k] if flags else None
        m.transquant_bypass = self._all["bypass"] if flags else None
        m.ipcm = self._all["ipcm"] if flags else None

    def fill(self, meta, coeffs):
        self._fill_meta(meta)
        for k in range(3):
            self.levels[k][:] = coeffs.arrays[k].reshape(-1)
        self.coeffs = self._dense

    def fill_compact(self, lib, seq, meta, coeffs):
        """lib: the loaded libhmgpu (hmgpu_pack_levels is host code); returns the number of level bytes that will cross the bus"""
        self._fill_meta(meta)
        lv = (C.c_void_p * 3)(*[self._compact.level[k] for k in range(3)])
        stt = (C.c_void_p * 3)(*[self._compact.ctu_level_start[k] for k in range(3)])
        st = lib.hmgpu_pack_levels(C.byref(seq), C.byref(meta.struct), C.byref(coeffs.struct), lv, stt)
        if st != 0:
            raise RuntimeError("hmgpu_pack_levels: status %d" % st)
        self.coeffs = self._compact
        return 2 * int(sum(int(self.starts[k][self.num_ctus]) for k in range(3)))


class CoeffHolder:
    def __init__(self, y, cb, cr, pcm=None):
        self.arrays = [np.ascontiguousarray(a, dtype=np.int16) for a in (y, cb, cr)]
        self.pcm = [np.ascontiguousarray(a, dtype=np.int16) for a in pcm] if pcm is not None else None
        self.struct = Coeffs()
        for i in range(3):
            self.struct.level[i] = _ptr(self.arrays[i])
            if self.pcm is not None:
                self.struct.pcm_sample[i] = _ptr(self.pcm[i])


def make_slice(slice_type, ref_pic=((), ()), ref_poc=((), ()), cb_qp_offset=0, cr_qp_offset=0, pps_cb=0, pps_cr=0,
               deblocking_disable=0, beta_offset_div2=0, tc_offset_div2=0, lf_across_slices=1, lf_across_tiles=1):
    s = SliceParams()
    s.slice_type = slice_type
    s.cb_qp_offset, s.cr_qp_offset = cb_qp_offset, cr_qp_offset
    s.pps_cb_qp_offset, s.pps_cr_qp_offset = pps_cb, pps_cr
    s.deblocking_disable = deblocking_disable
    s.beta_offset_div2, s.tc_offset_div2 = beta_offset_div2, tc_offset_div2
    s.lf_across_slices = lf_across_slices
    s.lf_across_tiles = lf_across_tiles
    for l in range(2):
        s.num_ref_idx[l] = len(ref_pic[l])
        for i in range(MAX_REF):
            s.ref_pic[l][i] = NO_PIC
        for i, (h, p) in enumerate(zip(ref_pic[l], ref_poc[l])):
            s.ref_pic[l][i] = int(h)
            s.ref_poc[l][i] = int(p)
    return s


def clone_slice(s):
    """byte copy of a SliceParams (copy.copy refuses ctypes structures that hold pointers)"""
    return SliceParams.from_buffer_copy(s)


def make_pic_params(sao_enabled=1, lf_across_tiles=1, sao_offset_shift=(0, 0)):
    p = PicParams()
    p.sao_enabled, p.lf_across_tiles = sao_enabled, lf_across_tiles
    p.sao_offset_shift_luma, p.sao_offset_shift_chroma = sao_offset_shift
    return p


def sao_array_from_raw(raw):
    """raw: int32 [num_ctus, 3, 35] (mode, type, aux, offset[32]) -> ctypes array of SaoParam [num_ctus*3]"""
    raw = np.ascontiguousarray(raw, dtype=np.int32)
    n = raw.shape[0] * 3
    arr = (SaoParam * n)()
    C.memmove(arr, raw.ctypes.data, n * C.sizeof(SaoParam))
    return arr


def sao_array_to_np(arr, n_ctus):
    out = np.zeros((n_ctus, 3, 35), dtype=np.int32)
    C.memmove(out.ctypes.data, arr, n_ctus * 3 * C.sizeof(SaoParam))
    return out
