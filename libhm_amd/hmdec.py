"""ctypes mirror of include/hmdec.h (libhmdec.so): the libHMDecoder-compatible decoder on top of the device path.
Used by the tests and tools; applications written against libHM's libHMDecoder.h link the .so directly."""
import ctypes as C
import os

import numpy as np

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

LIBHMDEC_OK = 0


def lib():
    global _lib
    if _lib is None:
        from . import lib as gpu_lib          # libhmgpu first (shares the HIP runtime with torch when torch is loaded)
        gpu_lib()
        path = os.path.join(HERE, "libhmdec.so")
        if not os.path.exists(path):
            raise RuntimeError("libhmdec.so is missing: run `python libhm_amd/build.py`")
        L = C.CDLL(path, mode=C.RTLD_GLOBAL)
        L.libHMDec_get_version.restype = C.c_char_p
        L.libHMDec_new_decoder.restype = C.c_void_p
        L.libHMDec_free_decoder.argtypes = [C.c_void_p]
        L.libHMDec_set_SEI_Check.argtypes = [C.c_void_p, C.c_bool]
        L.libHMDec_set_max_temporal_layer.argtypes = [C.c_void_p, C.c_int]
        L.libHMDec_push_nal_unit.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_bool, C.POINTER(C.c_bool), C.POINTER(C.c_bool)]
        L.libHMDec_get_picture.argtypes = [C.c_void_p]
        L.libHMDec_get_picture.restype = C.c_void_p
        for f in ("libHMDEC_get_picture_width", "libHMDEC_get_picture_height", "libHMDEC_get_picture_stride"):
            getattr(L, f).argtypes = [C.c_void_p, C.c_int]
        L.libHMDEC_get_POC.argtypes = [C.c_void_p]
        L.libHMDEC_get_image_plane.argtypes = [C.c_void_p, C.c_int]
        L.libHMDEC_get_image_plane.restype = C.POINTER(C.c_int16)
        L.libHMDEC_get_chroma_format.argtypes = [C.c_void_p]
        L.libHMDEC_get_internal_bit_depth.argtypes = [C.c_int]
        L.hmdec_set_device.argtypes = [C.c_void_p, C.c_int]
        L.hmdec_set_devices.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
        L.hmdec_num_devices.argtypes = [C.c_void_p]
        L.hmdec_transfer_bytes.argtypes = [C.c_void_p]
        L.hmdec_transfer_bytes.restype = C.c_ulonglong
        L.hmdec_set_parse_only.argtypes = [C.c_void_p, C.c_int]
        L.hmdec_set_packed_input.argtypes = [C.c_void_p, C.c_int]
        L.hmdec_packed_pictures.argtypes = [C.c_void_p]
        L.hmdec_set_threads.argtypes = [C.c_void_p, C.c_int]
        L.hmdec_hash_mismatches.argtypes = [C.c_void_p]
        L.hmdec_pictures_decoded.argtypes = [C.c_void_p]
        L.hmdec_device_batches.argtypes = [C.c_void_p]
        L.hmdec_set_concealment.argtypes = [C.c_void_p, C.c_int]
        L.hmdec_set_concealment.restype = None
        L.hmdec_picture_concealed.argtypes = [C.c_void_p]
        L.hmdec_concealed_pictures.argtypes = [C.c_void_p]
        L.hmdec_concealed_ctus.argtypes = [C.c_void_p]
        L.hmdec_concealed_ctus.restype = C.c_longlong
        L.hmdec_picture_range_ext_flags.argtypes = [C.c_void_p]
        L.hmdec_picture_chroma_format.argtypes = [C.c_void_p]
        L.hmdec_picture_sao_offset_shift.argtypes = [C.c_void_p, C.c_int]
        L.hmdec_set_device_md5.argtypes = [C.c_void_p, C.c_int]
        L.hmdec_last_error.argtypes = [C.c_void_p]
        L.hmdec_last_error.restype = C.c_char_p
        L.hmdec_last_decoded_picture.argtypes = [C.c_void_p]
        L.hmdec_last_decoded_picture.restype = C.c_void_p
        L.hmdec_open_picture.argtypes = [C.c_void_p]
        L.hmdec_open_picture.restype = C.c_void_p
        L.hmdec_picture_array.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        L.hmdec_picture_num_slices.argtypes = [C.c_void_p]
        L.hmdec_picture_slice_params.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.hmdec_picture_hash_sei.argtypes = [C.c_void_p, C.c_void_p]
        L.hmdec_picture_geometry.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.hmdec_picture_conformance_window.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.hmdec_set_device_output.argtypes = [C.c_void_p, C.c_int]
        L.hmdec_download_bytes.argtypes = [C.c_void_p]
        L.hmdec_download_bytes.restype = C.c_ulonglong
        L.hmdec_picture_export.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(abi.ExportDesc), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                           C.c_int, C.c_void_p]
        L.hmdec_picture_export_scaled.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                  C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int, C.c_void_p]
        L.hmdec_pictures_export.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                            C.POINTER(abi.ExportTensor), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                            C.c_int, C.c_void_p]
        L.hmdec_pictures_export_windows.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(abi.ExportDesc),
                                                    C.POINTER(abi.ExportScale), C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                    C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int, C.c_void_p]
        L.hmdec_pictures_export_pixels.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(abi.ExportDesc),
                                                   C.POINTER(abi.ExportScale), C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                   C.POINTER(abi.ExportPixel), C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
        L.hmdec_colour_lut_create.argtypes = [C.c_void_p, C.POINTER(abi.ColourLutDesc), C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.hmdec_colour_lut_destroy.argtypes = [C.c_void_p, C.c_int64]
        L.hmdec_pictures_export_colour.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(abi.ExportDesc),
                                                   C.POINTER(abi.ExportScale), C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                   C.POINTER(abi.ExportPixel), C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                   C.POINTER(C.c_int64), C.c_int, C.c_void_p]
        L.hmdec_pictures_export_chroma.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(abi.ExportDesc),
                                                   C.POINTER(abi.ExportScale), C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                   C.POINTER(abi.ExportPixel), C.c_int64, C.POINTER(abi.ExportChroma), C.POINTER(C.c_void_p),
                                                   C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int, C.c_void_p]
        L.hmdec_pictures_export_format.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(abi.ExportDesc),
                                                   C.POINTER(abi.ExportScale), C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                   C.POINTER(abi.ExportFormat), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                   C.POINTER(C.c_int64), C.c_int, C.c_void_p]
        L.hmdec_pictures_export_yuvpack.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(abi.ExportDesc),
                                                    C.POINTER(abi.ExportScale), C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                    C.POINTER(abi.ExportFormat), C.POINTER(abi.ExportYuvPack), C.POINTER(C.c_void_p),
                                                    C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int, C.c_void_p]
        L.hmdec_pictures_export_warp.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(abi.ExportDesc),
                                                 C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow), C.POINTER(abi.ExportPixel),
                                                 C.c_int64, C.POINTER(abi.ExportChroma), C.POINTER(abi.ExportWarp), C.POINTER(abi.WarpMap),
                                                 C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int, C.c_void_p]
        L.hmdec_picture_chroma_loc.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.hmdec_pictures_export_motion.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(abi.MotionDesc),
                                                   C.POINTER(abi.ExportScale), C.POINTER(abi.ExportWindow), C.POINTER(C.c_void_p), C.c_void_p,
                                                   C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int,
                                                   C.c_void_p]
        L.hmdec_pictures_export_residual.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(abi.ResidualDesc),
                                                     C.POINTER(abi.ExportScale), C.POINTER(abi.ExportWindow), C.POINTER(C.c_void_p),
                                                     C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int, C.c_void_p]
        L.hmdec_pictures_export_transform.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(abi.TransformDesc),
                                                      C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                                      C.POINTER(C.c_int64), C.c_int, C.c_void_p]
        L.hmdec_pictures_export_loopfilter.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(abi.LoopfilterDesc),
                                                       C.POINTER(abi.ExportScale), C.POINTER(abi.ExportWindow), C.POINTER(C.c_void_p),
                                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int, C.c_void_p]
        L.hmdec_pictures_metrics.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(abi.MetricsDesc), C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        L.hmdec_pictures_metrics_map.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(abi.MetricsDesc),
                                                 C.POINTER(abi.MetricsMapDesc), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                                 C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int,
                                                 C.c_void_p]
        L.hmdec_pictures_histogram.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(abi.HistogramDesc), C.POINTER(C.c_void_p),
                                               C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        L.hmdec_picture_device.argtypes = [C.c_void_p]
        L.hmdec_picture_colour.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.hmdec_internal_info.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.POINTER(BlockValue))]
        _lib = L
    return _lib


class BlockValue(C.Structure):
    _fields_ = [("x", C.c_ushort), ("y", C.c_ushort), ("w", C.c_ushort), ("h", C.c_ushort), ("value", C.c_int), ("value2", C.c_int)]


INFO = {n: i for i, n in enumerate(
    ["CTU_SLICE_INDEX", "CU_PREDICTION_MODE", "CU_TRQ_BYPASS", "CU_SKIP_FLAG", "CU_PART_MODE", "CU_INTRA_MODE_LUMA", "CU_INTRA_MODE_CHROMA",
     "CU_ROOT_CBF", "PU_MERGE_FLAG", "PU_MERGE_INDEX", "PU_UNI_BI_PREDICTION", "PU_REFERENCE_POC_0", "PU_MV_0", "PU_REFERENCE_POC_1", "PU_MV_1",
     "TU_CBF_Y", "TU_CBF_CB", "TU_CBF_CR", "TU_COEFF_TR_SKIP_Y", "TU_COEFF_TR_SKIP_Cb", "TU_COEFF_TR_SKIP_Cr", "TU_COEFF_ENERGY_Y",
     "TU_COEFF_ENERGY_CB", "TU_COEFF_ENERGY_CR"])}


def split_nal_units(stream):
    """Annex B byte stream -> list of NAL units (without start codes)"""
    b = bytes(stream)
    starts, i = [], 0
    while True:
        j = b.find(b"\x00\x00\x01", i)
        if j < 0:
            break
        starts.append(j + 3)
        i = j + 3
    out = []
    for k, s in enumerate(starts):
        e = starts[k + 1] - 3 if k + 1 < len(starts) else len(b)
        while e > s and b[e - 1] == 0:           # trailing_zero_8bits / the zero_byte of the next start code
            e -= 1
        out.append(b[s:e])
    return out


_DTYPES = {"depth": np.uint8, "part_size": np.int8, "pred_mode": np.int8, "qp": np.int8, "tr_idx": np.uint8, "bypass": np.uint8,
           "ipcm": np.uint8, "skip": np.uint8, "merge": np.uint8, "slice_idx": np.uint16, "tile_idx": np.uint16, "sao": np.int32}


class Picture:
    """a decoded picture handle (valid until the decoder reuses the buffer)"""

    def __init__(self, handle, ctx=None):
        self.h = handle
        self.ctx = ctx                            # the decoder (libHMDec_context) the picture came from: export() needs it

    @property
    def poc(self):
        return lib().libHMDEC_get_POC(self.h)

    @property
    def concealed(self):
        """CTUs of the picture that were concealed (hmdec_picture_concealed): 0 for an undamaged picture, all of them for the
        stand-in of a missing reference picture and for a picture none of whose slices could be decoded"""
        return lib().hmdec_picture_concealed(self.h)

    def size(self, c=0):
        return lib().libHMDEC_get_picture_width(self.h, c), lib().libHMDEC_get_picture_height(self.h, c)

    def plane(self, c):
        w, h = self.size(c)
        stride = lib().libHMDEC_get_picture_stride(self.h, c)
        p = lib().libHMDEC_get_image_plane(self.h, c)
        if not p:
            raise RuntimeError("no samples: the decoder runs parse-only or the picture was never reconstructed")
        return np.ctypeslib.as_array(p, shape=(h, stride))[:, :w].copy()

    def array(self, name):
        ptr, n = C.c_void_p(), C.c_int64()
        if lib().hmdec_picture_array(self.h, name.encode(), C.byref(ptr), C.byref(n)) != 0:
            raise KeyError(name)
        base = name.rstrip("012")
        dt = _DTYPES.get(name, _DTYPES.get(base, None))
        if dt is None:
            dt = {"cbf": np.uint8, "ts": np.uint8, "mv": np.int16, "ref_idx": np.int8, "intra_dir": np.uint8, "coeff": np.int16,
                  "pcm": np.int16, "plane": np.int16, "ccp": np.int8}[base]
        if n.value == 0:
            return np.zeros(0, dtype=dt)
        buf = (C.c_char * n.value).from_address(ptr.value)
        return np.frombuffer(buf, dtype=dt).copy()

    def geometry(self):
        g = (C.c_int32 * 12)()
        lib().hmdec_picture_geometry(self.h, g)
        keys = ("width", "height", "log2_ctb", "bd_y", "bd_c", "pcm_bd_y", "pcm_bd_c", "pcm_lf_disable", "strong_intra", "sao", "lf_across_tiles", "num_ctbs")
        out = dict(zip(keys, (int(v) for v in g)))
        out["range_ext"] = int(lib().hmdec_picture_range_ext_flags(self.h))
        out["chroma_format"] = int(lib().hmdec_picture_chroma_format(self.h))
        out["csx"], out["csy"] = (0 if out["chroma_format"] == 3 else 1), (1 if out["chroma_format"] in (0, 1) else 0)
        out["sao_shift"] = (int(lib().hmdec_picture_sao_offset_shift(self.h, 0)), int(lib().hmdec_picture_sao_offset_shift(self.h, 1)))
        return out

    def conformance_window(self):
        w = (C.c_int32 * 4)()
        lib().hmdec_picture_conformance_window(self.h, w)
        return tuple(w)

    def cropped_plane(self, c):
        g = self.geometry()
        l, r, t, b = self.conformance_window()
        if c:
            l, r, t, b = l >> g["csx"], r >> g["csx"], t >> g["csy"], b >> g["csy"]
        p = self.plane(c)
        return p[t:p.shape[0] - b, l:p.shape[1] - r]

    def num_slices(self):
        return lib().hmdec_picture_num_slices(self.h)

    def slice_params(self, i):
        sp, sl = abi.SliceParams(), abi.ScalingLists()
        if lib().hmdec_picture_slice_params(self.h, i, C.byref(sp), C.byref(sl)) != 0:
            raise IndexError(i)
        return sp, sl

    def hash_sei(self):
        d = (C.c_uint8 * 48)()
        m = lib().hmdec_picture_hash_sei(self.h, d)
        return m, bytes(d)

    @property
    def device(self):
        """GPU ordinal that holds the picture's samples (hmdec_picture_device), -1: none"""
        return lib().hmdec_picture_device(self.h)

    def colour(self):
        """VUI colour description: dict of full_range, primaries, transfer, matrix, video_format (E.3.1 defaults when absent)"""
        v = (C.c_int32 * 5)()
        lib().hmdec_picture_colour(self.h, v)
        return dict(zip(("full_range", "primaries", "transfer", "matrix", "video_format"), (int(x) for x in v)))

    def chroma_loc(self):
        """VUI chroma sample location: dict of present, top_field, bottom_field (chroma_sample_loc_type 0 .. 5; 0 when absent)"""
        v = (C.c_int32 * 3)()
        lib().hmdec_picture_chroma_loc(self.h, v)
        return dict(zip(("present", "top_field", "bottom_field"), (int(x) for x in v)))

    def export_into(self, desc, ptrs, pitches, on_stream=1, stream=0, scale=None):
        """hmdec_picture_export (scale: an abi.ExportScale, hmdec_picture_export_scaled) into device memory the caller owns"""
        p, q = abi.ptr_array(ptrs), abi.i64_array(pitches)
        if scale is None:
            st, name = lib().hmdec_picture_export(self.ctx, self.h, C.byref(desc), p, q, on_stream, abi.addr(stream)), "hmdec_picture_export"
        else:
            st = lib().hmdec_picture_export_scaled(self.ctx, self.h, C.byref(desc), C.byref(scale), p, q, on_stream, abi.addr(stream))
            name = "hmdec_picture_export_scaled"
        if st != 0:
            from . import HmgpuError
            raise HmgpuError(st, name)

    def export(self, layout="rgb", bit_depth=8, crop="conformance", matrix=None, full_range=None, msb_aligned=False, size=None,
               filter="bilinear", out=None, dtype=None, mean=None, std=None, scale=None, bias=None, pixel=None, alpha=None, lut=None,
               chroma="replicate", chroma_loc=None, warp=None, border="edge", fill=None, chroma_format=None, chroma_down="drop", yuv=None,
               row_align=1):
        """The picture converted on its GPU into new torch tensors, written on torch.cuda.current_stream() (libhm_amd.export):
        RGB [3, H, W]; planar (Y, Cb, Cr); semi-planar (Y, CbCr [H, W, 2]).  bit_depth: int, (luma, chroma) or None (coding depths);
        crop: "conformance", None (whole picture) or (left, right, top, bottom) luma samples; matrix / full_range: None = from the
        VUI (the colour policy of libhm_amd.export); size: (height, width) of the output, resized with `filter` ("nearest",
        "bilinear", "bicubic", "area"), None = the crop's size; out: a tensor (or tuple of planes) of the planned shape to write
        instead of new ones; dtype: torch.float16 / bfloat16 / float32 gives normalised float elements (export_batch with one
        picture, without the batch dimension; mean / std / scale / bias as there); pixel ("rgb", "bgr", "rgba", "bgra", "argb",
        "abgr"; layout "rgb"): one [H, W, C] tensor of packed pixels, alpha its A element (None: opaque).  lut (layout "rgb"): a
        colour LUT of the picture's decoder (Decoder.colour_lut) of the output depth, or "sdr": the LUT export.colour_lut builds
        from the stream's own colour description (VUI primaries and transfer; unspecified codes raise) to BT.709 with the sRGB
        curve, tone-mapped with BT.2390, made once per decoder, source and depth.  chroma (layout "rgb"): "replicate", or "linear":
        Cb and Cr interpolated to the luma grid before the matrix at chroma_loc, a chroma_sample_loc_type 0 .. 5 or None: the
        stream's own (chroma_loc()["top_field"], 0 when absent).  warp (layout "rgb"): one inverse affine map of six Q16 ints
        (export.affine_map, export.orientation_map) from the size= output, then required, onto the crop; filter "bilinear" or
        "nearest", border "edge" or "fill" with fill=(r, g, b) (hmdec_pictures_export_warp).  chroma_format (layouts "planar" /
        "semiplanar"): None, or "400" / "420" / "422" / "444" (0 .. 3): Cb and Cr at that chroma format (hmdec_pictures_export_format)
        -- chroma "replicate" / "linear" where an axis gains samples, chroma_down "drop" / "linear" where it loses them, at
        chroma_loc as above; planar with "444" returns ONE [3, H, W] tensor (Y, Cb, Cr), as Context.export does.  yuv ("uyvy" ... "y416"), with
        alpha and row_align: Y, Cb and Cr interleaved into words, one tensor, as Context.export_batch describes
        (hmdec_pictures_export_yuvpack).  Valid until the next push into the decoder."""
        from . import export
        return _export([self], None, layout, bit_depth, crop, matrix, full_range, msb_aligned, size, filter, out, dtype, mean, std, scale, bias,
                       pixel=pixel, alpha=alpha, lut=lut, chroma=chroma, chroma_loc=chroma_loc, warp=export.one_map(warp), border=border,
                       fill=fill, chroma_format=chroma_format, chroma_down=chroma_down, yuv=yuv, row_align=row_align)

    def motion(self, form="blocks", lists=(0, 1), size=None, window=None, flip=False, dtype=None, crop=None):
        """export_motion_batch of this picture alone, the tensors without the batch dimension; window: one (x, y, w, h) or None"""
        out = export_motion_batch([self], form, lists, size, None if window is None else [window],
                                  [flip] if (flip or window is not None) and _form_is_dense(form) else None, dtype, None, crop)
        return {k: t[0] for k, t in out.items()}

    def residual(self, form="planes", components=(0, 1, 2), size=None, window=None, flip=False, dtype=None, scale=None, crop=None):
        """export_residual_batch of this picture alone, the tensors without the batch dimension; window: one (x, y, w, h) or None.
        window and flip belong to form="dense": with form="planes" they are refused (ValueError), as by Context.export_residual"""
        out = export_residual_batch([self], form, components, size, None if window is None else [window],
                                    [flip] if flip or window is not None else None, dtype, scale, None, crop)
        return {k: t[0] for k, t in out.items()}

    def transform(self, value="levels", components=(0, 1, 2), dtype=None, scale=None):
        """export_transform_batch of this picture alone, the tensors without the batch dimension"""
        out = export_transform_batch([self], value, components, dtype, scale)
        return {k: t[0] for k, t in out.items()}

    def loopfilter(self, form="grids", grids=("edge", "sao"), size=None, window=None, flip=False, dtype=None, scale=None, crop=None):
        """export_loopfilter_batch of this picture alone, the tensors without the batch dimension; window: one (x, y, w, h) or None.
        window and flip belong to form="dense": with form="grids" they are refused (ValueError), as by Context.export_loopfilter"""
        out = export_loopfilter_batch([self], form, grids, size, None if window is None else [window],
                                      [flip] if flip or window is not None else None, dtype, scale, None, crop)
        return {k: t[0] for k, t in out.items()}

    def metrics(self, ref, components=(0, 1, 2), ssim=True, crop=None):
        """metrics_batch of this picture alone: ref the planes [h_c, w_c] per component; the fields without the batch dimension"""
        out = metrics_batch([self], [None if t is None else t[None] for t in ref], components, ssim, crop)
        return {k: {f: t[0] for f, t in v.items()} for k, v in out.items()}

    def metrics_map(self, ref, block=16, components=(0, 1, 2), ssim=True, crop=None):
        """metrics_map_batch of this picture alone: ref the planes [h_c, w_c] per component; the maps [Hb, Wb] without the batch dimension"""
        out = metrics_map_batch([self], [None if t is None else t[None] for t in ref], block, components, ssim, crop)
        return {k: {f: t[0] for f, t in v.items()} for k, v in out.items()}

    def histogram(self, channels=("y", "cb", "cr"), bins=None, crop="conformance", matrix=None, full_range=None, rgb_bit_depth=0,
                  histogram=True):
        """histogram_batch of this picture alone: the histograms and fields without the batch dimension"""
        out = histogram_batch([self], channels, bins, crop, matrix, full_range, rgb_bit_depth, histogram)
        return {k: {f: t[0] for f, t in v.items()} for k, v in out.items()}


def _form_is_dense(form):
    from . import motion
    return motion.form_code(form) == abi.MOTION_DENSE


def _prologue(pictures, name, crop, none_crop):
    """what the batch exports start with: (the first picture, its sequence, the crop resolved -- "conformance": the picture's window,
    None: none_crop()); _device(first, name) follows, after whatever else a caller takes from the picture"""
    first = pictures[0]
    if first.ctx is None:
        raise RuntimeError("%s: the picture does not know its decoder" % name)
    g = first.geometry()
    seq = abi.make_seq(g["width"], g["height"], g["bd_y"], g["bd_c"], log2_ctu=g["log2_ctb"])
    seq.chroma_format = g["chroma_format"]
    if crop is None:
        crop = none_crop()
    if crop == "conformance":
        crop = first.conformance_window()
    return first, seq, crop


def _device(first, name):
    dev = first.device
    if dev < 0:
        raise RuntimeError("%s: the picture is not on a device (parse-only, or its sequence has ended)" % name)
    return dev


def _handles(pictures):
    return abi.ptr_array([p.h for p in pictures], len(pictures))


def export_residual_batch(pictures, form="planes", components=(0, 1, 2), size=None, windows=None, flip=None, dtype=None, scale=None, out=None,
                          crop=None, enqueue=True, n=None):
    """The decoded residual of up to 16 pictures a decoder has put out (fetched since the last push, one sequence, one GPU:
    hmdec_pictures_export_residual) as a dict of torch tensors with a leading batch dimension, written on
    torch.cuda.current_stream(): libhm_amd.residual describes the forms and keys.  crop: None = the whole coded picture for
    form="planes" and the conformance window for form="dense" (what export_batch shows: the same windows, flips and size give
    aligned pixels, vectors and residuals), "conformance", or (left, right, top, bottom).  enqueue False / n: only the tensors of n
    pictures are allocated (Decoder.frames)."""
    from . import HmgpuError, residual
    pictures = list(pictures)
    if not pictures:
        raise ValueError("export_residual_batch: no pictures")
    first, seq, crop = _prologue(pictures, "export_residual_batch", crop,
                                 lambda: (0, 0, 0, 0) if residual.form_code(form) == abi.RESIDUAL_PLANES else "conformance")
    dev = _device(first, "export_residual_batch")

    def call(desc, sc, win, ptrs, pitches, pstrides, bstrides, st):
        r = lib().hmdec_pictures_export_residual(first.ctx, len(pictures), _handles(pictures), C.byref(desc), abi.ref(sc), abi.window_array(win),
                                                 *residual.c_args(ptrs, pitches, pstrides, bstrides), 1, abi.addr(st))
        if r != 0:
            raise HmgpuError(r, "hmdec_pictures_export_residual")
    return residual.export_residual(call, seq, dev, len(pictures) if n is None else n, form, components, size, windows, flip, dtype, scale, out,
                                    crop, enqueue)


def export_loopfilter_batch(pictures, form="grids", grids=("edge", "sao"), size=None, windows=None, flip=None, dtype=None, scale=None,
                            out=None, crop=None):
    """The loop-filter decisions of up to 16 pictures a decoder has put out (fetched since the last push, one sequence, one GPU:
    hmdec_pictures_export_loopfilter) as a dict of torch tensors with a leading batch dimension, written on
    torch.cuda.current_stream(): libhm_amd.loopfilter describes the forms and keys.  crop: None = the whole coded picture for
    form="grids" and the conformance window for form="dense" (what export_batch shows: the same windows, flips and size give aligned
    pixels and edge strengths), "conformance", or (left, right, top, bottom)."""
    from . import HmgpuError, loopfilter
    pictures = list(pictures)
    if not pictures:
        raise ValueError("export_loopfilter_batch: no pictures")
    first, seq, crop = _prologue(pictures, "export_loopfilter_batch", crop,
                                 lambda: (0, 0, 0, 0) if loopfilter.form_code(form) == abi.LOOPFILTER_GRIDS else "conformance")
    dev = _device(first, "export_loopfilter_batch")

    def call(desc, sc, win, ptrs, pitches, pstrides, bstrides, st):
        r = lib().hmdec_pictures_export_loopfilter(first.ctx, len(pictures), _handles(pictures), C.byref(desc), abi.ref(sc),
                                                   abi.window_array(win), *loopfilter.c_args(ptrs, pitches, pstrides, bstrides), 1, abi.addr(st))
        if r != 0:
            raise HmgpuError(r, "hmdec_pictures_export_loopfilter")
    return loopfilter.export_loopfilter(call, seq, dev, len(pictures), form, grids, size, windows, flip, dtype, scale, out, crop)


def export_transform_batch(pictures, value="levels", components=(0, 1, 2), dtype=None, scale=None, out=None):
    """The quantised levels ("levels") or de-quantised transform coefficients ("coeffs") of up to 16 pictures a decoder has put out
    (fetched since the last push, one sequence, one GPU: hmdec_pictures_export_transform) and their transform-unit info grid as a
    dict of torch tensors with a leading batch dimension, written on torch.cuda.current_stream(): libhm_amd.transform describes the
    keys.  The planes are the coded picture; a conformance crop is a slice of the tensors."""
    from . import HmgpuError, transform
    pictures = list(pictures)
    if not pictures:
        raise ValueError("export_transform_batch: no pictures")
    first, seq, _ = _prologue(pictures, "export_transform_batch", (0, 0, 0, 0), None)
    dev = _device(first, "export_transform_batch")

    def call(desc, ptrs, pitches, pstrides, bstrides, st):
        r = lib().hmdec_pictures_export_transform(first.ctx, len(pictures), _handles(pictures), C.byref(desc),
                                                  *transform.c_args(ptrs, pitches, pstrides, bstrides), 1, abi.addr(st))
        if r != 0:
            raise HmgpuError(r, "hmdec_pictures_export_transform")
    return transform.export_transform(call, seq, dev, len(pictures), value, components, dtype, scale, out)


def metrics_batch(pictures, ref, components=(0, 1, 2), ssim=True, crop=None):
    """Up to 16 pictures a decoder has put out with device output on (fetched since the last push, one sequence, one GPU) compared
    on the device with planar torch tensors -- decoded against original (hmdec_pictures_metrics): ref a sequence of [n, h_c, w_c]
    tensors per component, uint8 or uint16 / int16 storage; the result dict of libhm_amd.metrics, written on
    torch.cuda.current_stream().  crop: None = the whole coded picture, "conformance", or (left, right, top, bottom)."""
    from . import HmgpuError, metrics
    pictures = list(pictures)
    if not pictures:
        raise ValueError("metrics_batch: no pictures")
    first, seq, crop = _prologue(pictures, "metrics_batch", crop, lambda: (0, 0, 0, 0))
    dev = _device(first, "metrics_batch")

    def call(desc, ref_pics, ptrs, pitches, bstrides, res, rs, st):
        r = lib().hmdec_pictures_metrics(first.ctx, len(pictures), _handles(pictures), C.byref(desc), *metrics.c_args(None, ptrs, pitches, bstrides)[1:],
                                         abi.addr(res), rs, 1, abi.addr(st))
        if r != 0:
            why = lib().hmdec_last_error(first.ctx).decode() if r == abi.HMGPU_EUNSUPPORTED else ""
            raise HmgpuError(r, "hmdec_pictures_metrics" + (": " + why if why else ""))
    return metrics.metrics(call, seq, dev, len(pictures), None, ref, components, ssim, crop)


def metrics_map_batch(pictures, ref, block=16, components=(0, 1, 2), ssim=True, crop=None):
    """The comparison of metrics_batch kept per block of block x block luma samples (hmdec_pictures_metrics_map): the pictures, ref and
    crop as there; the result dict of libhm_amd.metrics.metrics_map, maps [n, Hb, Wb] per component and field, written on
    torch.cuda.current_stream()."""
    from . import HmgpuError, metrics
    pictures = list(pictures)
    if not pictures:
        raise ValueError("metrics_map_batch: no pictures")
    first, seq, crop = _prologue(pictures, "metrics_map_batch", crop, lambda: (0, 0, 0, 0))
    dev = _device(first, "metrics_map_batch")

    def call(desc, md, ref_pics, ptrs, pitches, bstrides, maps, mp, mf, mb, st):
        r = lib().hmdec_pictures_metrics_map(first.ctx, len(pictures), _handles(pictures), C.byref(desc), C.byref(md),
                                             *metrics.c_args(None, ptrs, pitches, bstrides)[1:], *metrics.map_c_args(maps, mp, mf, mb), 1,
                                             abi.addr(st))
        if r != 0:
            why = lib().hmdec_last_error(first.ctx).decode() if r == abi.HMGPU_EUNSUPPORTED else ""
            raise HmgpuError(r, "hmdec_pictures_metrics_map" + (": " + why if why else ""))
    return metrics.metrics_map(call, seq, dev, len(pictures), None, ref, block, components, ssim, crop)


def histogram_batch(pictures, channels=("y", "cb", "cr"), bins=None, crop="conformance", matrix=None, full_range=None, rgb_bit_depth=0,
                    histogram=True):
    """What up to 16 pictures a decoder has put out with device output on (fetched since the last push, one sequence, one GPU)
    contain (hmdec_pictures_histogram): the result dict of libhm_amd.histogram -- per channel "y", "cb", "cr", "maxrgb" the histogram
    and samples, sum, sum_sq, min, max -- written on torch.cuda.current_stream().  crop: "conformance", None (the whole coded picture)
    or (left, right, top, bottom); matrix / full_range of "maxrgb": None = from the VUI, as in the RGB exports."""
    from . import HmgpuError, export
    from . import histogram as hg
    pictures = list(pictures)
    if not pictures:
        raise ValueError("histogram_batch: no pictures")
    first, seq, crop = _prologue(pictures, "histogram_batch", crop, lambda: (0, 0, 0, 0))
    col = first.colour()
    matrix, full_range = export.resolve_colour(matrix, full_range, col["matrix"], col["full_range"])

    def call(desc, ptrs, strides, rec, rs, st):
        r = lib().hmdec_pictures_histogram(first.ctx, len(pictures), _handles(pictures), C.byref(desc), *hg.c_args(ptrs, strides), abi.addr(rec), rs,
                                           1, abi.addr(st))
        if r != 0:
            why = lib().hmdec_last_error(first.ctx).decode() if r == abi.HMGPU_EINVAL else ""
            raise HmgpuError(r, "hmdec_pictures_histogram" + (": " + why if why.startswith("hmdec_pictures_histogram") else ""))
    # (a decoder without device output: the library's own refusal, with its message, rather than "not on a device")
    dev = first.device if first.device >= 0 else 0
    return hg.histogram(call, seq, dev, len(pictures), channels, bins, crop, matrix, full_range, rgb_bit_depth, histogram)


def export_motion_batch(pictures, form="blocks", lists=(0, 1), size=None, windows=None, flip=None, dtype=None, out=None, crop=None,
                        enqueue=True, n=None):
    """Motion vectors, reference POCs and block information of up to 16 pictures a decoder has put out (fetched since the last push,
    one sequence, one GPU: hmdec_pictures_export_motion) as a dict of torch tensors with a leading batch dimension, written on
    torch.cuda.current_stream(): libhm_amd.motion describes the forms and keys.  crop: None = the whole coded picture for
    form="blocks" and the conformance window for form="dense" (what export_batch shows: the same windows, flips and size give
    aligned pixels and vectors), "conformance", or (left, right, top, bottom).  enqueue False / n: only the tensors of n pictures are
    allocated (Decoder.frames)."""
    from . import HmgpuError, motion
    pictures = list(pictures)
    if not pictures:
        raise ValueError("export_motion_batch: no pictures")
    first, seq, crop = _prologue(pictures, "export_motion_batch", crop,
                                 lambda: (0, 0, 0, 0) if motion.form_code(form) == abi.MOTION_BLOCKS else "conformance")
    dev = _device(first, "export_motion_batch")

    def call(desc, sc, win, ptrs, pitches, pstrides, bstrides, st):
        r = lib().hmdec_pictures_export_motion(first.ctx, len(pictures), _handles(pictures), C.byref(desc), abi.ref(sc), abi.window_array(win),
                                               *motion.c_args(ptrs, pitches, pstrides, bstrides), 1, abi.addr(st))
        if r != 0:
            raise HmgpuError(r, "hmdec_pictures_export_motion")
    return motion.export_motion(call, seq, dev, len(pictures) if n is None else n, form, lists, size, windows, flip, dtype, out, crop, enqueue)


def _export(pictures, n, layout, bit_depth, crop, matrix, full_range, msb_aligned, size, filter, out, dtype=None, mean=None, std=None,
            scale=None, bias=None, enqueue=True, windows=None, flip=None, pixel=None, alpha=None, memory_format=None, lut=None,
            chroma="replicate", chroma_loc=None, warp=None, border="edge", fill=None, chroma_format=None, chroma_down="drop", yuv=None,
            row_align=1):
    """Picture.export (n None: pictures[0], no batch dimension) and export_batch (n = len(pictures)): geometry, crop and colour from
    the first picture; libhm_amd.export.export_tensors does the rest.  enqueue False: only the tensors of n pictures are allocated.
    windows / flip: per picture, relative to crop (export.make_windows); pixel / alpha / memory_format: packed pixels
    (export.make_pixel, hmdec_pictures_export_pixels); lut: a DecoderColourLut, a raw handle or "sdr"
    (hmdec_pictures_export_colour); chroma / chroma_loc: "linear" goes through hmdec_pictures_export_chroma, with the first picture's
    VUI sample location for chroma_loc None; "replicate" through the entries it always took; warp / border / fill: one map per
    picture (abi.warp_stage) through hmdec_pictures_export_warp, whatever the other stages; chroma_format / chroma_down: the YUV
    layouts at another chroma format through hmdec_pictures_export_format, chroma= then its up-conversion, the sample location
    found as for chroma "linear"; yuv / alpha / row_align: YUV interleaved into words through hmdec_pictures_export_yuvpack
    (export.export_yuvpack), the conversion keywords as for chroma_format"""
    from . import export
    first, seq, crop = _prologue(pictures, "export", crop, lambda: (0, 0, 0, 0))
    col = first.colour()
    count = n if not enqueue else len(pictures)
    if yuv is None and row_align != 1:
        raise ValueError("row_align belongs to yuv=")
    if yuv is not None:
        export.yuvpack_only(size=size, dtype=dtype, mean=mean, std=std, scale=scale, bias=bias, pixel=pixel, memory_format=memory_format, lut=lut,
                            warp=warp, fill=fill, chroma_format=chroma_format, msb_aligned=msb_aligned)
        return export.export_yuvpack(lambda desc, stages, ptrs, pitches, bstrides, st:
                                     _export_stages(pictures, seq, desc, stages, ptrs, pitches, bstrides, st) if enqueue else None,
                                     seq, _device(first, "export"), yuv, alpha, crop, export.make_windows(seq, crop, windows, flip, count),
                                     chroma, chroma_down, first.chroma_loc()["top_field"] if chroma_loc is None else chroma_loc, True, out, n,
                                     row_align)
    fmt = abi.format_stage(chroma_format, chroma, chroma_down, chroma_loc, first.chroma_loc()["top_field"] if chroma_format is not None else 0)
    chr_ = abi.chroma_stage(chroma, chroma_loc, first.chroma_loc()["top_field"]) if fmt is None else None
    wrp = abi.warp_stage(warp, size, filter, border, fill, count)
    if isinstance(lut, str):
        if lut != "sdr":
            raise ValueError("lut: a colour LUT of the decoder, or \"sdr\"")
        depth = bit_depth if isinstance(bit_depth, int) else (bit_depth or (0, 0))[0]
        lut = _sdr_lut(first.ctx, export.vui_source(col["primaries"], col["transfer"]), depth or seq.bit_depth_luma) if enqueue else 0
    matrix, full_range = export.resolve_colour(matrix, full_range, col["matrix"], col["full_range"])
    return export.export_tensors(lambda desc, stages, ptrs, pitches, bstrides, st:
                                 _export_stages(pictures, seq, desc, stages, ptrs, pitches, bstrides, st) if enqueue else None,
                                 seq, _device(first, "export"), layout, bit_depth, crop, matrix, full_range, msb_aligned, True, size, filter,
                                 out, n, dtype, mean, std, scale, bias, export.make_windows(seq, crop, windows, flip, count), pixel=pixel,
                                 alpha=alpha, memory_format=memory_format, lut=lut, chroma=chr_, warp=wrp, format=fmt)


def _export_stages(pictures, seq, desc, stages, ptrs, pitches, bstrides, stream):
    """the export of `stages` (export.Stages) on torch's stream `stream` through the narrowest hmdec_pictures_export* entry that
    carries them, as libhm_amd.Context.export_stages_into chooses among hmgpu's.  bstrides None: one picture, through
    hmdec_picture_export(_scaled) where it has integer elements and no further stage, else as a batch of one"""
    from . import HmgpuError, export, export_stages_plan
    s = stages
    if bstrides is None:
        if s[1:] == (None,) * 8:
            return pictures[0].export_into(desc, ptrs, pitches, 1, stream, s.scale)
        bstrides = export.stage_extents(export_stages_plan(seq, desc, s.shape_only(), 1), pitches)
    head = (pictures[0].ctx, len(pictures), _handles(pictures), C.byref(desc))
    mid = (abi.ref(s.scale), abi.ref(s.tensor), abi.window_array(s.windows), abi.ref(s.pixel))
    tail = (abi.ptr_array(ptrs), abi.i64_array(pitches), abi.i64_array(bstrides), 1, abi.addr(stream))
    handle = getattr(s.lut, "handle", s.lut)
    if s.yuvpack is not None:
        name, args = "hmdec_pictures_export_yuvpack", head + mid[:3] + (abi.ref(s.format), C.byref(s.yuvpack)) + tail
    elif s.format is not None:
        name, args = "hmdec_pictures_export_format", head + mid[:3] + (C.byref(s.format),) + tail
    elif s.warp is not None:
        name, args = "hmdec_pictures_export_warp", head + mid[1:] + (handle or 0, abi.ref(s.chroma), C.byref(s.warp[0]), s.warp[1]) + tail
    elif s.chroma is not None:
        name, args = "hmdec_pictures_export_chroma", head + mid + (handle or 0, C.byref(s.chroma)) + tail
    elif s.lut is not None:
        name, args = "hmdec_pictures_export_colour", head + mid + (handle,) + tail
    elif s.pixel is not None:
        name, args = "hmdec_pictures_export_pixels", head + mid + (abi.addr(ptrs[0]), pitches[0], bstrides[0], 1, abi.addr(stream))
    elif s.windows is not None:
        name, args = "hmdec_pictures_export_windows", head + mid[:3] + tail
    else:
        name, args = "hmdec_pictures_export", head + mid[:2] + tail
    r = getattr(lib(), name)(*args)
    if r != 0:
        raise HmgpuError(r, name)


def export_batch(pictures, layout="rgb", bit_depth=8, crop="conformance", matrix=None, full_range=None, msb_aligned=False, size=None,
                 filter="bilinear", out=None, dtype=None, mean=None, std=None, scale=None, bias=None, windows=None, flip=None,
                 pixel=None, alpha=None, memory_format=None, lut=None, chroma="replicate", chroma_loc=None, warp=None, border="edge",
                 fill=None, chroma_format=None, chroma_down="drop", yuv=None, row_align=1):
    """Up to 16 pictures a decoder has put out (and that are still valid: fetched since the last push), of one sequence and on one
    GPU, converted in one call (hmdec_pictures_export) into tensors with a leading batch dimension, written on
    torch.cuda.current_stream(): RGB [N, 3, H, W]; planar ([N, H, W], ...); semi-planar ([N, H, W], [N, Hc, Wc, 2]).  The arguments
    of Picture.export (crop and colour are taken from the first picture) and of libhm_amd.Context.export_batch (dtype, mean, std;
    windows: one (x, y, w, h) per picture relative to crop, flip: one boolean per picture -- hmdec_pictures_export_windows;
    pixel / alpha: one [N, H, W, C] tensor of packed pixels, memory_format=torch.channels_last: [N, 3, H, W] with channels-last
    strides -- hmdec_pictures_export_pixels; lut: a colour LUT of the pictures' decoder, Decoder.colour_lut, or "sdr" as in
    Picture.export -- hmdec_pictures_export_colour; chroma / chroma_loc as in Picture.export, the sample location that of the first
    picture -- hmdec_pictures_export_chroma; warp / border / fill as in Context.export_batch: one inverse affine map per picture,
    size= the output size, the windows of any sizes -- hmdec_pictures_export_warp; chroma_format / chroma_down as in
    Picture.export: the YUV layouts at another chroma format, planar "444" as ONE [N, 3, H, W] tensor --
    hmdec_pictures_export_format; yuv / alpha / row_align as in Context.export_batch: YUV interleaved into words, one tensor --
    hmdec_pictures_export_yuvpack)."""
    pictures = list(pictures)
    if not pictures:
        raise ValueError("export_batch: no pictures")
    return _export(pictures, len(pictures), layout, bit_depth, crop, matrix, full_range, msb_aligned, size, filter, out, dtype, mean, std,
                   scale, bias, windows=windows, flip=flip, pixel=pixel, alpha=alpha, memory_format=memory_format, lut=lut, chroma=chroma,
                   chroma_loc=chroma_loc, warp=warp, border=border, fill=fill, chroma_format=chroma_format, chroma_down=chroma_down, yuv=yuv,
                   row_align=row_align)


class DecoderColourLut:
    """a colour LUT of one Decoder (hmdec_colour_lut_create): the decoder keeps the tables and makes the device copies itself;
    close() releases it"""

    def __init__(self, ctx, handle, desc):
        self.ctx, self.handle, self.depth, self.size, self.has_shaper = ctx, handle, desc.depth, desc.size, bool(desc.has_shaper)

    def close(self):
        if self.handle and self.ctx:
            lib().hmdec_colour_lut_destroy(self.ctx, self.handle)
        self.handle = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _colour_lut(ctx, lattice, shaper, depth):
    from . import HmgpuError, colour_lut_arrays
    desc, sh, la = colour_lut_arrays(lattice, shaper, depth)
    h = C.c_int64(0)
    r = lib().hmdec_colour_lut_create(ctx, C.byref(desc), sh.ctypes.data_as(C.c_void_p) if sh is not None else None,
                                      la.ctypes.data_as(C.c_void_p) if la is not None else None, C.byref(h))
    if r != 0:
        raise HmgpuError(r, "hmdec_colour_lut_create")
    return DecoderColourLut(ctx, h.value, desc)


_sdr_luts = {}     # (decoder, source, depth) -> the LUT of lut="sdr"; a decoder's entries go when it is closed


def _sdr_lut(ctx, src, depth):
    from . import export
    key = (ctx, src, int(depth))
    if key not in _sdr_luts:
        lattice, shaper = export.colour_lut(src, (1, 13), int(depth), tone="bt2390")
        _sdr_luts[key] = _colour_lut(ctx, lattice, shaper, int(depth))
    return _sdr_luts[key]


CONCEALMENT = {None: 0, "copy": 1, "motion": 2}


class Decoder:
    def __init__(self, parse_only=False, device=0, check_hash=True, max_temporal_layer=-1, threads=1, device_md5=None, devices=None,
                 packed_input=False, device_output=False, concealment=None):
        """concealment: None (damaged streams as ever), "copy" or "motion" (hmdec_set_concealment): lost CTUs are filled from the
        closest picture, a picture without a decodable slice is filled whole, a missing reference picture gets a stand-in.
        devices: GPU ordinals of several device contexts (hmdec_set_devices; the same ordinal twice = two contexts on one GPU).
        packed_input: 4:0:0 / 4:2:0 pictures reach the device as packed inputs (hmdec_set_packed_input).
        device_output: pictures put out stay on the device (hmdec_set_device_output): Picture.export, planes downloaded lazily"""
        self.ctx = lib().libHMDec_new_decoder()
        if not self.ctx:
            raise MemoryError("libHMDec_new_decoder")
        lib().hmdec_set_parse_only(self.ctx, 1 if parse_only else 0)
        lib().hmdec_set_device(self.ctx, device)
        if devices:
            lib().hmdec_set_devices(self.ctx, (C.c_int * len(devices))(*devices), len(devices))
        lib().hmdec_set_threads(self.ctx, threads)
        lib().hmdec_set_packed_input(self.ctx, 1 if packed_input else 0)
        lib().hmdec_set_device_output(self.ctx, 1 if device_output else 0)
        if concealment not in CONCEALMENT:
            lib().libHMDec_free_decoder(self.ctx)
            self.ctx = None
            raise ValueError("concealment: None, \"copy\" or \"motion\"")
        lib().hmdec_set_concealment(self.ctx, CONCEALMENT[concealment])
        lib().libHMDec_set_SEI_Check(self.ctx, check_hash)
        lib().libHMDec_set_max_temporal_layer(self.ctx, max_temporal_layer)
        if device_md5 is not None:                 # MD5 hash SEIs checked on the device (default: the decoder's hash threads / HMDEC_DEVICE_MD5)
            lib().hmdec_set_device_md5(self.ctx, 1 if device_md5 else 0)

    def close(self):
        if self.ctx:
            for key in [k for k in _sdr_luts if k[0] == self.ctx]:
                del _sdr_luts[key]
            lib().libHMDec_free_decoder(self.ctx)
            self.ctx = None

    def colour_lut(self, lattice, shaper=None, depth=8):
        """a colour LUT of this decoder for lut= of Picture.export, export_batch and frames (libhm_amd.Context.colour_lut describes
        the tables); it lasts across the sequences of a stream until close()"""
        return _colour_lut(self.ctx, lattice, shaper, depth)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def push(self, nal, eof=False):
        """returns (new_picture, check_output)"""
        new_pic, check = C.c_bool(False), C.c_bool(False)
        buf = (C.c_uint8 * len(nal)).from_buffer_copy(nal)
        r = lib().libHMDec_push_nal_unit(self.ctx, buf, len(nal), eof, C.byref(new_pic), C.byref(check))
        if r != LIBHMDEC_OK:
            raise RuntimeError("libHMDec_push_nal_unit failed (%d): %s" % (r, lib().hmdec_last_error(self.ctx).decode()))
        return new_pic.value, check.value

    def get_picture(self):
        h = lib().libHMDec_get_picture(self.ctx)
        return Picture(h, self.ctx) if h else None

    def internal_info(self, pic, kind):
        """libHMDEC_get_internal_info as a list of (x, y, w, h, value, value2)"""
        data = C.POINTER(BlockValue)()
        n = lib().hmdec_internal_info(self.ctx, pic.h, INFO[kind], C.byref(data))
        if n < 0:
            raise RuntimeError("hmdec_internal_info")
        return [(data[i].x, data[i].y, data[i].w, data[i].h, data[i].value, data[i].value2) for i in range(n)]

    def last_decoded(self):
        h = lib().hmdec_last_decoded_picture(self.ctx)
        return Picture(h, self.ctx) if h else None

    @property
    def hash_mismatches(self):
        return lib().hmdec_hash_mismatches(self.ctx)

    @property
    def pictures_decoded(self):
        return lib().hmdec_pictures_decoded(self.ctx)

    def concealed_pictures(self):
        """pictures concealed so far, whole or in part, stand-ins of missing reference pictures included (hmdec_concealed_pictures)"""
        return lib().hmdec_concealed_pictures(self.ctx)

    def concealed_ctus(self):
        """CTUs concealed so far (hmdec_concealed_ctus)"""
        return int(lib().hmdec_concealed_ctus(self.ctx))

    @property
    def packed_pictures(self):
        """pictures handed to the device as packed inputs so far"""
        return lib().hmdec_packed_pictures(self.ctx)

    @property
    def device_batches(self):
        return lib().hmdec_device_batches(self.ctx)

    @property
    def num_devices(self):
        return lib().hmdec_num_devices(self.ctx)

    @property
    def transfer_bytes(self):
        return int(lib().hmdec_transfer_bytes(self.ctx))

    @property
    def download_bytes(self):
        """plane bytes copied device -> host so far (hmdec_download_bytes)"""
        return int(lib().hmdec_download_bytes(self.ctx))

    def decode_stream(self, stream, on_decoded=None, on_output=None):
        """libHM's documented loop (libHMDecoder.h:36-77) over an Annex B stream"""
        nals = split_nal_units(stream)
        seen = 0
        for i, nal in enumerate(nals):
            eof = i == len(nals) - 1
            while True:
                new_pic, check = self.push(nal, eof)
                if on_decoded and self.pictures_decoded > seen:
                    seen = self.pictures_decoded
                    on_decoded(self.last_decoded())
                if check:
                    while True:
                        p = self.get_picture()
                        if p is None:
                            break
                        if on_output:
                            on_output(p)
                if not new_pic:
                    break

    def frames(self, stream, batch=None, windows=None, motion=None, residual=None, **export_kw):
        """(poc, exported tensors) of every picture in output order: decode_stream's loop with Picture.export(**export_kw) in place
        of a download (chroma="linear" among them: the stream's own chroma sample location unless chroma_loc= names one).  Each export is enqueued before the next unit is pushed (the picture's lifetime); the tensors are torch's.
        batch=N: (pocs, tensors) with up to N (<= 16) pictures per item instead, the tensors those of export_batch: slots are filled
        in output order, the pictures fetched after one push in one batched call each; an item is yielded when it is full, the
        remainder at the end of the stream as a view of the first n slots.  windows (batch=N only): a function; fn(n) returns
        (windows, flips) for the n pictures of one batched call (export.random_resized_crop with the picture's size bound).
        motion (batch=N only): True, or a dict of export_motion_batch arguments (form, lists, dtype, ...): the items become
        (pocs, tensors, motion dict), the motion tensors allocated and filled slot by slot like the picture tensors; with the
        dense form the windows and flips fn(n) returned, and size=, apply to both.  motion=None leaves the items as they were.
        residual (batch=N only): True, or a dict of export_residual_batch arguments (form, components, dtype, scale, ...): the
        residual dict is appended to the items in the same way -- (pocs, tensors, residual dict), or (pocs, tensors, motion dict,
        residual dict) with motion= -- and its dense form takes each call's windows, flips and size= like the pixels and the motion.
        warp (with size=, border=, fill= among the export arguments): one map per picture as in Picture.export; with batch=N a
        function, fn(n) returns the maps of the n pictures of one batched call (export.random_affine with the sizes bound).  The
        dense motion and residual forms cannot be aligned with a warp and are refused with it."""
        if windows is not None and batch is None:
            raise ValueError("frames(windows=) needs batch=")
        if motion is not None and motion is not False and batch is None:
            raise ValueError("frames(motion=) needs batch=")
        if residual is not None and residual is not False and batch is None:
            raise ValueError("frames(residual=) needs batch=")
        if batch is not None:
            yield from self._frames_batched(stream, int(batch), export_kw, windows, None if motion is False else motion,
                                            None if residual is False else residual)
            return
        nals = split_nal_units(stream)
        for i, nal in enumerate(nals):
            eof = i == len(nals) - 1
            while True:
                new_pic, check = self.push(nal, eof)
                if check:
                    while True:
                        p = self.get_picture()
                        if p is None:
                            break
                        if callable(export_kw.get("warp")):      # fn(n), as with batch=N: the map of this picture
                            yield p.poc, p.export(**dict(export_kw, warp=list(export_kw["warp"](1))))
                        else:
                            yield p.poc, p.export(**export_kw)
                if not new_pic:
                    break

    def _frames_batched(self, stream, batch, export_kw, windows=None, motion=None, residual=None):
        if not 1 <= batch <= abi.EXPORT_MAX_BATCH:
            raise ValueError("batch: 1 .. %d" % abi.EXPORT_MAX_BATCH)
        if "out" in export_kw:
            raise ValueError("frames(batch=): the items are allocated here")
        kw = dict(layout="rgb", bit_depth=8, crop="conformance", matrix=None, full_range=None, msb_aligned=False, size=None,
                  filter="bilinear", out=None)
        kw.update(export_kw)
        warp = export_kw.get("warp")                  # a function: fn(n) returns the maps of one batched call's n pictures
        if callable(warp):
            export_kw = {k: v for k, v in export_kw.items() if k != "warp"}
        from . import export as _export_mod
        if warp is not None:                          # (the item's allocation: any n maps do)
            kw["warp"] = [_export_mod.WARP_IDENTITY] * batch
        mkw = None
        from . import motion as _motion
        if motion is not None:
            mkw = dict(form="blocks") if motion is True else dict(motion)
            for key in ("out", "windows", "flip"):
                if key in mkw:
                    raise ValueError("frames(motion=): no %s= in the motion dict (the items are allocated here; windows and flips come "
                                     "from frames(windows=fn))" % key)
            mkw["form"] = _motion.form_code(mkw.get("form", "blocks"))
            if mkw["form"] == abi.MOTION_DENSE:
                if warp is not None:
                    raise ValueError("frames(warp=): the dense motion form cannot be aligned with a warp")
                mkw.setdefault("size", kw["size"])
                mkw.setdefault("crop", kw["crop"])
        rkw = None
        from . import residual as _residual
        if residual is not None:
            rkw = dict(form="planes") if residual is True else dict(residual)
            for key in ("out", "windows", "flip"):
                if key in rkw:
                    raise ValueError("frames(residual=): no %s= in the residual dict (the items are allocated here; windows and flips come "
                                     "from frames(windows=fn))" % key)
            rkw["form"] = _residual.form_code(rkw.get("form", "planes"))
            if rkw["form"] == abi.RESIDUAL_DENSE:
                if warp is not None:
                    raise ValueError("frames(warp=): the dense residual form cannot be aligned with a warp")
                rkw.setdefault("size", kw["size"])
                rkw.setdefault("crop", kw["crop"])
        sides = lambda: tuple(t for t in (mitem if mkw is not None else None, ritem if rkw is not None else None) if t is not None)
        nals = split_nal_units(stream)
        item, pocs, mitem, ritem = None, [], None, None
        for i, nal in enumerate(nals):
            eof = i == len(nals) - 1
            while True:
                new_pic, check = self.push(nal, eof)
                if check:
                    got = []
                    while True:
                        p = self.get_picture()
                        if p is None:
                            break
                        got.append(p)
                    while got:                       # into the free slots of the item being filled, one call per item touched
                        take, got = got[:batch - len(pocs)], got[batch - len(pocs):]
                        wkw = {}
                        if windows is not None:      # the windows and flips of this call's pictures
                            w, f = windows(len(take))
                            wkw = dict(windows=list(w), flip=None if f is None else list(f))
                        pkw = dict(wkw)              # the picture export's own: the maps of this call's pictures
                        if callable(warp):
                            pkw["warp"] = list(warp(len(take)))
                        elif warp is not None:
                            raise ValueError("frames(batch=, warp=): a function, fn(n) returns the maps of n pictures")
                        if item is None:            # the first picture of an item allocates all N slots
                            item = _export(take[:1], batch, enqueue=False, windows=[wkw["windows"][0]] * batch if wkw else None, **kw)
                        export_batch(take, out=_slots(item, len(pocs), len(pocs) + len(take)), **pkw, **export_kw)
                        if mkw is not None:
                            mw = wkw if mkw["form"] == abi.MOTION_DENSE else {}
                            if mitem is None:
                                mitem = export_motion_batch(take[:1], enqueue=False, n=batch,
                                                            **dict(mkw, **({"windows": [mw["windows"][0]] * batch} if mw else {})))
                            export_motion_batch(take, out={k: t[len(pocs):len(pocs) + len(take)] for k, t in mitem.items()}, **mw, **mkw)
                        if rkw is not None:
                            rw = wkw if rkw["form"] == abi.RESIDUAL_DENSE else {}
                            if ritem is None:
                                ritem = export_residual_batch(take[:1], enqueue=False, n=batch,
                                                              **dict(rkw, **({"windows": [rw["windows"][0]] * batch} if rw else {})))
                            export_residual_batch(take, out={k: t[len(pocs):len(pocs) + len(take)] for k, t in ritem.items()}, **rw, **rkw)
                        pocs += [p.poc for p in take]
                        if len(pocs) == batch:
                            yield (pocs, _slots(item, 0, batch)) + sides()
                            item, pocs, mitem, ritem = None, [], None, None
                if not new_pic:
                    break
        if pocs:
            yield (pocs, _slots(item, 0, len(pocs))) + tuple({k: t[:len(pocs)] for k, t in d.items()} for d in sides())


def _slots(item, a, b):
    """slots a .. b - 1 of an item: a tensor (RGB) or a tuple of planes"""
    return tuple(t[a:b] for t in item) if isinstance(item, tuple) else item[a:b]
