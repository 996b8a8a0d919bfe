"""libhm_amd -- MI355X-native pixel reconstruction for the HM (HEVC) decoder.

The product is libhm_amd/libhmgpu.so: hand-written HIP kernels for gfx950 behind the C ABI of include/hmgpu.h
(drop-in for HM's TDecGop::decompressSlice / filterPicture).  This package is only the thin ctypes
binding used by tests and bench.py; it contains no compute and NO fallback: if the shared library or a GPU is missing,
every entry point raises.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhmgpu.so")
_lib = None


class HmgpuError(RuntimeError):
    def __init__(self, status, what, device_error=0):
        self.status = status
        self.device_error = device_error
        names = {1: "HMGPU_EINVAL", 2: "HMGPU_EDEVICE", 3: "HMGPU_EUNSUPPORTED", 4: "HMGPU_ENOMEM"}
        super().__init__("%s failed: %s%s" % (what, names.get(status, status),
                                              " (hipError %d)" % device_error if status == 2 else ""))


def _share_torch_hip_runtime():
    """One HIP runtime per process: PyTorch ships its own libamdhip64 and a process that has already initialised the
    system copy (through libhmgpu.so) can no longer bring up torch's ("No HIP GPUs are available").  The frame-parallel
    path needs both (RCCL through torch.distributed on this library's stream), so when torch is installed its runtime is
    loaded first and libhmgpu.so's NEEDED libamdhip64 resolves to it (same soname)."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
        path = os.path.join(os.path.dirname(spec.origin), "lib", name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                pass
            return


def lib():
    """Load libhmgpu.so.  No fallback: a missing library is an error."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libhm_amd/libhmgpu.so is missing: build it with `python libhm_amd/build.py` "
                               "(or __graft_entry__.build()); there is no CPU fallback")
        _share_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        L.hmgpu_create.argtypes = [C.POINTER(abi.SeqParams), C.c_int, C.POINTER(C.c_void_p)]
        L.hmgpu_destroy.argtypes = [C.c_void_p]
        L.hmgpu_destroy.restype = None
        L.hmgpu_last_device_error.argtypes = [C.c_void_p]
        L.hmgpu_debug_stall_intra.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.hmgpu_sync.argtypes = [C.c_void_p]
        L.hmgpu_status_string.restype = C.c_char_p
        L.hmgpu_kernel_name.restype = C.c_char_p
        L.hmgpu_num_ctus.argtypes = [C.POINTER(abi.SeqParams)]
        L.hmgpu_parts_per_ctu.argtypes = [C.POINTER(abi.SeqParams)]
        L.hmgpu_picture_acquire.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.hmgpu_picture_release.argtypes = [C.c_void_p, C.c_int32]
        L.hmgpu_picture_upload.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]
        L.hmgpu_picture_download.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]
        L.hmgpu_set_streams.argtypes = [C.c_void_p, C.c_int32]
        L.hmgpu_picture_download_packed.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)] + [C.c_int32] * 5
        L.hmgpu_picture_hash.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]
        L.hmgpu_picture_device_region.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        L.hmgpu_picture_commit_received.argtypes = [C.c_void_p, C.c_int32]
        L.hmgpu_picture_transfer.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.hmgpu_transfer_bytes.argtypes = [C.c_void_p]
        L.hmgpu_transfer_bytes.restype = C.c_uint64
        L.hmgpu_export_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportPlan)]
        L.hmgpu_picture_export.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.ExportDesc), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                           C.c_int32, C.c_void_p]
        L.hmgpu_export_scaled_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                   C.POINTER(abi.ExportPlan)]
        L.hmgpu_export_scale_taps.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale), C.c_int32,
                                              C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int16)]
        L.hmgpu_picture_export_scaled.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                  C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int32, C.c_void_p]
        L.hmgpu_export_tensor_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                   C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportPlan)]
        L.hmgpu_pictures_export.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                            C.POINTER(abi.ExportTensor), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                            C.c_int32, C.c_void_p]
        L.hmgpu_export_destination_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                     C.POINTER(abi.ExportTensor), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                     C.POINTER(C.c_int64)]
        L.hmgpu_export_windows_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                    C.POINTER(abi.ExportTensor), C.c_int32, C.POINTER(abi.ExportWindow),
                                                    C.POINTER(abi.ExportPlan)]
        L.hmgpu_pictures_export_windows.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.ExportDesc),
                                                    C.POINTER(abi.ExportScale), C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                    C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_void_p]
        L.hmgpu_export_windows_destination_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                             C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow), C.POINTER(C.c_void_p),
                                                             C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.hmgpu_export_pixels_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                   C.POINTER(abi.ExportTensor), C.c_int32, C.POINTER(abi.ExportWindow),
                                                   C.POINTER(abi.ExportPixel), C.POINTER(abi.ExportPlan)]
        L.hmgpu_pictures_export_pixels.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.ExportDesc),
                                                   C.POINTER(abi.ExportScale), C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                   C.POINTER(abi.ExportPixel), C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]
        L.hmgpu_export_pixels_destination_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                            C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                            C.POINTER(abi.ExportPixel), C.c_void_p, C.c_int64, C.c_int64]
        L.hmgpu_colour_lut_check.argtypes = [C.POINTER(abi.ColourLutDesc), C.c_void_p, C.c_void_p]
        L.hmgpu_colour_lut_create.argtypes = [C.c_void_p, C.POINTER(abi.ColourLutDesc), C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.hmgpu_colour_lut_destroy.argtypes = [C.c_void_p, C.c_int64]
        L.hmgpu_export_colour_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                   C.POINTER(abi.ExportTensor), C.c_int32, C.POINTER(abi.ExportWindow),
                                                   C.POINTER(abi.ExportPixel), C.POINTER(abi.ColourLutDesc), C.POINTER(abi.ExportPlan)]
        L.hmgpu_pictures_export_colour.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.ExportDesc),
                                                   C.POINTER(abi.ExportScale), C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                   C.POINTER(abi.ExportPixel), C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                   C.POINTER(C.c_int64), C.c_int32, C.c_void_p]
        L.hmgpu_export_colour_destination_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                            C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                            C.POINTER(abi.ExportPixel), C.c_int64, C.POINTER(C.c_void_p),
                                                            C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.hmgpu_export_chroma_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                   C.POINTER(abi.ExportTensor), C.c_int32, C.POINTER(abi.ExportWindow),
                                                   C.POINTER(abi.ExportPixel), C.POINTER(abi.ColourLutDesc), C.POINTER(abi.ExportChroma),
                                                   C.POINTER(abi.ExportPlan)]
        L.hmgpu_pictures_export_chroma.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.ExportDesc),
                                                   C.POINTER(abi.ExportScale), C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                   C.POINTER(abi.ExportPixel), C.c_int64, C.POINTER(abi.ExportChroma),
                                                   C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_void_p]
        L.hmgpu_export_chroma_destination_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                            C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                            C.POINTER(abi.ExportPixel), C.c_int64, C.POINTER(abi.ExportChroma),
                                                            C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.hmgpu_export_format_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                   C.POINTER(abi.ExportTensor), C.c_int32, C.POINTER(abi.ExportWindow),
                                                   C.POINTER(abi.ExportFormat), C.POINTER(abi.ExportPlan)]
        L.hmgpu_pictures_export_format.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.ExportDesc),
                                                   C.POINTER(abi.ExportScale), C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                   C.POINTER(abi.ExportFormat), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                   C.POINTER(C.c_int64), C.c_int32, C.c_void_p]
        L.hmgpu_export_format_destination_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                            C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                            C.POINTER(abi.ExportFormat), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                            C.POINTER(C.c_int64)]
        L.hmgpu_export_format_scale_taps.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                     C.POINTER(abi.ExportFormat), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                                     C.POINTER(C.c_int32), C.POINTER(C.c_int16)]
        L.hmgpu_export_yuvpack_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportTensor), C.c_int32,
                                                    C.POINTER(abi.ExportWindow), C.POINTER(abi.ExportFormat), C.POINTER(abi.ExportYuvPack),
                                                    C.POINTER(abi.ExportPlan)]
        L.hmgpu_pictures_export_yuvpack.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.ExportDesc),
                                                    C.POINTER(abi.ExportScale), C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                    C.POINTER(abi.ExportFormat), C.POINTER(abi.ExportYuvPack), C.POINTER(C.c_void_p),
                                                    C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_void_p]
        L.hmgpu_export_yuvpack_destination_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportScale),
                                                             C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow),
                                                             C.POINTER(abi.ExportFormat), C.POINTER(abi.ExportYuvPack),
                                                             C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.hmgpu_export_warp_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportTensor), C.c_int32,
                                                 C.POINTER(abi.ExportWindow), C.POINTER(abi.ExportPixel), C.POINTER(abi.ColourLutDesc),
                                                 C.POINTER(abi.ExportChroma), C.POINTER(abi.ExportWarp), C.POINTER(abi.WarpMap),
                                                 C.POINTER(abi.ExportPlan)]
        L.hmgpu_pictures_export_warp.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.ExportDesc),
                                                 C.POINTER(abi.ExportTensor), C.POINTER(abi.ExportWindow), C.POINTER(abi.ExportPixel),
                                                 C.c_int64, C.POINTER(abi.ExportChroma), C.POINTER(abi.ExportWarp), C.POINTER(abi.WarpMap),
                                                 C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_void_p]
        L.hmgpu_export_warp_destination_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.ExportDesc), C.POINTER(abi.ExportTensor),
                                                          C.POINTER(abi.ExportWindow), C.POINTER(abi.ExportPixel), C.c_int64,
                                                          C.POINTER(abi.ExportChroma), C.POINTER(abi.ExportWarp), C.POINTER(abi.WarpMap),
                                                          C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.hmgpu_motion_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.MotionDesc), C.POINTER(abi.ExportScale), C.c_int32,
                                            C.POINTER(abi.ExportWindow), C.POINTER(abi.MotionPlan)]
        L.hmgpu_pictures_export_motion.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.MotionDesc),
                                                   C.POINTER(abi.ExportScale), C.POINTER(abi.ExportWindow), C.POINTER(C.c_void_p), C.c_void_p,
                                                   C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32,
                                                   C.c_void_p]
        L.hmgpu_pictures_motion_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.hmgpu_motion_destination_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.MotionDesc), C.POINTER(abi.ExportScale),
                                                     C.POINTER(abi.ExportWindow), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p,
                                                     C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.hmgpu_residual_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.ResidualDesc), C.POINTER(abi.ExportScale), C.c_int32,
                                              C.POINTER(abi.ExportWindow), C.POINTER(abi.ResidualPlan)]
        L.hmgpu_pictures_export_residual.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.ResidualDesc),
                                                     C.POINTER(abi.ExportScale), C.POINTER(abi.ExportWindow), C.POINTER(C.c_void_p),
                                                     C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_void_p]
        L.hmgpu_pictures_residual_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.hmgpu_residual_destination_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.ResidualDesc), C.POINTER(abi.ExportScale),
                                                       C.POINTER(abi.ExportWindow), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.hmgpu_transform_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.TransformDesc), C.c_int32, C.POINTER(abi.TransformPlan)]
        L.hmgpu_pictures_export_transform.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.TransformDesc),
                                                      C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                                      C.POINTER(C.c_int64), C.c_int32, C.c_void_p]
        L.hmgpu_pictures_transform_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.hmgpu_transform_destination_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.TransformDesc), C.POINTER(C.c_void_p), C.c_void_p,
                                                        C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.hmgpu_loopfilter_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.LoopfilterDesc), C.POINTER(abi.ExportScale), C.c_int32,
                                                C.POINTER(abi.ExportWindow), C.POINTER(abi.LoopfilterPlan)]
        L.hmgpu_pictures_export_loopfilter.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.LoopfilterDesc),
                                                       C.POINTER(abi.ExportScale), C.POINTER(abi.ExportWindow), C.POINTER(C.c_void_p),
                                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_void_p]
        L.hmgpu_pictures_loopfilter_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32]
        L.hmgpu_loopfilter_destination_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.LoopfilterDesc), C.POINTER(abi.ExportScale),
                                                         C.POINTER(abi.ExportWindow), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.hmgpu_metrics_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.MetricsDesc), C.POINTER(abi.MetricsPlan)]
        L.hmgpu_metrics_psnr.argtypes = [C.POINTER(abi.MetricsResult), C.c_int32]
        L.hmgpu_metrics_psnr.restype = C.c_double
        L.hmgpu_pictures_metrics.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.MetricsDesc), C.POINTER(C.c_int32),
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p, C.c_int64,
                                             C.c_int32, C.c_void_p]
        L.hmgpu_metrics_check.argtypes = L.hmgpu_pictures_metrics.argtypes[:10]
        L.hmgpu_metrics_map_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.MetricsDesc), C.POINTER(abi.MetricsMapDesc),
                                                 C.POINTER(abi.MetricsMapPlan)]
        L.hmgpu_pictures_metrics_map.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.MetricsDesc),
                                                 C.POINTER(abi.MetricsMapDesc), C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                 C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                                 C.POINTER(C.c_int64), C.c_int32, C.c_void_p]
        L.hmgpu_metrics_map_check.argtypes = L.hmgpu_pictures_metrics_map.argtypes[:13]
        L.hmgpu_histogram_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.HistogramDesc), C.POINTER(abi.HistogramPlan)]
        L.hmgpu_pictures_histogram.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.HistogramDesc),
                                               C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        L.hmgpu_histogram_check.argtypes = L.hmgpu_pictures_histogram.argtypes[:8]
        L.hmgpu_stream.argtypes = [C.c_void_p]
        L.hmgpu_stream.restype = C.c_void_p
        L.hmgpu_decompress_slice.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(abi.SliceParams), C.POINTER(abi.CtuMeta),
                                             C.POINTER(abi.Coeffs), C.c_int32, C.c_int32]
        L.hmgpu_filter_picture.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.PicParams), C.c_void_p]
        L.hmgpu_filter_picture_stages.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.PicParams), C.c_void_p, C.c_int32]
        L.hmgpu_decompress_pictures.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.PictureJob)]
        L.hmgpu_filter_pictures.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.FilterJob)]
        L.hmgpu_staging_alloc.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(abi.CtuMeta), C.POINTER(abi.Coeffs)]
        L.hmgpu_staging_free.argtypes = [C.c_void_p, C.c_void_p]
        L.hmgpu_staging_free.restype = None
        L.hmgpu_pack_levels.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.CtuMeta), C.POINTER(abi.Coeffs), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.hmgpu_packed_max_bytes.argtypes = [C.POINTER(abi.SeqParams)]
        L.hmgpu_packed_max_bytes.restype = C.c_size_t
        L.hmgpu_pack_input.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.CtuMeta), C.POINTER(abi.Coeffs), C.c_void_p, C.c_size_t,
                                       C.POINTER(C.c_size_t)]
        L.hmgpu_unpack_input.argtypes = [C.POINTER(abi.SeqParams), C.c_void_p, C.c_size_t, C.POINTER(abi.CtuMetaOut), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_void_p)]
        L.hmgpu_decompress_pictures_packed.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.PackedJob)]
        L.hmgpu_packed_wait.argtypes = [C.c_void_p, C.c_void_p]
        L.hmgpu_import_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.ImportDesc), C.POINTER(abi.ImportPlan)]
        L.hmgpu_pictures_import.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.ImportDesc), C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_void_p]
        L.hmgpu_import_source_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.ImportDesc), C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.hmgpu_import_yuvpack_plan_for.argtypes = [C.POINTER(abi.SeqParams), C.POINTER(abi.ImportDesc), C.POINTER(abi.ImportYuvPack),
                                                    C.POINTER(abi.ImportPlan)]
        L.hmgpu_pictures_import_yuvpack.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.ImportDesc),
                                                    C.POINTER(abi.ImportYuvPack), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                    C.POINTER(C.c_int64), C.c_int32, C.c_void_p]
        L.hmgpu_import_yuvpack_source_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.ImportDesc), C.POINTER(abi.ImportYuvPack),
                                                        C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.hmgpu_conceal_check.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.ConcealJob)]
        L.hmgpu_pictures_conceal.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.ConcealJob)]
        L.hmgpu_picture_concealed_ctus.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.hmgpu_host_alloc.argtypes = [C.c_size_t]
        L.hmgpu_host_alloc.restype = C.c_void_p
        L.hmgpu_host_free.argtypes = [C.c_void_p]
        L.hmgpu_host_free.restype = None
        L.hmgpu_replay.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.hmgpu_replay_batch.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32]
        L.hmgpu_set_profiling.argtypes = [C.c_void_p, C.c_int32]
        L.hmgpu_get_stats.argtypes = [C.c_void_p, C.POINTER(abi.Stats), C.c_int32]
        L.hmgpu_inverse_transform_batch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 5
        L.hmgpu_mc_batch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_void_p, C.c_int32, C.c_void_p]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pack_levels(seq, meta, coeffs):
    """HM's dense level arrays -> a CoeffHolder with compact levels (coded TUs only) + CTU starts (hmgpu_pack_levels: host code)"""
    n = abi.num_ctus(seq)
    ctu = 1 << seq.log2_ctu_size
    out = abi.CoeffHolder(*[np.zeros(n * ctu * ctu >> (2 if k else 0), dtype=np.int16) for k in range(3)])
    out.starts = [np.zeros(n + 1, dtype=np.uint32) for _ in range(3)]
    lv = (C.c_void_p * 3)(*[out.struct.level[k] for k in range(3)])
    stt = (C.c_void_p * 3)(*[s.ctypes.data for s in out.starts])
    st = lib().hmgpu_pack_levels(C.byref(seq), C.byref(meta.struct), C.byref(coeffs.struct), lv, stt)
    if st != 0:
        raise HmgpuError(st, "hmgpu_pack_levels")
    for k in range(3):
        out.struct.ctu_level_start[k] = out.starts[k].ctypes.data
    return out


def export_plan(seq, desc):
    """what an export with `desc` writes for pictures of `seq` (hmgpu_export_plan_for: host code, no GPU)"""
    plan = abi.ExportPlan()
    st = lib().hmgpu_export_plan_for(C.byref(seq), C.byref(desc), C.byref(plan))
    if st != 0:
        raise HmgpuError(st, "hmgpu_export_plan_for")
    return plan


def import_status(seq, desc):
    """(status, plan) of hmgpu_import_plan_for: host code, no GPU"""
    plan = abi.ImportPlan()
    return lib().hmgpu_import_plan_for(C.byref(seq), abi.ref(desc), C.byref(plan)), plan


def import_yuvpack_status(seq, desc, yuvpack):
    """(status, plan) of hmgpu_import_yuvpack_plan_for: host code, no GPU; yuvpack: an abi.ImportYuvPack or None"""
    plan = abi.ImportPlan()
    return lib().hmgpu_import_yuvpack_plan_for(abi.ref(seq), abi.ref(desc), abi.ref(yuvpack), C.byref(plan)), plan


def import_plan(seq, desc=None, **kw):
    """what a picture import reads for pictures of `seq` (hmgpu_import_plan_for: host code, no GPU); desc: an abi.ImportDesc, or
    the keywords of abi.make_import_desc"""
    st, plan = import_status(seq, abi.make_import_desc(**kw) if desc is None else desc)
    if st != abi.HMGPU_OK:
        raise HmgpuError(st, "hmgpu_import_plan_for")
    return plan


def export_scaled_plan(seq, desc, scale):
    """what a scaled export writes (hmgpu_export_scaled_plan_for: host code, no GPU)"""
    plan = abi.ExportPlan()
    st = lib().hmgpu_export_scaled_plan_for(C.byref(seq), C.byref(desc), C.byref(scale), C.byref(plan))
    if st != 0:
        raise HmgpuError(st, "hmgpu_export_scaled_plan_for")
    return plan


def export_tensor_plan(seq, desc, scale=None, tensor=None):
    """what an export writes (hmgpu_export_tensor_plan_for: host code, no GPU): scale None = unscaled, tensor None = unsigned integers"""
    plan = abi.ExportPlan()
    st = lib().hmgpu_export_tensor_plan_for(C.byref(seq), C.byref(desc), abi.ref(scale), abi.ref(tensor), C.byref(plan))
    if st != abi.HMGPU_OK:
        raise HmgpuError(st, "hmgpu_export_tensor_plan_for")
    return plan


def export_windows_plan(seq, desc, scale, tensor, windows):
    """what an export with a window per picture writes per slot (hmgpu_export_windows_plan_for: host code, no GPU); windows: a
    sequence of abi.ExportWindow (desc.crop 0)"""
    plan = abi.ExportPlan()
    windows = list(windows)
    st = lib().hmgpu_export_windows_plan_for(C.byref(seq), C.byref(desc), abi.ref(scale), abi.ref(tensor), len(windows),
                                             abi.window_array(windows), C.byref(plan))
    if st != abi.HMGPU_OK:
        raise HmgpuError(st, "hmgpu_export_windows_plan_for")
    return plan


def export_pixels_plan(seq, desc, scale, tensor, windows, pixel):
    """what a packed-pixel export writes per slot (hmgpu_export_pixels_plan_for: host code, no GPU): one plane of [H, W, C] pixels;
    windows: None (desc.crop) or a sequence of abi.ExportWindow; pixel: an abi.ExportPixel"""
    plan = abi.ExportPlan()
    windows = None if windows is None else list(windows)
    st = lib().hmgpu_export_pixels_plan_for(C.byref(seq), C.byref(desc), abi.ref(scale), abi.ref(tensor),
                                            len(windows) if windows is not None else 1, abi.window_array(windows), abi.ref(pixel), C.byref(plan))
    if st != 0:
        raise HmgpuError(st, "hmgpu_export_pixels_plan_for")
    return plan


def export_colour_plan(seq, desc, scale, tensor, windows, pixel, lut_desc):
    """what a colour export writes per slot (hmgpu_export_colour_plan_for: host code, no GPU): the plan of the matching call without
    the colour stage; lut_desc: an abi.ColourLutDesc; pixel None: planes"""
    plan = abi.ExportPlan()
    windows = None if windows is None else list(windows)
    st = lib().hmgpu_export_colour_plan_for(C.byref(seq), C.byref(desc), abi.ref(scale), abi.ref(tensor),
                                            len(windows) if windows is not None else 1, abi.window_array(windows), abi.ref(pixel),
                                            abi.ref(lut_desc), C.byref(plan))
    if st != 0:
        raise HmgpuError(st, "hmgpu_export_colour_plan_for")
    return plan


def export_chroma_status(seq, desc, scale, tensor, windows, pixel, lut_desc, chroma):
    """(status, plan) of hmgpu_export_chroma_plan_for (host code, no GPU): the plan of the matching call without the chroma stage;
    lut_desc None: no colour stage; chroma: an abi.ExportChroma or None"""
    plan = abi.ExportPlan()
    windows = list(windows) if windows is not None else None
    st = lib().hmgpu_export_chroma_plan_for(C.byref(seq), C.byref(desc), abi.ref(scale), abi.ref(tensor),
                                            len(windows) if windows is not None else 1, abi.window_array(windows), abi.ref(pixel),
                                            abi.ref(lut_desc), abi.ref(chroma), C.byref(plan))
    return st, plan


def export_chroma_plan(seq, desc, scale, tensor, windows, pixel, lut_desc, chroma):
    """what a chroma export writes per slot: export_chroma_status, a refusal raised"""
    st, plan = export_chroma_status(seq, desc, scale, tensor, windows, pixel, lut_desc, chroma)
    if st != abi.HMGPU_OK:
        raise HmgpuError(st, "hmgpu_export_chroma_plan_for")
    return plan


def export_format_status(seq, desc, scale, tensor, windows, format, n=None):
    """(status, plan) of hmgpu_export_format_plan_for (host code, no GPU): the planes of format.chroma_format; windows None: the
    plan of desc's crop; format: an abi.ExportFormat or None; n: another count than len(windows)"""
    plan = abi.ExportPlan()
    windows = list(windows) if windows is not None else None
    if n is None:
        n = len(windows) if windows is not None else 1
    st = lib().hmgpu_export_format_plan_for(C.byref(seq), C.byref(desc), abi.ref(scale), abi.ref(tensor), n, abi.window_array(windows),
                                            abi.ref(format), C.byref(plan))
    return st, plan


def export_format_plan(seq, desc, scale, tensor, windows, format):
    """what a format export writes per slot: export_format_status, a refusal raised"""
    st, plan = export_format_status(seq, desc, scale, tensor, windows, format)
    if st != abi.HMGPU_OK:
        raise HmgpuError(st, "hmgpu_export_format_plan_for")
    return plan


def export_format_scale_taps(seq, desc, scale, format, chroma, axis):
    """(first, count, weights[out, taps]) of one resampling table of a scaled format export (hmgpu_export_format_scale_taps):
    export_scale_taps with plane class 1 going from the cropped source chroma plane to the output format's chroma size"""
    import numpy as np
    plan = export_format_plan(seq, desc, scale, None, None, format)
    out = (plan.width, plan.height)[axis][1 if chroma else 0]
    taps = max(plan.coef[12 + axis], 1)
    first, count, w = np.zeros(out, np.int32), np.zeros(out, np.int32), np.zeros((out, taps), np.int16)
    st = lib().hmgpu_export_format_scale_taps(C.byref(seq), C.byref(desc), C.byref(scale), abi.ref(format), chroma, axis, taps,
                                              first.ctypes.data_as(C.POINTER(C.c_int32)), count.ctypes.data_as(C.POINTER(C.c_int32)),
                                              w.ctypes.data_as(C.POINTER(C.c_int16)))
    if st != abi.HMGPU_OK:
        raise HmgpuError(st, "hmgpu_export_format_scale_taps")
    return first, count, w


def export_yuvpack_status(seq, desc, tensor, windows, format, yuvpack, n=None):
    """(status, plan) of hmgpu_export_yuvpack_plan_for (host code, no GPU): the one plane of words; windows None: the plan of desc's
    crop; format: an abi.ExportFormat or None; yuvpack: an abi.ExportYuvPack or None; n: another count than len(windows)"""
    windows = None if windows is None else list(windows)
    if n is None:
        n = len(windows) if windows is not None else 1
    plan = abi.ExportPlan()
    st = lib().hmgpu_export_yuvpack_plan_for(abi.ref(seq), abi.ref(desc), abi.ref(tensor), n, abi.window_array(windows), abi.ref(format),
                                             abi.ref(yuvpack), C.byref(plan))
    return st, plan


def export_yuvpack_plan(seq, desc, tensor, windows, format, yuvpack):
    """what a packed YUV export writes per slot: export_yuvpack_status, a refusal raised"""
    st, plan = export_yuvpack_status(seq, desc, tensor, windows, format, yuvpack)
    if st != abi.HMGPU_OK:
        raise HmgpuError(st, "hmgpu_export_yuvpack_plan_for")
    return plan


def export_warp_status(seq, desc, tensor, windows, pixel, lut_desc, chroma, warp, maps, n=None):
    """(status, plan) of hmgpu_export_warp_plan_for (host code, no GPU): the plan of the matching planar or packed call with every
    plane warp.width x warp.height.  warp: an abi.ExportWarp or None; maps: an abi.WarpMap array (abi.warp_map_array) or None;
    n: the pictures (default: one per window, else one per map, else 1)"""
    plan = abi.ExportPlan()
    windows = list(windows) if windows is not None else None
    if n is None:
        n = len(windows) if windows is not None else len(maps) if maps is not None else 1
    st = lib().hmgpu_export_warp_plan_for(C.byref(seq), C.byref(desc), abi.ref(tensor), n, abi.window_array(windows), abi.ref(pixel),
                                          abi.ref(lut_desc), abi.ref(chroma), abi.ref(warp), maps, C.byref(plan))
    return st, plan


def export_warp_plan(seq, desc, tensor, windows, pixel, lut_desc, chroma, warp, maps, n=None):
    """what a warp export writes per slot: export_warp_status, a refusal raised"""
    st, plan = export_warp_status(seq, desc, tensor, windows, pixel, lut_desc, chroma, warp, maps, n)
    if st != abi.HMGPU_OK:
        raise HmgpuError(st, "hmgpu_export_warp_plan_for")
    return plan


def export_stages_plan(seq, desc, stages, n=None):
    """what an export of `stages` (export.Stages) writes per slot: the plan function of the narrowest entry that carries them, as
    Context.export_stages_into chooses the export.  stages.lut: an abi.ColourLutDesc, or a colour LUT object, which knows its own; a
    raw handle describes nothing and adds no rule.  n: the pictures of a warp (export_warp_status)"""
    s, ld = stages, stages.lut
    if ld is not None and not isinstance(ld, abi.ColourLutDesc):
        ld = abi.make_colour_lut_desc(ld.depth, ld.size, ld.has_shaper) if hasattr(ld, "has_shaper") else None
    if s.yuvpack is not None:
        return export_yuvpack_plan(seq, desc, s.tensor, s.windows, s.format, s.yuvpack)
    if s.format is not None:
        return export_format_plan(seq, desc, s.scale, s.tensor, s.windows, s.format)
    if s.warp is not None:
        return export_warp_plan(seq, desc, s.tensor, s.windows, s.pixel, ld, s.chroma, s.warp[0], s.warp[1], n)
    if s.chroma is not None:
        return export_chroma_plan(seq, desc, s.scale, s.tensor, s.windows, s.pixel, ld, s.chroma)
    if ld is not None:
        return export_colour_plan(seq, desc, s.scale, s.tensor, s.windows, s.pixel, ld)
    if s.pixel is not None:
        return export_pixels_plan(seq, desc, s.scale, s.tensor, s.windows, s.pixel)
    if s.windows is not None:
        return export_windows_plan(seq, desc, s.scale, s.tensor, s.windows)
    return export_tensor_plan(seq, desc, s.scale, s.tensor)


def colour_lut_arrays(lattice, shaper, depth):
    """(abi.ColourLutDesc, shaper, lattice) of a LUT as the C calls take it: lattice None or [L, L, L, 3] (b, g, r, channel), shaper
    None or [3, 2^depth], both converted to contiguous uint16 (values outside 0 .. 65535 raise)"""
    import numpy as np

    def u16(a, what):
        a = np.asarray(a)
        if a.dtype != np.uint16:
            if a.size and (a.min() < 0 or a.max() > 65535):
                raise ValueError("%s: values outside 0 .. 65535" % what)
            a = a.astype(np.uint16)
        return np.ascontiguousarray(a)
    size = 0
    if lattice is not None:
        lattice = u16(lattice, "lattice")
        if lattice.ndim != 4 or lattice.shape[3] != 3 or len(set(lattice.shape[:3])) != 1:
            raise ValueError("lattice: shape [L, L, L, 3], got %s" % (lattice.shape,))
        size = lattice.shape[0]
    if shaper is not None:
        shaper = u16(shaper, "shaper")
        if shaper.shape != (3, 1 << int(depth)):
            raise ValueError("shaper: shape [3, %d], got %s" % (1 << int(depth), shaper.shape))
    return abi.make_colour_lut_desc(depth, size, shaper is not None), shaper, lattice


def colour_lut_status(lattice, shaper=None, depth=8, desc=None):
    """hmgpu_colour_lut_check (host code, no GPU): the status hmgpu_colour_lut_create gives these tables before it looks at a
    context; desc: an abi.ColourLutDesc in place of the one the arrays imply"""
    d, sh, la = colour_lut_arrays(lattice, shaper, depth)
    return lib().hmgpu_colour_lut_check(C.byref(desc if desc is not None else d), _p(sh) if sh is not None else None,
                                        _p(la) if la is not None else None)


class ColourLut:
    """a colour LUT in device memory of one Context (hmgpu_colour_lut_create); close() releases it, also while exports that read it
    are in flight"""

    def __init__(self, ctx, handle, desc):
        self.ctx, self.handle, self.depth, self.size, self.has_shaper = ctx, handle, desc.depth, desc.size, bool(desc.has_shaper)

    def close(self):
        if self.handle and self.ctx._h:
            self.ctx._chk(lib().hmgpu_colour_lut_destroy(self.ctx._h, self.handle), "hmgpu_colour_lut_destroy")
        self.handle = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def motion_plan(seq, form="blocks", lists=(0, 1), size=None, windows=None, flip=None, dtype=None, crop=(0, 0, 0, 0), n=None):
    """what Context.export_motion with these arguments writes per picture (hmgpu_motion_plan_for: host code, no GPU): an
    abi.MotionPlan -- per destination slot (abi.MOTION_DST_*) the channels, width, height, element size and row bytes.  dtype: a
    torch float dtype, or an abi.SAMPLE_* code (dense; None: float32).  n: the number of pictures (default: one per window, else 1)"""
    from . import motion
    count = n if n is not None else (len(list(windows)) if windows is not None and motion.form_code(form) == abi.MOTION_DENSE else 1)
    desc, sc, win = motion.describe(seq, count, form, lists, size, windows, flip, dtype, crop, strict=False)
    return motion.plan_for(seq, desc, sc, win, count)


def residual_plan(seq, form="planes", components=(0, 1, 2), size=None, windows=None, flip=None, dtype=None, scale=None, crop=(0, 0, 0, 0),
                  n=None):
    """what Context.export_residual with these arguments writes per picture (libhm_amd.residual.residual_plan: host code, no GPU)"""
    from . import residual
    return residual.residual_plan(seq, form, components, size, windows, flip, dtype, scale, crop, n)


def transform_plan(seq, value="levels", components=(0, 1, 2), dtype=None, scale=None, n=1):
    """what Context.export_transform with these arguments writes per picture (libhm_amd.transform.transform_plan: host code, no GPU)"""
    from . import transform
    return transform.transform_plan(seq, value, components, dtype, scale, n)


def loopfilter_plan(seq, form="grids", size=None, windows=None, flip=None, dtype=None, scale=None, crop=(0, 0, 0, 0), n=None):
    """what Context.export_loopfilter with these arguments writes per picture (libhm_amd.loopfilter.loopfilter_plan: host code, no GPU)"""
    from . import loopfilter
    return loopfilter.loopfilter_plan(seq, form, size, windows, flip, dtype, scale, crop, n)


def metrics_plan(seq, reference="pictures", components=(0, 1, 2), ssim=True, crop=(0, 0, 0, 0), ref_bytes_per_sample=2):
    """what Context.metrics with these arguments compares (hmgpu_metrics_plan_for: host code, no GPU): an abi.MetricsPlan -- per
    component width, height, SSIM windows and the least reference pitch.  reference: "pictures" or "planes" (then ref_bytes_per_sample 1 or 2)"""
    from . import metrics
    planes = {"pictures": False, "planes": True}[reference]
    desc = abi.make_metrics_desc(abi.METRICS_REF_PLANES if planes else abi.METRICS_REF_PICTURES, metrics.components_mask(components),
                                 1 if ssim else 0, ref_bytes_per_sample if planes else 0, crop)
    return metrics.plan_for(seq, desc)


def metrics_map_plan(seq, block=16, reference="pictures", components=(0, 1, 2), ssim=True, crop=(0, 0, 0, 0), ref_bytes_per_sample=2):
    """what Context.metrics_map with these arguments writes (hmgpu_metrics_map_plan_for: host code, no GPU): an abi.MetricsMapPlan -- the
    block grid, per component the block and the cropped plane, the fields of a map"""
    from . import metrics
    planes = {"pictures": False, "planes": True}[reference]
    desc = abi.make_metrics_desc(abi.METRICS_REF_PLANES if planes else abi.METRICS_REF_PICTURES, metrics.components_mask(components),
                                 1 if ssim else 0, ref_bytes_per_sample if planes else 0, crop)
    return metrics.map_plan_for(seq, desc, abi.make_metrics_map_desc(block))


def histogram_plan(seq, channels=("y", "cb", "cr"), bins=None, crop=(0, 0, 0, 0), matrix=None, full_range=None, rgb_bit_depth=0,
                   histogram=True):
    """what Context.histogram with these arguments counts (hmgpu_histogram_plan_for: host code, no GPU): an abi.HistogramPlan -- per
    channel width, height, depth, log2 of the bins, the bytes of a histogram, and the RGB constants of maxRGB"""
    from . import histogram as hg
    return hg.plan_for(seq, hg.describe(channels, bins, crop, matrix, full_range, rgb_bit_depth, histogram))


def export_scale_taps(seq, desc, scale, chroma, axis):
    """one resampling table of a scaled export (hmgpu_export_scale_taps): (first, count, weights [out, taps]) as numpy arrays"""
    plan = export_scaled_plan(seq, desc, scale)
    taps = max(1, plan.coef[12 + axis])
    n = (scale.width, scale.height)[axis]
    if chroma:
        fmt = seq.chroma_format
        n >>= (0 if fmt == 3 else 1) if axis == 0 else (1 if fmt in (0, 1) else 0)
    first, count = np.zeros(n, np.int32), np.zeros(n, np.int32)
    w = np.zeros((n, taps), np.int16)
    st = lib().hmgpu_export_scale_taps(C.byref(seq), C.byref(desc), C.byref(scale), chroma, axis, taps, first.ctypes.data_as(C.POINTER(C.c_int32)),
                                       count.ctypes.data_as(C.POINTER(C.c_int32)),
                                       w.ctypes.data_as(C.POINTER(C.c_int16)))
    if st != 0:
        raise HmgpuError(st, "hmgpu_export_scale_taps")
    return first, count, w


def packed_max_bytes(seq):
    """worst-case size of a packed picture input (hmgpu_packed_max_bytes)"""
    return int(lib().hmgpu_packed_max_bytes(C.byref(seq)))


def pack_input(seq, meta, coeffs, out=None):
    """HM's arrays (MetaHolder; CoeffHolder with dense levels, or with compact ones as pack_levels returns) -> the packed input
    (hmgpu_pack_input: host code).  out: a uint8 array of at least packed_max_bytes(seq) (e.g. page-locked memory) to pack into;
    returns the blob as a uint8 array (a view of `out` when given).  Raises HmgpuError on a bad status."""
    cap = packed_max_bytes(seq)
    if out is None:
        out = np.zeros(cap + 16, dtype=np.uint8)
        out = out[(-out.ctypes.data) % 16:][:cap]           # (16-byte aligned)
    n = C.c_size_t(0)
    st = lib().hmgpu_pack_input(C.byref(seq), C.byref(meta.struct), C.byref(coeffs.struct), out.ctypes.data, out.nbytes, C.byref(n))
    if st != 0:
        raise HmgpuError(st, "hmgpu_pack_input")
    return out[:n.value]


def unpack_input_status(seq, blob, meta_arrays=None, levels=None, starts=None):
    """hmgpu_unpack_input on a uint8 array; returns the status (no exception): the validator"""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    if blob.ctypes.data % 4:                                 # (the contract asks for a 4-byte aligned blob)
        b = np.zeros(blob.nbytes + 4, dtype=np.uint8)
        b = b[(-b.ctypes.data) % 4:][:blob.nbytes]
        b[:] = blob
        blob = b
    m = abi.MetaHolder(meta_arrays or {})
    out = abi.CtuMetaOut.from_buffer_copy(m.struct)
    lv = (C.c_void_p * 3)(*[None if levels is None else levels[k].ctypes.data for k in range(3)])
    stt = (C.c_void_p * 3)(*[None if starts is None else starts[k].ctypes.data for k in range(3)])
    return int(lib().hmgpu_unpack_input(C.byref(seq), blob.ctypes.data, blob.nbytes, C.byref(out), lv, stt))


def unpack_input(seq, blob):
    """the host reference expansion (hmgpu_unpack_input): returns (meta arrays by abi.META_ARRAYS name, compact levels [3], CTU starts [3])"""
    n, parts, ctu = abi.num_ctus(seq), abi.parts_per_ctu(seq), 1 << seq.log2_ctu_size
    arrays = {}
    for name, dt in abi.META_ARRAYS:
        if name in ("ccp_u", "ccp_v"):
            continue
        shape = (n,) if name in ("slice_idx", "tile_idx") else ((n, parts * 2) if name in ("mv0", "mv1") else (n, parts))
        arrays[name] = np.zeros(shape, dtype=dt)
    levels = [np.zeros(n * ctu * ctu >> (2 if k else 0), dtype=np.int16) for k in range(3)]
    starts = [np.zeros(n + 1, dtype=np.uint32) for _ in range(3)]
    st = unpack_input_status(seq, blob, arrays, levels, starts)
    if st != 0:
        raise HmgpuError(st, "hmgpu_unpack_input")
    return arrays, [levels[k][:int(starts[k][n])] for k in range(3)], starts


class PinnedBuffer:
    """page-locked host memory (hmgpu_host_alloc) as a uint8 array; .free() gives it back"""

    def __init__(self, nbytes):
        self.ptr = lib().hmgpu_host_alloc(nbytes)
        if not self.ptr:
            raise HmgpuError(abi.HMGPU_ENOMEM, "hmgpu_host_alloc")
        self.array = np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_uint8)), shape=(nbytes,))

    def free(self):
        if self.ptr:
            lib().hmgpu_host_free(self.ptr)
            self.ptr, self.array = None, None


class Context:
    """One hmgpu context = one GPU + one HIP stream + a pool of device pictures (HM: one TDecTop)."""

    def __init__(self, seq, device=0):
        self.seq = seq
        self.device = device
        self._h = C.c_void_p()
        st = lib().hmgpu_create(C.byref(seq), device, C.byref(self._h))
        if st != 0:
            raise HmgpuError(st, "hmgpu_create")
        self.num_ctus = lib().hmgpu_num_ctus(C.byref(seq))
        self.parts = lib().hmgpu_parts_per_ctu(C.byref(seq))

    def _chk(self, st, what):
        if st != 0:
            raise HmgpuError(st, what, lib().hmgpu_last_device_error(self._h))

    def close(self):
        if self._h:
            lib().hmgpu_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def chroma_scale(self):
        """(log2 SubWidthC, log2 SubHeightC) of the context's chroma planes; monochrome keeps 4:2:0-shaped dummies"""
        f = self.seq.chroma_format
        return (0 if f == 3 else 1, 1 if f in (0, 1) else 0)

    def sync(self):
        self._chk(lib().hmgpu_sync(self._h), "hmgpu_sync")

    def debug_stall_intra(self, pic, ctu):
        """test hook: the intra wavefront leaves CTU `ctu` of the picture out (-1: off)"""
        self._chk(lib().hmgpu_debug_stall_intra(self._h, pic, ctu), "hmgpu_debug_stall_intra")

    # ---- pictures
    def acquire(self):
        h = C.c_int32(-1)
        self._chk(lib().hmgpu_picture_acquire(self._h, C.byref(h)), "hmgpu_picture_acquire")
        return h.value

    def release(self, pic):
        self._chk(lib().hmgpu_picture_release(self._h, pic), "hmgpu_picture_release")

    def upload(self, pic, planes):
        planes = [np.ascontiguousarray(p, dtype=np.int16) for p in planes]
        ptrs = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
        strides = (C.c_int32 * 3)(*[p.shape[1] for p in planes])
        self._chk(lib().hmgpu_picture_upload(self._h, pic, ptrs, strides), "hmgpu_picture_upload")

    def download(self, pic):
        w, h = self.seq.width, self.seq.height
        sx, sy = self.chroma_scale
        planes = [np.zeros((h, w), dtype=np.int16), np.zeros((h >> sy, w >> sx), dtype=np.int16), np.zeros((h >> sy, w >> sx), dtype=np.int16)]
        ptrs = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
        strides = (C.c_int32 * 3)(*[p.shape[1] for p in planes])
        self._chk(lib().hmgpu_picture_download(self._h, pic, ptrs, strides), "hmgpu_picture_download")
        return planes

    def export_into(self, pic, desc, ptrs, pitches, on_stream=0, stream=0, scale=None):
        """hmgpu_picture_export (scale: an abi.ExportScale, hmgpu_picture_export_scaled) into device memory the caller owns:
        ptrs / pitches (bytes) per plane"""
        p, q = abi.ptr_array(ptrs), abi.i64_array(pitches)
        if scale is None:
            self._chk(lib().hmgpu_picture_export(self._h, pic, C.byref(desc), p, q, on_stream, abi.addr(stream)), "hmgpu_picture_export")
        else:
            self._chk(lib().hmgpu_picture_export_scaled(self._h, pic, C.byref(desc), C.byref(scale), p, q, on_stream, abi.addr(stream)),
                      "hmgpu_picture_export_scaled")

    def export_batch_into(self, pics, desc, ptrs, pitches, bstrides, on_stream=0, stream=0, scale=None, tensor=None, windows=None):
        """hmgpu_pictures_export into device memory the caller owns: plane k of picture i at ptrs[k] + i * bstrides[k] (bytes);
        windows: one abi.ExportWindow per picture (hmgpu_pictures_export_windows, desc.crop 0)"""
        pics = list(pics)
        head = (self._h, len(pics), abi.handle_array(pics), C.byref(desc), abi.ref(scale), abi.ref(tensor))
        tail = (abi.ptr_array(ptrs), abi.i64_array(pitches), abi.i64_array(bstrides), on_stream, abi.addr(stream))
        if windows is not None:
            self._chk(lib().hmgpu_pictures_export_windows(*head, abi.window_array(windows), *tail), "hmgpu_pictures_export_windows")
        else:
            self._chk(lib().hmgpu_pictures_export(*head, *tail), "hmgpu_pictures_export")

    def export_pixels_into(self, pics, desc, pixel, ptr, pitch, bstride, on_stream=0, stream=0, scale=None, tensor=None, windows=None):
        """hmgpu_pictures_export_pixels into device memory the caller owns: pixel x of row y of picture i at
        ptr + i * bstride + y * pitch (bytes); pixel: an abi.ExportPixel; windows: None or one abi.ExportWindow per picture"""
        pics = list(pics)
        self._chk(lib().hmgpu_pictures_export_pixels(self._h, len(pics), abi.handle_array(pics), C.byref(desc), abi.ref(scale), abi.ref(tensor),
                                                     abi.window_array(windows), abi.ref(pixel), abi.addr(ptr), pitch, bstride, on_stream,
                                                     abi.addr(stream)), "hmgpu_pictures_export_pixels")

    def export_pixels_destination_status(self, n, desc, pixel, ptr, pitch, bstride, scale=None, tensor=None, windows=None):
        """hmgpu_export_pixels_destination_check: the status hmgpu_pictures_export_pixels would give this destination; enqueues nothing"""
        return lib().hmgpu_export_pixels_destination_check(self._h, n, C.byref(desc), abi.ref(scale), abi.ref(tensor), abi.window_array(windows),
                                                           abi.ref(pixel), abi.addr(ptr), pitch, bstride)

    def colour_lut(self, lattice, shaper=None, depth=8):
        """a ColourLut of this context (hmgpu_colour_lut_create; include/hmgpu.h "colour export"): lattice None (shaper only) or
        [L, L, L, 3] uint16 output code values of `depth` bits indexed (b, g, r) -- the order of a .cube file -- and shaper None or
        [3, 2^depth] uint16 positions 0 .. 65535 (shaper only: code values).  Pass it as lut= to export / export_batch; a context
        manager."""
        desc, sh, la = colour_lut_arrays(lattice, shaper, depth)
        h = C.c_int64(0)
        self._chk(lib().hmgpu_colour_lut_create(self._h, C.byref(desc), _p(sh) if sh is not None else None,
                                                _p(la) if la is not None else None, C.byref(h)), "hmgpu_colour_lut_create")
        return ColourLut(self, h.value, desc)

    def export_colour_into(self, pics, desc, lut, ptrs, pitches, bstrides, on_stream=0, stream=0, scale=None, tensor=None, windows=None,
                           pixel=None):
        """hmgpu_pictures_export_colour into device memory the caller owns: the RGB export of export_batch_into (pixel None) or of
        export_pixels_into (ptrs[0] / pitches[0] / bstrides[0] the one destination) through `lut`, a ColourLut or a raw handle"""
        pics = list(pics)
        self._chk(lib().hmgpu_pictures_export_colour(self._h, len(pics), abi.handle_array(pics), C.byref(desc), abi.ref(scale), abi.ref(tensor),
                                                     abi.window_array(windows), abi.ref(pixel), getattr(lut, "handle", lut),
                                                     abi.ptr_array(ptrs), abi.i64_array(pitches), abi.i64_array(bstrides), on_stream,
                                                     abi.addr(stream)), "hmgpu_pictures_export_colour")

    def export_colour_destination_status(self, n, desc, lut, ptrs, pitches, bstrides, scale=None, tensor=None, windows=None, pixel=None):
        """hmgpu_export_colour_destination_check: the status hmgpu_pictures_export_colour would give; enqueues nothing"""
        return lib().hmgpu_export_colour_destination_check(self._h, n, C.byref(desc), abi.ref(scale), abi.ref(tensor), abi.window_array(windows),
                                                           abi.ref(pixel), getattr(lut, "handle", lut), abi.ptr_array(ptrs),
                                                           abi.i64_array(pitches), abi.i64_array(bstrides))

    def export_chroma_into(self, pics, desc, chroma, ptrs, pitches, bstrides, on_stream=0, stream=0, scale=None, tensor=None, windows=None,
                           pixel=None, lut=None):
        """hmgpu_pictures_export_chroma into device memory the caller owns: export_colour_into (lut None or 0: no colour stage) with the
        chroma stage of `chroma`, an abi.ExportChroma, in front"""
        pics = list(pics)
        self._chk(lib().hmgpu_pictures_export_chroma(self._h, len(pics), abi.handle_array(pics), C.byref(desc), abi.ref(scale), abi.ref(tensor),
                                                     abi.window_array(windows), abi.ref(pixel), getattr(lut, "handle", lut) or 0,
                                                     abi.ref(chroma), abi.ptr_array(ptrs), abi.i64_array(pitches), abi.i64_array(bstrides),
                                                     on_stream, abi.addr(stream)), "hmgpu_pictures_export_chroma")

    def export_chroma_destination_status(self, n, desc, chroma, ptrs, pitches, bstrides, scale=None, tensor=None, windows=None, pixel=None,
                                         lut=None):
        """hmgpu_export_chroma_destination_check: the status hmgpu_pictures_export_chroma would give; enqueues nothing"""
        return lib().hmgpu_export_chroma_destination_check(self._h, n, C.byref(desc), abi.ref(scale), abi.ref(tensor), abi.window_array(windows),
                                                           abi.ref(pixel), getattr(lut, "handle", lut) or 0, abi.ref(chroma),
                                                           abi.ptr_array(ptrs), abi.i64_array(pitches), abi.i64_array(bstrides))

    def export_format_into(self, pics, desc, format, ptrs, pitches, bstrides, on_stream=0, stream=0, scale=None, tensor=None, windows=None):
        """hmgpu_pictures_export_format into device memory the caller owns: export_batch_into with Cb / Cr at the chroma format of
        `format`, an abi.ExportFormat"""
        pics = list(pics)
        self._chk(lib().hmgpu_pictures_export_format(self._h, len(pics), abi.handle_array(pics), C.byref(desc), abi.ref(scale), abi.ref(tensor),
                                                     abi.window_array(windows), abi.ref(format), abi.ptr_array(ptrs), abi.i64_array(pitches),
                                                     abi.i64_array(bstrides), on_stream, abi.addr(stream)), "hmgpu_pictures_export_format")

    def export_format_destination_status(self, n, desc, format, ptrs, pitches, bstrides, scale=None, tensor=None, windows=None):
        """hmgpu_export_format_destination_check: the status hmgpu_pictures_export_format would give; enqueues nothing"""
        return lib().hmgpu_export_format_destination_check(self._h, n, C.byref(desc), abi.ref(scale), abi.ref(tensor), abi.window_array(windows),
                                                           abi.ref(format), abi.ptr_array(ptrs), abi.i64_array(pitches),
                                                           abi.i64_array(bstrides))

    def export_yuvpack_into(self, pics, desc, format, yuvpack, ptr, pitch, bstride, on_stream=0, stream=0, scale=None, tensor=None, windows=None):
        """hmgpu_pictures_export_yuvpack into device memory the caller owns: picture i's words at ptr + i * bstride (bytes), rows
        pitch apart; format: the abi.ExportFormat of the words' chroma format, yuvpack: an abi.ExportYuvPack"""
        pics = list(pics)
        self._chk(lib().hmgpu_pictures_export_yuvpack(self._h, len(pics), abi.handle_array(pics), abi.ref(desc), abi.ref(scale), abi.ref(tensor),
                                                      abi.window_array(windows), abi.ref(format), abi.ref(yuvpack), abi.ptr_array([ptr]),
                                                      abi.i64_array([pitch]), abi.i64_array([bstride]), on_stream, abi.addr(stream)),
                  "hmgpu_pictures_export_yuvpack")

    def export_yuvpack_status(self, pics, desc, format, yuvpack, ptrs, pitches, bstrides, on_stream=0, stream=0, scale=None, tensor=None,
                              windows=None):
        """hmgpu_pictures_export_yuvpack, the status returned instead of raised; ptrs / pitches / bstrides: up to three each"""
        pics = list(pics)
        return lib().hmgpu_pictures_export_yuvpack(self._h, len(pics), abi.handle_array(pics), abi.ref(desc), abi.ref(scale), abi.ref(tensor),
                                                   abi.window_array(windows), abi.ref(format), abi.ref(yuvpack), abi.ptr_array(ptrs),
                                                   abi.i64_array(pitches), abi.i64_array(bstrides), on_stream, abi.addr(stream))

    def export_yuvpack_destination_status(self, n, desc, format, yuvpack, ptrs, pitches, bstrides, scale=None, tensor=None, windows=None):
        """hmgpu_export_yuvpack_destination_check: the status hmgpu_pictures_export_yuvpack would give; enqueues nothing"""
        return lib().hmgpu_export_yuvpack_destination_check(self._h, n, abi.ref(desc), abi.ref(scale), abi.ref(tensor), abi.window_array(windows),
                                                            abi.ref(format), abi.ref(yuvpack), abi.ptr_array(ptrs), abi.i64_array(pitches),
                                                            abi.i64_array(bstrides))

    def export_warp_into(self, pics, desc, warp, ptrs, pitches, bstrides, on_stream=0, stream=0, tensor=None, windows=None, pixel=None,
                         lut=None, chroma=None):
        """hmgpu_pictures_export_warp into device memory the caller owns: export_chroma_into without a scale (chroma None: replicate),
        every picture through its own inverse affine map; warp: (abi.ExportWarp, abi.WarpMap array), either of them None for NULL"""
        pics = list(pics)
        self._chk(lib().hmgpu_pictures_export_warp(self._h, len(pics), abi.handle_array(pics), C.byref(desc), abi.ref(tensor),
                                                   abi.window_array(windows), abi.ref(pixel), getattr(lut, "handle", lut) or 0,
                                                   abi.ref(chroma), abi.ref(warp[0]), warp[1], abi.ptr_array(ptrs), abi.i64_array(pitches),
                                                   abi.i64_array(bstrides), on_stream, abi.addr(stream)), "hmgpu_pictures_export_warp")

    def export_warp_destination_status(self, n, desc, warp, ptrs, pitches, bstrides, tensor=None, windows=None, pixel=None, lut=None,
                                       chroma=None):
        """hmgpu_export_warp_destination_check: the status hmgpu_pictures_export_warp would give; enqueues nothing"""
        return lib().hmgpu_export_warp_destination_check(self._h, n, C.byref(desc), abi.ref(tensor), abi.window_array(windows), abi.ref(pixel),
                                                         getattr(lut, "handle", lut) or 0, abi.ref(chroma), abi.ref(warp[0]), warp[1],
                                                         abi.ptr_array(ptrs), abi.i64_array(pitches), abi.i64_array(bstrides))

    def export_destination_status(self, n, desc, ptrs, pitches, bstrides, scale=None, tensor=None):
        """hmgpu_export_destination_check: the status hmgpu_pictures_export would give this destination for n pictures; enqueues nothing"""
        return lib().hmgpu_export_destination_check(self._h, n, C.byref(desc), abi.ref(scale), abi.ref(tensor), abi.ptr_array(ptrs),
                                                    abi.i64_array(pitches), abi.i64_array(bstrides))

    def export_windows_destination_status(self, desc, ptrs, pitches, bstrides, windows, scale=None, tensor=None, n=None):
        """hmgpu_export_windows_destination_check: the status hmgpu_pictures_export_windows would give these windows (abi.ExportWindow,
        one per picture; n: another count than len(windows)) and this destination; enqueues nothing"""
        windows = list(windows)
        return lib().hmgpu_export_windows_destination_check(self._h, len(windows) if n is None else n, C.byref(desc), abi.ref(scale),
                                                            abi.ref(tensor), abi.window_array(windows), abi.ptr_array(ptrs),
                                                            abi.i64_array(pitches), abi.i64_array(bstrides))

    def export_stages_into(self, pics, desc, stages, ptrs, pitches, bstrides, on_stream=0, stream=0):
        """the export of `stages` (export.Stages) into device memory the caller owns, through the narrowest hmgpu_pictures_export*
        entry that carries them: yuvpack (YUV interleaved into words: ptrs[0] / pitches[0] / bstrides[0] the one destination), else
        format (the YUV layouts at another chroma format), else warp, else chroma, else colour, else pixels (ptrs[0] / pitches[0] /
        bstrides[0] the one destination),
        else windows or the plain batch -- the only ones that take a YUV layout.  bstrides None: one picture, through
        hmgpu_picture_export(_scaled) where it has integer elements and no further stage, else as a batch of one"""
        s = stages
        if bstrides is None:
            if s[1:] == (None,) * 8:
                return self.export_into(pics[0], desc, ptrs, pitches, on_stream, stream, s.scale)
            from . import export
            bstrides = export.stage_extents(export_stages_plan(self.seq, desc, s.shape_only(), 1), pitches)
        if s.yuvpack is not None:
            return self.export_yuvpack_into(pics, desc, s.format, s.yuvpack, ptrs[0], pitches[0], bstrides[0], on_stream, stream, s.scale, s.tensor,
                                            s.windows)
        if s.format is not None:
            return self.export_format_into(pics, desc, s.format, ptrs, pitches, bstrides, on_stream, stream, s.scale, s.tensor, s.windows)
        if s.warp is not None:
            return self.export_warp_into(pics, desc, s.warp, ptrs, pitches, bstrides, on_stream, stream, s.tensor, s.windows, s.pixel, s.lut, s.chroma)
        if s.chroma is not None:
            return self.export_chroma_into(pics, desc, s.chroma, ptrs, pitches, bstrides, on_stream, stream, s.scale, s.tensor, s.windows, s.pixel,
                                           s.lut)
        if s.lut is not None:
            return self.export_colour_into(pics, desc, s.lut, ptrs, pitches, bstrides, on_stream, stream, s.scale, s.tensor, s.windows, s.pixel)
        if s.pixel is not None:
            return self.export_pixels_into(pics, desc, s.pixel, ptrs[0], pitches[0], bstrides[0], on_stream, stream, s.scale, s.tensor, s.windows)
        return self.export_batch_into(pics, desc, ptrs, pitches, bstrides, on_stream, stream, s.scale, s.tensor, s.windows)

    def export(self, pic, layout="rgb", bit_depth=8, crop=(0, 0, 0, 0), matrix=1, full_range=0, msb_aligned=False, on_stream=True,
               size=None, filter="bilinear", out=None, dtype=None, mean=None, std=None, scale=None, bias=None, pixel=None, alpha=None,
               lut=None, chroma="replicate", chroma_loc=None, warp=None, border="edge", fill=None, chroma_format=None, chroma_down="drop",
               yuv=None, row_align=1):
        """the picture as torch tensors on this context's GPU (libhm_amd.export.export_tensors), written on torch's current stream
        (on_stream) or on the context's own; size (height, width) resizes (filter), out receives it.  dtype: a torch float dtype
        gives normalised float elements (export_batch with one picture, without the batch dimension).  pixel ("rgb", "bgr", "rgba",
        "bgra", "argb", "abgr"; layout "rgb"): one [H, W, C] tensor of packed pixels instead, alpha the A element (None: opaque).
        lut (layout "rgb"): a ColourLut of this context (colour_lut) of the output depth: every pixel through it before the store.
        chroma (layout "rgb"): "replicate", or "linear": Cb and Cr interpolated to the luma grid at chroma_loc, the stream's
        chroma_sample_loc_type 0 .. 5 (None: 0), before the matrix (hmgpu_pictures_export_chroma).
        warp (layout "rgb"): one inverse affine map of six Q16 ints (export.affine_map, export.orientation_map), as export_batch
        takes one per picture; size is then required and is the output size, filter "bilinear" or "nearest", border "edge" or "fill"
        with fill=(r, g, b) (hmgpu_pictures_export_warp).
        chroma_format (layouts "planar" / "semiplanar"): None, or "400" / "420" / "422" / "444" (0 .. 3) -- Cb and Cr at that chroma
        format (hmgpu_pictures_export_format), as export_batch describes; planar with "444" returns ONE [3, H, W] tensor.
        yuv / alpha / row_align: YUV interleaved into words, as export_batch describes, without the batch dimension"""
        from . import export
        os_ = 1 if on_stream else 0
        if yuv is None and row_align != 1:
            raise ValueError("row_align belongs to yuv=")
        if yuv is not None:
            export.yuvpack_only(size=size, dtype=dtype, mean=mean, std=std, scale=scale, bias=bias, pixel=pixel, lut=lut, warp=warp, fill=fill,
                                chroma_format=chroma_format, msb_aligned=msb_aligned)
            return export.export_yuvpack(lambda desc, stages, ptrs, pitches, bstrides, st:
                                         self.export_stages_into([pic], desc, stages, ptrs, pitches, bstrides, os_, st),
                                         self.seq, self.device, yuv, alpha, crop, None, chroma, chroma_down, chroma_loc, on_stream, out, None,
                                         row_align)
        fmt = abi.format_stage(chroma_format, chroma, chroma_down, chroma_loc)
        return export.export_tensors(lambda desc, stages, ptrs, pitches, bstrides, st:
                                     self.export_stages_into([pic], desc, stages, ptrs, pitches, bstrides, os_, st),
                                     self.seq, self.device, layout, bit_depth, crop, matrix, full_range, msb_aligned, on_stream, size, filter,
                                     out, None, dtype, mean, std, scale, bias, pixel=pixel, alpha=alpha, lut=lut,
                                     chroma=abi.chroma_stage(chroma, chroma_loc) if fmt is None else None,
                                     warp=abi.warp_stage(export.one_map(warp), size, filter, border, fill, 1), format=fmt)

    def export_batch(self, pics, layout="rgb", bit_depth=8, crop=(0, 0, 0, 0), matrix=1, full_range=0, msb_aligned=False, on_stream=True,
                     size=None, filter="bilinear", out=None, dtype=None, mean=None, std=None, scale=None, bias=None, windows=None, flip=None,
                     pixel=None, alpha=None, memory_format=None, lut=None, chroma="replicate", chroma_loc=None, warp=None, border="edge",
                     fill=None, chroma_format=None, chroma_down="drop", yuv=None, row_align=1):
        """up to 16 pictures in one call (hmgpu_pictures_export: one launch, the stream ordering once) as one torch tensor per plane
        with a leading batch dimension: RGB [N, 3, H, W]; planar ([N, H, W], ...); semi-planar ([N, H, W], [N, Hc, Wc, 2]).
        dtype None: the unsigned integers of `export`; torch.float16 / bfloat16 / float32: fl(fl(v * scale_k) + bias_k) with
        (scale, bias) = export.affine(output depth, mean, std) -- (v / (2^D - 1) - mean_k) / std_k -- or explicit scale= / bias=
        triples.  out: a tensor (or tuple of planes) of that shape; rows, planes and batch entries may be any stride apart.
        windows: one (x, y, w, h) per picture, luma samples relative to `crop`: the part of the picture slot i shows, resized to
        `size` (size None: all of one (w, h), the output's); flip: one boolean per picture (None: none), the slot mirrored left to
        right.  Still one launch (hmgpu_pictures_export_windows): random-resized-crop and random flip per sample
        (export.random_resized_crop).
        pixel ("rgb", "bgr", "rgba", "bgra", "argb", "abgr"; layout "rgb"): ONE tensor [N, H, W, C] of packed pixels instead
        (hmgpu_pictures_export_pixels), alpha the A element (None: opaque; an integer code value, or a float for float dtypes).
        memory_format=torch.channels_last (layout "rgb", no pixel): a [N, 3, H, W] tensor whose strides are channels-last, the bytes
        of pixel="rgb".  out: either form, its pixels dense.
        lut (layout "rgb"; any of the forms above): a ColourLut of this context (colour_lut) of the output depth -- every output
        pixel goes through its shaper and lattice between the final clip and the store, still in the one launch
        (hmgpu_pictures_export_colour).
        chroma (layout "rgb"; any of the forms above): "replicate", or "linear" -- Cb and Cr of 4:2:0 / 4:2:2 pictures interpolated
        to the luma grid at chroma_loc (chroma_sample_loc_type 0 .. 5; None: 0) before the matrix, still in the one launch
        (hmgpu_pictures_export_chroma).  "replicate" goes through the entries above.
        warp (layout "rgb"; any of the forms above): one inverse affine map per picture, six Q16 ints each or an [n, 6] integer array
        (export.affine_map, export.random_affine, export.orientation_map) -- rotation, shear, zoom, sub-sample shifts and the display
        orientations, still in the one launch (hmgpu_pictures_export_warp).  size is then required and is the output size; the
        windows, the source of each map, may differ in size; filter "bilinear" or "nearest"; border "edge", or "fill" with
        fill=(r, g, b) code values of the output depth.  There is no prefilter: resize by more than about 2x with size= alone.
        chroma_format (layouts "planar" / "semiplanar"; with size, windows, flip, dtype and out): None -- Cb and Cr at the picture's
        own chroma format, through the entries above -- or "400" / "420" / "422" / "444" (0 .. 3): at that format
        (hmgpu_pictures_export_format), still one launch.  Where an axis gains samples chroma= decides: "replicate", or "linear" at
        chroma_loc as for layout "rgb"; where it loses them chroma_down= does: "drop" (every second sample), or "linear" (taps in
        quarters at the same sample location).  4:0:0 pictures give Cb = Cr = half scale, "400" gives Y alone.  The planar layout
        with "444" returns ONE [N, 3, H, W] tensor, Y, Cb and Cr its channels (dtype / mean / std per channel) -- the input of a
        model that takes Y'CbCr; every other case the tuples of the YUV layouts with the new chroma shapes (semi-planar "420" is
        NV12 / P010).  With size= chroma is resampled straight to the output format's chroma size and chroma / chroma_down /
        chroma_loc have no part.
        yuv ("uyvy", "yuy2", "y210", "y216", "v210", "ayuv", "y410", "y416"; with crop, windows, flip, chroma, chroma_down, chroma_loc,
        out and on_stream, and nothing else): Y, Cb and Cr interleaved into the words of that format (hmgpu_pictures_export_yuvpack,
        include/hmgpu.h "packed YUV"), one launch: the values of the planar export at the format's chroma format ("422" / "444") and
        depth (8, 10 or 16), converted by chroma / chroma_down / chroma_loc where the picture's format differs.  alpha: the A of
        "ayuv" (0 .. 255), "y410" (0 .. 3) and "y416" (0 .. 65535); None: 0.  ONE tensor: uint8 [N, H, W, 2] ("uyvy", "yuy2") or
        [N, H, W, 4] ("ayuv"); 16-bit [N, H, W, 2] ("y210", "y216") or [N, H, W, 4] ("y416") in the dtype of the 16-bit exports; int32
        [N, H, W] ("y410"); int32 [N, H, P / 4] ("v210") with P the row's ceil(W / 6) * 16 bytes rounded up to row_align -- 128 gives
        the customary stride (v210 rows are whole dwords: row_align is 1 or a multiple of 4, and 1 rounds to 4); bytes behind the last
        group of a row are not written."""
        from . import export
        pics = list(pics)
        win = export.make_windows(self.seq, crop, windows, flip, len(pics))
        os_ = 1 if on_stream else 0
        if yuv is None and row_align != 1:
            raise ValueError("row_align belongs to yuv=")
        if yuv is not None:
            export.yuvpack_only(size=size, dtype=dtype, mean=mean, std=std, scale=scale, bias=bias, pixel=pixel, memory_format=memory_format,
                                lut=lut, warp=warp, fill=fill, chroma_format=chroma_format, msb_aligned=msb_aligned)
            return export.export_yuvpack(lambda desc, stages, ptrs, pitches, bstrides, st:
                                         self.export_stages_into(pics, desc, stages, ptrs, pitches, bstrides, os_, st),
                                         self.seq, self.device, yuv, alpha, crop, win, chroma, chroma_down, chroma_loc, on_stream, out,
                                         len(pics), row_align)
        fmt = abi.format_stage(chroma_format, chroma, chroma_down, chroma_loc)
        return export.export_tensors(lambda desc, stages, ptrs, pitches, bstrides, st:
                                     self.export_stages_into(pics, desc, stages, ptrs, pitches, bstrides, os_, st),
                                     self.seq, self.device, layout, bit_depth, crop, matrix, full_range, msb_aligned, on_stream, size, filter,
                                     out, len(pics), dtype, mean, std, scale, bias, win, pixel=pixel, alpha=alpha, memory_format=memory_format,
                                     lut=lut, chroma=abi.chroma_stage(chroma, chroma_loc) if fmt is None else None,
                                     warp=abi.warp_stage(warp, size, filter, border, fill, len(pics)), format=fmt)

    # ---- picture import
    def import_into(self, pics, desc, ptrs, pitches, bstrides, on_stream=0, stream=0):
        """hmgpu_pictures_import from device memory the caller owns: plane k of picture i at ptrs[k] + i * bstrides[k] (bytes), rows
        pitches[k] apart; desc: an abi.ImportDesc"""
        pics = list(pics)
        self._chk(lib().hmgpu_pictures_import(self._h, len(pics), abi.handle_array(pics), abi.ref(desc), abi.ptr_array(ptrs),
                                              abi.i64_array(pitches), abi.i64_array(bstrides), on_stream, abi.addr(stream)),
                  "hmgpu_pictures_import")

    def import_status(self, pics, desc, ptrs, pitches, bstrides, on_stream=0, stream=0):
        """import_into, the status returned instead of raised"""
        pics = list(pics)
        return lib().hmgpu_pictures_import(self._h, len(pics), abi.handle_array(pics), abi.ref(desc), abi.ptr_array(ptrs),
                                           abi.i64_array(pitches), abi.i64_array(bstrides), on_stream, abi.addr(stream))

    def import_source_status(self, n, desc, ptrs, pitches, bstrides):
        """hmgpu_import_source_check: the status hmgpu_pictures_import would give this descriptor and source; enqueues nothing"""
        return lib().hmgpu_import_source_check(self._h, n, abi.ref(desc), abi.ptr_array(ptrs), abi.i64_array(pitches),
                                               abi.i64_array(bstrides))

    def import_yuvpack_status(self, pics, desc, yuvpack, ptrs, pitches, bstrides, on_stream=0, stream=0):
        """hmgpu_pictures_import_yuvpack, the status returned: the words of yuvpack (an abi.ImportYuvPack) in ptrs[0], picture i at
        ptrs[0] + i * bstrides[0] (bytes), rows pitches[0] apart; desc: the abi.ImportDesc of the planar source they stand for"""
        pics = list(pics)
        return lib().hmgpu_pictures_import_yuvpack(self._h, len(pics), abi.handle_array(pics), abi.ref(desc), abi.ref(yuvpack),
                                                   abi.ptr_array(ptrs), abi.i64_array(pitches), abi.i64_array(bstrides), on_stream,
                                                   abi.addr(stream))

    def import_yuvpack_into(self, pics, desc, yuvpack, ptr, pitch, bstride, on_stream=0, stream=0):
        """import_yuvpack_status of one source, a refusal raised"""
        self._chk(self.import_yuvpack_status(pics, desc, yuvpack, [ptr], [pitch], [bstride], on_stream, stream), "hmgpu_pictures_import_yuvpack")

    def import_yuvpack_source_status(self, n, desc, yuvpack, ptrs, pitches, bstrides):
        """hmgpu_import_yuvpack_source_check: the status the import would give this descriptor and source; enqueues nothing"""
        return lib().hmgpu_import_yuvpack_source_check(self._h, n, abi.ref(desc), abi.ref(yuvpack), abi.ptr_array(ptrs),
                                                       abi.i64_array(pitches), abi.i64_array(bstrides))

    def import_batch(self, pics, tensors, layout="rgb", pixel=None, bit_depth=None, chroma_format=None, chroma_down="drop", chroma_loc=0,
                     matrix=1, full_range=0, msb_aligned=False, scale=None, bias=None, mean=None, std=None, size=None, on_stream=True,
                     yuv=None):
        """torch tensors on this context's GPU become the samples of up to 16 acquired pictures (hmgpu_pictures_import: one launch,
        no host copy, no wait), read on torch's current stream (on_stream) or on the context's own.  `tensors` is what export_batch
        returns for the same keywords: layout "rgb" one [N, 3, H, W] tensor (channels-last strides go through the packed path) or
        a tuple of three [N, H, W] planes, with pixel= ("rgb", "bgr", "rgba", "bgra", "argb", "abgr") one [N, H, W, C] tensor;
        "planar" a tuple (Y, Cb, Cr) or one [N, 3, H, W] tensor of a 4:4:4 source; "semiplanar" (Y [N, H, W], CbCr [N, Hc, Wc, 2]).
        The element type is the tensors' dtype: uint8, uint16 / int16, or float16 / bfloat16 / float32, which become integers of
        bit_depth as rint(x * scale_k + bias_k) -- scale= / bias= triples, or the inverse of export_batch's mean= / std= convention,
        scale_k = (2^D - 1) * std_k, bias_k = (2^D - 1) * mean_k (defaults: values in [0, 1]).  bit_depth: the source depth, an int
        or (luma, chroma); None: the coding depths.  chroma_format ("400" / "420" / "422" / "444", 0 .. 3; None: the context's):
        the source's format; where the picture has fewer chroma samples chroma_down decides, "drop" or "linear" at chroma_loc.
        size (height, width): the source size when it is smaller than the coded picture (None: the tensors' own), the last column
        and row repeated.  matrix / full_range: of the picture made from RGB.  The pictures are left as `upload` leaves them.
        yuv ("uyvy" ... "y416"; with chroma_down, chroma_loc, size and on_stream only): `tensors` is the ONE tensor of words
        export_batch(yuv=) returns (hmgpu_pictures_import_yuvpack); a "v210" tensor [N, H, P / 4] needs size= where the width is
        not the 6 * P / 16 pixels its rows have room for."""
        from . import imports
        if yuv is not None:
            from . import export
            export.yuvpack_only(pixel=pixel, bit_depth=bit_depth, chroma_format=chroma_format, msb_aligned=msb_aligned, scale=scale, bias=bias,
                                mean=mean, std=std)
            return imports.import_yuvpack(self, list(pics), tensors, yuv, chroma_down, chroma_loc, size, on_stream)
        imports.import_tensors(self, list(pics), tensors, layout, pixel, bit_depth, chroma_format, chroma_down, chroma_loc, matrix,
                               full_range, msb_aligned, scale, bias, mean, std, size, on_stream)

    def import_picture(self, pic, tensors, **kw):
        """import_batch of one picture, its tensors without the batch dimension"""
        from . import imports
        self.import_batch([pic], imports.unsqueeze(tensors), **kw)

    # ---- error concealment
    def conceal_status(self, jobs, check_only=False):
        """hmgpu_pictures_conceal (check_only: hmgpu_conceal_check, nothing enqueued), the status returned; jobs: abi.conceal_job_array"""
        jobs = list(jobs)
        arr, keep = abi.conceal_job_array(jobs, self.num_ctus)       # (keep: the masks live until the call has copied them)
        f = lib().hmgpu_conceal_check if check_only else lib().hmgpu_pictures_conceal
        return f(self._h, len(jobs), arr)

    def conceal(self, jobs):
        """Fill CTUs of up to 16 pictures from other pictures of the context, or with a constant (hmgpu_pictures_conceal: one launch).
        jobs: dicts with dst, src (None: fill), mode ("copy" / "motion"), dst_poc, src_poc, fill, mask (None: every CTU) -- abi.conceal_job_array"""
        jobs = list(jobs)
        self._chk(self.conceal_status(jobs), "hmgpu_pictures_conceal")

    def concealed_ctus(self, pic):
        """hmgpu_picture_concealed_ctus: the CTUs of the picture concealed since it was acquired"""
        n = C.c_int32(-1)
        self._chk(lib().hmgpu_picture_concealed_ctus(self._h, pic, C.byref(n)), "hmgpu_picture_concealed_ctus")
        return n.value

    def export_motion_into(self, pics, desc, ptrs, pitches, pstrides, bstrides, on_stream=0, stream=0, scale=None, windows=None):
        """hmgpu_pictures_export_motion into device memory the caller owns: ptrs / pitches / plane strides / batch strides (bytes) per
        destination slot (abi.MOTION_DST_*: vectors 0 and 1, ref_poc, block; a pointer None / 0 = not written)"""
        from . import motion
        pics = list(pics)
        self._chk(lib().hmgpu_pictures_export_motion(self._h, len(pics), abi.handle_array(pics), C.byref(desc), abi.ref(scale),
                                                     abi.window_array(windows), *motion.c_args(ptrs, pitches, pstrides, bstrides), on_stream,
                                                     abi.addr(stream)), "hmgpu_pictures_export_motion")

    def motion_destination_status(self, n, desc, ptrs, pitches, pstrides, bstrides, scale=None, windows=None):
        """hmgpu_motion_destination_check: the status hmgpu_pictures_export_motion would give this destination; enqueues nothing"""
        from . import motion
        return lib().hmgpu_motion_destination_check(self._h, n, C.byref(desc), abi.ref(scale), abi.window_array(windows),
                                                    *motion.c_args(ptrs, pitches, pstrides, bstrides))

    def export_motion(self, pics, form="blocks", lists=(0, 1), size=None, windows=None, flip=None, dtype=None, out=None, crop=(0, 0, 0, 0),
                      on_stream=True):
        """motion vectors, reference POCs and block information of up to 16 decoded pictures as a dict of torch tensors on this
        context's GPU (libhm_amd.motion: "mv" or "flow0" / "flow1", "ref_poc", "block"), one launch, written on
        torch.cuda.current_stream() (on_stream) or on the context's own stream.  form "blocks": the grid of 4x4 luma blocks, crop in
        multiples of 4 luma samples.  form "dense": one value per output sample of export_batch(windows=, flip=, size=,
        filter="nearest") with the same arguments; dtype torch.float16 / bfloat16 / float32.  out: a dict with some of those keys
        (only they are written); rows, planes and batch entries may be any stride apart.  Pictures that were uploaded, received or
        only partly decoded have no side information (HMGPU_EINVAL)."""
        from . import motion
        pics = list(pics)
        return motion.export_motion(lambda desc, sc, win, ptrs, pitches, pstrides, bstrides, st:
                                    self.export_motion_into(pics, desc, ptrs, pitches, pstrides, bstrides, 1 if on_stream else 0, st, sc, win),
                                    self.seq, self.device, len(pics), form, lists, size, windows, flip, dtype, out, crop)

    def export_residual_into(self, pics, desc, ptrs, pitches, pstrides, bstrides, on_stream=0, stream=0, scale=None, windows=None):
        """hmgpu_pictures_export_residual into device memory the caller owns: ptrs / pitches / plane strides / batch strides (bytes) per
        destination slot (planes: one per component; dense: slot 0; a pointer None / 0 = not written)"""
        from . import residual
        pics = list(pics)
        self._chk(lib().hmgpu_pictures_export_residual(self._h, len(pics), abi.handle_array(pics), C.byref(desc), abi.ref(scale),
                                                       abi.window_array(windows), *residual.c_args(ptrs, pitches, pstrides, bstrides), on_stream,
                                                       abi.addr(stream)), "hmgpu_pictures_export_residual")

    def residual_destination_status(self, n, desc, ptrs, pitches, pstrides, bstrides, scale=None, windows=None):
        """hmgpu_residual_destination_check: the status hmgpu_pictures_export_residual would give this destination; enqueues nothing"""
        from . import residual
        return lib().hmgpu_residual_destination_check(self._h, n, C.byref(desc), abi.ref(scale), abi.window_array(windows),
                                                      *residual.c_args(ptrs, pitches, pstrides, bstrides))

    def residual_status(self, pics):
        """hmgpu_pictures_residual_check: HMGPU_OK when every picture of the list has a residual to export; enqueues nothing"""
        pics = list(pics)
        return lib().hmgpu_pictures_residual_check(self._h, len(pics), abi.handle_array(pics))

    def export_residual(self, pics, form="planes", components=(0, 1, 2), size=None, windows=None, flip=None, dtype=None, scale=None,
                        out=None, crop=(0, 0, 0, 0), on_stream=True):
        """the decoded residual of up to 16 decoded pictures as a dict of torch tensors on this context's GPU (libhm_amd.residual), one
        launch, written on torch.cuda.current_stream() (on_stream) or on the context's own stream.  form "planes": int16 "y" [N, H, W],
        "cb" / "cr" [N, H / 2, W / 2], crop in multiples of 8 luma samples.  form "dense": "residual" [N, C, H, W], one value per output
        sample of export_batch(windows=, flip=, size=, filter="nearest") with the same arguments; dtype None (int16) or torch.float16 /
        bfloat16 / float32 with scale (one factor per component).  out: a dict with some of those keys (only they are written); rows,
        planes and batch entries may be any stride apart.  4:0:0 and 4:2:0 pictures; pictures that were uploaded, received or only
        partly decoded have no residual (HMGPU_EINVAL)."""
        from . import residual
        pics = list(pics)
        return residual.export_residual(lambda desc, sc, win, ptrs, pitches, pstrides, bstrides, st:
                                        self.export_residual_into(pics, desc, ptrs, pitches, pstrides, bstrides, 1 if on_stream else 0, st, sc, win),
                                        self.seq, self.device, len(pics), form, components, size, windows, flip, dtype, scale, out, crop)

    def export_transform_into(self, pics, desc, ptrs, pitches, pstrides, bstrides, on_stream=0, stream=0):
        """hmgpu_pictures_export_transform into device memory the caller owns: ptrs / pitches / plane strides / batch strides (bytes) per
        destination slot (0 .. 2 the component planes, 3 the info grid; a pointer None / 0 = not written)"""
        from . import transform
        pics = list(pics)
        self._chk(lib().hmgpu_pictures_export_transform(self._h, len(pics), abi.handle_array(pics), C.byref(desc),
                                                        *transform.c_args(ptrs, pitches, pstrides, bstrides), on_stream, abi.addr(stream)),
                  "hmgpu_pictures_export_transform")

    def transform_destination_status(self, n, desc, ptrs, pitches, pstrides, bstrides):
        """hmgpu_transform_destination_check: the status hmgpu_pictures_export_transform would give this destination; enqueues nothing"""
        from . import transform
        return lib().hmgpu_transform_destination_check(self._h, n, C.byref(desc), *transform.c_args(ptrs, pitches, pstrides, bstrides))

    def transform_status(self, pics):
        """hmgpu_pictures_transform_check: HMGPU_OK when every picture of the list has levels and arrays to export; enqueues nothing"""
        pics = list(pics)
        return lib().hmgpu_pictures_transform_check(self._h, len(pics), abi.handle_array(pics))

    def export_transform(self, pics, value="levels", components=(0, 1, 2), dtype=None, scale=None, out=None, on_stream=True):
        """the quantised levels ("levels") or the de-quantised transform coefficients ("coeffs") of up to 16 decoded pictures and their
        transform-unit structure as a dict of torch tensors on this context's GPU (libhm_amd.transform), one launch, written on
        torch.cuda.current_stream() (on_stream) or on the context's own stream: "y" [N, H, W], "cb" / "cr" at the format's chroma
        resolution (every block's coefficients at the block's position, 0 elsewhere), "info" int8 [N, 6, H / 4, W / 4].  dtype None
        (int16) or torch.float16 / bfloat16 / float32 with scale (one factor per component).  out: a dict with some of those keys
        (only they are written).  All four chroma formats; pictures that were uploaded, received or only partly decoded give
        HMGPU_EINVAL."""
        from . import transform
        pics = list(pics)
        return transform.export_transform(lambda desc, ptrs, pitches, pstrides, bstrides, st:
                                          self.export_transform_into(pics, desc, ptrs, pitches, pstrides, bstrides, 1 if on_stream else 0, st),
                                          self.seq, self.device, len(pics), value, components, dtype, scale, out)

    def export_loopfilter_into(self, pics, desc, ptrs, pitches, pstrides, bstrides, on_stream=0, stream=0, scale=None, windows=None):
        """hmgpu_pictures_export_loopfilter into device memory the caller owns: ptrs / pitches / plane strides / batch strides (bytes) per
        destination slot (0 the edge grid, 1 the SAO grid, 2 the dense form; a pointer None / 0 = not written)"""
        from . import loopfilter
        pics = list(pics)
        self._chk(lib().hmgpu_pictures_export_loopfilter(self._h, len(pics), abi.handle_array(pics), C.byref(desc), abi.ref(scale),
                                                         abi.window_array(windows), *loopfilter.c_args(ptrs, pitches, pstrides, bstrides),
                                                         on_stream, abi.addr(stream)), "hmgpu_pictures_export_loopfilter")

    def loopfilter_destination_status(self, n, desc, ptrs, pitches, pstrides, bstrides, scale=None, windows=None):
        """hmgpu_loopfilter_destination_check: the status hmgpu_pictures_export_loopfilter would give this destination; enqueues nothing"""
        from . import loopfilter
        return lib().hmgpu_loopfilter_destination_check(self._h, n, C.byref(desc), abi.ref(scale), abi.window_array(windows),
                                                        *loopfilter.c_args(ptrs, pitches, pstrides, bstrides))

    def loopfilter_status(self, pics, need_filter=True):
        """hmgpu_pictures_loopfilter_check: HMGPU_OK when every picture of the list is covered by decompress calls and (need_filter: the
        SAO grid, the dense form) a filter call has run on it; enqueues nothing"""
        pics = list(pics)
        return lib().hmgpu_pictures_loopfilter_check(self._h, len(pics), abi.handle_array(pics), 1 if need_filter else 0)

    def export_loopfilter(self, pics, form="grids", grids=("edge", "sao"), size=None, windows=None, flip=None, dtype=None, scale=None,
                          out=None, crop=(0, 0, 0, 0), on_stream=True):
        """the loop-filter decisions of up to 16 decoded pictures as a dict of torch tensors on this context's GPU (libhm_amd.loopfilter),
        one launch, written on torch.cuda.current_stream() (on_stream) or on the context's own stream.  form "grids": "edge" int16
        [N, 13, H / 4, W / 4] (Bs, mean QP, tc, beta, chroma tc and exemptions of the edge units on every 4x4 block's left and top
        border; crop in multiples of 8 luma samples) and "sao" int8 [N, 3, 6, ctus_h, ctus_w] (type, band and offsets per CTB and
        component); grids= selects one of them.  form "dense": "loopfilter" [N, 3, H, W], one value per output sample of
        export_batch(windows=, flip=, size=, filter="nearest"): Bs of the vertical / horizontal edge that can reach the sample and the
        luma SAO type + 1; dtype None (uint8) or torch.float16 / bfloat16 / float32 with scale (one factor per channel).  out: a dict
        with some of those keys (only they are written).  Pictures that were uploaded, received or only partly decoded give
        HMGPU_EINVAL, and so do the SAO grid and the dense form of a picture no filter call has run on."""
        from . import loopfilter
        pics = list(pics)
        return loopfilter.export_loopfilter(lambda desc, sc, win, ptrs, pitches, pstrides, bstrides, st:
                                            self.export_loopfilter_into(pics, desc, ptrs, pitches, pstrides, bstrides, 1 if on_stream else 0, st, sc, win),
                                            self.seq, self.device, len(pics), form, grids, size, windows, flip, dtype, scale, out, crop)

    def set_streams(self, n):
        """lanes of replay(): 1 = serial kernels, 2 = two half-batches on two streams"""
        self._chk(lib().hmgpu_set_streams(self._h, n), "hmgpu_set_streams")

    def metrics_into(self, pics, desc, results, results_stride, ref_pics=None, ptrs=None, pitches=None, bstrides=None, on_stream=0, stream=0):
        """hmgpu_pictures_metrics into device memory the caller owns: `results` the address of [n][3] records, results_stride bytes
        from picture to picture; ref_pics (handles) or ptrs / pitches / batch strides (bytes) of the reference planes"""
        from . import metrics
        pics = list(pics)
        self._chk(lib().hmgpu_pictures_metrics(self._h, len(pics), abi.handle_array(pics), C.byref(desc),
                                               *metrics.c_args(ref_pics, ptrs, pitches, bstrides), abi.addr(results), results_stride, on_stream,
                                               abi.addr(stream)), "hmgpu_pictures_metrics")

    def metrics_status(self, pics, desc, results, results_stride, ref_pics=None, ptrs=None, pitches=None, bstrides=None):
        """hmgpu_metrics_check: the status hmgpu_pictures_metrics would give these arguments; enqueues nothing"""
        from . import metrics
        pics = list(pics)
        return lib().hmgpu_metrics_check(self._h, len(pics), abi.handle_array(pics), C.byref(desc),
                                         *metrics.c_args(ref_pics, ptrs, pitches, bstrides), abi.addr(results), results_stride)

    def metrics(self, pics, ref_pics=None, ref=None, components=(0, 1, 2), ssim=True, crop=(0, 0, 0, 0), on_stream=True):
        """up to 16 pictures compared on this context's GPU with other pictures of the context (ref_pics: handles) or with planar torch
        tensors (ref: [n, h_c, w_c] per component, uint8 or uint16 / int16 storage): {"y": {...}, "cb": {...}, "cr": {...}}, per
        component int64 tensors [n] of samples, sse, sad, differing, first_diff, ssim_q32, ssim_windows and max_abs (libhm_amd.metrics;
        metrics.psnr / metrics.ssim turn them into HM's PSNR and the mean SSIM).  One launch on torch's current stream (on_stream) or
        the context's own; nothing synchronises."""
        from . import metrics
        pics = list(pics)
        return metrics.metrics(lambda desc, rp, ptrs, pitches, bstrides, res, rs, st:
                               self.metrics_into(pics, desc, res, rs, rp, ptrs, pitches, bstrides, 1 if on_stream else 0, st),
                               self.seq, self.device, len(pics), None if ref_pics is None else list(ref_pics), ref, components, ssim, crop)

    def metrics_map_into(self, pics, desc, map_desc, maps, map_pitches, map_fstrides, map_bstrides, ref_pics=None, ptrs=None, pitches=None,
                         bstrides=None, on_stream=0, stream=0):
        """hmgpu_pictures_metrics_map into device memory the caller owns: maps the addresses of the three components' maps (None: not
        written), map_pitches / map_fstrides / map_bstrides the bytes from row to row, field to field and picture to picture; the
        reference as for metrics_into"""
        from . import metrics
        pics = list(pics)
        self._chk(lib().hmgpu_pictures_metrics_map(self._h, len(pics), abi.handle_array(pics), C.byref(desc), abi.ref(map_desc),
                                                   *metrics.c_args(ref_pics, ptrs, pitches, bstrides),
                                                   *metrics.map_c_args(maps, map_pitches, map_fstrides, map_bstrides), on_stream, abi.addr(stream)),
                  "hmgpu_pictures_metrics_map")

    def metrics_map_status(self, pics, desc, map_desc, maps, map_pitches, map_fstrides, map_bstrides, ref_pics=None, ptrs=None, pitches=None,
                           bstrides=None):
        """hmgpu_metrics_map_check: the status hmgpu_pictures_metrics_map would give these arguments; enqueues nothing"""
        from . import metrics
        pics = list(pics)
        return lib().hmgpu_metrics_map_check(self._h, len(pics), abi.handle_array(pics), C.byref(desc), abi.ref(map_desc),
                                             *metrics.c_args(ref_pics, ptrs, pitches, bstrides),
                                             *metrics.map_c_args(maps, map_pitches, map_fstrides, map_bstrides))

    def metrics_map(self, pics, ref_pics=None, ref=None, block=16, components=(0, 1, 2), ssim=True, crop=(0, 0, 0, 0), on_stream=True):
        """where up to 16 pictures differ from their reference (given as for metrics): per block of block x block luma samples (8, 16, 32
        or 64; a chroma block covers the same area) {"y": {"sse": [n, Hb, Wb], "sad", "differing", "max_abs", "ssim_q32",
        "ssim_windows"}, "cb": ..., "cr": ...}, int64 tensors on the device (libhm_amd.metrics: map_psnr, map_ssim, mismatch_blocks).
        Summed over the blocks a field is the field Context.metrics gives.  One launch on torch's current stream (on_stream) or the
        context's own; nothing synchronises."""
        from . import metrics
        pics = list(pics)
        return metrics.metrics_map(lambda desc, md, rp, ptrs, pitches, bstrides, maps, mp, mf, mb, st:
                                   self.metrics_map_into(pics, desc, md, maps, mp, mf, mb, rp, ptrs, pitches, bstrides, 1 if on_stream else 0, st),
                                   self.seq, self.device, len(pics), None if ref_pics is None else list(ref_pics), ref, block, components, ssim,
                                   crop)

    def histogram_into(self, pics, desc, records, records_stride, ptrs=None, strides=None, on_stream=0, stream=0):
        """hmgpu_pictures_histogram into device memory the caller owns: `records` the address of [n][4] records, records_stride bytes
        from picture to picture; ptrs / strides: per channel the address of its n histograms and the bytes from one to the next"""
        from . import histogram as hg
        pics = list(pics)
        self._chk(lib().hmgpu_pictures_histogram(self._h, len(pics), abi.handle_array(pics), C.byref(desc), *hg.c_args(ptrs, strides),
                                                 abi.addr(records), records_stride, on_stream, abi.addr(stream)), "hmgpu_pictures_histogram")

    def histogram_status(self, pics, desc, records, records_stride, ptrs=None, strides=None):
        """hmgpu_histogram_check: the status hmgpu_pictures_histogram would give these arguments; enqueues nothing"""
        from . import histogram as hg
        pics = list(pics)
        return lib().hmgpu_histogram_check(self._h, len(pics), abi.handle_array(pics), C.byref(desc), *hg.c_args(ptrs, strides),
                                           abi.addr(records), records_stride)

    def histogram(self, pics, channels=("y", "cb", "cr"), bins=None, crop=(0, 0, 0, 0), matrix=None, full_range=None, rgb_bit_depth=0,
                  histogram=True, on_stream=True):
        """what up to 16 pictures contain, counted on this context's GPU: {"y": {...}, "cb": {...}, "cr": {...}, "maxrgb": {...}}, per
        channel "hist" (int32 [n, bins]; one bin per code value, or bins= a power of two 16 .. 4096; absent with histogram=False) and
        tensors [n] of samples, sum, sum_sq (int64), min and max (int32) over the values (libhm_amd.histogram; its mean / variance / percentile /
        distance / light_level read them).  "maxrgb" is max(R, G, B) of the RGB export with the same crop, matrix and full_range (None:
        BT.709, limited) at rgb_bit_depth bits (0: the luma coding depth).  One launch on torch's current stream (on_stream) or the
        context's own; nothing synchronises."""
        from . import histogram as hg
        pics = list(pics)
        return hg.histogram(lambda desc, ptrs, strides, rec, rs, st:
                            self.histogram_into(pics, desc, rec, rs, ptrs, strides, 1 if on_stream else 0, st),
                            self.seq, self.device, len(pics), channels, bins, crop, matrix, full_range, rgb_bit_depth, histogram)

    def download_packed(self, pic, bytes_per_sample, crop=(0, 0, 0, 0)):
        """the picture as 8- or 16-bit planes cropped by (left, right, top, bottom) luma samples"""
        l, r, t, b = crop
        W, H = self.seq.width - l - r, self.seq.height - t - b
        dt = np.uint8 if bytes_per_sample == 1 else np.uint16
        sx, sy = self.chroma_scale
        planes = [np.zeros((H, W), dtype=dt), np.zeros((H >> sy, W >> sx), dtype=dt), np.zeros((H >> sy, W >> sx), dtype=dt)]
        ptrs = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
        strides = (C.c_int32 * 3)(*[p.strides[0] for p in planes])
        self._chk(lib().hmgpu_picture_download_packed(self._h, pic, ptrs, strides, bytes_per_sample, l, r, t, b), "hmgpu_picture_download_packed")
        return planes

    def picture_hash(self, pic, method):
        """method 1 = MD5, 2 = CRC, 3 = checksum (decoded-picture-hash SEI); returns the bytes of Y, Cb, Cr concatenated"""
        dig = (C.c_uint8 * 48)()
        n = C.c_int32()
        self._chk(lib().hmgpu_picture_hash(self._h, pic, method, dig, C.byref(n)), "hmgpu_picture_hash")
        return np.array([dig[16 * k + i] for k in range(3) for i in range(n.value)], dtype=np.uint8)

    # ---- frame-parallel exchange (hmgpu.h: hmgpu_picture_device_region)
    def device_region(self, pic, receive=False):
        """(device address, bytes) of the contiguous plane region of `pic`: the finished picture, or where to receive one"""
        base, nbytes = C.c_void_p(), C.c_int64()
        self._chk(lib().hmgpu_picture_device_region(self._h, pic, 1 if receive else 0, C.byref(base), C.byref(nbytes)),
                  "hmgpu_picture_device_region")
        return int(base.value), int(nbytes.value)

    def commit_received(self, pic):
        self._chk(lib().hmgpu_picture_commit_received(self._h, pic), "hmgpu_picture_commit_received")

    def transfer_to(self, pic, other, other_pic):
        """the finished picture `pic` into picture `other_pic` of another context (same process; another GPU or this one)"""
        self._chk(lib().hmgpu_picture_transfer(self._h, pic, other._h, other_pic), "hmgpu_picture_transfer")

    @property
    def transfer_bytes(self):
        return int(lib().hmgpu_transfer_bytes(self._h))

    def stream_handle(self):
        return int(lib().hmgpu_stream(self._h) or 0)

    # ---- the two calls
    def decompress_slice(self, pic, slice_idx, slice_params, meta, coeffs, first_ctu=0, num_ctus=None):
        n = self.num_ctus - first_ctu if num_ctus is None else num_ctus
        st = lib().hmgpu_decompress_slice(self._h, pic, slice_idx, C.byref(slice_params), C.byref(meta.struct),
                                          C.byref(coeffs.struct), first_ctu, n)
        self._chk(st, "hmgpu_decompress_slice")

    def filter_picture(self, pic, pic_params, sao_raw=None, stages=7):
        arr = abi.sao_array_from_raw(sao_raw) if sao_raw is not None else None
        st = lib().hmgpu_filter_picture_stages(self._h, pic, C.byref(pic_params), arr, stages)
        self._chk(st, "hmgpu_filter_picture_stages")

    # ---- the same for several independent pictures per call
    @staticmethod
    def picture_jobs(jobs):
        """jobs: [(pic, [slice_params, ...], meta, coeffs), ...] with meta / coeffs anything that has .struct (MetaHolder, CoeffHolder)
        or a StagingHolder passed for both -> the C array (reusable; keeps what it points to alive)"""
        arr = (abi.PictureJob * len(jobs))()
        arr._keep = [jobs]
        for i, (pic, slices, meta, coeffs) in enumerate(jobs):
            sl = (C.POINTER(abi.SliceParams) * len(slices))(*[C.pointer(s) for s in slices])
            arr._keep.append(sl)
            arr[i].pic, arr[i].num_slices, arr[i].slices = pic, len(slices), sl
            arr[i].meta = C.pointer(meta.struct)
            arr[i].coeffs = C.pointer(coeffs.coeffs if isinstance(coeffs, abi.StagingHolder) else coeffs.struct)
        return arr

    @staticmethod
    def filter_jobs(jobs):
        """jobs: [(pic, pic_params, sao_array or None), ...]; sao_array = abi.sao_array_from_raw(...)"""
        arr = (abi.FilterJob * len(jobs))()
        arr._keep = [jobs]
        for i, (pic, pp, sao) in enumerate(jobs):
            arr[i].pic, arr[i].pp = pic, C.pointer(pp)
            arr[i].sao = C.cast(sao, C.c_void_p) if sao is not None else None
        return arr

    def decompress_pictures(self, jobs):
        arr = jobs if isinstance(jobs, C.Array) else self.picture_jobs(jobs)
        self._chk(lib().hmgpu_decompress_pictures(self._h, len(arr), arr), "hmgpu_decompress_pictures")

    @staticmethod
    def packed_jobs(jobs):
        """jobs: [(pic, [slice_params, ...], blob (uint8 array from pack_input), pcm (three int16 arrays) or None), ...] -> the C array"""
        arr = (abi.PackedJob * len(jobs))()
        arr._keep = [jobs]
        for i, job in enumerate(jobs):
            pic, slices, blob = job[:3]
            pcm = job[3] if len(job) > 3 else None
            sl = (C.POINTER(abi.SliceParams) * len(slices))(*[C.pointer(s) for s in slices])
            arr._keep.append(sl)
            arr[i].pic, arr[i].num_slices, arr[i].slices = pic, len(slices), sl
            arr[i].blob, arr[i].bytes = blob.ctypes.data, blob.nbytes
            if pcm is not None:
                for k in range(3):
                    arr[i].pcm_sample[k] = pcm[k].ctypes.data
        return arr

    def decompress_pictures_packed(self, jobs):
        """hmgpu_decompress_pictures with packed inputs (see packed_jobs)"""
        arr = jobs if isinstance(jobs, C.Array) else self.packed_jobs(jobs)
        self._chk(lib().hmgpu_decompress_pictures_packed(self._h, len(arr), arr), "hmgpu_decompress_pictures_packed")

    def packed_wait(self, blob):
        self._chk(lib().hmgpu_packed_wait(self._h, blob.ctypes.data), "hmgpu_packed_wait")

    def filter_pictures(self, jobs):
        arr = jobs if isinstance(jobs, C.Array) else self.filter_jobs(jobs)
        self._chk(lib().hmgpu_filter_pictures(self._h, len(arr), arr), "hmgpu_filter_pictures")

    def staging_alloc(self):
        h = C.c_void_p()
        m, co = abi.CtuMeta(), abi.Coeffs()
        self._chk(lib().hmgpu_staging_alloc(self._h, C.byref(h), C.byref(m), C.byref(co)), "hmgpu_staging_alloc")
        return abi.StagingHolder(h, m, co, self.num_ctus, abi.parts_per_ctu(self.seq), 1 << self.seq.log2_ctu_size,
                                 chroma_shift=sum(self.chroma_scale))

    def pack_levels(self, meta, coeffs):
        return pack_levels(self.seq, meta, coeffs)

    def staging_free(self, st):
        lib().hmgpu_staging_free(self._h, st.handle)

    def replay(self, pics, stages, iters):
        pics = list(pics) if isinstance(pics, (list, tuple)) else [pics]
        arr = (C.c_int32 * len(pics))(*pics)
        self._chk(lib().hmgpu_replay_batch(self._h, arr, len(pics), stages, iters), "hmgpu_replay_batch")

    def set_profiling(self, on):
        self._chk(lib().hmgpu_set_profiling(self._h, int(on)), "hmgpu_set_profiling")

    def stats(self, reset=False):
        s = abi.Stats()
        self._chk(lib().hmgpu_get_stats(self._h, C.byref(s), int(reset)), "hmgpu_get_stats")
        out = {"intra_partitions": int(s.intra_partitions), "inter_partitions": int(s.inter_partitions), "kernels": {}}
        for k in range(abi.NUM_KERNELS):
            out["kernels"][lib().hmgpu_kernel_name(k).decode()] = (float(s.kernel_ms[k]), int(s.kernel_launches[k]))
        return out

    # ---- finer seams
    def inverse_transform_batch(self, levels, log2_size, bit_depth, qp_per, qp_rem, flags):
        levels = np.ascontiguousarray(levels, dtype=np.int16)
        n = levels.shape[0]
        per = np.ascontiguousarray(qp_per, dtype=np.int8)
        rem = np.ascontiguousarray(qp_rem, dtype=np.int8)
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        out = np.zeros_like(levels)
        st = lib().hmgpu_inverse_transform_batch(self._h, log2_size, bit_depth, n, _p(levels), _p(per), _p(rem), _p(fl), _p(out))
        self._chk(st, "hmgpu_inverse_transform_batch")
        return out

    def mc_batch(self, is_chroma, bit_depth, plane, blocks, bi):
        """blocks: int32 [n, 6] = x, y, w, h, mvx, mvy.  returns list of (h, w) arrays"""
        plane = np.ascontiguousarray(plane, dtype=np.int16)
        blocks = np.ascontiguousarray(blocks, dtype=np.int32)
        total = int((blocks[:, 2] * blocks[:, 3]).sum())
        dst = np.zeros(total, dtype=np.int16)
        st = lib().hmgpu_mc_batch(self._h, int(is_chroma), bit_depth, _p(plane), plane.shape[1], plane.shape[1], plane.shape[0],
                                  blocks.shape[0], _p(blocks), int(bi), _p(dst))
        self._chk(st, "hmgpu_mc_batch")
        out, pos = [], 0
        for b in blocks:
            w, h = int(b[2]), int(b[3])
            out.append(dst[pos:pos + w * h].reshape(h, w))
            pos += w * h
        return out
