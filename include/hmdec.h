/* hmdec.h -- C interface of libhmdec.so: a complete HEVC (Main / Main10) decoder whose pixel path is libhmgpu (MI355X) and whose
 * bitstream side is a from-scratch host parser.
 *
 * The first block below is call-compatible with ChristianFeldmann/libHM's libHMDecoder (source/App/libHMDecoder/libHMDecoder.h:111-298):
 * same names, argument lists, enumerator values and protocol, so a client built against that header links against libhmdec.so
 * unchanged.  Each declaration cites the function it stands in for.  The protocol in short:
 *
 *   ctx = libHMDec_new_decoder();
 *   for every NAL unit:  libHMDec_push_nal_unit(ctx, data, len, eof, newPicture, checkOutput);
 *                        if (newPicture)  push the same unit again after draining the output
 *                        if (checkOutput) while ((pic = libHMDec_get_picture(ctx))) { ... libHMDEC_get_image_plane(pic, c) ... }
 *   libHMDec_free_decoder(ctx);
 *
 * The second block (hmdec_*) is this library's own: device selection, a parse-only mode for hosts without a GPU, and read access
 * to what the parser produced (the arrays that cross include/hmgpu.h), which the parity tests compare with HM's.
 */
#ifndef HMDEC_H
#define HMDEC_H

#include <stdint.h>

#ifdef __cplusplus
#include <vector>
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------- libHMDecoder-compatible part */
typedef enum { LIBHMDEC_OK = 0, LIBHMDEC_ERROR, LIBHMDEC_ERROR_READ_ERROR } libHMDec_error;            /* libHMDecoder.h:99-104 */
typedef void libHMDec_context;
typedef void libHMDec_picture;
typedef enum { LIBHMDEC_LUMA = 0, LIBHMDEC_CHROMA_U, LIBHMDEC_CHROMA_V } libHMDec_ColorComponent;     /* :166-171 */
typedef enum { LIBHMDEC_CHROMA_400 = 0, LIBHMDEC_CHROMA_420, LIBHMDEC_CHROMA_422, LIBHMDEC_CHROMA_444, LIBHMDEC_CHROMA_UNKNOWN } libHMDec_ChromaFormat; /* :222-229 */

const char* libHMDec_get_version(void);                                       /* :108  "16.0": the HM version whose output is matched */
libHMDec_context* libHMDec_new_decoder(void);                                 /* :119 */
libHMDec_error libHMDec_free_decoder(libHMDec_context* decCtx);               /* :125 */
void libHMDec_set_SEI_Check(libHMDec_context* decCtx, bool check_hash);       /* :132  decoded-picture-hash SEI check on/off (default on) */
void libHMDec_set_max_temporal_layer(libHMDec_context* decCtx, int max_layer);/* :139  -1 = all layers */
#ifdef __cplusplus
/* :152  one NAL unit, start code optional.  bNewPicture: the unit opened a new picture, the finished one may now be read, and the
 * unit must be pushed again.  checkOutputPictures: call libHMDec_get_picture until it returns NULL. */
libHMDec_error libHMDec_push_nal_unit(libHMDec_context* decCtx, const void* data8, int length, bool eof, bool& bNewPicture, bool& checkOutputPictures);
#endif
libHMDec_picture* libHMDec_get_picture(libHMDec_context* decCtx);             /* :180  next picture in output order or NULL */
int libHMDEC_get_POC(libHMDec_picture* pic);                                  /* :188 */
int libHMDEC_get_picture_width(libHMDec_picture* pic, libHMDec_ColorComponent c);   /* :196  coded size, conformance window not applied */
int libHMDEC_get_picture_height(libHMDec_picture* pic, libHMDec_ColorComponent c);  /* :200 */
int libHMDEC_get_picture_stride(libHMDec_picture* pic, libHMDec_ColorComponent c);  /* :208  in samples */
short* libHMDEC_get_image_plane(libHMDec_picture* pic, libHMDec_ColorComponent c);  /* :217  valid until the picture buffer is reused */
libHMDec_ChromaFormat libHMDEC_get_chroma_format(libHMDec_picture* pic);      /* :235 */
int libHMDEC_get_internal_bit_depth(libHMDec_ColorComponent c);               /* :241  of the most recently activated SPS (HM: a global) */

typedef struct { unsigned short x, y, w, h; int value; int value2; } libHMDec_BlockValue;   /* :248-253 */
typedef enum {                                                                /* :257-282 */
  LIBHMDEC_CTU_SLICE_INDEX = 0, LIBHMDEC_CU_PREDICTION_MODE, LIBHMDEC_CU_TRQ_BYPASS, LIBHMDEC_CU_SKIP_FLAG, LIBHMDEC_CU_PART_MODE,
  LIBHMDEC_CU_INTRA_MODE_LUMA, LIBHMDEC_CU_INTRA_MODE_CHROMA, LIBHMDEC_CU_ROOT_CBF, LIBHMDEC_PU_MERGE_FLAG, LIBHMDEC_PU_MERGE_INDEX,
  LIBHMDEC_PU_UNI_BI_PREDICTION, LIBHMDEC_PU_REFERENCE_POC_0, LIBHMDEC_PU_MV_0, LIBHMDEC_PU_REFERENCE_POC_1, LIBHMDEC_PU_MV_1,
  LIBHMDEC_TU_CBF_Y, LIBHMDEC_TU_CBF_CB, LIBHMDEC_TU_CBF_CR, LIBHMDEC_TU_COEFF_TR_SKIP_Y, LIBHMDEC_TU_COEFF_TR_SKIP_Cb,
  LIBHMDEC_TU_COEFF_TR_SKIP_Cr, LIBHMDEC_TU_COEFF_ENERGY_Y, LIBHMDEC_TU_COEFF_ENERGY_CB, LIBHMDEC_TU_COEFF_ENERGY_CR
} libHMDec_info_type;
#ifdef __cplusplus
std::vector<libHMDec_BlockValue>* libHMDEC_get_internal_info(libHMDec_context* decCtx, libHMDec_picture* pic, libHMDec_info_type type);  /* :293 */
#endif
libHMDec_error libHMDEC_clear_internal_info(libHMDec_context* decCtx);        /* :300 */

/* ---------------------------------------------------------------------------------------------- this library's own additions */
void hmdec_set_device(libHMDec_context* ctx, int device_ordinal);             /* GPU to decode on (default 0); before the first NAL unit */
/* Several device contexts, one per entry (GPU ordinals; the same ordinal twice: two contexts on one GPU).  The pictures libHM would
 * reconstruct one after the other and that do not predict from each other -- the B pictures of one temporal level, TDecTop.cpp:672 /
 * TDecGop.cpp:105 per picture -- are placed round-robin on the contexts; a reference picture is copied once to each context that
 * predicts from it (hmgpu_picture_transfer: over xGMI between GPUs), reference picture sets and lists (TComSlice.cpp:318-376), hash
 * checks and the output order (TDecTop.cpp:192-213) are as with one.  Before the first NAL unit.  hmdec_transfer_bytes: bytes copied. */
void hmdec_set_devices(libHMDec_context* ctx, const int* device_ordinals, int n);
int hmdec_num_devices(libHMDec_context* ctx);
unsigned long long hmdec_transfer_bytes(libHMDec_context* ctx);
/* parser threads (1..16, default 1): slice data of several pictures is parsed concurrently (frame-parallel, a picture at most one
 * CTB row behind the picture it takes temporal motion vectors from); pictures come out in the same order, later.  Before the first NAL unit. */
void hmdec_set_threads(libHMDec_context* ctx, int n);
void hmdec_set_parse_only(libHMDec_context* ctx, int on);                     /* no device work: parser output only (planes unavailable) */
/* before the first NAL unit: 4:0:0 / 4:2:0 pictures are packed (hmgpu_pack_input, into page-locked memory) and handed over through
 * hmgpu_decompress_pictures_packed; other pictures, and a picture the packer refuses, take the array path.  Off by default. */
void hmdec_set_packed_input(libHMDec_context* ctx, int on);
/* Device output (before the first NAL unit, off by default): libHMDec_get_picture no longer downloads the planes of the pictures it
 * puts out; libHMDEC_get_image_plane and hmdec_picture_array("plane*") download them when first asked.  hmdec_picture_export converts
 * a picture into caller device memory (hmgpu_picture_export on the context that holds it; returns an hmgpu_status).  It is valid from
 * libHMDec_get_picture until the next libHMDec_push_nal_unit; a picture of a sequence that has ended (its context is gone) gives
 * HMGPU_EINVAL.  hmdec_download_bytes: plane bytes copied device -> host so far, for any reason (output, host hash checks). */
#ifndef HMGPU_H
typedef struct hmgpu_export_desc hmgpu_export_desc;
typedef struct hmgpu_export_scale hmgpu_export_scale;
typedef struct hmgpu_export_tensor hmgpu_export_tensor;
typedef struct hmgpu_export_window hmgpu_export_window;
typedef struct hmgpu_export_pixel hmgpu_export_pixel;
typedef struct hmgpu_colour_lut_desc hmgpu_colour_lut_desc;
typedef struct hmgpu_export_chroma hmgpu_export_chroma;
typedef struct hmgpu_export_format hmgpu_export_format;
typedef struct hmgpu_export_yuvpack hmgpu_export_yuvpack;
typedef struct hmgpu_export_warp hmgpu_export_warp;
typedef struct hmgpu_warp_map hmgpu_warp_map;
typedef struct hmgpu_motion_desc hmgpu_motion_desc;
typedef struct hmgpu_residual_desc hmgpu_residual_desc;
typedef struct hmgpu_transform_desc hmgpu_transform_desc;
typedef struct hmgpu_loopfilter_desc hmgpu_loopfilter_desc;
typedef struct hmgpu_metrics_desc hmgpu_metrics_desc;
typedef struct hmgpu_metrics_map_desc hmgpu_metrics_map_desc;
typedef struct hmgpu_histogram_desc hmgpu_histogram_desc;
#endif
void hmdec_set_device_output(libHMDec_context* ctx, int on);
int hmdec_picture_export(libHMDec_context* ctx, libHMDec_picture* pic, const hmgpu_export_desc* desc, void* const dst[3],
                         const int64_t pitch_bytes[3], int on_stream, void* stream);
/* the same with scaling (hmgpu_picture_export_scaled), under the same rules */
int hmdec_picture_export_scaled(libHMDec_context* ctx, libHMDec_picture* pic, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                void* const dst[3], const int64_t pitch_bytes[3], int on_stream, void* stream);
/* Up to 16 pictures in one call (hmgpu_pictures_export: scale NULL = unscaled, tensor NULL = unsigned integers; plane k of picture i at
 * dst[k] + i * batch_stride_bytes[k]).  Every picture must have been put out by this decoder and still be valid (fetched since the last
 * push), be of one sequence and sit on one GPU ordinal, else HMGPU_EINVAL and nothing is written.  With hmdec_set_devices the pictures
 * may sit in several device contexts of that GPU: the destination is validated once for the whole batch
 * (hmgpu_export_destination_check), then each context gets one call for its slots (more where its slots are not equally far apart). */
int hmdec_pictures_export(libHMDec_context* ctx, int n, libHMDec_picture* const pics[], const hmgpu_export_desc* desc,
                          const hmgpu_export_scale* scale, const hmgpu_export_tensor* tensor, void* const dst[3],
                          const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3], int on_stream, void* stream);
/* hmdec_pictures_export with a source window and a mirror flag per picture (hmgpu_pictures_export_windows: desc->crop 0, windows[i] for
 * pics[i]), under the same rules.  Where the pictures sit in several device contexts of the GPU the destination and every window are
 * validated once for the whole batch (hmgpu_export_windows_destination_check), then each run of slots carries its own windows. */
int hmdec_pictures_export_windows(libHMDec_context* ctx, int n, libHMDec_picture* const pics[], const hmgpu_export_desc* desc,
                                  const hmgpu_export_scale* scale, const hmgpu_export_tensor* tensor, const hmgpu_export_window windows[],
                                  void* const dst[3], const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3], int on_stream,
                                  void* stream);
/* hmdec_pictures_export as packed pixels (hmgpu_pictures_export_pixels: RGB / BGR / RGBA / BGRA / ARGB / ABGR into the one destination
 * dst, pixel x of row y of picture i at dst + i * batch_stride_bytes + y * pitch_bytes; windows NULL or one per picture), under the
 * same rules.  Where the pictures sit in several device contexts of the GPU the destination, the pixel description and every window
 * are validated once for the whole batch (hmgpu_export_pixels_destination_check), then each run of slots carries its own windows. */
int hmdec_pictures_export_pixels(libHMDec_context* ctx, int n, libHMDec_picture* const pics[], const hmgpu_export_desc* desc,
                                 const hmgpu_export_scale* scale, const hmgpu_export_tensor* tensor, const hmgpu_export_window windows[],
                                 const hmgpu_export_pixel* pixel, void* dst, int64_t pitch_bytes, int64_t batch_stride_bytes, int on_stream,
                                 void* stream);
/* A colour LUT of the decoder (include/hmgpu.h "colour export"): the decoder validates the tables (hmgpu_colour_lut_check) and keeps
 * a host copy; the LUT is created in a device context when an export first needs it there and goes with the contexts of a sequence
 * that ends (the next sequence's contexts get it the same way).  *out: a handle of this decoder, never 0.  hmdec_colour_lut_destroy
 * releases it everywhere; an unknown handle is HMGPU_EINVAL. */
int hmdec_colour_lut_create(libHMDec_context* ctx, const hmgpu_colour_lut_desc* desc, const uint16_t* shaper, const uint16_t* lattice,
                            int64_t* out);
int hmdec_colour_lut_destroy(libHMDec_context* ctx, int64_t lut);
/* hmdec_pictures_export / _windows / _pixels (windows NULL: desc->crop; pixel NULL: three planes, else packed pixels in dst[0]) through
 * the colour stage of `lut` (hmgpu_pictures_export_colour), under the same rules: the whole batch is validated once
 * (hmgpu_export_colour_destination_check), then each run of slots of a device context is one call. */
int hmdec_pictures_export_colour(libHMDec_context* ctx, int n, libHMDec_picture* const pics[], const hmgpu_export_desc* desc,
                                 const hmgpu_export_scale* scale, const hmgpu_export_tensor* tensor, const hmgpu_export_window windows[],
                                 const hmgpu_export_pixel* pixel, int64_t lut, void* const dst[3], const int64_t pitch_bytes[3],
                                 const int64_t batch_stride_bytes[3], int on_stream, void* stream);
/* hmdec_pictures_export_colour with the chroma stage of `chroma` in front (hmgpu_pictures_export_chroma; include/hmgpu.h "chroma
 * export"): lut 0 means no colour stage.  The whole batch is validated once (hmgpu_export_chroma_destination_check), then each run of
 * slots of a device context is one call.  The caller names the sample location; hmdec_picture_chroma_loc reports the stream's. */
int hmdec_pictures_export_chroma(libHMDec_context* ctx, int n, libHMDec_picture* const pics[], const hmgpu_export_desc* desc,
                                 const hmgpu_export_scale* scale, const hmgpu_export_tensor* tensor, const hmgpu_export_window windows[],
                                 const hmgpu_export_pixel* pixel, int64_t lut, const hmgpu_export_chroma* chroma, void* const dst[3],
                                 const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3], int on_stream, void* stream);
/* hmdec_pictures_export / _windows (windows NULL: desc->crop) of the planar and semi-planar layouts with Cb / Cr at the chroma format
 * of `format` (hmgpu_pictures_export_format; include/hmgpu.h "format export").  The whole batch is validated once
 * (hmgpu_export_format_destination_check), then each run of slots of a device context is one call.  The caller names the sample
 * location; hmdec_picture_chroma_loc reports the stream's. */
int hmdec_pictures_export_format(libHMDec_context* ctx, int n, libHMDec_picture* const pics[], const hmgpu_export_desc* desc,
                                 const hmgpu_export_scale* scale, const hmgpu_export_tensor* tensor, const hmgpu_export_window windows[],
                                 const hmgpu_export_format* format, void* const dst[3], const int64_t pitch_bytes[3],
                                 const int64_t batch_stride_bytes[3], int on_stream, void* stream);
/* Y, Cb and Cr interleaved into the words of `pack` (hmgpu_pictures_export_yuvpack; include/hmgpu.h "packed YUV"): the arguments of
 * hmdec_pictures_export_format and the word format, dst[0] the one destination.  The whole batch is validated once
 * (hmgpu_export_yuvpack_destination_check), then each run of slots of a device context is one call. */
int hmdec_pictures_export_yuvpack(libHMDec_context* ctx, int n, libHMDec_picture* const pics[], const hmgpu_export_desc* desc,
                                  const hmgpu_export_scale* scale, const hmgpu_export_tensor* tensor, const hmgpu_export_window windows[],
                                  const hmgpu_export_format* format, const hmgpu_export_yuvpack* pack, void* const dst[3],
                                  const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3], int on_stream, void* stream);
/* The RGB exports through one inverse affine map per picture (hmgpu_pictures_export_warp; include/hmgpu.h "affine warp export"): the
 * arguments of hmdec_pictures_export_chroma without `scale` (chroma NULL: replicate; lut 0: no colour stage), then the warp
 * descriptor and n maps.  The whole batch is validated once (hmgpu_export_warp_destination_check), then each run of slots of a device
 * context is one call with the windows and maps of its own slots. */
int hmdec_pictures_export_warp(libHMDec_context* ctx, int n, libHMDec_picture* const pics[], const hmgpu_export_desc* desc,
                               const hmgpu_export_tensor* tensor, const hmgpu_export_window windows[], const hmgpu_export_pixel* pixel,
                               int64_t lut, const hmgpu_export_chroma* chroma, const hmgpu_export_warp* warp, const hmgpu_warp_map maps[],
                               void* const dst[3], const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3], int on_stream,
                               void* stream);
/* Motion vectors, reference POCs and block information of up to 16 pictures in one call (hmgpu_pictures_export_motion: the BLOCKS
 * grid or the DENSE per-sample form; destinations, strides and statuses as there), under the validity rule of hmdec_pictures_export:
 * every picture put out by this decoder and fetched since the last push, of one sequence and on one GPU ordinal, else HMGPU_EINVAL
 * and nothing is written.  A picture's side information lies in the device context that decoded it: with hmdec_set_devices the
 * destination and every window are validated once for the whole batch (hmgpu_motion_destination_check) and every context is asked
 * whether its pictures all have side information (hmgpu_pictures_motion_check) before any context is given work; then each context
 * gets one call per run of equally spaced slots.  The POC of a picture itself: libHMDEC_get_POC. */
int hmdec_pictures_export_motion(libHMDec_context* ctx, int n, libHMDec_picture* const pics[], const hmgpu_motion_desc* desc,
                                 const hmgpu_export_scale* scale, const hmgpu_export_window windows[], void* const dst_mv[2], void* dst_ref,
                                 void* dst_block, const int64_t pitch_bytes[4], const int64_t plane_stride_bytes[4],
                                 const int64_t batch_stride_bytes[4], int on_stream, void* stream);
/* The decoded residual of up to 16 pictures in one call (hmgpu_pictures_export_residual: int16 PLANES or the DENSE per-sample form;
 * destinations, strides and statuses as there), under the rules of hmdec_pictures_export_motion: the residual lies in the device
 * context that decoded a picture, everything is validated before any context is given work (hmgpu_residual_destination_check,
 * hmgpu_pictures_residual_check), then each context gets one call per run of equally spaced slots. */
int hmdec_pictures_export_residual(libHMDec_context* ctx, int n, libHMDec_picture* const pics[], const hmgpu_residual_desc* desc,
                                   const hmgpu_export_scale* scale, const hmgpu_export_window windows[], void* const dst[3],
                                   const int64_t pitch_bytes[3], const int64_t plane_stride_bytes[3], const int64_t batch_stride_bytes[3],
                                   int on_stream, void* stream);
/* The quantised levels or de-quantised transform coefficients of up to 16 pictures and their transform-unit info grid in one call
 * (hmgpu_pictures_export_transform: destinations, strides and statuses as there), under the rules of hmdec_pictures_export_motion:
 * levels and arrays lie in the device context that decoded a picture, everything is validated before any context is given work
 * (hmgpu_transform_destination_check, hmgpu_pictures_transform_check), then each context gets one call per run of equally spaced
 * slots. */
int hmdec_pictures_export_transform(libHMDec_context* ctx, int n, libHMDec_picture* const pics[], const hmgpu_transform_desc* desc,
                                    void* const dst[3], void* dst_info, const int64_t pitch_bytes[4], const int64_t plane_stride_bytes[4],
                                    const int64_t batch_stride_bytes[4], int on_stream, void* stream);
/* The loop-filter decisions of up to 16 pictures -- the edge grid and the SAO grid, or their dense form -- in one call
 * (hmgpu_pictures_export_loopfilter: destinations, strides and statuses as there), under the rules of hmdec_pictures_export_motion:
 * the edge records and SAO parameters lie in the device context that decoded a picture, everything is validated before any context is
 * given work (hmgpu_loopfilter_destination_check, hmgpu_pictures_loopfilter_check), then each context gets one call per run of
 * equally spaced slots. */
int hmdec_pictures_export_loopfilter(libHMDec_context* ctx, int n, libHMDec_picture* const pics[], const hmgpu_loopfilter_desc* desc,
                                     const hmgpu_export_scale* scale, const hmgpu_export_window windows[], void* const dst[3],
                                     const int64_t pitch_bytes[3], const int64_t plane_stride_bytes[3], const int64_t batch_stride_bytes[3],
                                     int on_stream, void* stream);
/* Up to 16 output pictures kept on the device compared with planes the caller holds in device memory -- decoded against original
 * (hmgpu_pictures_metrics with HMGPU_METRICS_REF_PLANES: records, reference planes, strides and statuses as there), under the rules of
 * hmdec_pictures_export_residual: everything is validated before any context is given work (hmgpu_metrics_check), then each context
 * gets one call per run of equally spaced slots.  HMGPU_METRICS_REF_PICTURES is refused (HMGPU_EUNSUPPORTED, hmdec_last_error says
 * why): the pictures a decoder puts out are compared with the caller's planes only. */
int hmdec_pictures_metrics(libHMDec_context* ctx, int n, libHMDec_picture* const pics[], const hmgpu_metrics_desc* desc, const void* const ref[3],
                           const int64_t ref_pitch_bytes[3], const int64_t ref_batch_stride_bytes[3], void* results,
                           int64_t results_batch_stride_bytes, int on_stream, void* stream);
/* The same comparison kept per block (hmgpu_pictures_metrics_map with HMGPU_METRICS_REF_PLANES: description, maps, strides and statuses as
 * there), under the rules of hmdec_pictures_metrics: everything is validated before any context is given work
 * (hmgpu_metrics_map_check), then each context gets one call per run of equally spaced slots.  HMGPU_METRICS_REF_PICTURES is refused
 * (HMGPU_EUNSUPPORTED, hmdec_last_error says why). */
int hmdec_pictures_metrics_map(libHMDec_context* ctx, int n, libHMDec_picture* const pics[], const hmgpu_metrics_desc* desc,
                               const hmgpu_metrics_map_desc* map, const void* const ref[3], const int64_t ref_pitch_bytes[3],
                               const int64_t ref_batch_stride_bytes[3], void* const maps[3], const int64_t map_pitch_bytes[3],
                               const int64_t map_field_stride_bytes[3], const int64_t map_batch_stride_bytes[3], int on_stream, void* stream);
/* What up to 16 output pictures kept on the device contain: histograms and moments of Y, Cb, Cr and maxRGB (hmgpu_pictures_histogram:
 * description, destinations, strides and statuses as there, desc->crop in luma samples of the coded picture), under the rules of
 * hmdec_pictures_metrics: everything is validated before any context is given work (hmgpu_histogram_check), then each context gets
 * one call per run of equally spaced slots.  The pictures must be kept on the device (hmdec_set_device_output): without it the call
 * is refused (HMGPU_EINVAL, hmdec_last_error says why). */
int hmdec_pictures_histogram(libHMDec_context* ctx, int n, libHMDec_picture* const pics[], const hmgpu_histogram_desc* desc, void* const hist[4],
                             const int64_t hist_batch_stride_bytes[4], void* records, int64_t records_batch_stride_bytes, int on_stream,
                             void* stream);
unsigned long long hmdec_download_bytes(libHMDec_context* ctx);
int hmdec_picture_device(libHMDec_picture* pic);                             /* GPU ordinal that holds the picture's samples, -1: none */
/* VUI colour description of the picture's SPS (E.2.1; absent: the E.3.1 defaults): video_full_range_flag, colour_primaries,
 * transfer_characteristics, matrix_coefficients, video_format */
int hmdec_picture_colour(libHMDec_picture* pic, int32_t out[5]);
/* VUI chroma sample location of the picture's SPS (E.2.1): chroma_loc_info_present_flag, chroma_sample_loc_type_top_field,
 * chroma_sample_loc_type_bottom_field; the types are 0 when absent */
int hmdec_picture_chroma_loc(libHMDec_picture* pic, int32_t out[3]);
int hmdec_hash_mismatches(libHMDec_context* ctx);                             /* pictures whose reconstruction disagreed with the hash SEI */
int hmdec_pictures_decoded(libHMDec_context* ctx);
/* Error concealment (DESIGN.md §9 "Damaged streams", §9v), for pictures started after the call: 0 off (the default: CTUs no slice
 * delivered stay as they are, a picture without a decodable slice is dropped, a picture whose reference picture set names a missing
 * picture as used is refused), 1 copy, 2 motion copy (hmgpu_pictures_conceal).  With 1 or 2:
 *   - the CTUs of a picture that no slice delivered are filled, behind its loop filters, from the picture of the DPB closest in POC
 *     (the smaller POC on a tie; with hmdec_set_devices: among the pictures the picture's own context holds; none: mid-grey);
 *   - a picture none of whose slices could be decoded is not dropped: it is filled whole and stays what its header made it;
 *   - a missing reference picture that an RPS names as used is replaced by a stand-in of that POC, filled whole, marked as a reference
 *     (long-term if the entry is) and for output -- once the first IRAP picture of the stream has been started, and while a buffer is free.
 * Mode 2 moves blocks only along the vectors of a source that was decoded (in the same device context); a stand-in, a picture filled
 * whole or a copy transferred between contexts is copied as in mode 1.  A stand-in made for a picture that is refused after all
 * (another used entry of its RPS cannot be replaced) leaves again.  An end of sequence ends the making of stand-ins until the next
 * IRAP picture.  Concealed pictures are not checked against their hash SEI.  hmdec_picture_concealed: the CTUs of the picture that were concealed (all
 * of them for a stand-in); hmdec_concealed_pictures / hmdec_concealed_ctus: the totals so far.  A parse-only decoder keeps the same books. */
void hmdec_set_concealment(libHMDec_context* ctx, int mode);
int hmdec_picture_concealed(libHMDec_picture* pic);
int hmdec_concealed_pictures(libHMDec_context* ctx);
long long hmdec_concealed_ctus(libHMDec_context* ctx);
void hmdec_set_device_md5(libHMDec_context* ctx, int on);                     /* MD5 hash SEIs checked on the device (hmgpu_picture_hash_begin) (the default;
                                                                                  HMDEC_DEVICE_MD5=0 or 0 here: on the decoder's hash threads) */
int hmdec_packed_pictures(libHMDec_context* ctx);                             /* pictures handed to the device as packed inputs so far */
int hmdec_device_batches(libHMDec_context* ctx);                              /* calls of hmgpu_decompress_pictures so far (pictures retired together share one) */
const char* hmdec_last_error(libHMDec_context* ctx);
libHMDec_picture* hmdec_last_decoded_picture(libHMDec_context* ctx);          /* the picture finished most recently, decoding order */
libHMDec_picture* hmdec_open_picture(libHMDec_context* ctx);                  /* the picture whose slices are still arriving, or NULL */
/* parser output of a picture by name: "depth", "part_size", "pred_mode", "qp", "tr_idx", "cbf0".."cbf2", "ts0".."ts2", "mv0", "mv1",
 * "ref_idx0", "ref_idx1", "intra_dir0", "intra_dir1", "bypass", "ipcm", "skip", "merge", "slice_idx", "tile_idx", "coeff0".."coeff2",
 * "pcm0".."pcm2", "sao", "plane0".."plane2" -- the HM-layout arrays of include/hmgpu.h.  Returns 0 and pointer/size on success. */
int hmdec_picture_array(libHMDec_picture* pic, const char* name, const void** data, int64_t* bytes);
int hmdec_picture_num_slices(libHMDec_picture* pic);
int hmdec_picture_slice_params(libHMDec_picture* pic, int slice, void* out /* hmgpu_slice_params */, void* lists_out /* hmgpu_scaling_lists or NULL */);
/* geometry and sequence-level constants of a picture: width, height, log2 CTB size, bit depth luma, bit depth chroma, PCM bit depth
 * luma, PCM bit depth chroma, pcm_loop_filter_disabled (and PCM enabled), strong_intra_smoothing, SAO enabled, loop filter across
 * tiles, number of CTBs -- what hmgpu_seq_params / hmgpu_pic_params are filled from */
int hmdec_picture_geometry(libHMDec_picture* pic, int32_t out[12]);
/* HMGPU_REXT_* of the picture's SPS (hmgpu_seq_params.range_ext_flags) */
int hmdec_picture_range_ext_flags(libHMDec_picture* pic);
/* chroma_format_idc of the picture's SPS (hmgpu_seq_params.chroma_format): 0 4:0:0, 1 4:2:0, 2 4:2:2, 3 4:4:4 */
int hmdec_picture_chroma_format(libHMDec_picture* pic);
/* PPS log2_sao_offset_scale_luma / _chroma of the picture (hmgpu_pic_params.sao_offset_shift_*) */
int hmdec_picture_sao_offset_shift(libHMDec_picture* pic, int chroma);
/* conformance window of the picture's SPS in luma samples: left, right, top, bottom (libHM hands out the uncropped picture) */
int hmdec_picture_conformance_window(libHMDec_picture* pic, int32_t window[4]);
/* libHMDEC_get_internal_info for C callers: pointer to the first element and the count (same storage, same lifetime) */
int hmdec_internal_info(libHMDec_context* ctx, libHMDec_picture* pic, int type, const libHMDec_BlockValue** data);
int hmdec_picture_hash_sei(libHMDec_picture* pic, uint8_t digest[48]);        /* returns the method (0 none, 1 MD5, 2 CRC, 3 checksum) */

#ifdef __cplusplus
}
#endif
#endif
