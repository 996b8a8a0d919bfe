/* hmgpu.h -- C ABI of libhmgpu.so: MI355X-native pixel reconstruction for the HM (HEVC) decoder.
 *
 * This is the drop-in boundary for the one hot path of ChristianFeldmann/libHM (HM 16.0) that is
 * accelerated: everything HM does between the end of CABAC parsing of a slice and the finished,
 * loop-filtered picture.  HM has no plugin seam there, so the seam sits at the two
 * calls HM itself isolates and times:
 *
 *     TDecGop::decompressSlice()  TLibDecoder/TDecGop.cpp:105   -> hmgpu_decompress_slice()
 *     TDecGop::filterPicture()    TLibDecoder/TDecGop.cpp:157   -> hmgpu_filter_picture()
 *
 * Parsing stays with the (host) caller.  What crosses the boundary is exactly what HM's parser leaves
 * behind in TComPicSym: per-CTU TComDataCU arrays (4x4-partition granularity, z-scan order,
 * TComDataCU.h:86-157), coefficient levels (TComDataCU.cpp:165-173), SAOBlkParam per CTU
 * (TypeDef.h:754-779) and a handful of slice/PPS/SPS constants that HM keeps in globals.  The
 * reference-side shim is a field-by-field memcpy.  All traversal (CU/TU/PU
 * quadtrees, boundary strengths, SAO merge resolution ...) happens behind this interface, on the GPU.
 *
 * Conventions: plain C, no HIP/torch types; every function returns an hmgpu_status (never aborts,
 * unlike HM's assert/exit: TComTrQuant.cpp:925); one context per host thread and per GPU; calls on one
 * context are serialised by the caller; work is enqueued on the context's HIP stream and completes at
 * hmgpu_sync()/hmgpu_picture_download().  Samples are HM's Pel = int16, levels int16 (HM's TCoeff
 * int32 narrowed by the shim; exact for bit depth <= 10 because xDeQuant clips its input to 16 bits
 * first: TComTrQuant.cpp:1284-1287).
 */
#ifndef HMGPU_H
#define HMGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMGPU_VERSION 1

typedef enum hmgpu_status {
  HMGPU_OK = 0,
  HMGPU_EINVAL = 1,       /* bad argument / inconsistent geometry (HM: assert) */
  HMGPU_EDEVICE = 2,      /* HIP error; code via hmgpu_last_device_error() */
  HMGPU_EUNSUPPORTED = 3, /* coding tool outside the supported envelope; nothing was enqueued */
  HMGPU_ENOMEM = 4
} hmgpu_status;

#define HMGPU_MAX_REF 16         /* MAX_NUM_REF in HM (CommonDef.h) */
#define HMGPU_MAX_SLICES 600     /* slices per picture kept on the device */
#define HMGPU_NO_PIC (-1)

/* HM enums that appear in the metadata (TypeDef.h:374-443) */
enum { HMGPU_B_SLICE = 0, HMGPU_P_SLICE = 1, HMGPU_I_SLICE = 2 };
enum { HMGPU_MODE_INTER = 0, HMGPU_MODE_INTRA = 1 };
enum { HMGPU_SIZE_2Nx2N = 0, HMGPU_SIZE_2NxN = 1, HMGPU_SIZE_Nx2N = 2, HMGPU_SIZE_NxN = 3, HMGPU_SIZE_2NxnU = 4,
       HMGPU_SIZE_2NxnD = 5, HMGPU_SIZE_nLx2N = 6, HMGPU_SIZE_nRx2N = 7, HMGPU_SIZE_NONE = 8 /* NUMBER_OF_PART_SIZES: not decoded */ };
enum { HMGPU_SAO_OFF = 0, HMGPU_SAO_NEW = 1, HMGPU_SAO_MERGE = 2 };                   /* SAOMode, TypeDef.h:604 */
enum { HMGPU_SAO_EO_0 = 0, HMGPU_SAO_EO_90 = 1, HMGPU_SAO_EO_135 = 2, HMGPU_SAO_EO_45 = 3, HMGPU_SAO_BO = 4 }; /* :620 */
enum { HMGPU_SAO_MERGE_LEFT = 0, HMGPU_SAO_MERGE_ABOVE = 1 };                         /* :612 */

typedef struct hmgpu_ctx hmgpu_ctx;
typedef int32_t hmgpu_pic;       /* handle of a device-resident picture (TComPic/TComPicYuv counterpart) */

/* What TDecTop::xActivateParameterSets turns into globals (TDecTop.cpp:283-348: g_bitDepth, g_uiMaxCUWidth,
 * g_uiMaxCUDepth ...).  Fixed for the life of a context. */
typedef struct hmgpu_seq_params {
  int32_t width, height;          /* SPS pic_{width,height}_in_luma_samples (multiple of the 8x8 minimum CU) */
  int32_t bit_depth_luma;         /* g_bitDepth[CHANNEL_TYPE_LUMA]   (8..12; without extended_precision_processing) */
  int32_t bit_depth_chroma;       /* g_bitDepth[CHANNEL_TYPE_CHROMA] (8..12) */
  int32_t chroma_format;          /* chroma_format_idc: 1 (4:2:0), 2 (4:2:2), 3 (4:4:4), or 0 (4:0:0, monochrome: the chroma arrays hold no coded
                                     blocks, the chroma planes are allocated like those of 4:2:0 and left alone; picture hashes: the first
                                     digest).  Chroma planes, level arrays and PCM buffers have (width >> sx) x (height >> sy) samples per
                                     luma area, sx = 1 unless 4:4:4, sy = 1 only for 4:2:0 (getComponentScaleX/Y, TComChromaFormat.h:59-62) */
  int32_t log2_ctu_size;          /* log2 g_uiMaxCUWidth: 4, 5 or 6.  partitions are 4x4 => (1<<(2*log2_ctu_size-4)) per CTU */
  int32_t max_pictures;           /* device pictures to pre-allocate (DPB size + pictures in flight) */
  int32_t pcm_loop_filter_disable;/* SPS pcm_loop_filter_disabled_flag && pcm_enabled_flag */
  int32_t strong_intra_smoothing; /* SPS strong_intra_smoothing_enabled_flag (TComPattern.cpp:201-216) */
  int32_t pcm_bit_depth_luma, pcm_bit_depth_chroma;   /* SPS pcm_sample_bit_depth_*: PCM samples are shifted up to the coding bit depth (TDecCu.cpp:770-789) */
  int32_t range_ext_flags;        /* HMGPU_REXT_*: the sps_range_extension() tools that change reconstruction (0 for version-1 streams) */
  int32_t reserved[4];
} hmgpu_seq_params;

/* hmgpu_seq_params.range_ext_flags: what TComSPS keeps of sps_range_extension() for the residual path */
enum {
  HMGPU_REXT_ROTATION = 1,        /* getUseResidualRotation(): 4x4 intra transform-skip / bypass blocks are read back to front
                                     (TComTU::isNonTransformedResidualRotated, TComTU.cpp:227-233) */
  HMGPU_REXT_IMPLICIT_RDPCM = 2,  /* getUseResidualDPCM(RDPCM_SIGNAL_IMPLICIT): intra transform-skip / bypass blocks predicted
                                     horizontally (10) or vertically (26) accumulate their residual along that direction
                                     (invRdpcmNxN, TComTrQuant.cpp:1737-1792); bypass CUs also lose the intra edge filters
                                     (TComPrediction.cpp:476) */
  HMGPU_REXT_EXPLICIT_RDPCM = 4,  /* getUseResidualDPCM(RDPCM_SIGNAL_EXPLICIT): inter blocks carry their mode in transform_skip[] */
  HMGPU_REXT_INTRA_SMOOTHING_DISABLED = 8   /* getDisableIntraReferenceSmoothing(): intra reference samples are never filtered
                                               (TComPrediction::filteringIntraReferenceSamples, called from TDecCu.cpp:532) */
};

/* Scaling lists as TDecTop activates them for a slice (TDecTop.cpp:651-668: PPS lists, else SPS lists, else the defaults):
 * TComScalingList's own storage.  De-quantisation with them: TComTrQuant.cpp:1238-1275, tables :2992-3012, 3092-3106. */
typedef struct hmgpu_scaling_lists {
  int32_t coef[4][6][64];   /* getScalingListAddress(sizeId 4x4..32x32, listId = 3 * inter + component): raster order; 16 values for
                               4x4, 8x8 values otherwise (16x16 / 32x32 replicate every value over ratio x ratio positions) */
  int32_t dc[4][6];         /* getScalingListDC: replaces position 0 for 16x16 and 32x32 */
} hmgpu_scaling_lists;

/* Per-slice constants the hot path reads through pcCU->getSlice() */
typedef struct hmgpu_slice_params {
  int32_t slice_type;                   /* HMGPU_{B,P,I}_SLICE */
  int32_t cb_qp_offset, cr_qp_offset;   /* pps_cb/cr_qp_offset + slice_cb/cr_qp_offset: dequant QpParam (TComTrQuant.cpp:107-112) */
  int32_t pps_cb_qp_offset, pps_cr_qp_offset; /* PPS part only: chroma deblocking (TComLoopFilter.cpp:759) */
  int32_t deblocking_disable;           /* getDeblockingFilterDisable() */
  int32_t beta_offset_div2, tc_offset_div2;
  int32_t lf_across_slices;             /* getLFCrossSliceBoundaryFlag() */
  int32_t weighted_pred;                /* TComSlice::applyWP(): explicit weighted prediction is active for this slice (P slice with
                                           weighted_pred_flag, B slice with weighted_bipred_flag); the tables below are then read */
  int32_t lf_across_tiles;              /* PPS loop_filter_across_tiles_enabled_flag (TDecGop.cpp:165) */
  int32_t num_ref_idx[2];
  hmgpu_pic ref_pic[2][HMGPU_MAX_REF];  /* getRefPic(list, idx) as device picture handles */
  int32_t ref_poc[2][HMGPU_MAX_REF];    /* getRefPOC(list, idx) (identical-motion test, TComPrediction.cpp:497-512) */
  int32_t constrained_intra_pred;       /* PPS constrained_intra_pred_flag (TComPattern.cpp:558-572) */
  int32_t reserved[4];
  /* explicit weighted prediction (TComWeightPrediction.cpp:44-57, 211-271), after TComSlice::initWpScaling: per list,
   * reference index and component the weight (iWeight; 1 << log2 denominator where the header carried none) and the offset
   * already scaled to the bit depth (iOffset << (bitDepth - 8) unless high_precision_offsets) */
  int32_t wp_log2_denom[2];             /* luma, chroma */
  int16_t wp_weight[2][HMGPU_MAX_REF][3];
  int16_t wp_offset[2][HMGPU_MAX_REF][3];
  const hmgpu_scaling_lists* scaling_lists;   /* SPS scaling_list_enabled_flag: the lists in force, else NULL (flat, m = 16).  All slices of a
                                               * picture name one PPS (7.4.7.1), i.e. the same lists: the device keeps ONE table per picture,
                                               * written by every slice call */
} hmgpu_slice_params;

/* The picture-persistent TComDataCU arrays of TComPicSym (TComPicSym.cpp:93-114).  Every array covers the WHOLE
 * picture: [num_ctus][parts_per_ctu] in CTU raster order and HM z-scan order inside the CTU; a call only reads the
 * CTUs it is asked to process.  Optional arrays may be NULL (treated as all zero). */
typedef struct hmgpu_ctu_meta {
  const uint8_t* depth;              /* m_puhDepth */
  const int8_t*  part_size;          /* m_pePartSize (HMGPU_SIZE_*; HMGPU_SIZE_NONE = CTU part never decoded) */
  const int8_t*  pred_mode;          /* m_pePredMode */
  const int8_t*  qp;                 /* m_phQP */
  const uint8_t* tr_idx;             /* m_puhTrIdx */
  const uint8_t* cbf[3];             /* m_puhCbf[Y,Cb,Cr]: bit d = cbf at transform depth d (TComDataCU.h:310) */
  const uint8_t* transform_skip[3];  /* bit 0: m_puhTransformSkip[Y,Cb,Cr]; bits 1-2: m_explicitRdpcmMode[Y,Cb,Cr] of inter
                                        transform-skip / bypass blocks (RDPCM_OFF 0, RDPCM_HOR 1, RDPCM_VER 2: TypeDef.h)   (optional) */
  const int16_t* mv[2];              /* m_acCUMvField[list].m_pcMv as {hor,ver} pairs: [num_ctus][parts][2] */
  const int8_t*  ref_idx[2];         /* m_acCUMvField[list].m_piRefIdx (-1 = list unused) */
  const uint8_t* intra_dir[2];       /* m_puhIntraDir[luma,chroma]                          (optional; intra path) */
  const uint8_t* transquant_bypass;  /* m_CUTransquantBypass: lossless CUs (residual = levels, exempt from the loop filters)  (optional) */
  const uint8_t* ipcm;               /* m_pbIPCMFlag: PCM CUs (samples from coeffs->pcm_sample)                               (optional) */
  const uint16_t* slice_idx;         /* [num_ctus] index into the picture's slice table     (optional: all 0) */
  const uint16_t* tile_idx;          /* [num_ctus] TComPicSym::getTileIdxMap                (optional: all 0) */
  const int8_t*  ccp_alpha[2];       /* m_crossComponentPredictionAlpha[Cb, Cr] (4:4:4 with cross_component_prediction_enabled_flag: the chroma
                                        residual of a transform unit takes (alpha * luma residual) >> 3 on top, TComTrQuant.cpp:3294-3335)  (optional) */
} hmgpu_ctu_meta;

/* Coefficient levels, HM layout (m_pcTrCoeff: TU blocks contiguous in z-order, raster inside a TU, offset of a TU =
 * 16 * z-index of its first partition for luma, 4 * ... for chroma; TComTU.cpp:64-76,186): whole-picture arrays
 * y: [num_ctus][ctu*ctu], cb/cr: [num_ctus][ctu*ctu/4] (4:2:2: /2 -- a chroma block of a transform unit is two squares, the upper one
 * first, TComTU::VERTICAL_SPLIT, TComTrQuant.cpp:1436-1462; 4:4:4: /1).  In 4:2:2 cbf[1..2] carry, one transform depth below the unit's
 * own bit, the flags of the two squares over the upper / lower half of its partitions (TDecSbac.cpp:1058-1095). */
typedef struct hmgpu_coeffs {
  const int16_t* level[3];
  const int16_t* pcm_sample[3];   /* TComDataCU::getPCMSample (m_pcIPCMSample*): the transmitted samples of PCM CUs, same layout as
                                     the levels; needed only if meta->ipcm marks PCM CUs (may be NULL otherwise) */
  /* Compact levels (optional; all three NULL = HM's dense layout above).  level[c] then holds ONLY the coded transform units of
   * component c -- the blocks HM's layout would hold, in the same order (CTU by CTU, z-order of the TU origins inside a CTU, raster
   * inside a TU), with the uncoded ones left out; a TU is coded iff its cbf bits are set down to its transform depth
   * (TComTrQuant.cpp:1558-1564).  ctu_level_start[c][a] = element offset of CTU a's first coded TU, [num_ctus] = total: only that
   * many elements cross the bus.  Whole-picture calls only.  hmgpu_pack_levels() converts HM's arrays. */
  const uint32_t* ctu_level_start[3];
} hmgpu_coeffs;

/* SAOBlkParam as parsed (TDecSbac::parseSAOBlkParam), before reconstructBlkSAOParams: [num_ctus][3] */
typedef struct hmgpu_sao_param {
  int32_t mode_idc;       /* HMGPU_SAO_OFF / NEW / MERGE */
  int32_t type_idc;       /* NEW: HMGPU_SAO_EO_* / BO; MERGE: HMGPU_SAO_MERGE_LEFT / ABOVE */
  int32_t type_aux_info;  /* BO: first band */
  int32_t offset[32];     /* coded offsets (EO: classes 0..4; BO: by band) */
} hmgpu_sao_param;

typedef struct hmgpu_pic_params {
  int32_t lf_across_tiles;       /* PPS loop_filter_across_tiles_enabled_flag */
  int32_t sao_enabled;           /* SPS sample_adaptive_offset_enabled_flag (TDecGop.cpp:169) */
  int32_t sao_offset_shift_luma, sao_offset_shift_chroma;  /* log2_sao_offset_scale_* (0 for Main/Main10) */
  int32_t reserved[8];
} hmgpu_pic_params;

/* ------------------------------------------------------------------------------------------------ context */
hmgpu_status hmgpu_create(const hmgpu_seq_params* seq, int device_ordinal, hmgpu_ctx** out);
void         hmgpu_destroy(hmgpu_ctx* ctx);
int32_t      hmgpu_last_device_error(const hmgpu_ctx* ctx);        /* hipError_t of the last HMGPU_EDEVICE; -2: an intra wavefront gave up
                                                                       waiting for a neighbouring CTU (reported by hmgpu_sync / hmgpu_picture_download) */
/* Test hook for the error path above: from the next hmgpu_decompress_* call on `pic`, the intra wavefront leaves CTU `ctu` out (no samples,
 * no progress published), so the CTUs that predict from it run into their bounded wait and the call sequence ends in HMGPU_EDEVICE with
 * hmgpu_last_device_error() == -2 instead of hanging.  ctu = -1 switches it off.  Not for production use. */
hmgpu_status hmgpu_debug_stall_intra(hmgpu_ctx* ctx, hmgpu_pic pic, int32_t ctu);
const char*  hmgpu_status_string(hmgpu_status s);
hmgpu_status hmgpu_sync(hmgpu_ctx* ctx);                           /* wait for everything enqueued so far */

/* Page-locked host memory for the caller's arrays (metadata, levels, SAO parameters, download targets): staging from it is a true
 * asynchronous DMA at full link speed, from ordinary memory the runtime copies through a bounce buffer while the caller waits.
 * Returns NULL when no device memory manager is available (no GPU): use malloc then. */
void* hmgpu_host_alloc(size_t bytes);
void  hmgpu_host_free(void* p);

/* geometry helpers (TComPicSym::create, TComPicSym.cpp:73-92) */
int32_t hmgpu_num_ctus(const hmgpu_seq_params* seq);
int32_t hmgpu_parts_per_ctu(const hmgpu_seq_params* seq);

/* ------------------------------------------------------------------------------------------------ pictures
 * Counterpart of TDecTop::xGetNewPicBuffer (TDecTop.cpp:134): pictures live in HBM for as long as they are
 * referenced; planes never leave the device unless downloaded.  Host plane layout at upload/download is HM's
 * TComPicYuv convention reduced to the visible area: pointer to sample (0,0) + stride in samples. */
hmgpu_status hmgpu_picture_acquire(hmgpu_ctx* ctx, hmgpu_pic* out);
hmgpu_status hmgpu_picture_release(hmgpu_ctx* ctx, hmgpu_pic pic);
hmgpu_status hmgpu_picture_upload(hmgpu_ctx* ctx, hmgpu_pic pic, const int16_t* const planes[3], const int32_t strides[3]);
hmgpu_status hmgpu_picture_download(hmgpu_ctx* ctx, hmgpu_pic pic, int16_t* const planes[3], const int32_t strides[3]);

/* The same without waiting: the copies are enqueued and the call returns a ticket; hmgpu_download_wait(ticket) blocks until those
 * copies have landed.  hmgpu_download_wait may be called from another thread than the one that drives the context (a thread that
 * hashes or writes out pictures while the decoding thread keeps the device fed); planes should be page-locked (hmgpu_host_alloc). */
hmgpu_status hmgpu_picture_download_begin(hmgpu_ctx* ctx, hmgpu_pic pic, int16_t* const planes[3], const int32_t strides[3], uint64_t* ticket);
hmgpu_status hmgpu_download_wait(hmgpu_ctx* ctx, uint64_t ticket);

/* Output side.  hmgpu_picture_download_packed: the finished picture as the application wants it -- one or two
 * bytes per sample (TVideoIOYuv::write, TVideoIOYuv.cpp:706-790: 8-bit files take the low byte), cropped to a window given in
 * luma samples (conformance / display window; 0,0,0,0 = the whole picture) -- converted on the device, so an 8-bit picture crosses
 * PCIe in half the bytes.  hmgpu_picture_hash: the decoded-picture-hash SEI check (TDecGop.cpp:199-208) without moving the
 * picture: method 1 = MD5 (TComPicYuvMD5.cpp:183-205; HM's default and the hash its own streams carry), 2 = CRC, 3 = checksum
 * (:89-170).  MD5 is one serial chain of 64-byte blocks per plane -- about 0.2 s for a 3840x2160 10-bit luma plane on a GPU lane,
 * eight times what a host core needs -- so hmgpu_picture_hash(.., 1, ..) is for verification and tests.  A decoder uses
 * hmgpu_picture_hash_begin: it packs the planes behind the picture's filters (the picture buffer is free again at once) and the
 * chains of up to 32 pictures at a time run side by side, one LANE per plane, on a low-priority stream of their own; 48 bytes come
 * back per picture.  hmgpu_hash_wait(ticket, block = 0) polls, (block = 1) waits -- and launches the batch the ticket belongs to
 * if it is still collecting.  At most 96 tickets may be outstanding. */
hmgpu_status hmgpu_picture_download_packed(hmgpu_ctx* ctx, hmgpu_pic pic, void* const planes[3], const int32_t stride_bytes[3],
                                           int32_t bytes_per_sample, int32_t crop_left, int32_t crop_right, int32_t crop_top, int32_t crop_bottom);
hmgpu_status hmgpu_picture_hash(hmgpu_ctx* ctx, hmgpu_pic pic, int32_t method, uint8_t digest[3][16], int32_t* digest_len);
hmgpu_status hmgpu_picture_hash_begin(hmgpu_ctx* ctx, hmgpu_pic pic, int32_t method /* 1 */, uint64_t* ticket);
hmgpu_status hmgpu_hash_wait(hmgpu_ctx* ctx, uint64_t ticket, int32_t block, uint8_t digest[3][16], int32_t* digest_len, int32_t* ready);

/* Frame-parallel exchange (BASELINE config #5): a finished picture is ONE contiguous device region (three
 * planes, replicated margins included -- HM's TComPicYuv after extendPicBorder, TComPicYuv.cpp:89-100) that another GPU
 * needs before it can predict from the picture (TComPrediction.cpp:593).  The collective itself (RCCL broadcast /
 * send-recv between the owner's region and the receivers' regions) is issued by the caller on hmgpu_stream():
 *   sender:    hmgpu_picture_device_region(ctx, pic, HMGPU_REGION_FINISHED, &base, &bytes)   (extends the border if needed)
 *   receiver:  hmgpu_picture_device_region(ctx, pic, HMGPU_REGION_RECEIVE, &base, &bytes); <collective>;
 *              hmgpu_picture_commit_received(ctx, pic)        (the picture can now be named in ref_pic[][])
 * Regions of two contexts with equal hmgpu_seq_params have equal size and layout. */
typedef enum { HMGPU_REGION_FINISHED = 0, HMGPU_REGION_RECEIVE = 1 } hmgpu_region;
/* Within ONE process that drives several devices (a decoder that places the pictures of one temporal level on different GPUs,
 * TDecTop.cpp:672 / TDecGop.cpp:105 per picture): hmgpu_picture_transfer copies the finished picture `src_pic` of `src` into
 * `dst_pic` of `dst` -- a context of the same geometry on another GPU (peer copy over xGMI, hipMemcpyPeerAsync) or on the same one --
 * ordered behind everything enqueued on both contexts' streams, margins included, and commits it: dst_pic can be named in
 * ref_pic[][] of dst at once.  hmgpu_transfer_bytes: bytes a context has sent so far. */
hmgpu_status hmgpu_picture_transfer(hmgpu_ctx* src, hmgpu_pic src_pic, hmgpu_ctx* dst, hmgpu_pic dst_pic);
uint64_t     hmgpu_transfer_bytes(const hmgpu_ctx* ctx);
hmgpu_status hmgpu_picture_device_region(hmgpu_ctx* ctx, hmgpu_pic pic, int32_t which, void** base, int64_t* bytes);
hmgpu_status hmgpu_picture_commit_received(hmgpu_ctx* ctx, hmgpu_pic pic);
/* the context's HIP stream (a hipStream_t), for callers that order their own device work against the library's */
void* hmgpu_stream(hmgpu_ctx* ctx);

/* ------------------------------------------------------------------------------------------------ device export
 * A finished picture converted on the device straight into caller-owned device memory.  Three layouts:
 *   HMGPU_EXPORT_PLANAR      Y, Cb, Cr at the picture's chroma format (Y only for 4:0:0) -- what TAppDecoder -d N -o writes
 *   HMGPU_EXPORT_SEMIPLANAR  Y + one interleaved CbCr plane (NV12 / NV16 / NV24; P010 / P016 with msb_aligned) (Y only for 4:0:0)
 *   HMGPU_EXPORT_RGB         three planes R, G, B (CHW), full range 0 .. 2^bit_depth - 1
 * Bit depth of the YUV layouts (and of matrix 0), per channel type, HM 16.0 TVideoIOYuv::write with CLIP_TO_709_RANGE 0
 * (TVideoIOYuv.cpp:70-87): s = out - coding depth; s >= 0: v << s; s < 0: Clip3(0, 2^out - 1, (v + (1 << (-s - 1))) >> -s).
 * 2-byte samples are LSB-aligned, or shifted left by 16 - out when msb_aligned.  The crop window is in luma samples and must cover
 * whole chroma samples (else HMGPU_EINVAL).  RGB: the chroma sample of luma (x, y) is (x >> csx, y >> csy), replicated, unless the
 * call asks for interpolation at the signalled sample location (hmgpu_pictures_export_chroma, "chroma export" below); 4:0:0 uses
 * Cb = Cr = 1 << (bdC - 1); `matrix` takes the VUI matrix_coefficients codes 1 (BT.709), 5 / 6 (BT.601), 9 (BT.2020 non-constant
 * luminance) -- H.273's Kr / Kb equations, limited or full range (full_range) -- and 0 (identity / GBR: G = Y, B = Cb, R = Cr, then
 * the bit-depth rule; 4:4:4 only); any other code gives HMGPU_EUNSUPPORTED.  The integers the kernel uses are derived on the host
 * in double precision (rounded half away from zero) and published in hmgpu_export_plan.coef:
 *   coef[0] S (shift)      coef[1] 1 << (S - 1)     coef[2] Y offset      coef[3] chroma offset (1 << (bdC - 1))
 *   coef[4] cY             coef[5] cR<-Cr           coef[6] cG<-Cb        coef[7] cG<-Cr        coef[8] cB<-Cb
 *   coef[9] 2^bit_depth - 1                         coef[10] 1: identity (matrix 0)            coef[11..15] 0
 *   t = cY * (Y - coef[2]) + coef[1];  u = Cb - coef[3];  v = Cr - coef[3]
 *   R = Clip3(0, coef[9], (t + cR<-Cr * v) >> S)   G = Clip3(0, coef[9], (t + cG<-Cb * u + cG<-Cr * v) >> S)   B = Clip3(0, coef[9], (t + cB<-Cb * u) >> S)
 * in 32-bit integers: S is the largest shift (<= 30) for which no sum can overflow for any sample of the coding bit depths. */
enum { HMGPU_EXPORT_PLANAR = 0, HMGPU_EXPORT_SEMIPLANAR = 1, HMGPU_EXPORT_RGB = 2 };
typedef struct hmgpu_export_desc {
  int32_t layout;              /* HMGPU_EXPORT_* */
  int32_t bit_depth[2];        /* output depth luma / chroma (RGB: [0] for all three; 8..16); 0 = the coding bit depth */
  int32_t bytes_per_sample;    /* 1 (bit depth <= 8) or 2 */
  int32_t msb_aligned;         /* 2-byte samples only: shifted left by 16 - bit depth (P010 / P016) */
  int32_t crop[4];             /* left, right, top, bottom, luma samples */
  int32_t matrix, full_range;  /* RGB only: VUI matrix_coefficients, video_full_range_flag of the input */
  int32_t reserved[6];         /* 0 */
} hmgpu_export_desc;
typedef struct hmgpu_export_plan {
  int32_t planes;              /* planes written: 1 .. 3 */
  int32_t width[3], height[3]; /* per plane, in samples (semi-planar CbCr: in CbCr pairs) */
  int32_t row_bytes[3];        /* bytes of one row: the least pitch */
  int32_t coef[16];            /* RGB: see above; else 0 */
} hmgpu_export_plan;
/* validates a descriptor against a sequence and reports what an export writes; host code, no device needed */
hmgpu_status hmgpu_export_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* desc, hmgpu_export_plan* out);
/* Enqueues the conversion of picture `pic` into dst[k] (device memory of the context's GPU, rows pitch_bytes[k] apart) and returns
 * without waiting.  on_stream 0: on the context's stream; 1: on `stream`, a hipStream_t of the context's device (0: the null
 * stream; another device's stream gives HMGPU_EINVAL).  Either way the kernel runs after all work enqueued for the picture and after
 * everything already on `stream`, and every later operation of the context waits for it.  Everything is validated before anything
 * is enqueued. */
hmgpu_status hmgpu_picture_export(hmgpu_ctx* ctx, hmgpu_pic pic, const hmgpu_export_desc* desc, void* const dst[3],
                                  const int64_t pitch_bytes[3], int32_t on_stream, void* stream);
/* Scaled export: the unscaled export of the same descriptor resized to scale->width x scale->height.
 *   s = what hmgpu_picture_export writes for `desc` (crop window, layout, matrix, output depth D), before the msb_aligned shift
 *   each output plane is resampled separably, horizontally first, from its own cropped source plane; only samples inside the crop
 *   window contribute.  RGB: three width x height planes (chroma replicated to the luma grid before the matrix, as unscaled).
 *   PLANAR / SEMIPLANAR: Y width x height, Cb and Cr (width >> csx) x (height >> csy), each from its cropped plane with half-sample
 *   centres (align_corners=False); width / height must be whole chroma samples (else HMGPU_EINVAL).  4:0:0: Y only (YUV layouts).
 * One table per plane class (0: luma / RGB planes, 1: chroma planes) and axis (0: horizontal, 1: vertical): for output index i the
 * first source index first[i] (in the cropped plane), count[i] taps and int16 weights w[i][0 .. count[i]) in Q14 summing to 16384.
 * The host derives them in double precision from the weights torch uses (in = source size, out = output size, scale = in / out):
 *   HMGPU_SCALE_NEAREST   mode="nearest-exact": one tap at min(floor((2i + 1) * in / (2 * out)), in - 1), computed exactly in
 *                         integers (torch forms (i + 0.5) * scale with a float32 scale and can land one below where that product
 *                         is a whole number: an exact tie)
 *   HMGPU_SCALE_BILINEAR  mode="bilinear", antialias=True, align_corners=False: PIL's triangle, support 1 widened by scale when scale > 1
 *   HMGPU_SCALE_BICUBIC   mode="bicubic", antialias=True, align_corners=False: Keys' cubic with a = -0.5, support 2 widened the same way
 *                         (centre (i + 0.5) * scale; taps int(centre - support + 0.5) .. int(centre + support + 0.5) - 1, clamped to
 *                         the plane, weight f((j - centre + 0.5) / max(scale, 1)), normalised to sum 1)
 *   HMGPU_SCALE_AREA      mode="area" (adaptive average): taps floor(i * in / out) .. ceil((i + 1) * in / out) - 1, equal weights
 * Q14 by largest remainders: each weight times 16384 is rounded down, then the weights with the largest remainders (the lower index
 * first on a tie) gain one unit each until the row sums to 16384, so every weight is within one unit of its exact value; zero weights
 * at either end are dropped.  At equal size every table is the identity, so a scaled export at the crop's own size equals the unscaled one.
 * Integer arithmetic, 32-bit, E = 16 - D fractional bits kept between the passes (hmgpu_export_plan.coef[11]), D the output depth of the
 * plane (RGB: bit_depth[0]), except that E is one value per export: for the YUV layouts with different luma and chroma output depths
 * E = 16 - max(D luma, D chroma), while each plane is clipped to its own D:
 *   t = (sum_j wx[j] * s[y][first + j] + (1 << (13 - E))) >> (14 - E)          per source row y
 *   o = Clip3(0, 2^D - 1, (sum_k wy[k] * t[first + k] + (1 << (13 + E))) >> (14 + E)), then << (16 - D) when msb_aligned
 * (>> is an arithmetic shift: bicubic weights are negative in places).  Limits: per axis and plane class, in <= 32 * out (a 32x
 * reduction) and out <= 8 * in (an 8x enlargement), and at most 16384 output samples per side; outside them HMGPU_EUNSUPPORTED.
 * Within them no sum overflows for any input at any D of 8 .. 16 (the largest row sums of positive and of negative weights bound
 * every sum; the host evaluates that bound for the tables of each shape and refuses, HMGPU_EUNSUPPORTED, one that would overflow).  The plan is that of the unscaled export with every plane's size replaced and
 * coef[11] E, coef[12] / coef[13] the widest horizontal / vertical table (taps); coef[0..10] keep their RGB meaning. */
enum { HMGPU_SCALE_NEAREST = 0, HMGPU_SCALE_BILINEAR = 1, HMGPU_SCALE_BICUBIC = 2, HMGPU_SCALE_AREA = 3 };
typedef struct hmgpu_export_scale {
  int32_t width, height;       /* output size in luma samples (RGB: of every plane) */
  int32_t filter;              /* HMGPU_SCALE_* */
  int32_t reserved[5];         /* 0 */
} hmgpu_export_scale;
/* validates and reports what a scaled export writes; host code, no device needed */
hmgpu_status hmgpu_export_scaled_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                          hmgpu_export_plan* out);
/* the integers of one table (chroma 0 / 1: plane class, axis 0 / 1: horizontal / vertical), host code: first[out], count[out],
 * weights[out][max_taps] (row i zero beyond count[i]); max_taps below the widest table gives HMGPU_EINVAL.  A 4:0:0 sequence, or
 * the RGB layout, has no chroma class (HMGPU_EINVAL). */
hmgpu_status hmgpu_export_scale_taps(const hmgpu_seq_params* seq, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                     int32_t chroma, int32_t axis, int32_t max_taps, int32_t* first, int32_t* count, int16_t* weights);
/* hmgpu_picture_export with scaling: the same validation (destination spans, the stream's device) and the same stream ordering; the
 * tables live in device memory of the context, cached per shape (a repeated shape enqueues no copy; a slot is reused only after the
 * last export that read it has finished). */
hmgpu_status hmgpu_picture_export_scaled(hmgpu_ctx* ctx, hmgpu_pic pic, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                         void* const dst[3], const int64_t pitch_bytes[3], int32_t on_stream, void* stream);
/* Batched tensor export: up to HMGPU_EXPORT_MAX_BATCH pictures of the context in one call, as unsigned integers
 * (what the two calls above write) or as float16 / bfloat16 / float32 with a per-plane affine map, ready to feed a model.
 *   v = the integer the export of `desc` (scaled when `scale` is given) writes for a sample, before the msb_aligned shift
 *   HMGPU_SAMPLE_UINT   v, then the msb_aligned shift: slot i of a batch is bit for bit what the single-picture call writes
 *   a float type        convert(fadd(fmul((float)v, scale[k]), bias[k])) for output plane k: the product and the sum are two
 *                       separately rounded binary32 operations (never one fma), and the conversion to float16 / bfloat16 rounds to
 *                       nearest even, overflow to infinity, denormals kept.  numpy's float32 `*`, `+` and astype restate it exactly.
 * Float types: msb_aligned must be 0 and every scale / bias finite (else HMGPU_EINVAL); desc->bit_depth chooses the integer depth D
 * of v, and bytes_per_sample must be what an unsigned export of that depth needs (1 when no plane's depth exceeds 8, else 2; else
 * HMGPU_EINVAL); the RGB and planar layouts only (semi-planar: HMGPU_EUNSUPPORTED).  reserved must be 0 (else HMGPU_EINVAL). */
enum { HMGPU_SAMPLE_UINT = 0, HMGPU_SAMPLE_F16 = 1, HMGPU_SAMPLE_BF16 = 2, HMGPU_SAMPLE_F32 = 3 };
enum { HMGPU_EXPORT_MAX_BATCH = 16 };
typedef struct hmgpu_export_tensor {
  int32_t sample_type;         /* HMGPU_SAMPLE_* */
  float scale[3], bias[3];     /* float types: per output plane (R, G, B or Y, Cb, Cr); ignored for HMGPU_SAMPLE_UINT */
  int32_t reserved[5];         /* 0 */
} hmgpu_export_tensor;
/* the plan of the unscaled (scale NULL) or scaled export of `desc`, with row_bytes at the element size of tensor->sample_type
 * (tensor NULL: HMGPU_SAMPLE_UINT); host code, no device needed */
hmgpu_status hmgpu_export_tensor_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                          const hmgpu_export_tensor* tensor, hmgpu_export_plan* out);
/* Enqueues the export of pics[0 .. n) (n = 1 .. HMGPU_EXPORT_MAX_BATCH; a handle may appear more than once) and returns without
 * waiting: plane k of picture i goes to dst[k] + i * batch_stride_bytes[k], rows pitch_bytes[k] apart -- one [N, 3, H, W] tensor
 * (dst[k] = base + k * plane stride) as well as a tuple of [N, H, W] planes.  scale NULL: unscaled; tensor NULL: HMGPU_SAMPLE_UINT.
 * One kernel launch per call, and the stream ordering of hmgpu_picture_export once per call (one event pair in, one out, when
 * on_stream is 1).  Everything is validated before anything is enqueued and a refused call leaves the destination untouched:
 * an invalid handle anywhere in the list, n outside its range, a batch stride smaller than pitch * (height - 1) + row_bytes of its
 * plane, and a plane whose bytes [dst[k], dst[k] + (n - 1) * batch stride + pitch * (height - 1) + row_bytes) do not lie inside one
 * allocation of the context's device all give HMGPU_EINVAL. */
hmgpu_status hmgpu_pictures_export(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_export_desc* desc,
                                   const hmgpu_export_scale* scale, const hmgpu_export_tensor* tensor, void* const dst[3],
                                   const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream);
/* the validation hmgpu_pictures_export makes of a descriptor and a destination for n pictures, and nothing else: nothing is enqueued
 * and no picture is named.  For callers that spread one batch over several calls (libhmdec, pictures in several contexts of a GPU). */
hmgpu_status hmgpu_export_destination_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                            const hmgpu_export_tensor* tensor, void* const dst[3], const int64_t pitch_bytes[3],
                                            const int64_t batch_stride_bytes[3]);
/* Batched export with a source window and a horizontal mirror per picture: random-resized-crop and random flip per
 * sample, still one launch per call.  Slot i of the batch is, bit for bit,
 *   hmgpu_pictures_export of pics[i] alone with desc->crop replaced by windows[i].crop, the same `scale` and the same `tensor`,
 *   then, when windows[i].flip & 1, every output row of every plane reversed: the mirror acts on the output, after resampling and
 *   after the float map; a semi-planar CbCr plane is reversed pair by pair (Cb stays first).
 * desc->crop must be 0, 0, 0, 0: the window is the crop (else HMGPU_EINVAL).  Each window obeys the rules of hmgpu_export_plan_for
 * (non-negative, non-empty, whole chroma samples) and, with `scale`, on its own the limits of the scaled export (32x reduction, 8x
 * enlargement per axis and plane class, no 32-bit sum of its own tables overflows); one failing window refuses the whole call with
 * the status the single call would give (the first failing window's), nothing is enqueued and the destination stays untouched.
 * Without `scale` all windows must have one size (else HMGPU_EINVAL), which is the output's; their origins may differ, left edges
 * that are no multiple of 4 included.  A flip with a bit other than bit 0, a non-zero reserved word, windows NULL and n outside
 * 1 .. HMGPU_EXPORT_MAX_BATCH give HMGPU_EINVAL.  The plan is that of the single calls -- one output size for every slot -- with
 * coef[12] / coef[13] the widest tables over all windows.  Destination validation, stream ordering (one event pair in, one out, when
 * on_stream is 1) and the one launch per call are those of hmgpu_pictures_export.  A call whose windows are all equal uses the
 * table slot of that shape (a repeated shape enqueues no copy), and unflipped it writes what hmgpu_pictures_export with that crop
 * writes; a scaled call whose windows differ derives its tables per call (windows that share source size and output size on an axis
 * share a table) and sends them, with the per-picture descriptors, in one copy into one of a small ring of per-call buffers, each
 * rewritten only after the export that read it has finished. */
typedef struct hmgpu_export_window {
  int32_t crop[4];             /* left, right, top, bottom: luma samples removed from the coded picture, as hmgpu_export_desc::crop */
  int32_t flip;                /* bit 0: mirror each output row; every other bit 0 */
  int32_t reserved[3];         /* 0 */
} hmgpu_export_window;
/* validates and reports what hmgpu_pictures_export_windows writes per slot; host code, no device needed */
hmgpu_status hmgpu_export_windows_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                           const hmgpu_export_tensor* tensor, int32_t n, const hmgpu_export_window windows[],
                                           hmgpu_export_plan* out);
hmgpu_status hmgpu_pictures_export_windows(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_export_desc* desc,
                                           const hmgpu_export_scale* scale, const hmgpu_export_tensor* tensor,
                                           const hmgpu_export_window windows[], void* const dst[3], const int64_t pitch_bytes[3],
                                           const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream);
/* hmgpu_export_destination_check for hmgpu_pictures_export_windows */
hmgpu_status hmgpu_export_windows_destination_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                                    const hmgpu_export_tensor* tensor, const hmgpu_export_window windows[],
                                                    void* const dst[3], const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3]);

/* ------------------------------------------------------------------------------------------------ packed pixel export
 * The RGB layout as packed pixels: one destination whose pixels hold C = 3 (RGB, BGR) or 4 (RGBA, BGRA, ARGB, ABGR)
 * elements side by side -- [H, W, C] images, [N, H, W, C] batches, which are also the bytes of a channels-last [N, C, H, W] tensor.
 * No arithmetic of its own: let P be the three planes slot i receives from the existing call with the same `desc`, `scale` and
 * `tensor` -- hmgpu_pictures_export_windows with `windows`, else hmgpu_pictures_export with the crop of desc->crop -- with the
 * msb_aligned shift, the float map fl(fl(v * scale[k]) + bias[k]) and the mirror.  Element c of pixel (y, x) of slot i is
 * P[chan(order, c)][y][x], stored at
 *   dst + i * batch_stride_bytes + y * pitch_bytes + (x * C + c) * ES,   ES the element size of the tensor plan.
 * tensor->scale[k] / bias[k] belong to the colour (k = 0 R, 1 G, 2 B), not to the position inside the pixel; a mirrored row is
 * reversed pixel by pixel, the channels of a pixel in place.  The A element of the 4-channel orders is one value for the call:
 *   unsigned elements: alpha << (msb_aligned ? 16 - D : 0), D the output depth; alpha = -1 stands for 2^D - 1 (opaque), and a value
 *                      outside -1 .. 2^D - 1 gives HMGPU_EINVAL;
 *   float elements:    alpha_value converted like a sample (round to nearest even, overflow to infinity); a value that is not
 *                      finite gives HMGPU_EINVAL.
 * The three-channel orders ignore both fields.
 * desc->layout must be HMGPU_EXPORT_RGB (else HMGPU_EINVAL).  The plan has one plane: width[0] / height[0] in pixels, row_bytes[0] =
 * width * C * ES (pixels of 3, 4, 6, 8, 12 or 16 bytes), and the coef of the planar RGB plan.  Validation is that of the planar call,
 * made by the same code, with the same statuses and in the same order -- the descriptor, scale, tensor and every window, the limits
 * of the scaled export, n, the handles, the destination (one plane of row_bytes[0]: pitch, batch stride, the span inside one
 * allocation of the context's device), the stream -- and after the plan of the planar call: the layout, then an unknown `order` or
 * a non-zero reserved word, then the alpha rules, each HMGPU_EINVAL; `pixel` NULL is HMGPU_EINVAL.  Everything is validated before
 * anything is enqueued and a refused call leaves the destination untouched.  The table slots, the per-call ring of window buffers,
 * the stream ordering (one event pair in, one out, when on_stream is 1) and the one launch per call are those of the planar calls.
 * A full group of 4 pixels whose first byte is 4-byte aligned (dst, pitch_bytes and batch_stride_bytes multiples of 4) is written
 * with dword stores, any other element by element; no byte beyond row_bytes[0] of a row is written.  The launch is not accounted
 * in hmgpu_stats. */
enum { HMGPU_PIXEL_RGB = 0, HMGPU_PIXEL_BGR = 1, HMGPU_PIXEL_RGBA = 2, HMGPU_PIXEL_BGRA = 3, HMGPU_PIXEL_ARGB = 4, HMGPU_PIXEL_ABGR = 5 };
typedef struct hmgpu_export_pixel {
  int32_t order;               /* HMGPU_PIXEL_* */
  int32_t alpha;               /* unsigned elements, 4-channel orders: code value 0 .. 2^D - 1 of A; -1 = 2^D - 1 (opaque) */
  float   alpha_value;         /* float elements, 4-channel orders: A = convert(alpha_value); must be finite */
  int32_t reserved[5];         /* 0 */
} hmgpu_export_pixel;
/* validates and reports what hmgpu_pictures_export_pixels writes per slot; host code, no device needed.  windows NULL: the crop of
 * desc->crop (n is not looked at); else n windows under the rules of hmgpu_export_windows_plan_for */
hmgpu_status hmgpu_export_pixels_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                          const hmgpu_export_tensor* tensor, int32_t n, const hmgpu_export_window windows[],
                                          const hmgpu_export_pixel* pixel, hmgpu_export_plan* out);
hmgpu_status hmgpu_pictures_export_pixels(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_export_desc* desc,
                                          const hmgpu_export_scale* scale, const hmgpu_export_tensor* tensor,
                                          const hmgpu_export_window windows[], const hmgpu_export_pixel* pixel, void* dst,
                                          int64_t pitch_bytes, int64_t batch_stride_bytes, int32_t on_stream, void* stream);
/* hmgpu_export_destination_check for hmgpu_pictures_export_pixels */
hmgpu_status hmgpu_export_pixels_destination_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                                   const hmgpu_export_tensor* tensor, const hmgpu_export_window windows[],
                                                   const hmgpu_export_pixel* pixel, void* dst, int64_t pitch_bytes,
                                                   int64_t batch_stride_bytes);

/* ------------------------------------------------------------------------------------------------ colour export
 * A colour stage inside the RGB exports: a per-channel 1D shaper and a 3D lattice with tetrahedral interpolation,
 * the mechanism of .cube files -- transfer change (PQ / HLG to SDR), gamut change, tone mapping and grades as one table.  The colour
 * science stays on the host as data; the device part is integer arithmetic that tests/export_colour_ref.py restates exactly.
 *
 * Let D be the RGB output depth of the call (desc->bit_depth[0], or the coding luma depth when that is 0; 8 .. 16), M = 2^D - 1, and
 * (v_r, v_g, v_b) the integers the RGB export produces for an output pixel: after the matrix, after resampling and the final clip,
 * before the msb_aligned shift, the float map, the mirror and the packing.  A LUT has a depth (that D), an optional shaper
 * sh[3][2^D] of uint16 and a lattice of L^3 nodes, L = 0 (shaper only) or 2 .. 65; a node is three uint16 output code values <= M.
 * Host layout lattice[b][g][r][3], R fastest (the order of a .cube file).
 *   1. position per channel c: with a shaper u_c = sh[c][v_c] (0 .. 65535); without, u_c = (v_c << (16 - D)) | (v_c >> (2D - 16))
 *      (bit replication);
 *   2. L = 0: the result is u_c (the shaper's entries are then code values <= M, checked at creation);
 *   3. cell and fraction: t_c = u_c * (L - 1), i_c = t_c >> 16, f_c = t_c & 0xffff; so i_c <= L - 2: the last node is approached,
 *      never indexed past;
 *   4. tetrahedral interpolation: the three fractions in descending order f_a >= f_b >= f_c (on a tie either order gives the same
 *      result: the differing vertex has weight 0); vertices V0 at (i_r, i_g, i_b), V1 one step along a, V2 along b as well, V3 along
 *      c as well (the far corner); weights 65536 - f_a, f_a - f_b, f_b - f_c, f_c; per output channel
 *         out = (sum_k w_k * V_k + 32768) >> 16
 *      in unsigned 32-bit arithmetic (the sum stays below 2^32); no clip: a convex combination of values <= M;
 *   5. out takes the place of v in everything the existing calls do afterwards: the msb_aligned shift, the float map
 *      fl(fl(v * scale[k]) + bias[k]) with k the colour, the mirror, the alpha element and the channel order of packed pixels.
 *
 * hmgpu_colour_lut_create copies the tables from host memory into device memory of the context and returns when the copy is done;
 * at most HMGPU_COLOUR_MAX_LUTS are live per context (HMGPU_ENOMEM beyond).  HMGPU_EINVAL (hmgpu_colour_lut_check, host code: the
 * same rules without a context): depth outside 8 .. 16; size not 0 and not 2 .. 65; has_shaper not 0 / 1; neither shaper nor
 * lattice; a non-zero reserved word; a null pointer that is needed; a node above M; an entry of a shaper-only LUT above M.
 * hmgpu_colour_lut_destroy is safe while exports that read the LUT are in flight: it waits for the last of them before the memory is
 * released (the rule of the scale-table slots).  A destroyed handle, or one of another context, gives HMGPU_EINVAL wherever used.
 *
 * hmgpu_pictures_export_colour is one call for every RGB form: pixel NULL three planes (dst / pitch_bytes / batch_stride_bytes per
 * plane), else packed pixels in dst[0]; windows NULL the crop of desc; scale and tensor may be NULL.  Slot i receives what
 * hmgpu_pictures_export / _windows / _pixels write for the same arguments, with step 5 applied.  Validation is that of the matching
 * existing call, made by the same code with the same statuses in the same order; then, each HMGPU_EINVAL: a layout that is not RGB,
 * a `lut` not live in this context, a LUT depth different from D.  Everything is validated before anything is enqueued and a refused
 * call leaves the destination untouched.  One launch per call, the stream ordering of the existing calls; not accounted in
 * hmgpu_stats. */
enum { HMGPU_COLOUR_MAX_LUTS = 8 };
typedef int64_t hmgpu_lut;     /* handle of a LUT of one context; 0 is never a handle */
typedef struct hmgpu_colour_lut_desc {
  int32_t depth;               /* D: 8 .. 16 */
  int32_t size;                /* L: 0 (shaper only), 2 .. 65 */
  int32_t has_shaper;          /* 0 / 1 */
  int32_t reserved[5];         /* 0 */
} hmgpu_colour_lut_desc;
/* the rules of hmgpu_colour_lut_create that need no context; host code */
hmgpu_status hmgpu_colour_lut_check(const hmgpu_colour_lut_desc* desc, const uint16_t* shaper, const uint16_t* lattice);
hmgpu_status hmgpu_colour_lut_create(hmgpu_ctx* ctx, const hmgpu_colour_lut_desc* desc, const uint16_t* shaper, const uint16_t* lattice,
                                     hmgpu_lut* out);
hmgpu_status hmgpu_colour_lut_destroy(hmgpu_ctx* ctx, hmgpu_lut lut);
/* the plan of the matching existing call (pixel NULL: hmgpu_export_windows_plan_for / hmgpu_export_tensor_plan_for, else
 * hmgpu_export_pixels_plan_for) with its refusals, then: the layout not RGB, an invalid `lut` description (the rules above that
 * need no tables), its depth different from D, each HMGPU_EINVAL; host code, no device needed */
hmgpu_status hmgpu_export_colour_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                          const hmgpu_export_tensor* tensor, int32_t n, const hmgpu_export_window windows[],
                                          const hmgpu_export_pixel* pixel, const hmgpu_colour_lut_desc* lut, hmgpu_export_plan* out);
hmgpu_status hmgpu_pictures_export_colour(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_export_desc* desc,
                                          const hmgpu_export_scale* scale, const hmgpu_export_tensor* tensor,
                                          const hmgpu_export_window windows[], const hmgpu_export_pixel* pixel, hmgpu_lut lut,
                                          void* const dst[3], const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3],
                                          int32_t on_stream, void* stream);
/* hmgpu_export_destination_check for hmgpu_pictures_export_colour: the status it would give these arguments; enqueues nothing */
hmgpu_status hmgpu_export_colour_destination_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                                   const hmgpu_export_tensor* tensor, const hmgpu_export_window windows[],
                                                   const hmgpu_export_pixel* pixel, hmgpu_lut lut, void* const dst[3],
                                                   const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3]);

/* ------------------------------------------------------------------------------------------------ chroma export
 * A chroma stage inside the RGB exports, off by default: Cb and Cr of 4:2:0 and 4:2:2 pictures linearly interpolated
 * to the luma grid at the chroma sample location the stream signals (VUI chroma_sample_loc_type, H.265 figure E.1), before the
 * matrix, where the existing calls replicate each chroma sample.  Integer arithmetic that tests/export_chroma_ref.py restates exactly.
 *
 * Let C be one chroma component of the decoded picture, Wc x Hc samples: the whole decoded plane, not the crop or window.  Each axis
 * yields two taps (i0, w0) and (i0 + 1, 4 - w0), weights in quarters, tap indices clamped to 0 .. size - 1.  For the luma
 * coordinate x (or y) on an axis, with j = x >> 1:
 *                                                     x even                    x odd
 *   not subsampled                                    (x: 4)                    (x: 4)
 *   subsampled, co-sited                              (j: 4)                    (j: 2, j + 1: 2)
 *   subsampled, centred                               (j - 1: 1, j: 3)          (j: 3, j + 1: 1)
 *   subsampled, co-sited with the odd row (bottom)    (j - 1: 2, j: 2)          (j: 4)
 * 4:2:0 with loc = chroma_sample_loc_type: horizontally co-sited for loc 0, 2, 4 and centred for 1, 3, 5; vertically centred for
 * loc 0, 1, co-sited for 2, 3 and bottom for 4, 5.  4:2:2: horizontally co-sited, vertically not subsampled; loc is ignored, as the
 * standard says.  4:4:4 and 4:0:0: the stage is the identity.  The interpolated value, at the coding chroma depth, is
 *   c' = (sum over the 2 x 2 taps of wx * wy * C[iy][ix] + 8) >> 4
 * and takes the place of the replicated sample in everything the existing calls do afterwards: the matrix or the identity rule,
 * resampling, the clip, the colour stage, the msb_aligned shift, the float map, the mirror and the packing.  Taps may lie outside a
 * crop or window as long as they are inside the decoded plane, so the export of a window is the window of the whole picture's export.
 *
 * hmgpu_pictures_export_chroma is one call for every RGB form and takes the arguments of hmgpu_pictures_export_colour, with lut 0
 * meaning no colour stage.  Validation is that of the matching existing call (with a lut: hmgpu_pictures_export_colour), made by the
 * same code with the same statuses in the same order; then a layout that is not RGB (HMGPU_EINVAL); then `chroma` NULL, a non-zero
 * reserved word or loc outside 0 .. 5 (HMGPU_EINVAL); then an unknown filter (HMGPU_EUNSUPPORTED).  Everything is validated before
 * anything is enqueued and a refused call leaves the destination untouched.  With HMGPU_CHROMA_REPLICATE the call writes, bit for
 * bit, what the matching existing call writes.  One launch per call; the stream ordering, the table slots and the window ring of the
 * existing calls; not accounted in hmgpu_stats. */
enum { HMGPU_CHROMA_REPLICATE = 0, HMGPU_CHROMA_LINEAR = 1 };
typedef struct hmgpu_export_chroma {
  int32_t filter;              /* HMGPU_CHROMA_* */
  int32_t loc;                 /* chroma_sample_loc_type 0 .. 5 (4:2:0; validated and otherwise ignored for the other formats) */
  int32_t reserved[6];         /* 0 */
} hmgpu_export_chroma;
/* the plan of the matching existing call (lut NULL: hmgpu_export_pixels_plan_for / _windows_plan_for / _tensor_plan_for, else
 * hmgpu_export_colour_plan_for) with its refusals, then the rules above; host code, no device needed */
hmgpu_status hmgpu_export_chroma_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                          const hmgpu_export_tensor* tensor, int32_t n, const hmgpu_export_window windows[],
                                          const hmgpu_export_pixel* pixel, const hmgpu_colour_lut_desc* lut,
                                          const hmgpu_export_chroma* chroma, hmgpu_export_plan* out);
hmgpu_status hmgpu_pictures_export_chroma(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_export_desc* desc,
                                          const hmgpu_export_scale* scale, const hmgpu_export_tensor* tensor,
                                          const hmgpu_export_window windows[], const hmgpu_export_pixel* pixel, hmgpu_lut lut,
                                          const hmgpu_export_chroma* chroma, void* const dst[3], const int64_t pitch_bytes[3],
                                          const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream);
/* hmgpu_export_destination_check for hmgpu_pictures_export_chroma: the status it would give these arguments; enqueues nothing */
hmgpu_status hmgpu_export_chroma_destination_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                                   const hmgpu_export_tensor* tensor, const hmgpu_export_window windows[],
                                                   const hmgpu_export_pixel* pixel, hmgpu_lut lut, const hmgpu_export_chroma* chroma,
                                                   void* const dst[3], const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3]);

/* ------------------------------------------------------------------------------------------------ affine warp export
 * An inverse affine map per picture inside the RGB exports: rotation, shear, zoom, sub-sample shifts and the display
 * orientations, in the one launch, where the other calls offer a window, a resize and a mirror.  Integer arithmetic that
 * tests/export_warp_ref.py restates exactly.
 *
 * D is the RGB output depth of the call and M = 2^D - 1.  S is the Ws x Hs window of slot i (windows[i].crop, or desc->crop when
 * windows is NULL) as three planes of integers 0 .. M: exactly what the unscaled call writes for that window with the same desc and
 * chroma arguments before the colour stage, the msb_aligned shift, the float map, the mirror and the packing -- after the matrix or
 * the identity rule and after the clip.  With HMGPU_CHROMA_LINEAR the chroma is interpolated before the matrix as "chroma export"
 * says; its taps may lie outside the window but inside the decoded plane.  v, the integer of output pixel (ox, oy), 0 <= ox < width,
 * 0 <= oy < height, takes the place of the export's v in everything the existing calls do afterwards: the colour stage, the
 * msb_aligned shift, fl(fl(v * scale[k]) + bias[k]), the mirror of windows[i].flip, the alpha element and the channel order.
 *
 * A map is six int32 values in Q16, m[0..5].  All coordinate arithmetic is in signed 64-bit integers, >> an arithmetic shift.
 *   HMGPU_WARP_BILINEAR   X = m0*ox + m1*oy + m2 + 128, Y = m3*ox + m4*oy + m5 + 128; ix = X >> 16, fx = (X >> 8) & 255, iy and fy
 *                         alike.  Taps (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1) with the weights (256-fx)(256-fy), fx(256-fy),
 *                         (256-fx)fy, fx*fy, which sum to 65536; v = (sum of w * tap + 32768) >> 16 in unsigned 32-bit arithmetic
 *                         (at most 65535 * 65536 + 32768 < 2^32).  No clip: v is a convex combination of values <= M.
 *   HMGPU_WARP_NEAREST    the same X and Y with 32768 in place of 128; the one tap (X >> 16, Y >> 16).
 * Border, per tap and on the 64-bit values before anything is narrowed:
 *   HMGPU_WARP_EDGE       tap (x, y) = S[c][clamp(y, 0, Hs-1)][clamp(x, 0, Ws-1)]
 *   HMGPU_WARP_FILL       tap (x, y) = S[c][y][x] inside the window, else fill[c]: each tap decided on its own, the blending of
 *                         grid_sample(padding_mode="zeros") at the rim.  Samples of the decoded picture outside the window never
 *                         contribute (the scaled export's rule).
 * m = {65536, 0, 0, 0, 65536, 0} with width x height the window's size writes, bit for bit, what the matching existing call writes;
 * a map whose six values are multiples of 65536 is a permutation, shift or replication of S under either filter.  There is no
 * prefilter: a map that shrinks by more than about 2x aliases -- resize with the scaled export (hmgpu_export_scale) instead.
 * Perspective maps, reflect padding, bicubic taps and the YUV layouts are not offered.
 *
 * hmgpu_pictures_export_warp takes the arguments of hmgpu_pictures_export_chroma without `scale` (the map is the scale): pixel NULL
 * three planes, lut 0 no colour stage, chroma NULL replicate, windows NULL desc->crop.  Validation is that of the matching existing
 * call with scale NULL, made by the same code with the same statuses in the same order, except that the windows may differ in size
 * (the output size comes from `warp`; each window obeys hmgpu_export_plan_for's rules on its own) and that the destination is checked
 * against width x height.  Then the warp rules: `warp` or `maps` NULL, a non-zero reserved word in either struct, width / height
 * outside 1 .. 16384, a fill[c] outside 0 .. M under HMGPU_WARP_FILL (ignored under EDGE), a layout that is not RGB (HMGPU_EINVAL);
 * then an unknown filter or border (HMGPU_EUNSUPPORTED).  The six map values are unrestricted: any int32 is legal and defined above.
 * Everything is validated before anything is enqueued and a refused call leaves the destination untouched.  The plan is that of the
 * matching planar or packed call with every plane width x height.  One launch per call; the maps and window origins travel in one
 * copy through the window ring; the stream ordering of the existing calls; not accounted in hmgpu_stats. */
enum { HMGPU_WARP_NEAREST = 0, HMGPU_WARP_BILINEAR = 1 };
enum { HMGPU_WARP_EDGE = 0, HMGPU_WARP_FILL = 1 };
typedef struct hmgpu_export_warp {
  int32_t width, height;       /* the output, 1 .. 16384 each */
  int32_t filter;              /* HMGPU_WARP_NEAREST / _BILINEAR */
  int32_t border;              /* HMGPU_WARP_EDGE / _FILL */
  int32_t fill[3];             /* R, G, B code values 0 .. M of HMGPU_WARP_FILL */
  int32_t reserved[5];         /* 0 */
} hmgpu_export_warp;
typedef struct hmgpu_warp_map {
  int32_t m[6];                /* Q16: source x = m0*ox + m1*oy + m2, source y = m3*ox + m4*oy + m5 (sample indices of the window) */
  int32_t reserved[2];         /* 0 */
} hmgpu_warp_map;
/* host code, no device needed; n maps (and windows, unless NULL) */
hmgpu_status hmgpu_export_warp_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* desc, const hmgpu_export_tensor* tensor,
                                        int32_t n, const hmgpu_export_window windows[], const hmgpu_export_pixel* pixel,
                                        const hmgpu_colour_lut_desc* lut, const hmgpu_export_chroma* chroma,
                                        const hmgpu_export_warp* warp, const hmgpu_warp_map maps[], hmgpu_export_plan* out);
hmgpu_status hmgpu_pictures_export_warp(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_export_desc* desc,
                                        const hmgpu_export_tensor* tensor, const hmgpu_export_window windows[],
                                        const hmgpu_export_pixel* pixel, hmgpu_lut lut, const hmgpu_export_chroma* chroma,
                                        const hmgpu_export_warp* warp, const hmgpu_warp_map maps[], void* const dst[3],
                                        const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream);
/* hmgpu_export_destination_check for hmgpu_pictures_export_warp: the status it would give these arguments; enqueues nothing */
hmgpu_status hmgpu_export_warp_destination_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_export_desc* desc, const hmgpu_export_tensor* tensor,
                                                 const hmgpu_export_window windows[], const hmgpu_export_pixel* pixel, hmgpu_lut lut,
                                                 const hmgpu_export_chroma* chroma, const hmgpu_export_warp* warp,
                                                 const hmgpu_warp_map maps[], void* const dst[3], const int64_t pitch_bytes[3],
                                                 const int64_t batch_stride_bytes[3]);

/* ------------------------------------------------------------------------------------------------ format export
 * The planar and semi-planar layouts with Cb and Cr at a chroma format the caller chooses, where the calls above
 * write them at the picture's own: three full-resolution planes from a 4:2:0 stream, NV12 / P010 from a 4:2:2 or 4:4:4 one.
 * TVideoIOYuv::writePlane has the operation (fileFormat != srcFormat, TVideoIOYuv.cpp:362-483); its REPLICATE / DROP forms are
 * writePlane's index arithmetic, the LINEAR ones interpolate and decimate at the signalled sample location.  Integer arithmetic that
 * tests/export_format_ref.py restates exactly.
 *
 * Luma is written exactly as hmgpu_pictures_export(_windows) writes it.  Chroma is decided per axis, by comparing the subsampling of
 * the source format with that of `chroma_format`; no conversion gains samples on one axis and loses them on the other.  With C one
 * chroma component of the decoded picture (the whole decoded plane, not the crop or window) and j the output chroma index on the axis:
 *   same on the axis      the sample j itself, weight 4
 *   gain, REPLICATE       sample j >> 1, weight 4 (writePlane's src[x >> sx]; rows by the same rule -- writePlane's own row pointer runs
 *                         one row ahead on odd rows there, a path HM's applications never take)
 *   gain, LINEAR          the two taps of the table in "chroma export" for the luma coordinate j, with the siting of `loc`; a 4:2:2
 *                         source or output is horizontally co-sited whatever loc says.  4:2:0 -> 4:4:4 gives exactly the c' of that
 *                         section, 4:2:0 -> 4:2:2 uses its vertical taps only, 4:2:2 -> 4:4:4 its horizontal ones only
 *   loss, DROP            sample 2j, weight 4 (writePlane's src[x << sx], a row written only when (y444 & mask) == 0); loc is ignored
 *   loss, LINEAR          taps in quarters around j by the siting of the axis:
 *                           co-sited (horizontal loc 0, 2, 4 and every 4:2:2 output; vertical loc 2, 3)    (2j - 1: 1, 2j: 2, 2j + 1: 1)
 *                           centred (horizontal loc 1, 3, 5; vertical loc 0, 1)                           (2j: 2, 2j + 1: 2)
 *                           co-sited with the odd row (vertical loc 4, 5)                                 (2j: 1, 2j + 1: 2, 2j + 2: 1)
 * The converted value, at the coding chroma depth, is
 *   c = (sum over the taps of wx * wy * C[iy][ix] + 8) >> 4
 * with tap indices clamped to the decoded plane, 0 .. size - 1, so that the export of a window is the window of the whole picture's
 * export.  The decimation taps are the inverses in siting of the interpolation ones: a constant plane stays constant, and REPLICATE
 * followed by DROP returns the plane unchanged.  A 4:0:0 source with any other output writes Cb = Cr = 1 << (D - 1), D the chroma
 * output depth (writePlane's `value`, TVideoIOYuv.cpp:387); output 4:0:0 writes Y only, one plane; an output format equal to the
 * source's writes bit for bit what hmgpu_pictures_export / _windows writes.  The converted sample takes the place of the decoded
 * one in everything the two layouts do afterwards: the bit-depth rule, msb_aligned, the float map, the mirror, the CbCr interleave
 * (NV12 / NV16 / NV24, P010 / P016).
 *
 * With `scale`: Y is resampled as hmgpu_pictures_export resamples it; Cb / Cr are resampled straight from the cropped source chroma
 * plane to (width >> csx_out) x (height >> csy_out) with the table rule of plane class 1 ("scaled export": in = the cropped source
 * chroma size, out = that size, half-sample centres), each axis within the 32x / 8x limits.  up / down / loc are validated and then
 * unused.  A 4:0:0 source still gives the constant.  hmgpu_export_format_scale_taps reports these tables.
 *
 * Validation, in this order, everything before anything is enqueued and a refused call leaving the destination untouched:
 *   1. the rules of the matching existing call (hmgpu_pictures_export_windows; windows NULL: hmgpu_pictures_export), in their order
 *      -- semi-planar float elements stay HMGPU_EUNSUPPORTED;
 *   2. the RGB layout: HMGPU_EINVAL;
 *   3. `format` NULL, a non-zero reserved word, chroma_format outside 0 .. 3 or loc outside 0 .. 5: HMGPU_EINVAL; a 4:0:0 source
 *      whose chroma output depth the matching call did not have to look at (1 .. 16, within the container; float elements: the
 *      container the depths need): HMGPU_EINVAL;
 *   4. an unknown `up` or `down`: HMGPU_EUNSUPPORTED;
 *   5. a crop or window whose left / top edge or size, or a scaled output size, does not cover whole chroma samples of the output
 *      format as well: HMGPU_EINVAL; (scaled) a chroma axis beyond the scaling limits: HMGPU_EUNSUPPORTED;
 *   6. the destination against the plan of the output format.
 * One launch per call (a scaled call from a 4:0:0 source: two); the stream ordering, the table slots and the window ring of the
 * existing calls; not accounted in hmgpu_stats. */
enum { HMGPU_DOWN_DROP = 0, HMGPU_DOWN_LINEAR = 1 };
typedef struct hmgpu_export_format {
  int32_t chroma_format;       /* output: 0 4:0:0, 1 4:2:0, 2 4:2:2, 3 4:4:4 */
  int32_t up;                  /* HMGPU_CHROMA_REPLICATE | HMGPU_CHROMA_LINEAR, where an axis gains samples */
  int32_t down;                /* HMGPU_DOWN_*, where an axis loses samples */
  int32_t loc;                 /* chroma_sample_loc_type 0 .. 5 of the 4:2:0 side of the conversion */
  int32_t reserved[4];         /* 0 */
} hmgpu_export_format;
/* the plan of the output format: the plane sizes of `format`->chroma_format (semi-planar: plane 1 in CbCr pairs, row_bytes of both
 * components); windows NULL: the plan of desc's crop (n ignored); host code, no device needed */
hmgpu_status hmgpu_export_format_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                          const hmgpu_export_tensor* tensor, int32_t n, const hmgpu_export_window windows[],
                                          const hmgpu_export_format* format, hmgpu_export_plan* out);
hmgpu_status hmgpu_pictures_export_format(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_export_desc* desc,
                                          const hmgpu_export_scale* scale, const hmgpu_export_tensor* tensor,
                                          const hmgpu_export_window windows[], const hmgpu_export_format* format, void* const dst[3],
                                          const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3], int32_t on_stream,
                                          void* stream);
/* hmgpu_export_destination_check for hmgpu_pictures_export_format: the status it would give these arguments; enqueues nothing */
hmgpu_status hmgpu_export_format_destination_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                                   const hmgpu_export_tensor* tensor, const hmgpu_export_window windows[],
                                                   const hmgpu_export_format* format, void* const dst[3], const int64_t pitch_bytes[3],
                                                   const int64_t batch_stride_bytes[3]);
/* hmgpu_export_scale_taps for a scaled format export of desc's crop: the table of plane class `chroma` and `axis` as that export
 * uses it (class 1: from the cropped source chroma size to the output format's).  No chroma class where the source or the output
 * is 4:0:0 (HMGPU_EINVAL). */
hmgpu_status hmgpu_export_format_scale_taps(const hmgpu_seq_params* seq, const hmgpu_export_desc* desc, const hmgpu_export_scale* scale,
                                            const hmgpu_export_format* format, int32_t chroma, int32_t axis, int32_t max_taps,
                                            int32_t* first, int32_t* count, int16_t* weights);

/* ------------------------------------------------------------------------------------------------ packed YUV
 * Y, Cb and Cr interleaved into words: the layouts of capture cards, SDI and the display and encode APIs.  All words
 * are little endian; D is the depth of a format and cf its chroma format; values are D-bit unsigned integers.
 *
 *   format  cf     D   memory, per unit                                                              bytes per unit
 *   UYVY    4:2:2  8   bytes Cb Y0 Cr Y1 per two pixels                                              4
 *   YUY2    4:2:2  8   bytes Y0 Cb Y1 Cr per two pixels                                              4
 *   Y210    4:2:2  10  uint16 Y0 Cb Y1 Cr, each v << 6 (low six bits 0)                              8
 *   Y216    4:2:2  16  uint16 Y0 Cb Y1 Cr                                                            8
 *   V210    4:2:2  10  six pixels in four uint32, three values per word at bits 0-9, 10-19, 20-29,   16
 *                      bits 30-31 zero
 *   AYUV    4:4:4  8   bytes Cr Cb Y A per pixel                                                     4
 *   Y410    4:4:4  10  uint32 Cb | Y << 10 | Cr << 20 | A << 30 per pixel                            4
 *   Y416    4:4:4  16  uint16 Cb Y Cr A per pixel                                                    8
 *
 * V210, for the group of pixels 6g .. 6g + 5 with Cbm = Cb[3g + m] and Crm = Cr[3g + m]:
 *   w0 = Cb0 | Y0 << 10 | Cr0 << 20     w1 = Y1 | Cb1 << 10 | Y2 << 20     w2 = Cr1 | Y3 << 10 | Cb2 << 20     w3 = Y4 | Cr2 << 10 | Y5 << 20
 * A V210 row is ceil(W / 6) * 16 bytes: that is row_bytes, the least pitch.  A luma or chroma value whose pixel index is at or beyond
 * the output width is written as 0 inside the last group; bytes between the end of the last group and the pitch are never written.
 * The customary 128-byte row alignment (48 pixels) is the caller's choice of pitch.
 * A is a constant of the call: `alpha` is 0 .. 255 for AYUV, 0 .. 3 for Y410, 0 .. 65535 for Y416, and must be 0 for the 4:2:2 formats.
 *
 * hmgpu_pictures_export_yuvpack.  Let P be what hmgpu_pictures_export_format writes for the same pictures, crop or windows, flips and
 * `format` (up, down, loc) with layout HMGPU_EXPORT_PLANAR, format->chroma_format = cf, bit_depth {D, D}, unsigned elements of the
 * container D needs and msb_aligned 0: Y, Cb and Cr after the chroma-format conversion, the bit-depth rule and the mirror.  The
 * packed output holds exactly the values of P in the layout above; nothing else is computed.  So a 4:0:0 source gives Cb = Cr =
 * 1 << (D - 1), every source chroma format works with every word format, the export of a window is the window of the whole
 * picture's export, and the mirror reverses pixels (the pair Y0, Y1 of a 4:2:2 unit swaps with the unit; V210 groups are those of
 * the mirrored row).  Every argument but `pack` has the type and meaning it has in hmgpu_pictures_export_format.
 *
 * Validation, in this order, everything before anything is enqueued and a refused call leaving the destination untouched:
 *   1. `pack` NULL or a non-zero reserved word: HMGPU_EINVAL; an unknown pack->format: HMGPU_EUNSUPPORTED (the format names D and
 *      cf, which every later rule needs);
 *   2. `desc` NULL, desc->layout other than HMGPU_EXPORT_PLANAR, a desc->bit_depth[] that is neither 0 nor D, a bytes_per_sample that is neither 0
 *      nor the container of D, msb_aligned other than 0: HMGPU_EINVAL;
 *   3. `format` NULL or format->chroma_format other than cf: HMGPU_EINVAL;
 *   4. alpha outside the format's range (the 4:2:2 formats: other than 0): HMGPU_EINVAL;
 *   5. `scale` not NULL: HMGPU_EUNSUPPORTED (the scaled kernels resample planes separately); `tensor` with a float sample type:
 *      HMGPU_EUNSUPPORTED;
 *   6. the rules of hmgpu_pictures_export_format for the call that defines P, in their order: among them n, the crop or every
 *      window covering whole chroma samples of the source format and of cf (even left edges and widths for the 4:2:2 formats), one
 *      size for all windows, an unknown up or down;
 *   7. the destination against the plan: dst[1] or dst[2] not NULL; an address, pitch or batch stride that is no multiple of 1
 *      (UYVY, YUY2, AYUV), 2 (Y210, Y216, Y416) or 4 (V210, Y410) bytes; a pitch below row_bytes, a batch stride below
 *      pitch * (H - 1) + row_bytes, a span of the n pictures outside one allocation of the context's device: HMGPU_EINVAL.
 * The plan has one plane: width[0] / height[0] in pixels, row_bytes[0] as above.  Picture i is written at dst[0] +
 * i * batch_stride_bytes.  Up to HMGPU_EXPORT_MAX_BATCH pictures, handles may repeat, one launch per call (k_export_yuvpack.hip),
 * the stream ordering of hmgpu_pictures_export; not accounted in hmgpu_stats. */
enum { HMGPU_YUVPACK_UYVY = 0, HMGPU_YUVPACK_YUY2 = 1, HMGPU_YUVPACK_Y210 = 2, HMGPU_YUVPACK_Y216 = 3, HMGPU_YUVPACK_V210 = 4,
       HMGPU_YUVPACK_AYUV = 5, HMGPU_YUVPACK_Y410 = 6, HMGPU_YUVPACK_Y416 = 7 };
typedef struct hmgpu_export_yuvpack {
  int32_t format;              /* HMGPU_YUVPACK_* */
  int32_t alpha;               /* A of AYUV / Y410 / Y416; 0 for the 4:2:2 formats */
  int32_t reserved[6];         /* 0 */
} hmgpu_export_yuvpack;
/* the one-plane plan; windows NULL: the plan of desc's crop (n ignored); host code, no device needed */
hmgpu_status hmgpu_export_yuvpack_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* desc, const hmgpu_export_tensor* tensor,
                                           int32_t n, const hmgpu_export_window windows[], const hmgpu_export_format* format,
                                           const hmgpu_export_yuvpack* pack, hmgpu_export_plan* out);
hmgpu_status hmgpu_pictures_export_yuvpack(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_export_desc* desc,
                                           const hmgpu_export_scale* scale, const hmgpu_export_tensor* tensor,
                                           const hmgpu_export_window windows[], const hmgpu_export_format* format,
                                           const hmgpu_export_yuvpack* pack, void* const dst[3], const int64_t pitch_bytes[3],
                                           const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream);
/* hmgpu_export_destination_check for hmgpu_pictures_export_yuvpack: the status it would give these arguments; enqueues nothing */
hmgpu_status hmgpu_export_yuvpack_destination_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_export_desc* desc,
                                                    const hmgpu_export_scale* scale, const hmgpu_export_tensor* tensor,
                                                    const hmgpu_export_window windows[], const hmgpu_export_format* format,
                                                    const hmgpu_export_yuvpack* pack, void* const dst[3], const int64_t pitch_bytes[3],
                                                    const int64_t batch_stride_bytes[3]);

/* ------------------------------------------------------------------------------------------------ picture import
 * The way in from device memory: planar or semi-planar YUV, or RGB as three planes or as packed pixels, in
 * caller-owned memory of the context's GPU becomes the samples of up to HMGPU_EXPORT_MAX_BATCH acquired pictures -- one kernel
 * launch per call, no host copy, no wait.  It is the inverse direction of the exports above and restates TVideoIOYuv::read
 * (TVideoIOYuv.cpp:633-696) with readPlane (:227-349) and scalePlane (:70-87).  Integer arithmetic that tests/import_ref.py
 * restates exactly.  The descriptor describes the SOURCE:
 *
 * layout / order   HMGPU_EXPORT_PLANAR (Y, Cb, Cr planes), HMGPU_EXPORT_SEMIPLANAR (Y + one interleaved CbCr plane) or
 *                  HMGPU_EXPORT_RGB.  order = -1: planes (RGB: src[0] R, src[1] G, src[2] B); RGB with order = HMGPU_PIXEL_*: packed
 *                  pixels in src[0], 3 or 4 elements each, the A element read over.  The YUV layouts need order = -1.
 * width, height    the source size in luma samples, 0 = the picture's coded size; at most the coded size, and whole chroma samples
 *                  of the source's and of the picture's chroma format.  Padding (readPlane :333-345): with the converted planes
 *                  width x height (chroma: (width >> csx) x (height >> csy) of the PICTURE's format), sample (x, y) of the picture is
 *                  converted sample (min(x, width - 1), min(y, height - 1)) of its plane: the last column repeated, then the last row.
 * bit_depth[2]     the source depth D per channel type, luma / chroma (RGB: [0] for all three), 1 .. 16; 0 = the coding depth.
 * bytes_per_sample, msb_aligned, sample_type
 *                  HMGPU_SAMPLE_UINT: elements of 1 byte (D <= 8) or 2 bytes, LSB-aligned, or shifted left by 16 - D with
 *                  msb_aligned (2 bytes only; the element is shifted right by 16 - D).  An element above 2^D - 1 is read as 2^D - 1.
 *                  A float type (float16 / bfloat16 / float32 elements; msb_aligned 0, bytes_per_sample what the depths need, as in
 *                  hmgpu_export_tensor): element x of plane (RGB: colour) k becomes the integer
 *                    v = clip(rint(fadd(fmul((float)x, scale[k]), bias[k])), 0, 2^D - 1),  D = bit_depth[k ? 1 : 0] (RGB: [0])
 *                  -- the product and the sum two separately rounded binary32 operations (never one fma), rint to nearest with
 *                  ties to even, NaN gives 0, infinities the ends of the range.  numpy's float32 `*`, `+`, np.rint and np.clip
 *                  restate it.  Float elements: RGB and planar only (semi-planar: HMGPU_EUNSUPPORTED).
 * chroma_format    (YUV layouts) the source's format 0 .. 3, which may differ from the picture's; decided per axis by comparing
 *                  the subsampling of both, C a chroma component of the source at the source depth, j the picture's chroma index:
 *                    same on the axis                  the sample j itself
 *                    the picture has more samples      sample j >> 1 (readPlane :324)
 *                    the picture has fewer, DROP       sample 2j (:307; rows :286 / :297)
 *                    the picture has fewer, LINEAR     the decimation taps of "format export" (loss, LINEAR) at the siting of `loc`,
 *                                                      the picture's format in the place of the output's: c = (sum over the taps
 *                                                      of wx * wy * C[iy][ix] + 8) >> 4, tap indices clamped to the source plane
 *                  A 4:0:0 source gives Cb = Cr = 1 << (D - 1), D the source chroma depth (:263).  A 4:0:0 picture takes luma only.
 * bit-depth rule   per channel type after the conversion, scalePlane with CLIP_TO_709_RANGE 0; s = coding depth - D:
 *                    s >= 0: v << s;   s < 0: Clip3(0, 2^coding depth - 1, (v + (1 << (-s - 1))) >> -s)
 * matrix, full_range (RGB)   H.273's Kr / Kb equations forward, codes 1, 5, 6, 9 as in hmgpu_export_desc; code 0: Y = G, Cb = B,
 *                  Cr = R through the bit-depth rule, 4:4:4 pictures only (else HMGPU_EINVAL); other codes HMGPU_EUNSUPPORTED.
 *                  With M = 2^D - 1, ys = 219 << (bdY - 8) and cs = 224 << (bdC - 8) (limited) or 2^bdY - 1 and 2^bdC - 1 (full),
 *                  yo = 16 << (bdY - 8) or 0, co = 1 << (bdC - 1), Kg = 1 - Kr - Kb, rnd = round half away from zero, in double:
 *                    yR = rnd(Kr * ys / M * 2^S)   yB = rnd(Kb * ys / M * 2^S)   yG = rnd(ys / M * 2^S) - yR - yB
 *                    bB = rnd(cs / (2 M) * 2^S)    bR = rnd(-Kr / (1 - Kb) * cs / (2 M) * 2^S)    bG = -(bR + bB)
 *                    rR = rnd(cs / (2 M) * 2^S)    rB = rnd(-Kb / (1 - Kr) * cs / (2 M) * 2^S)    rG = -(rR + rB)
 *                    Y  = Clip3(0, 2^bdY - 1, ((yR * R + yG * G + yB * B + (1 << (S - 1))) >> S) + yo)
 *                    Cb = Clip3(0, 2^bdC - 1, ((bR * R + bG * G + bB * B + (1 << (S - 1))) >> S) + co)     Cr likewise with r*
 *                  (>> arithmetic), in 32-bit integers: S is the largest shift <= 30 for which, for every R, G, B in 0 .. M, no
 *                  sum leaves the int32 range: M * max(sum of the positive, -sum of the negative coefficients of a row) +
 *                  (1 << (S - 1)) <= 2^31 - 1.  S >= 17 always, so that M * (yR + yG + yB) is within 2^(S - 1) of ys * 2^S: black
 *                  and peak white give yo and yo + ys exactly; the chroma rows sum to 0, so R = G = B gives Cb = Cr = co exactly;
 *                  yR, yG, yB >= 0, so Y never falls when R, G or B rises.  Published in hmgpu_import_plan.coef:
 *                    coef[0] S   coef[1] 1 << (S - 1)   coef[2] yo   coef[3] co   coef[4..6] yR yG yB   coef[7..9] bR bG bB
 *                    coef[10..12] rR rG rB   coef[13] M   coef[14] 1: identity (matrix 0; coef[0..12] 0)   coef[15] 0
 *                  Cb and Cr are formed at every pixel and brought to the picture's format as a 4:4:4 source's are (`down`, `loc`).
 *
 * The plan: planes read (planar 3, semi-planar 2, a 4:0:0 source or picture 1 for the YUV layouts; RGB planes 3, packed pixels 1),
 * per plane width and height in samples (semi-planar CbCr: pairs; packed: pixels) and row_bytes, the least pitch.
 * Plane k of picture i is read from src[k] + i * batch_stride_bytes[k], rows pitch_bytes[k] apart: one [N, 3, H, W] tensor as well
 * as a tuple of planes.  Validation, in this order, everything before anything is enqueued, a refused call leaving every picture
 * untouched:
 *   1. the descriptor: NULL, a non-zero reserved word, layout, order, depths, container, a scale or bias that is not finite
 *      (float types), the size rules, chroma_format outside 0 .. 3, loc outside 0 .. 5, full_range, matrix 0 outside 4:4:4: HMGPU_EINVAL;
 *   2. an unknown matrix, `down` or sample type, semi-planar float elements: HMGPU_EUNSUPPORTED;
 *   3. n outside 1 .. HMGPU_EXPORT_MAX_BATCH: HMGPU_EINVAL;
 *   4. an invalid handle, or one handle twice (two writers): HMGPU_EINVAL;
 *   5. the source: a plane of the plan missing, an address, pitch or batch stride that is no multiple of the element size, a pitch
 *      below row_bytes, a batch stride below pitch * (height - 1) + row_bytes, a span of the n pictures that does not lie inside
 *      one allocation of the context's device: HMGPU_EINVAL;
 *   6. the stream, under the rules of hmgpu_picture_export.
 * The source is only read.  The picture is left as hmgpu_picture_upload leaves it, without the wait: it lives in the reconstruction
 * planes, carries no side information and no loop-filter record (the motion, residual, transform and loop-filter exports refuse
 * it), and its margins are filled when it is first used as a reference.  The kernel writes the picture's samples and nothing else.
 * Stream ordering is that of hmgpu_pictures_export, once per call: the kernel runs after all work enqueued for the pictures --
 * kernels that still read their old contents included -- and after everything already on `stream`, and every later operation of the
 * context waits for it.  Not accounted in hmgpu_stats. */
typedef struct hmgpu_import_desc {
  int32_t layout;              /* HMGPU_EXPORT_* of the source */
  int32_t order;               /* -1: planes; RGB: or HMGPU_PIXEL_*, packed pixels */
  int32_t width, height;       /* source size in luma samples; 0 = the coded size */
  int32_t bit_depth[2];        /* source depth luma / chroma (RGB: [0]); 1 .. 16, 0 = the coding depth */
  int32_t bytes_per_sample;    /* unsigned elements: 1 (depth <= 8) or 2 */
  int32_t msb_aligned;         /* 2-byte unsigned elements shifted left by 16 - depth */
  int32_t sample_type;         /* HMGPU_SAMPLE_* */
  float scale[3], bias[3];     /* float types: per source plane (Y, Cb, Cr) or colour (R, G, B) */
  int32_t chroma_format;       /* YUV layouts: the source's format 0 .. 3 */
  int32_t down, loc;           /* HMGPU_DOWN_* where the picture has fewer chroma samples; chroma_sample_loc_type 0 .. 5 */
  int32_t matrix, full_range;  /* RGB: matrix_coefficients and video_full_range_flag of the picture to make */
  int32_t reserved[8];         /* 0 */
} hmgpu_import_desc;
typedef struct hmgpu_import_plan {
  int32_t planes;              /* planes read: 1 .. 3 */
  int32_t width[3], height[3]; /* per plane, in samples (semi-planar CbCr: pairs; packed pixels: pixels) */
  int32_t row_bytes[3];        /* bytes of one row: the least pitch */
  int32_t coef[16];            /* RGB: see above; else 0 */
} hmgpu_import_plan;
/* validates a descriptor against a sequence (steps 1 and 2) and reports what an import reads; host code, no device needed */
hmgpu_status hmgpu_import_plan_for(const hmgpu_seq_params* seq, const hmgpu_import_desc* desc, hmgpu_import_plan* out);
hmgpu_status hmgpu_pictures_import(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_import_desc* desc,
                                   const void* const src[3], const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3],
                                   int32_t on_stream, void* stream);
/* steps 1, 2, 3 and 5 of the validation and nothing else: nothing is enqueued and no picture is named */
hmgpu_status hmgpu_import_source_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_import_desc* desc, const void* const src[3],
                                       const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3]);

/* hmgpu_pictures_import_yuvpack: the words of "packed YUV" on the way in.  The source is unpacked by that section's table into planes
 * Y, Cb, Cr of D-bit values -- V210 fields are (w >> s) & 0x3ff, Y210 elements e >> 6, A is read over, bits 30-31 of V210 words are
 * ignored, and so is everything in a V210 row's last group at or beyond the width -- and the pictures then receive exactly what
 * hmgpu_pictures_import gives for those planes with layout HMGPU_EXPORT_PLANAR, order -1, chroma_format cf, bit_depth {D, D},
 * unsigned LSB-aligned elements and the same width, height, down and loc: the padding rule, the down rule, the depth rule and the
 * picture state afterwards are those of that call.  Validation, in this order, a refused call leaving every picture untouched:
 *   1. `pack` NULL or a non-zero reserved word: HMGPU_EINVAL; an unknown pack->format: HMGPU_EUNSUPPORTED;
 *   2. `desc` NULL, a layout other than HMGPU_EXPORT_PLANAR, an order other than -1, a chroma_format other than cf, a bit_depth[]
 *      that is neither 0 nor D, a bytes_per_sample that is neither 0 nor the container of D, a sample_type other than
 *      HMGPU_SAMPLE_UINT, msb_aligned other than 0: HMGPU_EINVAL;
 *   3. the remaining steps of hmgpu_pictures_import for that planar source, in its order (reserved words, sizes, loc: HMGPU_EINVAL;
 *      an unknown `down`: HMGPU_EUNSUPPORTED; n; the handles; the source; the stream).  The source is one plane, src[0] (src[1] and
 *      src[2] must be NULL), whose address, pitch and batch stride are multiples of the format's element (1, 2 or 4 bytes, as for
 *      the export), with the pitch and stride rules of the plan: width[0] / height[0] in pixels, row_bytes[0] the bytes of a row. */
typedef struct hmgpu_import_yuvpack {
  int32_t format;              /* HMGPU_YUVPACK_* */
  int32_t reserved[7];         /* 0 */
} hmgpu_import_yuvpack;
/* steps 1 to 3 up to the descriptor's own rules, and the one-plane plan; host code, no device needed */
hmgpu_status hmgpu_import_yuvpack_plan_for(const hmgpu_seq_params* seq, const hmgpu_import_desc* desc, const hmgpu_import_yuvpack* pack,
                                           hmgpu_import_plan* out);
hmgpu_status hmgpu_pictures_import_yuvpack(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_import_desc* desc,
                                           const hmgpu_import_yuvpack* pack, const void* const src[3], const int64_t pitch_bytes[3],
                                           const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream);
/* the validation without the handles and the stream: nothing is enqueued and no picture is named */
hmgpu_status hmgpu_import_yuvpack_source_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_import_desc* desc, const hmgpu_import_yuvpack* pack,
                                               const void* const src[3], const int64_t pitch_bytes[3],
                                               const int64_t batch_stride_bytes[3]);

/* ------------------------------------------------------------------------------------------------ error concealment
 * The CTUs of a picture that a damaged stream did not deliver, filled on the device from another picture of the context or with a
 * constant: up to HMGPU_EXPORT_MAX_BATCH jobs and one kernel launch per call (plus the margin pass of the concealed
 * pictures).  The library decides nothing: the caller names the destination, the source, the CTUs and the mode.
 *
 * A job writes the FINAL planes of dst -- the planes hmgpu_picture_download reads: the SAO planes when the picture went through SAO,
 * else the reconstruction planes -- and reads the final planes of src.  Of a masked CTU (ctu_mask: bit (a & 7) of byte a >> 3 is CTU a
 * in raster order; NULL: every CTU) every sample inside width x height is written, in every component the format has; nothing else
 * is.  c: the component, w_c x h_c its plane, csx / csy its subsampling.
 *   HMGPU_CONCEAL_COPY    sample (x, y) = sample (x, y) of src.
 *   HMGPU_CONCEAL_MOTION  per 8x8 luma block of the CTU (its 4x4 / 4x8 / 8x8 chroma samples by format): look at the 4x4 block B of src
 *                         at the block's top-left corner.  When src has side information (the rule of the motion export below) and
 *                         list 0 is `used` in B by that export's rule, the slice-type term included, take mv and ref_poc of list 0;
 *                         else the same of list 1.  With td = clip3(-128, 127, src_poc - ref_poc), tb = clip3(-128, 127, dst_poc -
 *                         src_poc) (H.265 8.5.3.2.7): tx = (16384 + |td| / 2) / td (truncating), ds = clip3(-4096, 4095, (tb * tx + 32)
 *                         >> 6), v = clip3(-32768, 32767, sign(ds * mv) * ((|ds * mv| + 127) >> 8)) per coordinate.  v = 0 when td = 0,
 *                         no list is used, or src has no side information.  dx = (v.hor + 2) >> 2, dy = (v.ver + 2) >> 2 (arithmetic
 *                         shifts); chroma dx >> csx, dy >> csy.  Sample (x, y) = sample (clamp(x + dx, 0, w_c - 1), clamp(y + dy, 0,
 *                         h_c - 1)) of src: no vector leaves the plane, margins are never read.
 *   src == HMGPU_NO_PIC   sample = fill[c], or 1 << (bit_depth_c - 1) where fill[c] < 0 (either mode).
 *                         "Side information" is a property of the handle: the arrays decompress calls staged there since
 *                         hmgpu_picture_acquire, hmgpu_picture_upload or hmgpu_picture_commit_received last cleared the record.  This
 *                         call clears nothing, so a handle reused for a concealed picture without one of those calls still carries
 *                         the arrays of the picture decoded there before: ask for HMGPU_CONCEAL_COPY from such a source.
 * Afterwards the margins of dst are the replicated border of its final planes.  The side information of dst, its coverage and whether
 * it went through SAO stay as they are: a concealed CTU keeps part_size == HMGPU_SIZE_NONE in the side exports.  The launch is not
 * part of hmgpu_stats.
 *
 * The call is ordered on the context's stream: behind every earlier decompress / filter call, before every later one.  Masks are
 * copied before it returns.  Everything is validated before anything is enqueued and a refused call changes nothing; HMGPU_EINVAL
 * for: n outside 1 .. HMGPU_EXPORT_MAX_BATCH or jobs NULL; a dst that is no acquired picture; a src that is neither HMGPU_NO_PIC
 * nor one; dst == src; a dst that is the dst or src of another job of the call; a mode outside the enum; mask bits at or beyond
 * the number of CTUs set; fill[c] > 2^bit_depth_c - 1 (chroma of a 4:0:0 sequence is not looked at); a non-zero reserved word. */
enum { HMGPU_CONCEAL_COPY = 0, HMGPU_CONCEAL_MOTION = 1 };
typedef struct hmgpu_conceal_job {
  hmgpu_pic dst, src;          /* src: HMGPU_NO_PIC = fill */
  int32_t mode, dst_poc, src_poc;
  int32_t fill[3];
  const uint8_t* ctu_mask;     /* host; (num_ctus + 7) / 8 bytes; NULL = all CTUs */
  int32_t reserved[4];         /* 0 */
} hmgpu_conceal_job;
/* the validation alone: host code, nothing is enqueued */
hmgpu_status hmgpu_conceal_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_conceal_job jobs[]);
hmgpu_status hmgpu_pictures_conceal(hmgpu_ctx* ctx, int32_t n, const hmgpu_conceal_job jobs[]);
/* the CTUs of the picture concealed by hmgpu_pictures_conceal since hmgpu_picture_acquire handed it out (a CTU counts once) */
hmgpu_status hmgpu_picture_concealed_ctus(hmgpu_ctx* ctx, hmgpu_pic pic, int32_t* out);

/* ------------------------------------------------------------------------------------------------ motion and block export
 * The side information of finished pictures -- motion vectors, reference pictures, prediction mode, CU size, partitioning and QP --
 * written on the device straight into caller-owned device memory: up to HMGPU_EXPORT_MAX_BATCH pictures and one
 * kernel launch per call.  The source is what the decompress calls staged for the picture: HM's per-partition arrays
 * (hmgpu_ctu_meta) and the slice table.
 *
 * Source grid: the picture as W4 x H4 blocks of 4x4 luma samples, W4 = width / 4, H4 = height / 4 (exact: the SPS sizes are
 * multiples of the minimum CU size).  Block (bx, by) is partition z of CTU a: s = log2_ctu_size - 2, a = (by >> s) * ctus_w +
 * (bx >> s), z = the low s bits of bx on the even and of by on the odd bit positions (HM's z-scan, g_auiRasterToZscan).
 * Per block and list L (0, 1):
 *   used     part_size != HMGPU_SIZE_NONE, pred_mode == HMGPU_MODE_INTER, the slice of CTU a (slice_idx[a] -> slice table) is a P or
 *            B slice for list 0 / a B slice for list 1, and ref_idx[L] >= 0.  The slice-type term is part of the rule: the list-1
 *            arrays of a picture are not staged by calls without B slices and may hold an earlier picture's values;
 *            nothing the current picture did not supply is read.
 *   mv       the coded vector {hor, ver} in quarter luma samples as TComMv holds it, unclipped (reference sample = current +
 *            mv / 4); 0, 0 where the list is unused, whatever the array holds
 *   ref_poc  slice ref_poc[L][ref_idx[L]]; HMGPU_MOTION_NO_REF where the list is unused
 *   block    four int8 channels: 0 mode (-1 not decoded: part_size == HMGPU_SIZE_NONE; 0 inter; 1 intra; any other pred_mode: -1),
 *            1 log2 CU size (log2_ctu_size - depth), 2 part_size (-1 where not decoded), 3 QP
 * A picture has side information only when decompress calls have covered every one of its CTUs since it was acquired:
 * hmgpu_decompress_slice covers its CTU range, the picture, batch and packed entry points all CTUs; hmgpu_picture_acquire,
 * hmgpu_picture_upload and hmgpu_picture_commit_received (a transferred picture) clear the record.  A picture without full coverage
 * gives HMGPU_EINVAL.
 *
 * HMGPU_MOTION_BLOCKS: the grid itself, in integers.  desc->crop (left, right, top, bottom in luma samples, each a multiple of 4,
 * else HMGPU_EINVAL; 0,0,0,0 = the coded picture) selects w4 x h4 blocks; scale and windows must be NULL and sample_type
 * HMGPU_SAMPLE_UINT.  With L = the number of lists selected by desc->lists (bit 0: list 0, bit 1: list 1; selected lists in list order):
 *   dst_mv[0]   int16 [n][L][2][h4][w4]  (hor plane, then ver plane, per list);  dst_mv[1] must be NULL
 *   dst_ref     int32 [n][L][h4][w4]
 *   dst_block   int8  [n][4][h4][w4]
 * HMGPU_MOTION_DENSE: one value per output sample of hmgpu_pictures_export_windows with the same windows, output size and flips.
 * windows[i] (the rules of hmgpu_export_window: non-negative, non-empty, whole chroma samples of the sequence's format, flip bit 0
 * only, reserved 0; origins that are no multiple of 4 included) and either `scale` (width x height outputs; filter must be
 * HMGPU_SCALE_NEAREST, else HMGPU_EUNSUPPORTED) or no scale and windows of one size (the output's; else HMGPU_EINVAL); desc->crop
 * must be 0.  Limits per window and axis as for the scaled export: window <= 32 * output, output <= 8 * window, at most 16384
 * outputs per side (else HMGPU_EUNSUPPORTED).
 *   output sample (ox, oy) of slot i, window of win_w x win_h luma samples at (left, top), output W x H:
 *   sx = min(floor((2 * ox + 1) * win_w / (2 * W)), win_w - 1), sy alike (HMGPU_SCALE_NEAREST, in integers); block
 *   ((left + sx) >> 2, (top + sy) >> 2)
 *   dst_mv[l]   list l (selected by desc->lists, else must be NULL): sample_type F16 / BF16 / F32 (UINT: HMGPU_EINVAL) [n][2][H][W],
 *               channel 0 dx = convert(fmul((float)mv hor, kx)), channel 1 dy = convert(fmul((float)mv ver, ky)) in OUTPUT samples:
 *               kx = (float)((double)W / (4.0 * win_w)), ky = (float)((double)H / (4.0 * win_h)), derived per window on the host; one
 *               binary32 product, then the conversion of the batched tensor export (nearest even)
 *   dst_ref     int32 [n][L][H][W], dst_block int8 [n][4][H][W]: the block's values
 *   flip & 1    every output row reversed and dx negated -- the integer mv hor is negated before the product, which is exact and
 *               leaves a zero vector +0; ref_poc and block are reversed only
 * Destinations: slots 0 dst_mv[0], 1 dst_mv[1], 2 dst_ref, 3 dst_block index pitch_bytes (row to row), plane_stride_bytes (channel
 * to channel) and batch_stride_bytes (picture to picture), so a destination may be a strided view of a larger tensor.  Any
 * destination may be NULL (not written; its strides are ignored); at least one must be given.  Each must be aligned to its element,
 * as must its strides; pitch >= row_bytes, plane stride >= pitch * (height - 1) + row_bytes, batch stride >= plane stride *
 * (channels - 1) + that; and all n pictures of it must lie inside one allocation of the context's device.  Everything is validated
 * before anything is enqueued and a refused call leaves every destination untouched: an invalid handle anywhere in the list (a
 * handle may repeat), a picture without side information, n outside 1 .. HMGPU_EXPORT_MAX_BATCH, non-zero reserved words, a lists
 * mask outside 1 .. 3 and every destination rule give HMGPU_EINVAL.  Stream ordering is that of hmgpu_picture_export, once per call. */
enum { HMGPU_MOTION_BLOCKS = 0, HMGPU_MOTION_DENSE = 1 };
#define HMGPU_MOTION_NO_REF INT32_MIN
enum { HMGPU_MOTION_DST_MV0 = 0, HMGPU_MOTION_DST_MV1 = 1, HMGPU_MOTION_DST_REF = 2, HMGPU_MOTION_DST_BLOCK = 3, HMGPU_MOTION_DSTS = 4 };
typedef struct hmgpu_motion_desc {
  int32_t form;                /* HMGPU_MOTION_* */
  int32_t lists;               /* bit 0: list 0, bit 1: list 1 */
  int32_t sample_type;         /* DENSE: HMGPU_SAMPLE_F16 / BF16 / F32 of the vectors; BLOCKS: HMGPU_SAMPLE_UINT */
  int32_t crop[4];             /* BLOCKS: left, right, top, bottom in luma samples, multiples of 4; DENSE: 0 */
  int32_t reserved[5];         /* 0 */
} hmgpu_motion_desc;
typedef struct hmgpu_motion_plan {
  int32_t lists;               /* L: lists selected */
  int32_t channels[4];         /* per destination slot (HMGPU_MOTION_DST_*): planes per picture, 0 = the slot does not exist */
  int32_t width[4], height[4]; /* of every plane, in elements */
  int32_t elem_bytes[4];
  int32_t row_bytes[4];        /* width * elem_bytes: the least pitch */
  int32_t reserved[3];
} hmgpu_motion_plan;
/* validates a call's description and reports what it writes; host code, no device needed.  scale / windows: NULL for BLOCKS */
hmgpu_status hmgpu_motion_plan_for(const hmgpu_seq_params* seq, const hmgpu_motion_desc* desc, const hmgpu_export_scale* scale,
                                   int32_t n, const hmgpu_export_window windows[], hmgpu_motion_plan* out);
hmgpu_status hmgpu_pictures_export_motion(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_motion_desc* desc,
                                          const hmgpu_export_scale* scale, const hmgpu_export_window windows[], void* const dst_mv[2],
                                          void* dst_ref, void* dst_block, const int64_t pitch_bytes[4],
                                          const int64_t plane_stride_bytes[4], const int64_t batch_stride_bytes[4], int32_t on_stream,
                                          void* stream);
/* the validation hmgpu_pictures_export_motion makes of a description and a destination for n pictures, and nothing else: nothing is
 * enqueued and no picture is named (libhmdec: pictures in several contexts of a GPU) */
/* the other half of that validation: HMGPU_OK when pics[0 .. n) are all valid handles of pictures with side information, else
 * HMGPU_EINVAL; nothing is enqueued */
hmgpu_status hmgpu_pictures_motion_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[]);
hmgpu_status hmgpu_motion_destination_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_motion_desc* desc, const hmgpu_export_scale* scale,
                                            const hmgpu_export_window windows[], void* const dst_mv[2], void* dst_ref, void* dst_block,
                                            const int64_t pitch_bytes[4], const int64_t plane_stride_bytes[4],
                                            const int64_t batch_stride_bytes[4]);

/* ------------------------------------------------------------------------------------------------ residual export
 * The decoded residual of finished pictures -- what is added to the prediction -- written on the device straight into caller-owned
 * device memory: up to HMGPU_EXPORT_MAX_BATCH pictures and one kernel launch per call.  The source is what the
 * decompress calls left on the device for the picture: the residual of every coded transform unit, and HM's per-partition arrays.
 *
 * Value of a sample of component c: what HM adds to the prediction there, the int16 output of TComTrQuant::invRecurTransformNxN / xIT
 * for the transform block that covers it -- de-quantisation with scaling lists, inverse DCT / DST, transform skip, rotation, RDPCM,
 * and for cu_transquant_bypass CUs the level itself -- and exactly 0 wherever no coded transform block covers the sample.
 * Covered: the sample lies in a block whose cbf bits are set down to its transform unit's depth, (cbf & chain) == chain with
 * chain = (1 << (tr_idx + 1)) - 1, of a decoded partition (part_size != HMGPU_SIZE_NONE) with a transform size of 4 .. 32: the rule of
 * hmgpu_coeffs, the 4x4 chroma block under four 4x4 luma units (flagged at the first of them) included.  Codedness is taken from the
 * arrays cbf, tr_idx, depth, part_size, pred_mode and ipcm alone, never from what the device buffers hold.  Zero although flagged:
 *   PCM CUs (ipcm; their samples are not a residual);
 *   intra CUs of a picture decoded without intra_dir[] (the device leaves such CUs alone and computes nothing for them).
 * The flag group (transform_skip / transquant_bypass / ipcm) is read only for a picture it was staged for.  Intra CUs carry a
 * residual only when every decompress call that covers the picture came with intra_dir[]: a picture built with
 * hmgpu_decompress_slice whose calls disagree about intra_dir[] has the intra CUs of ALL its slices exported as 0 (a limitation:
 * the record is per picture, not per CTU).  Nothing an earlier picture of the handle left behind is returned.
 * Formats: 4:0:0 and 4:2:0 (8 .. 12 bits, CTUs of 16 / 32 / 64 samples).  4:2:2 and 4:4:4 give HMGPU_EUNSUPPORTED before anything is
 * enqueued: cross-component prediction rewrites their chroma residual in place, and a 4:2:2 chroma block is two squares.  For a 4:0:0
 * picture the chroma components do not exist: their bits in `components` are ignored and nothing is written for them (PLANES: dst[1] /
 * dst[2] are ignored; DENSE: their channels keep their place and are left untouched).
 * A picture has a residual under the rule of the motion export: decompress calls have covered every CTU since it was acquired (else
 * HMGPU_EINVAL); pictures decoded through the packed entry point qualify.
 *
 * HMGPU_RESIDUAL_PLANES: int16, each component at its own resolution.  desc->components (bit c: component c; at least one) selects;
 * desc->crop (left, right, top, bottom in luma samples, each a multiple of 8, else HMGPU_EINVAL; 0,0,0,0 = the coded picture) selects
 * w x h luma samples; scale and windows must be NULL, sample_type HMGPU_SAMPLE_UINT (the elements are SIGNED 16-bit integers).
 *   dst[0]  int16 [n][h][w];  dst[1], dst[2]  int16 [n][h / 2][w / 2]  (Cb, Cr); a dst of a component that is not selected must be NULL
 * HMGPU_RESIDUAL_DENSE: one value per output sample of hmgpu_pictures_export_windows with the same windows, output size and flips, by
 * the integer nearest rule of the dense motion export: output (ox, oy) of slot i takes luma position (left + sx, top + sy),
 * sx = min(floor((2 * ox + 1) * win_w / (2 * W)), win_w - 1), sy alike, and of a chroma component the sample ((left + sx) >> 1,
 * (top + sy) >> 1).  windows[i] as for the motion export; either `scale` (filter must be HMGPU_SCALE_NEAREST, else
 * HMGPU_EUNSUPPORTED) or windows of one size; desc->crop must be 0; the limits are those of the scaled export (HMGPU_EUNSUPPORTED).
 *   dst[0]  [n][C][H][W], C = the selected components in component order;  dst[1], dst[2] must be NULL
 *   sample_type HMGPU_SAMPLE_UINT: int16, the residual r itself.  F16 / BF16 / F32: convert(fmul((float)r, desc->scale[c])), one
 *   binary32 product, then the conversion of the batched tensor export (nearest even); every scale of a selected component finite
 *   flip & 1: every output row reversed; the values are unchanged
 * Destinations: pitch_bytes (row to row), plane_stride_bytes (DENSE: channel to channel; PLANES: ignored) and batch_stride_bytes
 * (picture to picture) per dst slot.  Any destination may be NULL (not written); at least one must be given.  Each must be aligned to
 * its element, as must its strides; pitch >= row_bytes, plane stride >= pitch * (height - 1) + row_bytes, batch stride >= plane stride *
 * (channels - 1) + that; and all n pictures of it must lie inside one allocation of the context's device.  Everything is validated
 * before anything is enqueued and a refused call leaves every destination untouched.  Stream ordering is that of
 * hmgpu_picture_export, once per call.  The launch is not accounted in hmgpu_stats. */
enum { HMGPU_RESIDUAL_PLANES = 0, HMGPU_RESIDUAL_DENSE = 1 };
typedef struct hmgpu_residual_desc {
  int32_t form;                /* HMGPU_RESIDUAL_* */
  int32_t components;          /* bit 0: Y, bit 1: Cb, bit 2: Cr */
  int32_t sample_type;         /* HMGPU_SAMPLE_UINT: int16; DENSE also HMGPU_SAMPLE_F16 / BF16 / F32 */
  int32_t crop[4];             /* PLANES: left, right, top, bottom in luma samples, multiples of 8; DENSE: 0 */
  float scale[3];              /* DENSE, float types: per component */
  int32_t reserved[6];         /* 0 */
} hmgpu_residual_desc;
typedef struct hmgpu_residual_plan {
  int32_t channels[3];         /* per destination slot: planes per picture, 0 = the slot does not exist (PLANES: 1 per selected component
                                  that the format has; DENSE: slot 0 holds C planes) */
  int32_t width[3], height[3]; /* of every plane, in elements */
  int32_t elem_bytes[3];
  int32_t row_bytes[3];        /* width * elem_bytes: the least pitch */
  int32_t reserved[1];
} hmgpu_residual_plan;
/* validates a call's description and reports what it writes; host code, no device needed.  scale / windows: NULL for PLANES */
hmgpu_status hmgpu_residual_plan_for(const hmgpu_seq_params* seq, const hmgpu_residual_desc* desc, const hmgpu_export_scale* scale,
                                     int32_t n, const hmgpu_export_window windows[], hmgpu_residual_plan* out);
hmgpu_status hmgpu_pictures_export_residual(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_residual_desc* desc,
                                            const hmgpu_export_scale* scale, const hmgpu_export_window windows[], void* const dst[3],
                                            const int64_t pitch_bytes[3], const int64_t plane_stride_bytes[3],
                                            const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream);
/* the two halves of that validation, nothing enqueued (libhmdec: pictures in several contexts of a GPU): HMGPU_OK when pics[0 .. n)
 * are all valid handles of pictures with a residual; the status hmgpu_pictures_export_residual would give a description and a
 * destination for n pictures */
hmgpu_status hmgpu_pictures_residual_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[]);
hmgpu_status hmgpu_residual_destination_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_residual_desc* desc, const hmgpu_export_scale* scale,
                                              const hmgpu_export_window windows[], void* const dst[3], const int64_t pitch_bytes[3],
                                              const int64_t plane_stride_bytes[3], const int64_t batch_stride_bytes[3]);

/* ------------------------------------------------------------------------------------------------ transform export
 * The frequency-domain side of finished pictures -- the quantised levels as parsed, or the de-quantised transform coefficients, and
 * the transform-unit structure needed to read them -- written on the device straight into caller-owned device memory (DESIGN.md
 * §9q): up to HMGPU_EXPORT_MAX_BATCH pictures and one kernel launch per call (k_transform.hip).  The source is what the decompress
 * calls staged for the picture and what lives as long as its handle: the levels (hmgpu_coeffs, dense or compact), HM's per-partition
 * arrays, the slice table and the picture's scaling-list matrices.  All four chroma formats (coefficients are taken before the
 * transform: cross-component prediction does not touch them), 8 .. 12 bits, CTUs of 16 / 32 / 64 samples.  There is no crop: the
 * planes are the coded picture, and a conformance crop is a tensor slice on the caller's side.
 *
 * Coefficient planes: dst[0] [n][H][W], dst[c] [n][H >> csy][W >> csx] for c = 1, 2 (csx / csy: the format's chroma subsampling).
 * For a 4:0:0 picture the chroma bits of `components` are ignored and nothing is written for them (dst[1] / dst[2] are ignored).
 * A block is coded by the rule of hmgpu_coeffs and hmgpu_pack_levels: the partition is decoded (part_size != HMGPU_SIZE_NONE), its
 * cbf bits are set down to the unit's transform depth, (cbf & chain) == chain with chain = (1 << (tr_idx + 1)) - 1, the transform size
 * is 4 .. 32; the 4x4 chroma block under four 4x4 luma units is flagged at the first of them; in 4:2:2 a chroma block is two squares,
 * the upper one first, each with its own flag one depth below (bit tr_idx + 1 at the first partition of the upper / lower half of the
 * block's partitions).  Element v * size + u of the level block of such a block of component c with top-left component sample
 * (x0, y0) goes to plane element (y0 + v, x0 + u).  Every element that no coded block covers is exactly 0, and so is every element
 * under a PCM CU (ipcm: PCM CUs carry cbf = 1 and their "levels" are not levels).  Nothing is rotated or accumulated: rotation and
 * RDPCM act after this stage.  Codedness comes from the arrays alone, never from what the level buffers hold.  The value, by
 * desc->value:
 *   HMGPU_TRANSFORM_LEVELS  the int16 level as the parser delivered it
 *   HMGPU_TRANSFORM_COEFFS  the output of TComTrQuant::xDeQuant for the block (TComTrQuant.cpp:1203-1311): QpParam from the QP at the
 *                           CU's first partition, the slice's Cb / Cr offsets and the chroma table of the picture's format; flat scaling,
 *                           or the picture's scaling-list matrix 3 * inter + component, which a transform-skip block takes only when it
 *                           is 4x4 (getUseScalingList); the level clip, the rounding shift or left shift and the clip to
 *                           [-32768, 32767] are xDeQuant's.  Transform-skip blocks get the same function: their values are scaled
 *                           spatial samples, which is why the info grid carries the flag.  cu_transquant_bypass blocks have no
 *                           de-quantisation in HM: the value is the level.
 *   sample_type HMGPU_SAMPLE_UINT: int16, the value v itself.  F16 / BF16 / F32 with either value: convert(fmul((float)v,
 *   desc->scale[c])), the rule and conversion of the dense residual form; every scale of a selected component finite.
 * Intra CUs are exported whether or not the picture was decoded with intra_dir[] -- the levels are staged either way and
 * de-quantisation needs only pred_mode; this differs from the residual export.  The flag group (transform_skip / transquant_bypass /
 * ipcm) is read only for a picture it was staged for.
 *
 * Info grid: dst_info int8 [n][HMGPU_TRANSFORM_INFO_CHANNELS][H / 4][W / 4], the motion export's grid of 4x4 luma blocks with the same
 * (bx, by) -> (CTU, z) map.  A block that is not decoded has -1 in all six channels; otherwise
 *   0  log2 of the luma transform size, log2_ctu_size - depth - tr_idx
 *   1  tr_idx
 *   2  bit c set iff the planes hold coefficients for the block of component c that covers this 4x4 luma block (the rule above, PCM
 *      excluded; 4:2:2: the square that covers it); chroma bits 0 in 4:0:0
 *   3  bits 0-2 transform_skip[c] & 1, read at the first partition of the covering block (4:2:0 / 4:2:2 chroma: of the 8x8 node under
 *      four 4x4 luma units; 4:2:2: of the covering square; chroma bits 0 in 4:0:0); bit 3 transquant_bypass; bit 4 ipcm; all 0 when the
 *      flag group was not staged for the picture
 *   4  intra_dir[0] for intra CUs of a picture all of whose decompress calls came with intra_dir[]; -1 otherwise
 *   5  intra_dir[1] as HM holds it (36 = derived from luma) under the same condition; -1 otherwise and in 4:0:0
 * Skip and merge flags are not part of hmgpu_ctu_meta: they stay with hmdec_internal_info.
 *
 * A picture qualifies under the coverage rule of the motion and residual exports (else HMGPU_EINVAL).  Destinations: slots 0 .. 2
 * the planes, 3 the info grid (HMGPU_TRANSFORM_DST_INFO) index pitch_bytes, plane_stride_bytes (info: channel to channel; ignored for
 * the planes) and batch_stride_bytes.  Any destination may be NULL (not written), at least one must be given, and the destination of
 * a component that is not selected must be NULL.  Each must be aligned to its element, as must its strides; pitch >= row_bytes, plane
 * stride >= pitch * (height - 1) + row_bytes, batch stride >= plane stride * (channels - 1) + that; all n pictures of it must lie
 * inside one allocation of the context's device.  Everything is validated before anything is enqueued, in the order of the residual
 * export, and a refused call leaves every destination untouched: n outside 1 .. HMGPU_EXPORT_MAX_BATCH, an unknown value, components
 * outside 1 .. 7, non-zero reserved words, a non-finite scale, an invalid handle, a picture without coverage and every destination rule
 * give HMGPU_EINVAL, an unknown sample_type HMGPU_EUNSUPPORTED.  Stream ordering is that of hmgpu_picture_export, once per call.  The
 * launch is not accounted in hmgpu_stats. */
enum { HMGPU_TRANSFORM_LEVELS = 0, HMGPU_TRANSFORM_COEFFS = 1 };
enum { HMGPU_TRANSFORM_DST_INFO = 3, HMGPU_TRANSFORM_DSTS = 4, HMGPU_TRANSFORM_INFO_CHANNELS = 6 };
typedef struct hmgpu_transform_desc {
  int32_t value;               /* HMGPU_TRANSFORM_* */
  int32_t components;          /* bit 0: Y, bit 1: Cb, bit 2: Cr */
  int32_t sample_type;         /* HMGPU_SAMPLE_UINT: int16; HMGPU_SAMPLE_F16 / BF16 / F32 */
  float scale[3];              /* float types: per component */
  int32_t reserved[6];         /* 0 */
} hmgpu_transform_desc;
typedef struct hmgpu_transform_plan {
  int32_t channels[4];         /* per destination slot (Y, Cb, Cr, info): planes per picture, 0 = the slot does not exist */
  int32_t width[4], height[4]; /* of every plane, in elements */
  int32_t elem_bytes[4];
  int32_t row_bytes[4];        /* width * elem_bytes: the least pitch */
  int32_t reserved[4];
} hmgpu_transform_plan;
/* validates a call's description and reports what it writes; host code, no device needed */
hmgpu_status hmgpu_transform_plan_for(const hmgpu_seq_params* seq, const hmgpu_transform_desc* desc, int32_t n, hmgpu_transform_plan* out);
hmgpu_status hmgpu_pictures_export_transform(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_transform_desc* desc,
                                             void* const dst[3], void* dst_info, const int64_t pitch_bytes[4],
                                             const int64_t plane_stride_bytes[4], const int64_t batch_stride_bytes[4], int32_t on_stream,
                                             void* stream);
/* the two halves of that validation, nothing enqueued (libhmdec: pictures in several contexts of a GPU): HMGPU_OK when pics[0 .. n)
 * are all valid handles of pictures that decompress calls have covered; the status hmgpu_pictures_export_transform would give a
 * description and a destination for n pictures */
hmgpu_status hmgpu_pictures_transform_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[]);
hmgpu_status hmgpu_transform_destination_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_transform_desc* desc, void* const dst[3],
                                               void* dst_info, const int64_t pitch_bytes[4], const int64_t plane_stride_bytes[4],
                                               const int64_t batch_stride_bytes[4]);

/* ------------------------------------------------------------------------------------------------ loop-filter export
 * What the decoder decided for the loop filters of finished pictures -- boundary strength, mean QP, tc and beta of every deblocking
 * edge unit, the exemptions of its two sides, and the reconstructed SAO parameters of every CTB -- written on the device straight
 * into caller-owned device memory: up to HMGPU_EXPORT_MAX_BATCH pictures and one kernel launch per call
 * (k_lfinfo.hip).  The source lives as long as the picture's handle: the edge-unit records the decompress calls derived for the
 * deblocking kernels, the slice table, and the SAO parameters the last filter call resolved.  All four chroma formats, 8 .. 12 bits,
 * CTUs of 16 / 32 / 64 samples.  The sample-dependent decisions (filter off / weak / strong, dE, dEp, dEq) are not exported: they
 * need the samples in front of deblocking, which a picture filtered in place no longer has.
 *
 * HMGPU_LOOPFILTER_GRIDS: two grids, each optional.
 * Edge grid: dst_edge int16 [n][HMGPU_LOOPFILTER_EDGE_CHANNELS][h4][w4] on the motion export's grid of 4x4 luma blocks; desc->crop
 * (left, right, top, bottom in luma samples, each a multiple of 8, else HMGPU_EINVAL; 0,0,0,0 = the coded picture) selects w4 x h4
 * blocks.  The VERTICAL unit of block (bx, by) is the 4-sample edge unit on its left border and exists where bx is even (x % 8 == 0),
 * its HORIZONTAL unit the one on its top border, where by is even; a block off the 8x8 grid in a direction holds 0 in every channel
 * of that direction.  Bs > 0 means the unit is filtered; Bs is 0 where there is no PU / TU edge, where deblocking is disabled for the
 * slice of the Q side (the block itself), where the P side (left / above) is not available across a slice or tile border, and where
 * xGetBoundaryStrengthSingle gives 0.  The slice constants of a unit are those of the CTU the Q side lies in.
 *   0, 1    BS_VER, BS_HOR        0 .. 2
 *   2, 3    QP_VER, QP_HOR        (QP_P + QP_Q + 1) >> 1 where Bs > 0, else 0
 *   4, 5    TC_VER, TC_HOR        luma tc: tcTable[clip(0, 53, qp + 2 * (Bs - 1) + 2 * tc_offset_div2)] << (bit_depth_luma - 8); 0 where Bs is 0
 *   6, 7    BETA_VER, BETA_HOR    betaTable[clip(0, 51, qp + 2 * beta_offset_div2)] << (bit_depth_luma - 8); 0 where Bs is 0
 *   8 .. 11 TC_CB_VER, TC_CB_HOR, TC_CR_VER, TC_CR_HOR: chroma tc (xEdgeFilterChroma): qPi = qp + pps_cb / cr_qp_offset through the
 *           chroma QP mapping of the format (the 4:2:0 table, min(qPi, 51) otherwise), tcTable[clip(0, 53, QpC + 2 + 2 * tc_offset_div2)]
 *           << (bit_depth_chroma - 8).  Non-zero only where the chroma filter acts: Bs is 2 and the unit lies on the 8-sample grid of
 *           the chroma plane (every 16 luma samples across a subsampled direction, every 8 otherwise); 0 everywhere in 4:0:0
 *   12      FLAGS  bit 0 / 1: the P / Q side of the vertical unit is exempt from the loop filters (lossless CU, PCM CU with
 *           pcm_loop_filter_disabled); bit 2 / 3: the same of the horizontal unit; 0 where Bs is 0
 * SAO grid: dst_sao int8 [n][3][HMGPU_LOOPFILTER_SAO_CHANNELS][ctus_h][ctus_w], per component and CTB, always the whole picture
 * (the crop does not apply).  The two leading dimensions are one run of 18 planes, plane_stride_bytes apart.
 *   0       TYPE   -1 off, else HMGPU_SAO_EO_0 .. HMGPU_SAO_BO (merge candidates resolved)
 *   1       BAND   BO: the first band; 0 otherwise
 *   2 .. 5  OFF0 .. OFF3: the offsets as applied (after << sao_offset_shift).  EO: categories 1, 2, 3, 4; BO: bands BAND + 0 .. 3; 0 when off
 * The chroma components of a 4:0:0 picture are left untouched.  A picture whose last filter call ran no SAO stage (sao_enabled 0, or
 * `stages` without bit 2) exports TYPE -1 and zeros: that is decided on the host, never from what the parameter buffer holds.
 *
 * HMGPU_LOOPFILTER_DENSE: dst_dense [n][3][H][W], one value per output sample of hmgpu_pictures_export_windows with the same windows,
 * output size and flips, by the integer nearest rule of the dense motion export (scale: filter HMGPU_SCALE_NEAREST, else
 * HMGPU_EUNSUPPORTED; or windows of one size; desc->crop 0).  For the source luma position (x, y) of an output sample:
 *   0  Bs of the vertical unit at column e = (x + 4) & ~7, row y >> 2 -- the edge whose filter can reach the sample (three samples
 *      modified and a fourth read on either side); 0 when e == 0 or e >= width
 *   1  the same with x and y exchanged
 *   2  TYPE + 1 of the luma SAO parameters of the sample's CTB (0 = off)
 * A mirrored slot has its positions reversed and its values unchanged.  sample_type HMGPU_SAMPLE_UINT: uint8, the value v itself;
 * F16 / BF16 / F32: convert(fmul((float)v, desc->scale[c])), the rule and conversion of the dense residual form; every scale finite.
 *
 * Which pictures qualify: the edge grid and dense channels 0 / 1 need the coverage rule of the motion export (decompress calls have
 * covered every CTU since the picture was acquired).  The SAO grid and the dense form need a filter call
 * (hmgpu_filter_pictures / hmgpu_filter_picture[_stages]) on the current occupant of the handle as well: acquire, upload, a received
 * picture and every later decompress call on the handle clear that record.  Else HMGPU_EINVAL, nothing written.
 * Destinations: slots 0 edge, 1 SAO, 2 dense index pitch_bytes, plane_stride_bytes and batch_stride_bytes.  A NULL destination is
 * not written, at least one must be given, and a destination of the other form must be NULL.  Alignment, stride and allocation rules,
 * the untouched destinations of a refused call and stream ordering are those of the motion export. */
enum { HMGPU_LOOPFILTER_GRIDS = 0, HMGPU_LOOPFILTER_DENSE = 1 };
enum { HMGPU_LOOPFILTER_DST_EDGE = 0, HMGPU_LOOPFILTER_DST_SAO = 1, HMGPU_LOOPFILTER_DST_DENSE = 2, HMGPU_LOOPFILTER_DSTS = 3 };
enum { HMGPU_LOOPFILTER_EDGE_CHANNELS = 13, HMGPU_LOOPFILTER_SAO_CHANNELS = 6 };
enum { HMGPU_LF_BS_VER = 0, HMGPU_LF_BS_HOR, HMGPU_LF_QP_VER, HMGPU_LF_QP_HOR, HMGPU_LF_TC_VER, HMGPU_LF_TC_HOR, HMGPU_LF_BETA_VER,
       HMGPU_LF_BETA_HOR, HMGPU_LF_TC_CB_VER, HMGPU_LF_TC_CB_HOR, HMGPU_LF_TC_CR_VER, HMGPU_LF_TC_CR_HOR, HMGPU_LF_FLAGS };
enum { HMGPU_LF_SAO_TYPE = 0, HMGPU_LF_SAO_BAND = 1, HMGPU_LF_SAO_OFF0 = 2 };
typedef struct hmgpu_loopfilter_desc {
  int32_t form;                /* HMGPU_LOOPFILTER_* */
  int32_t sample_type;         /* DENSE: HMGPU_SAMPLE_UINT (uint8) / F16 / BF16 / F32; GRIDS: HMGPU_SAMPLE_UINT */
  int32_t crop[4];             /* GRIDS: left, right, top, bottom in luma samples, multiples of 8 (edge grid); DENSE: 0 */
  float scale[3];              /* DENSE, float types: per channel */
  int32_t reserved[7];         /* 0 */
} hmgpu_loopfilter_desc;
typedef struct hmgpu_loopfilter_plan {
  int32_t channels[3];         /* per destination slot (HMGPU_LOOPFILTER_DST_*): planes per picture, 0 = the slot does not exist */
  int32_t width[3], height[3]; /* of every plane, in elements */
  int32_t elem_bytes[3];
  int32_t row_bytes[3];        /* width * elem_bytes: the least pitch */
  int32_t reserved[1];
} hmgpu_loopfilter_plan;
/* validates a call's description and reports what it writes; host code, no device needed.  scale / windows: NULL for GRIDS */
hmgpu_status hmgpu_loopfilter_plan_for(const hmgpu_seq_params* seq, const hmgpu_loopfilter_desc* desc, const hmgpu_export_scale* scale,
                                       int32_t n, const hmgpu_export_window windows[], hmgpu_loopfilter_plan* out);
hmgpu_status hmgpu_pictures_export_loopfilter(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_loopfilter_desc* desc,
                                              const hmgpu_export_scale* scale, const hmgpu_export_window windows[], void* const dst[3],
                                              const int64_t pitch_bytes[3], const int64_t plane_stride_bytes[3],
                                              const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream);
/* the two halves of that validation, nothing enqueued (libhmdec: pictures in several contexts of a GPU): HMGPU_OK when pics[0 .. n)
 * are all valid handles of covered pictures and, with need_filter != 0 (the SAO grid or the dense form is asked for), of pictures a
 * filter call has run on; the status hmgpu_pictures_export_loopfilter would give a description and a destination for n pictures */
hmgpu_status hmgpu_pictures_loopfilter_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], int32_t need_filter);
hmgpu_status hmgpu_loopfilter_destination_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_loopfilter_desc* desc, const hmgpu_export_scale* scale,
                                                const hmgpu_export_window windows[], void* const dst[3], const int64_t pitch_bytes[3],
                                                const int64_t plane_stride_bytes[3], const int64_t batch_stride_bytes[3]);

/* ------------------------------------------------------------------------------------------------ picture metrics
 * Finished pictures compared on the device, sample by sample, with other pictures of the context or with planes the caller holds in
 * device memory: up to HMGPU_EXPORT_MAX_BATCH pictures, one kernel launch per call (k_metrics.hip) behind one
 * hipMemsetAsync of the results, and one 64-byte record per picture and component.  Every field is an integer and exact: two calls on
 * the same inputs give the same bytes.
 *
 * a: the final sample of pics[i] -- the plane set the exports read -- inside desc->crop (left, right, top, bottom in luma samples,
 * whole chroma samples as in hmgpu_export_desc), each component at its own resolution, w_c x h_c.  All four chroma formats, 8 .. 12
 * bits.  b, by desc->reference:
 *   HMGPU_METRICS_REF_PICTURES  the same sample of ref_pics[i], a valid handle of the same context (it may be pics[i] itself); ref,
 *                               ref_pitch_bytes and ref_batch_stride_bytes must be NULL, desc->ref_bytes_per_sample 0
 *   HMGPU_METRICS_REF_PLANES    plane c of picture i at ref[c] + i * ref_batch_stride_bytes[c], rows ref_pitch_bytes[c] apart, elements
 *                               uint8 (ref_bytes_per_sample 1: only where the coding depth of every selected component is <= 8) or
 *                               uint16 (2), at the component's own resolution; row 0 / column 0 is the crop window's top-left sample.
 *                               ref[c] of every selected component the format has must be given, every other one NULL; ref_pics must
 *                               be NULL.  Alignment (to the element), strides and "all n planes inside one allocation of the context's
 *                               device" as for the destinations of the residual export.  The planes are only read.
 * desc->components (bit c: component c; at least one that the format has; the chroma bits of a 4:0:0 sequence are ignored).
 * results: device memory of the context's GPU, 8-byte aligned, record (i, c) at results + i * results_batch_stride_bytes + c * 64
 * (stride >= 192, a multiple of 8; all n * 3 records inside one allocation).  The record of a component that is not selected, or that
 * the format lacks, is written as all zero.  d = a - b:
 *   samples = w_c * h_c, sse = sum d^2, sad = sum |d|, differing = #(d != 0), max_abs = max |d|,
 *   first_diff = the least y * w_c + x with d != 0 in the cropped plane, UINT64_MAX if there is none.
 * SSIM (desc->ssim 1), the 8x8 / stride-4 integer form of x264 and FFmpeg's ssim filter: windows with their top-left at (4i, 4j) of the
 * cropped plane, 4i + 8 <= w_c, 4j + 8 <= h_c: ((w_c >> 2) - 1) * ((h_c >> 2) - 1) of them, none when a side is below 8.  Per window, in
 * 64-bit integers: s1 = sum a, s2 = sum b, ss = sum (a^2 + b^2), s12 = sum a b, vars = 64 ss - s1^2 - s2^2, covar = 64 s12 - s1 s2; with
 * maxv = 2^bd - 1 of the channel type, c1 = (int64)(.01 * .01 * maxv * maxv * 64 + .5), c2 = (int64)(.03 * .03 * maxv * maxv * 64 * 63 + .5);
 *   ssim = ((double)(2 s1 s2 + c1) * (double)(2 covar + c2)) / ((double)(s1^2 + s2^2 + c1) * (double)(vars + c2))      (binary64)
 * and the window adds llrint(ssim * 2^32) to ssim_q32 (identical planes: exactly ssim_windows << 32).
 * Everything is validated before anything is enqueued and a refused call leaves `results` untouched.  Stream ordering is that of
 * hmgpu_picture_export, once per call.  The launch is not accounted in hmgpu_stats. */
enum { HMGPU_METRICS_REF_PICTURES = 0, HMGPU_METRICS_REF_PLANES = 1 };
typedef struct hmgpu_metrics_desc {
  int32_t reference;           /* HMGPU_METRICS_REF_* */
  int32_t components;          /* bit c: component c; at least one */
  int32_t ssim;                /* 0: distortion only; 1: also SSIM */
  int32_t ref_bytes_per_sample; /* REF_PLANES: 1 (coding depth of that channel type <= 8) or 2 (uint16); REF_PICTURES: 0 */
  int32_t crop[4];             /* left, right, top, bottom in luma samples; must cover whole chroma samples, as in hmgpu_export_desc */
  int32_t reserved[7];         /* 0 */
} hmgpu_metrics_desc;
typedef struct hmgpu_metrics_result {   /* 64 bytes, one per picture and component */
  uint64_t samples;            /* w_c * h_c of the cropped component plane */
  uint64_t sse;                /* sum (a - b)^2 */
  uint64_t sad;                /* sum |a - b| */
  uint64_t differing;          /* samples with a != b */
  uint64_t first_diff;         /* least y * w_c + x with a != b inside the cropped plane; UINT64_MAX if none */
  int64_t  ssim_q32;           /* sum over windows of llrint(ssim * 2^32); 0 when desc->ssim == 0 */
  uint64_t ssim_windows;       /* windows summed; 0 when desc->ssim == 0 or the plane is smaller than 8x8 */
  uint32_t max_abs;            /* max |a - b| */
  uint32_t reserved;           /* 0 */
} hmgpu_metrics_result;
typedef struct hmgpu_metrics_plan {
  int32_t channels[3];         /* per component: 1 = compared (selected, and the format has it), 0 = its record is all zero */
  int32_t width[3], height[3]; /* w_c, h_c of the cropped component plane */
  int32_t elem_bytes[3];       /* REF_PLANES: desc->ref_bytes_per_sample; REF_PICTURES: 0 */
  int32_t row_bytes[3];        /* REF_PLANES: width * elem_bytes, the least reference pitch; REF_PICTURES: 0 */
  int32_t result_bytes;        /* per picture: 3 * sizeof(hmgpu_metrics_result), the least results_batch_stride_bytes */
  int64_t ssim_windows[3];     /* what the records will hold (0 when desc->ssim == 0) */
} hmgpu_metrics_plan;
/* validates a call's description and reports what it compares; host code, no device needed.  HMGPU_EUNSUPPORTED for a cropped component
 * plane of 2^32 - 1 samples or more */
hmgpu_status hmgpu_metrics_plan_for(const hmgpu_seq_params* seq, const hmgpu_metrics_desc* desc, hmgpu_metrics_plan* out);
/* HM's PSNR of a record (TEncGOP::xCalculateAddPSNR): maxval = 255 << (bit_depth - 8), 10 * log10(maxval^2 * samples / sse), 999.99
 * when sse == 0; host code.  NaN for a null record or a bit depth outside 8 .. 16 */
double hmgpu_metrics_psnr(const hmgpu_metrics_result* result, int32_t bit_depth);
hmgpu_status hmgpu_pictures_metrics(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_metrics_desc* desc,
                                    const hmgpu_pic ref_pics[], const void* const ref[3], const int64_t ref_pitch_bytes[3],
                                    const int64_t ref_batch_stride_bytes[3], void* results, int64_t results_batch_stride_bytes,
                                    int32_t on_stream, void* stream);
/* the validation of hmgpu_pictures_metrics alone, nothing enqueued: the status that call would give */
hmgpu_status hmgpu_metrics_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_metrics_desc* desc,
                                 const hmgpu_pic ref_pics[], const void* const ref[3], const int64_t ref_pitch_bytes[3],
                                 const int64_t ref_batch_stride_bytes[3], void* results, int64_t results_batch_stride_bytes);

/* ------------------------------------------------------------------------------------------------ picture metric maps
 * The sums of "picture metrics" kept per block instead of per picture: where two pictures differ, as device tensors
 * aligned with the picture.  Up to HMGPU_EXPORT_MAX_BATCH pictures, one kernel launch per call (k_metrics_map.hip), nothing zeroed and
 * no atomics: every map element is written exactly once, so two calls on the same inputs give the same bytes.
 *
 * desc is the hmgpu_metrics_desc of hmgpu_pictures_metrics with its meaning unchanged -- the reference as pictures or as uint8 / uint16
 * planes, components, ssim, crop -- and a, b, d = a - b, w_c, h_c are those of that section; its rules, and the order of the refusals
 * among its fields, are those of that call.  map->log2_block (3 .. 6, else HMGPU_EINVAL, as is a non-zero reserved word; both checked
 * after the refusals of desc) gives square blocks of B = 8, 16, 32 or 64 LUMA samples; the block of a chroma component is
 * bw_c x bh_c = (B >> csx) x (B >> csy) of its samples.
 * The block grid starts at the top-left sample of the cropped plane: blocks_x = ceil(W / B), blocks_y = ceil(H / B) with W x H the
 * cropped luma size, the same grid for all three components.  Block (bx, by) of component c covers its samples
 * [bx * bw_c, min((bx + 1) * bw_c, w_c)) x [by * bh_c, min((by + 1) * bh_c, h_c)): the blocks of the last column and row may be partial.
 * With no crop the grid is aligned with the CTUs and with the 4x4 grid of the motion export.
 * Fields (HMGPU_METRICS_MAP_*), int64 each:
 *   SSE, SAD, DIFFERING, MAX_ABS   sum d^2, sum |d|, #(d != 0), max |d| over the block's samples
 *   SSIM_Q32, SSIM_WINDOWS        the windows are the picture's own -- top-left at (4i, 4j) of the cropped component plane,
 *                                 4i + 8 <= w_c, 4j + 8 <= h_c -- each counted in the block that holds its top-left sample (it reads up to
 *                                 7 samples into the next block); the value of a window is the expression of "picture metrics", bit for
 *                                 bit.  Only with desc->ssim 1: without, a map has the first four fields.
 * Sum rule: for every picture and component the sum over the blocks of a field equals that field of hmgpu_metrics_result for the
 * same desc; for MAX_ABS it is the maximum.
 * Output: element (i, c, f, by, bx) at maps[c] + i * map_batch_stride_bytes[c] + f * map_field_stride_bytes[c] + by * map_pitch_bytes[c]
 * + bx * 8.  maps[c] must be given for every selected component the format has and be NULL for every other one (else HMGPU_EINVAL;
 * nothing is written for those).  Alignment 8 for the address and every stride; pitch >= row_bytes, field stride >= pitch *
 * (blocks_y - 1) + row_bytes, batch stride >= field stride * (fields - 1) + that; all n maps of a component inside one allocation of the
 * context's device.  Memory between rows, fields and pictures under padded strides is never touched.
 * Everything is validated before anything is enqueued and a refused call leaves the maps untouched.  Stream ordering is that of
 * hmgpu_pictures_metrics.  The launch is not accounted in hmgpu_stats. */
typedef struct hmgpu_metrics_map_desc {
  int32_t log2_block;          /* 3 .. 6: square blocks of 8, 16, 32, 64 LUMA samples; chroma blocks are (B >> csx) x (B >> csy) */
  int32_t reserved[7];         /* 0 */
} hmgpu_metrics_map_desc;
enum { HMGPU_METRICS_MAP_SSE = 0, HMGPU_METRICS_MAP_SAD, HMGPU_METRICS_MAP_DIFFERING, HMGPU_METRICS_MAP_MAX_ABS,
       HMGPU_METRICS_MAP_SSIM_Q32, HMGPU_METRICS_MAP_SSIM_WINDOWS, HMGPU_METRICS_MAP_FIELDS };   /* 6 */
typedef struct hmgpu_metrics_map_plan {
  int32_t blocks_x, blocks_y;  /* the map of every component */
  int32_t block_w[3], block_h[3]; /* bw_c, bh_c in samples of the component; 0 for a component that is not compared */
  int32_t width[3], height[3]; /* w_c, h_c of the cropped component plane */
  int32_t channels[3];         /* per component: 1 = compared (selected, and the format has it): maps[c] is written */
  int32_t fields;              /* 4 without SSIM, 6 with */
  int32_t row_bytes;           /* blocks_x * 8: the least pitch */
  int32_t reserved[5];         /* 0 */
} hmgpu_metrics_map_plan;
/* validates a call's description and reports what it writes; host code, no device needed */
hmgpu_status hmgpu_metrics_map_plan_for(const hmgpu_seq_params* seq, const hmgpu_metrics_desc* desc, const hmgpu_metrics_map_desc* map,
                                        hmgpu_metrics_map_plan* out);
hmgpu_status hmgpu_pictures_metrics_map(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_metrics_desc* desc,
                                        const hmgpu_metrics_map_desc* map, const hmgpu_pic ref_pics[], const void* const ref[3],
                                        const int64_t ref_pitch_bytes[3], const int64_t ref_batch_stride_bytes[3], void* const maps[3],
                                        const int64_t map_pitch_bytes[3], const int64_t map_field_stride_bytes[3],
                                        const int64_t map_batch_stride_bytes[3], int32_t on_stream, void* stream);
/* the validation of hmgpu_pictures_metrics_map alone, nothing enqueued: the status that call would give */
hmgpu_status hmgpu_metrics_map_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_metrics_desc* desc,
                                     const hmgpu_metrics_map_desc* map, const hmgpu_pic ref_pics[], const void* const ref[3],
                                     const int64_t ref_pitch_bytes[3], const int64_t ref_batch_stride_bytes[3], void* const maps[3],
                                     const int64_t map_pitch_bytes[3], const int64_t map_field_stride_bytes[3],
                                     const int64_t map_batch_stride_bytes[3]);

/* ------------------------------------------------------------------------------------------------ picture histograms
 * What finished pictures contain: per picture and channel a histogram of the sample values and one 64-byte record of
 * their moments and extrema.  Up to HMGPU_EXPORT_MAX_BATCH pictures, one kernel launch per call (k_histogram.hip) behind the memsets
 * that zero the destinations.  Everything is an integer sum, a minimum or a maximum: two calls on the same inputs give the same bytes.
 *
 * Channels (bit c of desc->channels):
 *   0 Y, 1 Cb, 2 Cr   the final samples of pics[i] -- the plane set the exports read -- inside desc->crop (left, right, top, bottom in
 *                     luma samples, whole chroma samples, as in hmgpu_metrics_desc), each component at its own resolution; the depth
 *                     D_c is the coding depth of its channel type
 *   3 maxRGB          one value per luma sample of the crop, max(R, G, B), where R, G, B are bit for bit what hmgpu_picture_export
 *                     writes for HMGPU_EXPORT_RGB with the same crop, matrix and full_range and bit_depth[0] = desc->rgb_bit_depth
 *                     (0: the luma coding depth; 8 .. 12, above 12 HMGPU_EUNSUPPORTED: the bins live in the LDS): chroma replicated,
 *                     no LUT, before any msb_aligned shift.  D_3 is that depth.  4:0:0 and matrix 0 as in the export (Cb = Cr = mid;
 *                     the identity is 4:4:4 only).  matrix and full_range are read only when bit 3 is set; a matrix the export does
 *                     not know is HMGPU_EUNSUPPORTED.
 * The chroma bits of a 4:0:0 sequence are ignored; at least one channel must remain.
 * Bins: desc->log2_bins 0: b_c = D_c, one bin per code value; 4 .. 12: b_c = min(log2_bins, D_c).  The bin of a value v is
 * v >> (D_c - b_c); counts are uint32.  The histogram of picture i, channel c is 2^b_c counts at hist[c] + i * hist_batch_stride_bytes[c]:
 * 4-byte aligned, the stride at least 4 << b_c and a multiple of 4, all n inside one allocation of the context's device; hist[c] is NULL
 * exactly for the channels that are not computed.  desc->histogram 0 is a records-only call: every hist[c] must be NULL (hist itself
 * and hist_batch_stride_bytes may then be NULL).
 * Records: hmgpu_histogram_result (i, c) at records + i * records_batch_stride_bytes + c * 64 (8-byte aligned, stride >= 256, a
 * multiple of 8, all n * 4 inside one allocation), always written, over the values v and not the bins -- exact when bins are reduced.
 * The record of a channel that is not computed is all zero.
 * Everything is validated before anything is enqueued and a refused call leaves hist and records untouched.  Stream ordering is that of
 * hmgpu_picture_export, once per call.  The launch is not accounted in hmgpu_stats. */
enum { HMGPU_HISTOGRAM_Y = 0, HMGPU_HISTOGRAM_CB = 1, HMGPU_HISTOGRAM_CR = 2, HMGPU_HISTOGRAM_MAXRGB = 3 };
typedef struct hmgpu_histogram_desc {
  int32_t channels;            /* bit c: channel c (HMGPU_HISTOGRAM_*); at least one */
  int32_t log2_bins;           /* 0: one bin per code value; 4 .. 12: at most 2^log2_bins bins per channel */
  int32_t histogram;           /* 1: histograms and records; 0: records only */
  int32_t rgb_bit_depth;       /* maxRGB: the depth of R, G, B, 8 .. 12; 0 = the luma coding depth */
  int32_t matrix, full_range;  /* maxRGB: as in hmgpu_export_desc; not read without bit 3 */
  int32_t crop[4];             /* left, right, top, bottom in luma samples; must cover whole chroma samples */
  int32_t reserved[6];         /* 0 */
} hmgpu_histogram_desc;
typedef struct hmgpu_histogram_result {   /* 64 bytes, one per picture and channel */
  uint64_t samples;            /* values counted: w_c * h_c */
  uint64_t sum;                /* sum v */
  uint64_t sum_sq;             /* sum v^2 */
  uint32_t min, max;           /* least and greatest v */
  uint32_t reserved[8];        /* 0 */
} hmgpu_histogram_result;
typedef struct hmgpu_histogram_plan {
  int32_t channels[4];         /* per channel: 1 = computed (selected, and the format has it), 0 = its record is all zero */
  int32_t width[4], height[4]; /* the cropped plane the channel counts (maxRGB: the luma one) */
  int32_t depth[4];            /* D_c */
  int32_t log2_bins[4];        /* b_c */
  int32_t hist_bytes[4];       /* 4 << b_c, the least hist_batch_stride_bytes; 0 when desc->histogram == 0 */
  int32_t record_bytes;        /* per picture: 4 * sizeof(hmgpu_histogram_result), the least records_batch_stride_bytes */
  int32_t coef[16];            /* maxRGB: hmgpu_export_plan.coef of the equivalent RGB descriptor; else 0 */
  int32_t reserved[3];         /* 0 */
} hmgpu_histogram_plan;
/* validates a call's description and reports what it counts; host code, no device needed.  HMGPU_EUNSUPPORTED for a cropped luma plane
 * of 2^31 samples or more (every count and the int32 views of them stay below 2^31) */
hmgpu_status hmgpu_histogram_plan_for(const hmgpu_seq_params* seq, const hmgpu_histogram_desc* desc, hmgpu_histogram_plan* out);
hmgpu_status hmgpu_pictures_histogram(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_histogram_desc* desc,
                                      void* const hist[4], const int64_t hist_batch_stride_bytes[4], void* records,
                                      int64_t records_batch_stride_bytes, int32_t on_stream, void* stream);
/* the validation of hmgpu_pictures_histogram alone, nothing enqueued: the status that call would give */
hmgpu_status hmgpu_histogram_check(hmgpu_ctx* ctx, int32_t n, const hmgpu_pic pics[], const hmgpu_histogram_desc* desc,
                                   void* const hist[4], const int64_t hist_batch_stride_bytes[4], void* records,
                                   int64_t records_batch_stride_bytes);

/* ------------------------------------------------------------------------------------------------ call 1
 * Replaces the reconstruction half of TDecGop::decompressSlice -> TDecSlice::decompressSlice ->
 * TDecCu::decompressCU (TDecSlice.cpp:334, TDecCu.cpp:142,373) for the CTUs [first_ctu, first_ctu+num_ctus) of
 * slice `slice_idx` of picture `cur`: motion compensation of every inter PU (TComPrediction::motionCompensation),
 * de-quantisation + inverse transform of every coded TU (TComTrQuant::invRecurTransformNxN) and
 * recon = ClipBD(pred + resid) into the picture (TComYuv::addClip, TDecCu::xCopyToPic).
 * Intra CUs (TDecCu::xReconIntraQT) are reconstructed too, in decoding order, when meta->intra_dir[] is supplied; without
 * the modes they are left untouched.  hmgpu_get_stats counts both kinds of partitions.
 * The metadata/coefficients are copied to the device before the call returns to the caller's thread?  No:
 * they are staged with hipMemcpyAsync from the caller's (ideally pinned) buffers, which must stay valid until
 * hmgpu_sync() or until a later call on the same context returns HMGPU_OK after a sync. */
hmgpu_status hmgpu_decompress_slice(hmgpu_ctx* ctx, hmgpu_pic cur, int32_t slice_idx, const hmgpu_slice_params* slice,
                                    const hmgpu_ctu_meta* meta, const hmgpu_coeffs* coeffs,
                                    int32_t first_ctu, int32_t num_ctus);

/* The same for a whole picture at once: every slice's constants first, then all CTUs in one batch of launches (meta->slice_idx
 * says which slice a CTU belongs to; required when num_slices > 1).  For callers that hold a complete parsed picture -- a decoder
 * that parses ahead of reconstruction, as libhmdec does -- and for pictures whose slices are not contiguous CTU ranges in raster
 * order (slices and tiles combined).  Equivalent to the hmgpu_decompress_slice calls of all slices. */
hmgpu_status hmgpu_decompress_picture(hmgpu_ctx* ctx, hmgpu_pic cur, int32_t num_slices, const hmgpu_slice_params* const* slices,
                                      const hmgpu_ctu_meta* meta, const hmgpu_coeffs* coeffs);

/* ------------------------------------------------------------------------------------------------ several pictures per call
 * TDecGop::decompressSlice / filterPicture (TDecGop.cpp:105,157) are called once per picture; a caller that holds several parsed
 * pictures which do not reference each other -- the B pictures of one temporal level, the pictures of independent streams -- hands
 * them over together: the inputs of all of them are staged on a copy stream of their own (so they travel while the kernels of the
 * previous call still run) and every kernel is launched ONCE for the whole set (n <= 16).  Equivalent to hmgpu_decompress_picture /
 * hmgpu_filter_picture per picture.  The copies are asynchronous: the input arrays must stay untouched until hmgpu_staging_wait()
 * (arrays of a staging block) or hmgpu_sync() (any arrays) has returned -- a later call that names the same picture only orders the
 * DEVICE side behind the earlier copy, it does not wait for it on the host. */
typedef struct hmgpu_picture_job {
  hmgpu_pic pic;
  int32_t num_slices;
  const hmgpu_slice_params* const* slices;
  const hmgpu_ctu_meta* meta;
  const hmgpu_coeffs* coeffs;
} hmgpu_picture_job;
typedef struct hmgpu_filter_job {
  hmgpu_pic pic;
  const hmgpu_pic_params* pp;
  const hmgpu_sao_param* sao;      /* [num_ctus][3], or NULL when pp->sao_enabled == 0 */
} hmgpu_filter_job;
hmgpu_status hmgpu_decompress_pictures(hmgpu_ctx* ctx, int32_t n, const hmgpu_picture_job* jobs);
hmgpu_status hmgpu_filter_pictures(hmgpu_ctx* ctx, int32_t n, const hmgpu_filter_job* jobs);

/* Staging blocks: ONE page-locked allocation that holds all input arrays of a picture (TComDataCU's arrays, TComDataCU.h:86-157, and
 * the levels m_pcTrCoeff*) in the order the device keeps them.  hmgpu_staging_alloc fills *meta and *coeffs with pointers into the
 * block -- a parser writes HM's arrays there directly, part_size pre-set to HMGPU_SIZE_NONE, ref_idx to -1, everything else to 0 --
 * and a whole-picture call that is handed exactly these structs moves the metadata in one DMA and the levels in another instead of
 * one copy per array.  PCM samples are not part of the block (coeffs->pcm_sample stays the caller's). */
typedef struct hmgpu_staging hmgpu_staging;
hmgpu_status hmgpu_staging_alloc(hmgpu_ctx* ctx, hmgpu_staging** out, hmgpu_ctu_meta* meta, hmgpu_coeffs* coeffs);
void         hmgpu_staging_free(hmgpu_ctx* ctx, hmgpu_staging* staging);
/* blocks until the copies of the last hmgpu_decompress_pictures call that read the block have been made: from then on a parser may
 * write the next picture into it (the kernels read the device copies).  A block no call has read yet returns at once. */
hmgpu_status hmgpu_staging_wait(hmgpu_ctx* ctx, hmgpu_staging* staging);
/* A caller that drives several contexts (one per GPU, pictures of one temporal level placed on different ones: hmgpu_picture_transfer)
 * parses into ONE set of blocks and decides late where a picture is decoded: after hmgpu_staging_share, `other` -- a context with equal
 * hmgpu_seq_params on any device -- takes the block's arrays in the same few DMAs as `owner`, which still owns and frees the block. */
hmgpu_status hmgpu_staging_share(hmgpu_ctx* owner, hmgpu_staging* staging, hmgpu_ctx* other);
/* (the block also holds the three ctu_level_start arrays: coeffs->ctu_level_start[] of hmgpu_staging_alloc points at them; a caller
 * that fills the block with HM's dense layout sets the three pointers to NULL in the struct it passes to the calls) */

/* HM's dense level arrays -> the compact form (host, no device involved): out_level[c] needs room for the dense size in the worst
 * case, out_start[c] for num_ctus + 1 entries.  The walk over depth / tr_idx / cbf is the one the device's flattener does. */
hmgpu_status hmgpu_pack_levels(const hmgpu_seq_params* seq, const hmgpu_ctu_meta* meta, const hmgpu_coeffs* dense,
                               int16_t* const out_level[3], uint32_t* const out_start[3]);

/* ------------------------------------------------------------------------------------------------ packed input
 * A picture's inputs in few bytes: per-partition arrays hold values that are constant over a CU, PU or TU (every CU and TU covers a
 * contiguous range of HM's z-scan), and most levels are zero.  The packed form stores the metadata as runs and the levels sparsely, in
 * ONE contiguous, self-describing blob; hmgpu_decompress_pictures_packed copies the blob in one DMA and expands it on the device into
 * exactly the arrays and compact levels the other entry points stage -- everything downstream is the same.  A P picture of 2160p moves
 * about 5.6 MB instead of 19 MB (DESIGN.md "Packed input").
 *
 * Envelope: whole pictures, chroma_format 0 (4:0:0) or 1 (4:2:0); other formats give HMGPU_EUNSUPPORTED.  PCM samples stay in the
 * caller's arrays (hmgpu_packed_job.pcm_sample), as with staging blocks.  Cross-component prediction weights are not carried (4:4:4).
 *
 * Layout (little endian, every section 16-byte aligned, the blob itself at least 4-byte aligned):
 *   header: uint32 magic 0x4B504D48 ("HMPK"), version 1, num_ctus, parts_per_ctu, groups (bit g: run group g is present; 0-2 always),
 *           bytes (of the whole blob), 2 reserved; then {offset, size} in bytes of 19 sections; padded to 192 bytes
 *   section 0: [num_ctus] uint32  slice_idx | tile_idx << 16
 *   sections 1 + 3g, 2 + 3g, 3 + 3g, for the run groups g = 0 CU (depth, part_size, pred_mode, qp, transquant_bypass, ipcm, 0, 0),
 *           1 TU (tr_idx, cbf[0..2], transform_skip[0..2], 0), 2 list 0 (mv[0] hor, ver as int16, ref_idx[0], 0, 0, 0), 3 list 1 (the same),
 *           4 intra (intra_dir[0], intra_dir[1], 0 x 6): [num_ctus + 1] uint32 run starts (CTU a has runs start[a] .. start[a+1] - 1, at
 *           least one), [runs] uint16 run ends (the z-index one past the run's last partition: strictly ascending inside a CTU, the last
 *           one = parts_per_ctu), [runs] 8-byte tuples as listed.  A group left out has three empty sections: list 1 then reads as
 *           mv 0 / ref_idx -1 everywhere (a picture without B slices), the intra modes as absent (intra CUs are left untouched, as when
 *           meta->intra_dir is NULL).
 *   section 16: [3][num_ctus + 1] uint32  the compact form's CTU starts (hmgpu_coeffs.ctu_level_start), per component
 *   section 17: [num_ctus][3] {uint32 offset in 4-byte units into section 18, uint32 mode}: mode 0x80000000 = the CTU's piece of the
 *           component is stored raw (its int16 levels, padded to 4 bytes), else mode = the number of pairs: that many uint16 positions in
 *           the piece (strictly ascending, padded to 4 bytes) followed by as many int16 values (padded); all other levels are zero
 *   section 18: the pieces
 * hmgpu_pack_input writes the smaller of the two forms of every piece and zeroes all padding: the blob depends on the input alone, and
 * dense and compact levels give the same bytes. */
typedef struct hmgpu_packed_job {
  hmgpu_pic pic;
  int32_t num_slices;
  const hmgpu_slice_params* const* slices;
  const void* blob;                 /* page-locked (hmgpu_host_alloc) for a true asynchronous copy */
  size_t bytes;
  const int16_t* pcm_sample[3];     /* as hmgpu_coeffs.pcm_sample: needed only if the picture has PCM CUs */
} hmgpu_packed_job;

/* where hmgpu_unpack_input writes HM's arrays: the fields of hmgpu_ctu_meta (same order, same layout), writable; NULL = not wanted */
typedef struct hmgpu_ctu_meta_out {
  uint8_t* depth; int8_t* part_size; int8_t* pred_mode; int8_t* qp; uint8_t* tr_idx;
  uint8_t* cbf[3]; uint8_t* transform_skip[3];
  int16_t* mv[2]; int8_t* ref_idx[2];
  uint8_t* intra_dir[2];
  uint8_t* transquant_bypass; uint8_t* ipcm;
  uint16_t* slice_idx; uint16_t* tile_idx;
  int8_t* ccp_alpha[2];             /* (not carried by the packed form: left untouched) */
} hmgpu_ctu_meta_out;

/* worst-case blob size for the geometry of `seq` (a different tuple in every partition, every level non-zero); 0 for bad parameters */
size_t       hmgpu_packed_max_bytes(const hmgpu_seq_params* seq);
/* HM's arrays (levels dense, or compact with ctu_level_start) -> the blob at `out` (capacity bytes, 4-byte aligned); *bytes = its size */
hmgpu_status hmgpu_pack_input(const hmgpu_seq_params* seq, const hmgpu_ctu_meta* meta, const hmgpu_coeffs* coeffs, void* out, size_t capacity,
                              size_t* bytes);
/* host reference expansion and validator: checks the whole blob (HMGPU_EINVAL if anything is out of place) and writes every non-NULL
 * array of *meta ([num_ctus][parts] as in hmgpu_ctu_meta; meta may be NULL) and the compact levels / CTU starts (out_level / out_start
 * may be NULL, or hold NULL entries; out_level[c] needs out_start[c][num_ctus] elements) */
hmgpu_status hmgpu_unpack_input(const hmgpu_seq_params* seq, const void* blob, size_t bytes, const hmgpu_ctu_meta_out* meta,
                                int16_t* const out_level[3], uint32_t* const out_start[3]);
/* hmgpu_decompress_pictures with packed inputs (n <= 16): every blob is validated in full before anything is enqueued -- the checks of
 * hmgpu_unpack_input, the blobs of a call on threads of their own; a malformed one gives HMGPU_EINVAL -- then copied in one DMA on the
 * copy stream and expanded by one kernel launch for the whole call.  The blob must stay untouched until hmgpu_packed_wait(ctx, blob) or
 * hmgpu_sync() has returned. */
hmgpu_status hmgpu_decompress_pictures_packed(hmgpu_ctx* ctx, int32_t n, const hmgpu_packed_job* jobs);
/* blocks until the copy of the last hmgpu_decompress_pictures_packed call that read `blob` has been made (at once for a blob no call has read) */
hmgpu_status hmgpu_packed_wait(hmgpu_ctx* ctx, const void* blob);

/* ------------------------------------------------------------------------------------------------ call 2
 * Replaces TDecGop::filterPicture (TDecGop.cpp:157-217): TComLoopFilter::loopFilterPic (all vertical edges, then
 * all horizontal edges), then reconstructBlkSAOParams + SAOProcess.  Uses the metadata of every CTU handed to
 * hmgpu_decompress_slice for this picture (HM: pcPic->getCU(addr), TComLoopFilter.cpp:133-135).
 * `sao` is [num_ctus][3] or NULL when pp->sao_enabled == 0. */
hmgpu_status hmgpu_filter_picture(hmgpu_ctx* ctx, hmgpu_pic cur, const hmgpu_pic_params* pp, const hmgpu_sao_param* sao);

/* ------------------------------------------------------------------------------------------------ finer seams
 * The kernel-level seams HM exposes to its own callers (SURVEY.md 8b "finer seams"), used by the parity tests.
 * All operate on host arrays (copied in and out synchronously). */

/* TComTrQuant::xDeQuant (flat) + xIT/xITransformSkip on `n` TUs of size (1<<log2_size)^2.
 * levels/resid: [n][size*size].  per TU: qp_per/qp_rem from QpParam, flags bit0 = 4x4 DST (intra luma), bit1 = transform skip.
 * bit_depth selects transformShift and the second-stage shift (TComTrQuant.cpp:898-899,1233-1236). */
hmgpu_status hmgpu_inverse_transform_batch(hmgpu_ctx* ctx, int32_t log2_size, int32_t bit_depth, int32_t n,
                                           const int16_t* levels, const int8_t* qp_per, const int8_t* qp_rem,
                                           const uint8_t* flags, int16_t* resid);

/* TComPrediction::xPredInterBlk (TComPrediction.cpp:660) for `n` blocks out of one reference plane.
 * blocks: n x {x, y, w, h, mvx, mvy} in samples of that plane / in 1/4 (luma) or 1/8 (chroma) sample units;
 * dst: concatenated w*h outputs.  bi != 0 -> 14-bit intermediate (no clip), else final clipped prediction. */
hmgpu_status hmgpu_mc_batch(hmgpu_ctx* ctx, int32_t is_chroma, int32_t bit_depth, const int16_t* ref_plane, int32_t ref_stride,
                            int32_t ref_w, int32_t ref_h, int32_t n, const int32_t* blocks, int32_t bi, int16_t* dst);

/* stage control for tests: run only part of hmgpu_filter_picture on `cur`:  1 = vertical edges, 2 = horizontal edges,
 * 4 = SAO; combine with |.  hmgpu_filter_picture == stages 7. */
hmgpu_status hmgpu_filter_picture_stages(hmgpu_ctx* ctx, hmgpu_pic cur, const hmgpu_pic_params* pp, const hmgpu_sao_param* sao,
                                         int32_t stages);

/* ------------------------------------------------------------------------------------------------ measurement
 * Resident replay: re-run the device work of the last hmgpu_decompress_slice calls / hmgpu_filter_picture of `cur`
 * from the inputs already staged in HBM (no host->device traffic, no host work), `iters` times.  This is what
 * bench.py times ("inputs already resident in HBM").  Kernel times are measured with hipEvents on the
 * context's own stream. */
hmgpu_status hmgpu_replay(hmgpu_ctx* ctx, hmgpu_pic cur, int32_t stages /* 8 = reconstruct | 1|2|4 filter */, int32_t iters);
/* the same for `n` mutually independent pictures at once (<= 16): every kernel is launched once for the whole batch
 * (one grid z-slice per picture) -- the frame-parallel mode used for throughput measurements */
hmgpu_status hmgpu_replay_batch(hmgpu_ctx* ctx, const hmgpu_pic* pics, int32_t n, int32_t stages, int32_t iters);

/* Lanes of hmgpu_replay_batch: 1 (default) = one stream, kernel after kernel; 2 = the batch is cut in two halves that run on two
 * streams, so that kernels of different kinds overlap (more pictures per second, per-kernel times no longer separable; profiling
 * forces one lane). */
hmgpu_status hmgpu_set_streams(hmgpu_ctx* ctx, int32_t n);

#define HMGPU_NUM_KERNELS 13
typedef struct hmgpu_stats {
  double   kernel_ms[HMGPU_NUM_KERNELS];      /* accumulated device time per kernel class since the last reset ("mc_cells": the launches of
                                               * the cells kernels, whose time "mc_luma" / "mc_chroma" include as well) */
  uint64_t kernel_launches[HMGPU_NUM_KERNELS];
  uint64_t intra_partitions;                  /* 4x4 partitions of intra CUs seen */
  uint64_t inter_partitions;
  uint64_t coded_tus[4][3];                   /* TUs with cbf by log2 size-2 and component */
} hmgpu_stats;
const char*  hmgpu_kernel_name(int32_t k);
hmgpu_status hmgpu_set_profiling(hmgpu_ctx* ctx, int32_t enable);   /* per-kernel hipEvent timing on/off (off by default) */
hmgpu_status hmgpu_get_stats(hmgpu_ctx* ctx, hmgpu_stats* out, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* HMGPU_H */
