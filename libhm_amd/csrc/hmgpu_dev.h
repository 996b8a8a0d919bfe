// hmgpu_dev.h -- device-side data model shared by the HIP kernels and the host runtime of libhmgpu.so.
//
// Design: the host hands over HM's per-CTU TComDataCU arrays untouched (z-scan SoA).  A
// "prep" kernel turns them, one thread per 4x4 partition, into
//   * a picture-wide raster grid of 16-byte BlkInfo records (motion, QP, intra/cbf flags, deblocking edge
//     flags) that the motion-compensation, deblocking and SAO kernels index by sample position, and
//   * per-size lists of coded transform units (TuRec) appended with wave-aggregated atomics.
// No quadtree is ever walked serially; every kernel is a flat grid over partitions, tiles, TUs or edges.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/hmgpu.h"

namespace hmgpu {

constexpr int kMaxBatch = 16;       // pictures per batched launch (blockIdx.z)
constexpr int kMaxPics = 64;        // device pictures per context
constexpr int kTuShards = 8;        // TU lists are sharded by (prep block index % 8) so that list appends do not pile on one word
// Chroma planes (round 4): Cb and Cr of a picture live in ONE plane, sample by sample -- Cb(x, y) at element y * pitch + 2 * x, Cr(x, y) one
// element on -- so that a window row of both components is one piece of one 128-byte line for motion compensation instead of a piece
// in each of two lines, and a row of reconstructed chroma leaves a wave as whole lines (measured on k_mc_chroma, timing only: 0.132 ->
// 0.107 ms per 16 pictures).  PicDev::rec[2] = rec[1] + 1, pitch[1] = pitch[2] = the pitch of the pair plane in int16 elements: sample
// (x, y) of component c > 0 is rec[c][y * pitch[c] + kCStep * x] everywhere.  The C ABI keeps HM's three planes (upload / download /
// packing / hashing take the components apart).
constexpr int kCStep = 2;

// ---- per-4x4-block record (raster grid over the CTU-padded picture) -------------------------------------------
struct __attribute__((aligned(16))) BlkInfo {
  int16_t mv[2][2];   // HM TComMv per list {hor, ver} in quarter luma samples, UNclipped (deblocking compares these); 0 if unused
  int8_t  ref[2];     // device picture handle per list (slice ref_pic[list][ref_idx]); -1 = list unused
  int8_t  qp;         // TComDataCU::getQP(partition)
  uint8_t flags;      // BF_*
  uint8_t edge;       // BE_*
  uint8_t log2cu;     // log2 CU size (3..6): clipMv needs the CU origin
  uint16_t slice;     // index into the picture's slice table
};
static_assert(sizeof(BlkInfo) == 16, "BlkInfo must be 16 bytes");

enum : uint8_t {
  BF_VALID = 1,    // partition decoded (part_size != NUMBER_OF_PART_SIZES) and inside the picture
  BF_INTRA = 2,
  BF_CBFY = 4,     // luma cbf at the partition's transform depth (Bs = 1 rule)
  BF_MC_L0 = 8,    // prediction uses list 0  (after the identical-motion collapse of xCheckIdenticalMotion)
  BF_MC_L1 = 16,   // prediction uses list 1
  BF_NOFILT = 32,  // lossless CU, or PCM CU with pcm_loop_filter_disabled: deblocking and SAO leave its samples alone
};
enum : uint8_t {
  BE_VER_FILTER = 1,     // left edge of this block is a deblocking edge (m_aapbEdgeFilter[EDGE_VER]) on the 8x8 grid
  BE_VER_TRANSFORM = 2,  // ... and it is a TU/CU edge (the m_aapucBS marker xGetBoundaryStrengthSingle reads)
  BE_HOR_FILTER = 4,
  BE_HOR_TRANSFORM = 8,
};

// ---- deblocking decisions of one 8x8 luma area (raster grid, grid_w/2 x grid_h/2), written by k_prep for the loop-filter kernels ----
// The four 4-sample edge units on the area's left border (v[k]: rows 4k .. 4k+3) and top border (h[k]: columns 4k .. 4k+3), 2 bytes
// each: what xGetBoundaryStrengthSingle, xEdgeFilterLuma and xEdgeFilterChroma take from the two blocks that face each other
// across the unit (TComLoopFilter.cpp:411-537, 587-600, 629-634) -- SURVEY.md a-12.  The slice constants of a unit are those of the
// CTU its Q side lies in (slices are whole CTUs).
//   bits 0-1  Bs; 0 = the unit is not filtered (no edge, deblocking disabled, unavailable neighbour or Bs 0)
//   bits 2-8  ((QP_P + QP_Q + 1) >> 1) + 32
//   bit 9/10  the P / Q side is exempt from the loop filters (lossless CU, PCM CU with pcm_loop_filter_disabled)
struct __attribute__((aligned(8))) EdgeRec { uint16_t v[2], h[2]; };
static_assert(sizeof(EdgeRec) == 8, "EdgeRec must be 8 bytes");
__host__ __device__ constexpr uint32_t edge_unit_pack(int bs, int qp, bool p_nf, bool q_nf) {
  return (uint32_t)bs | ((uint32_t)(qp + 32) << 2) | ((p_nf ? 1u : 0u) << 9) | ((q_nf ? 1u : 0u) << 10);
}

// ---- motion of one 8x8 luma tile (raster grid, grid_w/2 x grid_h/2), written by k_prep for the motion-compensation kernels --
// A tile is ACTIVE when its four 4x4 cells are inter-predicted with identical motion (k_mc.hip predicts those); slot 0 is
// the first list the tile predicts from, slot 1 is list 1 of a bi-predicted tile.  The vectors are CLIPPED (TComDataCU::clipMv)
// and split into integer luma samples and the quarter-sample fraction; unused fields are 0, so that two tiles continue each
// other vertically iff their first 12 bytes are equal.
struct __attribute__((aligned(16))) TileMv {
  int16_t ix0, iy0, ix1, iy1;   // integer parts of the clipped motion vectors of slot 0 / slot 1 (luma samples)
  uint8_t frac;                 // xf0 | yf0 << 2 | xf1 << 4 | yf1 << 6 (quarter samples)
  uint8_t ref0, ref1;           // device picture handles of slot 0 / slot 1
  uint8_t flags;                // TM_*
  uint8_t ridx;                 // reference indices of slot 0 | slot 1 << 4 (explicit weighted prediction)
  uint8_t rmask;                // TR_*: which parts of the tile carry a residual (written for every tile, active or not)
  uint16_t slice;               // index into the picture's slice table
};
static_assert(sizeof(TileMv) == 16, "TileMv must be 16 bytes");
enum : uint8_t { TM_ACTIVE = 1, TM_BI = 2, TM_FIRST_L1 = 4 };
__host__ __device__ constexpr int resid_slot(int row) { return ((row & 1) << 2) | ((row & 7) >> 1); }   // 16-byte slot of row `row` in its tile
// residual mask of an 8x8 luma tile: bits 0-3 its four 4x4 luma quadrants (raster order), bit 4 / 5 the 4x4 Cb / Cr block under it
enum : uint8_t { TR_LUMA = 15, TR_CB = 16, TR_CR = 32 };

// ---- coded transform unit ---------------------------------------------------------------------------------------
struct TuRec {
  uint16_t x4, y4;        // origin in 4-luma-sample units (picture coordinates)
  uint8_t  comp_flags;    // bits 0-1 component, bit 2 DST (4x4 intra luma), bit 3 transform skip, bit 4 cu_transquant_bypass, bits 5-6 RDPCM
                          // (1 horizontal, 2 vertical: explicit for inter blocks, implied by the prediction mode for intra ones), bit 7 intra CU
  int8_t   per, rem;      // QpParam per / rem
  uint8_t  xflags;        // bit 0: the 4x4 block is read back to front (transform_skip_rotation, intra)
  uint32_t coef_off;      // element offset into the component's coefficient array
};
static_assert(sizeof(TuRec) == 12, "TuRec must be 12 bytes");

// ---- slice constants on the device --------------------------------------------------------------------------------
struct SliceDev {
  int32_t slice_type;
  int32_t cb_qp_offset, cr_qp_offset;
  int32_t pps_cb_qp_offset, pps_cr_qp_offset;
  int32_t deblocking_disable, beta_offset_div2, tc_offset_div2, lf_across_slices;
  int32_t ref_poc[2][HMGPU_MAX_REF];
  int8_t  ref_pic[2][HMGPU_MAX_REF];
  int32_t constrained_intra_pred;
  int32_t weighted_pred;                // explicit weighted prediction active (TComSlice::applyWP)
  int32_t wp_log2_denom[2];
  int16_t wp_weight[2][HMGPU_MAX_REF][3];
  int16_t wp_offset[2][HMGPU_MAX_REF][3];
};

struct SaoDev {                 // reconstructed SAO parameters of one CTU component, 12 bytes
  int8_t  type;                 // -1 off, else HMGPU_SAO_EO_0..BO
  uint8_t band;                 // BO: first band
  uint16_t avail;               // 3x3 grid around the CTU, bit 3 * v + h (v: 0 above, 1 same row, 2 below; h: 0 left, 1 same
                                // column, 2 right): that CTU may be read by SAO (bit 4, the CTU itself, is always set)
  int8_t  off[8];               // EO: [0..4] by edge class (class 2 == 0); BO: [0..3] = offsets of bands band+0..3 (mod 32)
};
static_assert(sizeof(SaoDev) == 12, "SaoDev layout");

struct PlaneSet { int16_t* p[3]; };

// ---- everything the kernels need to know about one picture; one slot per device picture, resident in HBM ----------
struct PicDev {
  int32_t width, height;           // luma samples
  int32_t bd[3];                   // bit depth per component
  int32_t log2ctu, ctus_w, ctus_h, num_ctus, parts, pw;   // pw = partitions per CTU row
  int32_t pitch[3];                // int16 elements per row; chroma: of the plane that holds both components (kCStep)
  int32_t mx[3], my[3];            // margins (samples / rows) around every plane, border-extended like TComPicYuv::extendPicBorder
  int32_t grid_w, grid_h;          // BlkInfo grid (CTU padded)
  int32_t lf_across_tiles;
  int32_t sao_applied;             // final planes are sao[] (else rec[])
  int16_t* rec[3];                 // reconstruction / deblocked in place ([2] = [1] + 1: Cb and Cr alternate in one plane)
  int16_t* sao[3];                 // SAO output
  // raw HM arrays (device copies, whole picture)
  const uint8_t* depth; const int8_t* part_size; const int8_t* pred_mode; const int8_t* qp; const uint8_t* tr_idx;
  const uint8_t* cbf[3]; const uint8_t* tskip[3];
  const int16_t* mv[2]; const int8_t* ref_idx[2];
  const uint8_t* intra_dir[2];     // m_puhIntraDir[luma, chroma]
  const uint8_t* bypass; const uint8_t* ipcm;   // m_CUTransquantBypass, m_pbIPCMFlag
  const int16_t* pcm[3];           // PCM sample buffers (allocated on first use), layout of coef[]
  int32_t pcm_shift[3];            // bit depth - PCM bit depth per component
  int32_t pcm_lf_disable;          // SPS pcm_loop_filter_disabled_flag (with PCM enabled)
  int32_t any_nofilt;              // some partition of the picture carries BF_NOFILT (host-side scan): SAO looks at the flags
  const uint16_t* slice_idx; const uint16_t* tile_idx;
  const int16_t* coef[3];
  // residual of the inter TUs, written by k_itx and added by the motion-compensation kernels: per component 8x8-sample tiles of 128
  // bytes (8 rows x 16 bytes), tile (tx, ty) at index ty * (padded component width / 8) + tx; inside a tile the even rows come first
  // (resid_slot): a motion-compensation lane owns rows 2q, 2q+1, so each of its two loads reads 64 consecutive bytes per tile
  int16_t* resid[3];
  const uint32_t* coef_start[3];   // compact levels: element offset of every CTU's first coded TU (+ total), else null (HM's dense layout)
  const SliceDev* slices;
  // derived
  BlkInfo* blk;                    // written only for calls that run kernels which read it (mixed-motion tiles, exempt CUs): launch_prep
  EdgeRec* edges;                  // [grid_h / 2][grid_w / 2]
  TileMv* tmv;                     // [grid_h / 2][grid_w / 2]
  TuRec* tu[4];                    // by log2 size - 2: kTuShards shards of tu_cap[] records each
  uint32_t* tu_count;              // [4][kTuShards]: the lists' lengths, published by the last workgroup of k_prep
  uint32_t* tu_work;               // [4][kTuShards] + 1: the lengths while k_prep appends, and its arrival ticket; zero between launches
  uint32_t tu_cap[4];              // capacity of ONE shard
  SaoDev* saoprm;                  // [num_ctus][3]
  unsigned long long* stats;       // [2][kTuShards]: intra / inter partitions seen by the prep kernel
  // scaling lists: one byte per position, [size 4x4..32x32][list = 3 * inter + component][1024], or null (flat)
  const uint8_t* sl_m;
  // intra reconstruction (k_intra.hip)
  int32_t has_intra_dir;           // the caller supplied intra prediction modes (else intra CUs are left untouched)
  int32_t strong_intra_smoothing;  // SPS flag
  int32_t range_ext;               // HMGPU_REXT_* (sps_range_extension tools of the residual path)
  int32_t mono;                    // chroma_format_idc 0: no chroma blocks are coded, the chroma planes are never read back
  int32_t fmt, csx, csy;           // chroma_format_idc (0 kept as 1) and the chroma subsampling it implies (getComponentScaleX / Y, TComChromaFormat.h:59-62);
                                   // 4:2:2 / 4:4:4 pictures take their chroma through the format-generic kernels of k_cfmt.hip
  const int8_t* ccp[2];            // cross-component prediction weights per partition (Cb, Cr), or null
  uint8_t* ctu_intra;              // [num_ctus] number of the CTU's 8x8 areas that belong to intra CUs, 0 = none (written by k_prep)
  uint32_t* intra_done;            // [3][num_ctus]: the CTU's intra CUs of that component are reconstructed
  uint32_t* fault;                 // set by a kernel that gave up waiting (k_intra's bounded spin): checked by the host at hmgpu_sync
  int32_t debug_skip_ctu;          // test hook (hmgpu_debug_stall_intra): the intra workgroups of this CTU leave without reconstructing or publishing (-1: none)
};

// batched launch descriptor, passed by value
struct Batch {
  int32_t n;
  int32_t pic[kMaxBatch];          // index into the PicDev table
  int32_t first_ctu[kMaxBatch];
  int32_t num_ctus[kMaxBatch];
};

// everything the motion-compensation kernels need about a batch, in kernel-argument memory: nothing stands between a workgroup's
// start and the load of its tile records (k_mc.hip).  Filled by the host from its mirrors of the PicDev descriptors.
struct McArgs {
  int32_t n, mode, log2n, pad0_;               // pictures of the batch; grid mapping (launch_mc)
  int32_t width, height, log2ctu, ctus_w;      // geometry (the same for every picture of a context)
  int32_t tw, pitch, bd, npics;                // TileMv grid width; pitch / bit depth of the component; entries of finals[]
  int32_t first_ctu[kMaxBatch], num_ctus[kMaxBatch];   // the call's CTU range per picture (what launch_mc reads)
  // per blockIdx.x, precomputed by launch_mc: the raster range of CTUs that index walks (first CTU, count) and the CTU row it starts in
  int32_t walk_lo[kMaxBatch], walk_n[kMaxBatch], walk_row[kMaxBatch];
  const TileMv* tmv[kMaxBatch];
  int16_t* dst[kMaxBatch];                     // luma: the picture's reconstruction plane; chroma: Cb
  int16_t* dst2[kMaxBatch];                    // chroma: Cr
  const int16_t* resid[kMaxBatch];             // residual tiles of the component (luma / Cb), PicDev::resid
  const int16_t* resid2[kMaxBatch];            // chroma: Cr
  int32_t rtw, pad_;                           // residual tiles per tile row of the component
  const SliceDev* slices[kMaxBatch];           // slice tables (explicit weighted prediction)
  // final planes: every picture of a context lives in one slab, picture i at slab + i * pic_stride; its final luma plane (sample
  // (0,0)) is at + origin_off, or + sao_off + origin_off when bit i of the SAO mask is set (the picture went through SAO)
  const char* slab;
  uint64_t pic_stride, slab_bytes;
  uint32_t sao_off, origin_off, cr_off;        // origin_off: luma launch: Y plane; chroma launch: Cb plane; cr_off: Cb -> Cr
  uint32_t sao_mask_lo, sao_mask_hi;
};

// the same for the residual kernel (k_itx.hip)
struct ItxArgs {
  int32_t n; uint32_t class_mask;              // pictures of the batch; size classes to run (bit = log2 size - 2)
  int32_t blocks[4];                           // workgroups per shard and size class (launch_itx)
  int32_t rtw[3], bd[3];                       // residual tiles per tile row; bit depths
  int32_t csx, csy;                            // chroma subsampling (a TU record carries its LUMA position)
  uint32_t tu_cap[4];                          // capacity of one shard's list
  const TuRec* tu[kMaxBatch][4];
  const uint32_t* tu_count[kMaxBatch];         // [4][kTuShards]
  const int16_t* coef[kMaxBatch][3];
  int16_t* resid[kMaxBatch][3];
  const uint8_t* sl_m[kMaxBatch];
};

// Pointers stored inside PicDev / PlaneSet reach the kernels through memory, so the compiler only knows them as generic
// ("flat") pointers: flat loads cannot be counted separately from LDS traffic and force a full s_waitcnt after every
// batch.  Every hot pointer is therefore re-typed as a global-address-space pointer before use.
#define HMGPU_AS1 __attribute__((address_space(1)))
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x4 u32x4_a8 __attribute__((aligned(8)));
template <typename T> __device__ inline T ldg(const T* p) { return *(const T HMGPU_AS1*)p; }          // scalar types
template <typename T> __device__ inline void stg(T* p, T v) { *(T HMGPU_AS1*)p = v; }
__device__ inline u32x4 ldg4(const void* p) { return *(const u32x4 HMGPU_AS1*)p; }
__device__ inline u32x4 ldg4_a8(const void* p) { return *(const u32x4_a8 HMGPU_AS1*)p; }
__device__ inline u32x2 ldg2(const void* p) { return *(const u32x2 HMGPU_AS1*)p; }
__device__ inline void stg4(void* p, u32x4 v) { *(u32x4 HMGPU_AS1*)p = v; }
__device__ inline void stg4_a8(void* p, u32x4 v) { *(u32x4_a8 HMGPU_AS1*)p = v; }
__device__ inline void stg2(void* p, u32x2 v) { *(u32x2 HMGPU_AS1*)p = v; }

// ---- small device helpers ------------------------------------------------------------------------------------------
__host__ __device__ inline int zscan_x(int z) {   // HM g_auiZscanToRaster column: even bits of z
  int x = z & 0x5555; x = (x | (x >> 1)) & 0x3333; x = (x | (x >> 2)) & 0x0f0f; x = (x | (x >> 4)) & 0x00ff; return x;
}
__host__ __device__ inline int zscan_y(int z) { return zscan_x(z >> 1); }
// ... and its inverse: the low four bits of v on the even bit positions (HM's z-scan: column bits even, row bits odd)
__device__ inline int spread4(int v) { v = (v | (v << 2)) & 0x33; v = (v | (v << 1)) & 0x55; return v; }
// the 4x4 luma block (bx, by) in HM's per-partition arrays (CTU raster, z-scan inside a CTU): element (size_t)ctu * parts + z
struct Part { int ctu, z; };
__device__ inline Part part_of(int bx, int by, int log2ctu, int ctus_w) {
  const int sh = log2ctu - 2, m = (1 << sh) - 1;
  return {(by >> sh) * ctus_w + (bx >> sh), spread4(bx & m) | (spread4(by & m) << 1)};
}
// nearest-exact in integers, `in` samples to `out`: min(floor((2 o + 1) * in / (2 * out)), in - 1); (2 o + 1) * in < 2^32 for o < 16384 and in < 2^17
__device__ inline int nearest_src(int o, int in, int out) { return min((int)(((2u * o + 1u) * (uint32_t)in) / (2u * (uint32_t)out)), in - 1); }
// is the transform block at transform depth tr coded, of a partition whose cbf byte is `cbf`?  cbf bit d of a partition = cbf of its
// ancestor TU node at transform depth d (TComDataCU.h:310); HM descends only while every node on the way has its bit set
// (TComTrQuant.cpp:1558-1564).  The one rule under k_prep's TU lists, hmgpu_pack_levels and the residual and transform exports.
__host__ __device__ inline bool cbf_coded(uint32_t cbf, int tr) { const uint32_t chain = (1u << (tr + 1)) - 1u; return (cbf & chain) == chain; }
__device__ inline int clip3(int lo, int hi, int v) { return min(hi, max(lo, v)); }
__device__ inline BlkInfo ld_blk(const BlkInfo* p) { return __builtin_bit_cast(BlkInfo, ldg4(p)); }

// XCD-aware work distribution (speed only, never correctness): workgroups are dealt round-robin to the 8 XCDs, each
// with its own L2.  For a batch of n pictures with nb workgroups each, picture p is served by the XCDs x with
// x % n == p and each of those XCDs walks one contiguous band of the picture in raster order, so that neighbouring
// tiles (which share reference-picture rows) hit in the same L2.  Returns false for padding workgroups.
// (The motion-compensation launches keep this assignment but walk an XCD's range in bands of CTU columns: launch_mc, k_mc.hip.  The
// same order inside this function's range was measured on k_filter_fused, whose halo is 5 % of its reads, and did not pay:
// EXPERIMENTS.md round 8.)
__device__ inline bool xcd_remap(int bid, int n, int nb, int& slot, int& lb) {
  if (n < 0) { n = -n; slot = bid % n; lb = bid / n; return lb < nb; }     // tuning knob: plain interleave
  if (n <= 8 && (8 % n) == 0) {
    const int m = 8 / n;                       // XCDs per picture
    const int per = (nb + m - 1) / m;          // workgroups per band
    const int x = bid & 7, t = bid >> 3;
    slot = x % n;
    const int r = x / n;
    lb = r * per + t;
    return t < per && lb < nb;
  }
  slot = bid % n; lb = bid / n;
  return lb < nb;
}
__host__ inline int xcd_grid(int n, int nb) {
  if (n <= 8 && (8 % n) == 0) { const int m = 8 / n; return 8 * ((nb + m - 1) / m); }
  return n * nb;
}

// ---- launchers (one per kernel family; defined in the .hip files) ---------------------------------------------------
// packed picture input (k_unpack.hip): the device copy of every picture's blob, validated on the host
struct UnpackArgs {
  int32_t n;
  int32_t pic[kMaxBatch];
  const char* blob[kMaxBatch];
};
void launch_unpack_input(const PicDev* pics, const UnpackArgs& ua, int num_ctus, hipStream_t s);
// bi: the batch holds B slices (else list 1 is not read)
void launch_prep(const PicDev* pics, const Batch& b, int max_ctus, int parts, bool intra, bool bi, bool write_blk, int fmt, hipStream_t s);
// npics = entries of the finals table (device pictures of the context, <= kMaxPics)
// bi: the batch holds B slices (the variants that run the H and V passes once per list)
void launch_mc_luma(McArgs& a, int max_ctus, bool wp, bool bi, hipStream_t s);
void launch_mc_chroma(McArgs& a, int max_ctus, bool wp, bool bi, hipStream_t s);
// the 4x4 cells of tiles with mixed motion (8x4 / 4x8 PUs, AMP in 16x16 CUs): only for calls that contain such PUs
void launch_mc_luma_cells(const PicDev* pics, const PlaneSet* finals, const Batch& b, int max_ctus, int log2ctu, bool wp, hipStream_t s);
void launch_mc_chroma_cells(const PicDev* pics, const PlaneSet* finals, const Batch& b, int max_ctus, int log2ctu, bool wp, hipStream_t s);
void launch_itx(ItxArgs& a, uint32_t blocks_per_shard, hipStream_t s);
void launch_filter_fused(const PicDev* pics, const Batch& b, int width, int height, bool nofilt, hipStream_t s);
// step: distance of two samples of the plane in memory (1 luma, kCStep chroma)
void launch_pack(const int16_t* src, int pitch, int step, int x0, int y0, int w, int h, int bytes, uint8_t* dst, int dst_stride, hipStream_t s);
void launch_unpack(const int16_t* src, int w, int h, int16_t* dst, int pitch, int step, hipStream_t s);
void launch_checksum(const int16_t* src, int pitch, int step, int w, int h, int bd, uint32_t* out, hipStream_t s);
// MD5 chains, one per lane (k_out.hip): message, length, where the four state words a, b, c, d go
struct Md5Batch { int32_t n, pad_; const uint8_t* msg[128]; unsigned long long bytes[128]; uint32_t* out[128]; };
void launch_md5(const Md5Batch& job, hipStream_t s);
void launch_crc(const int16_t* src, int pitch, int step, int w, int h, int bd, uint32_t* rows, uint32_t* out, hipStream_t s);
void launch_intra(const PicDev* pics, const Batch& b, const int32_t* order, int num_ctus, bool lean, hipStream_t s);   // lean: no I slices in the call
// device export of finished pictures (k_export.hip, hmgpu_picture_export / hmgpu_pictures_export): everything by value, validated on
// the host.  A call converts n pictures (grid z); picture i writes plane k at dst[k] + i * bstride[k].
constexpr int kMaxExportBatch = 16;
// output element of an export kernel instance: 1- or 2-byte unsigned (container shift msb), or a float type that takes
// convert(v * scale[k] + bias[k]) of the integer v (two binary32 roundings, then round to nearest even)
enum { kElemU8 = 0, kElemU16 = 1, kElemF16 = 2, kElemBF16 = 3, kElemF32 = 4 };
template <int ELEM> constexpr int elem_bytes() { return ELEM == kElemU8 ? 1 : ELEM == kElemF32 ? 4 : 2; }
// one element from the integer v.  Float elements: the product and the sum are rounded separately (no contraction into an fma),
// overflow gives infinity, denormals stay.
template <int ELEM>
__device__ inline uint32_t export_conv(uint32_t v, int msb, float sc, float bi) {
  if constexpr (ELEM <= kElemU16) {
    return v << msb;
  } else {
#pragma clang fp contract(off)
    const float m = (float)(int)v * sc;
    const float f = m + bi;
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    if constexpr (ELEM == kElemF32) return u;
    else if constexpr (ELEM == kElemF16) return __builtin_bit_cast(uint16_t, (_Float16)f);
    else return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;      // bfloat16, nearest even (f is never a NaN: v, sc and bi are finite)
  }
}
// n (<= 4) consecutive elements of one plane from the integers v (export_conv); full groups of an aligned export as one 4-, 8- or
// 16-byte store.
template <int ELEM>
__device__ inline void export_store4(uint8_t* d, const uint32_t v[4], int n, bool vec, int msb, float sc, float bi) {
  uint32_t o[4];
  for (int i = 0; i < 4; i++) o[i] = export_conv<ELEM>(v[i], msb, sc, bi);
  constexpr int B = elem_bytes<ELEM>();
  if (vec && n == 4) {
    if constexpr (B == 1) stg(reinterpret_cast<uint32_t*>(d), o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24);
    else if constexpr (B == 2) { u32x2 w; w.x = o[0] | o[1] << 16; w.y = o[2] | o[3] << 16; stg2(d, w); }
    else { u32x4 w; w.x = o[0]; w.y = o[1]; w.z = o[2]; w.w = o[3]; stg4(d, w); }
    return;
  }
  for (int i = 0; i < n; i++) {
    if constexpr (B == 1) stg(d + i, (uint8_t)o[i]);
    else if constexpr (B == 2) stg(reinterpret_cast<uint16_t*>(d) + i, (uint16_t)o[i]);
    else stg(reinterpret_cast<uint32_t*>(d) + i, o[i]);
  }
}
// export_store4 of the group of n (<= 4) samples at column x of a row of w samples.  flip: the row is mirrored, so the group goes
// out reversed at columns w - x - n .. (the last, partial group of a row lands at the row's start); either way one vector store
// where the group's position is aligned, else sample by sample.
template <int ELEM>
__device__ inline void export_store_row(uint8_t* row, int x, int w, const uint32_t v[4], int n, bool vec, bool flip, int msb, float sc, float bi) {
  uint32_t r[4];
  for (int i = 0; i < 4; i++) r[i] = flip ? v[3 - i] : v[i];
  if (flip && n < 4) {                                         // a partial group: its samples are the last n of r
    if (n == 3) { r[0] = r[1]; r[1] = r[2]; r[2] = r[3]; }
    else if (n == 2) { r[0] = r[2]; r[1] = r[3]; }
    else r[0] = r[3];
  }
  const int xs = flip ? w - x - n : x;
  export_store4<ELEM>(row + (ptrdiff_t)xs * elem_bytes<ELEM>(), r, n, vec && !(xs & 3), msb, sc, bi);
}
// the same for n (<= 4) CbCr pairs o[2j], o[2j + 1] at pair x of a semi-planar row of cw pairs (integer elements): mirrored pair
// by pair, Cb stays first
template <int ELEM>
__device__ inline void export_store_pairs(uint8_t* row, int x, int cw, const uint32_t o[8], int n, bool vec, bool flip, int msb) {
  uint32_t r[8];
  for (int j = 0; j < 4; j++) { r[2 * j] = flip ? o[6 - 2 * j] : o[2 * j]; r[2 * j + 1] = flip ? o[7 - 2 * j] : o[2 * j + 1]; }
  if (flip && n < 4) {
    if (n == 3) { r[0] = r[2]; r[1] = r[3]; r[2] = r[4]; r[3] = r[5]; r[4] = r[6]; r[5] = r[7]; }
    else if (n == 2) { r[0] = r[4]; r[1] = r[5]; r[2] = r[6]; r[3] = r[7]; }
    else { r[0] = r[6]; r[1] = r[7]; }
  }
  const int xs = flip ? cw - x - n : x;
  const bool vv = vec && !(xs & 1);
  uint8_t* d = row + (ptrdiff_t)xs * 2 * elem_bytes<ELEM>();
  export_store4<ELEM>(d, r, min(4, 2 * n), vv, msb, 0.f, 0.f);
  if (n > 2) export_store4<ELEM>(d + 4 * elem_bytes<ELEM>(), r + 4, 2 * n - 4, vv, msb, 0.f, 0.f);
}
// packed pixels (k_export.hip, k_export_scale.hip, k_export_warp.hip; include/hmgpu.h "packed pixel export"): the channel order as two launch-uniform
// flags, the A element's bits, and whether dst, the pitch and the batch stride are multiples of 4 bytes (dword stores possible)
struct PxOrder {
  int32_t swap;                    // B first, R third (BGR, BGRA, ABGR)
  int32_t afirst;                  // 4 channels: A before the colours (ARGB, ABGR)
  uint32_t abits;                  // 4 channels: the A element as stored (host: the container shift, or the float conversion)
  uint32_t vst;
};
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));
typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
// the group of n (<= 4) pixels at column x of a packed row of w pixels, NCH (3, 4) elements each, from the integers R, G, B of the
// group (export_conv per colour: scale / bias belong to the colour, not to the position).  flip: the row is mirrored pixel by pixel
// (export_store_row's rule, the channels of a pixel in place).  A full group whose first byte is dword aligned (vst: dst, pitch and
// batch stride are) goes out as 4 * NCH * element bytes of dword stores, 12 .. 64 contiguous bytes; any other element by element.
// Never writes beyond pixel w - 1.
template <int ELEM, int NCH>
__device__ inline void export_store_px(uint8_t* row, int x, int w, const uint32_t R[4], const uint32_t G[4], const uint32_t B[4], int n,
                                       bool vst, bool flip, int mrb, int mg, const float sc[3], const float bi[3], const PxOrder& po) {
  constexpr int EB = elem_bytes<ELEM>();
  uint32_t e[4][NCH];
  for (int i = 0; i < 4; i++) {
    const uint32_t r = export_conv<ELEM>(flip ? R[3 - i] : R[i], mrb, sc[0], bi[0]);
    const uint32_t g = export_conv<ELEM>(flip ? G[3 - i] : G[i], mg, sc[1], bi[1]);
    const uint32_t b = export_conv<ELEM>(flip ? B[3 - i] : B[i], mrb, sc[2], bi[2]);
    const uint32_t c0 = po.swap ? b : r, c2 = po.swap ? r : b;
    if constexpr (NCH == 3) {
      e[i][0] = c0; e[i][1] = g; e[i][2] = c2;
    } else {
      e[i][0] = po.afirst ? po.abits : c0; e[i][1] = po.afirst ? c0 : g;
      e[i][2] = po.afirst ? g : c2; e[i][NCH - 1] = po.afirst ? c2 : po.abits;
    }
  }
  if (flip && n < 4) {                                         // a partial group: its pixels are the last n of e
    for (int c = 0; c < NCH; c++) {
      if (n == 3) { e[0][c] = e[1][c]; e[1][c] = e[2][c]; e[2][c] = e[3][c]; }
      else if (n == 2) { e[0][c] = e[2][c]; e[1][c] = e[3][c]; }
      else e[0][c] = e[3][c];
    }
  }
  const int xs = flip ? w - x - n : x;
  const ptrdiff_t off = (ptrdiff_t)xs * (NCH * EB);
  uint8_t* d = row + off;
  if (vst && n == 4 && !(off & 3)) {
    constexpr int DW = NCH * EB, PER = 4 / EB;                  // dwords of the group, elements per dword
    uint32_t q[DW];
    for (int k = 0; k < DW; k++) {
      q[k] = 0;
      for (int j = 0; j < PER; j++) {
        const int f = k * PER + j;
        q[k] |= e[f / NCH][f % NCH] << (8 * EB * j);
      }
    }
    for (int k = 0; k + 4 <= DW; k += 4) {
      u32x4_a4 v; v.x = q[k]; v.y = q[k + 1]; v.z = q[k + 2]; v.w = q[k + 3];
      *(u32x4_a4 HMGPU_AS1*)(d + 4 * k) = v;
    }
    constexpr int T = DW & ~3;
    if constexpr (DW - T == 3) { u32x3_a4 v; v.x = q[T]; v.y = q[T + 1]; v.z = q[T + 2]; *(u32x3_a4 HMGPU_AS1*)(d + 4 * T) = v; }
    if constexpr (DW - T == 2) { u32x2_a4 v; v.x = q[T]; v.y = q[T + 1]; *(u32x2_a4 HMGPU_AS1*)(d + 4 * T) = v; }
    return;
  }
  for (int i = 0; i < n; i++)
    for (int c = 0; c < NCH; c++) {
      if constexpr (EB == 1) stg(d + i * NCH + c, (uint8_t)e[i][c]);
      else if constexpr (EB == 2) stg(reinterpret_cast<uint16_t*>(d) + i * NCH + c, (uint16_t)e[i][c]);
      else stg(reinterpret_cast<uint32_t*>(d) + i * NCH + c, e[i][c]);
    }
}
struct ExportArgs {
  const int16_t* y[kMaxExportBatch];   // per picture: luma sample (crop left, crop top)
  const int16_t* c[kMaxExportBatch];   // Cb of chroma sample (crop left >> csx, crop top >> csy) in the pair plane (Cr one element on)
  int32_t pitch_y, pitch_c;        // int16 elements
  int32_t n;                       // pictures
  int32_t layout, elem, mono, csx, csy;   // elem: kElem*
  int32_t w, h, cw, ch;            // output luma / chroma size (chroma rows follow the luma rows in the grid, YUV layouts)
  int32_t sh[2], maxv[2];          // bit-depth rule per channel type: out - coding depth, 2^out - 1
  int32_t msb[2];                  // container shift per channel type (msb_aligned: 16 - out)
  uint32_t vec;                    // bit i: every group of 4 samples of picture i may use vector loads and stores (alignment of its
                                   // crop, of dst and of the pitches)
  uint32_t flip;                   // bit i: picture i is mirrored (every output row reversed)
  uint8_t* dst[3];
  int64_t pitch[3];                // bytes
  int64_t bstride[3];              // bytes between the planes of consecutive pictures
  float scale[3], bias[3];         // float elements: per output plane
  int32_t coef[16];                // hmgpu_export_plan.coef
};
// the colour stage of the RGB exports (colour_core.h, hmgpu_pictures_export_colour): one table in device memory of the context
struct ColourLut {
  const uint16_t* shaper;          // null, or [3][2^depth] positions 0 .. 65535 (size 0: output code values)
  const u32x2* nodes;              // null (size 0), or [size^3] nodes {R | G << 16, B}, R fastest
  int32_t size, depth;             // nodes per axis (0, 2 .. 65); the depth of the code values in and out
};
// the chroma stage of the RGB exports (chroma_core.h, hmgpu_pictures_export_chroma) for 4:2:0 and 4:2:2: the weights of the signalled
// sample location in quarters, and what clamping a tap to the decoded plane needs
struct ChromaSite {
  int32_t hx[2][3];                // [luma column parity]: weights of chroma columns j - 1, j, j + 1 (j = x >> 1)
  int32_t vy[2][2];                // [luma row parity]: first row relative to j = y >> csy (-1 / 0) and its weight; row + 1 has the rest
  int32_t wc, hc;                  // the decoded chroma plane, samples
  int16_t x0[kMaxExportBatch], y0[kMaxExportBatch];   // unscaled: per picture, the chroma sample ExportArgs::c points at
};
// The export of `a` (k_export.hip).  po: null, or (RGB) the channel order of packed pixels of nch (3 / 4) elements, written to the one
// destination dst[0] / pitch[0] / bstride[0] (a.vec then speaks of the loads only); cs / lut: null, or (RGB) the chroma / colour stage
void launch_export(const ExportArgs& a, const PxOrder* po, int nch, const ChromaSite* cs, const ColourLut* lut, hipStream_t s);
// format export (k_export_fmt.hip, hmgpu_pictures_export_format; include/hmgpu.h "format export"): the chroma rows of the YUV layouts
// read the pair plane of the source format and write one of another.  ExportArgs as launch_export takes it, with cw / ch the OUTPUT
// chroma size (csx / csy stay the source's).  A class per shape of the loads; the host's weights make REPLICATE and DROP exact in the
// same instances (a single weight 4 per axis: (4 * 4 * C + 8) >> 4 = C).
enum {
  kFmtConst = 0,                   // 4:0:0 source: Cb = Cr = constant, no loads
  kFmtUp = 1,                      // the horizontal axis gains (the vertical one gains or stays): chroma_core.h with cs's weights
  kFmtVert = 2,                    // the horizontal axis stays, the vertical one gains or loses: the group on one to three rows
  kFmtDown = 3                     // the horizontal axis loses (the vertical one loses or stays): 8 pairs and the one left of them, one to three rows
};
struct FmtConv {
  ChromaSite cs;                   // kFmtUp: the weights of the horizontal axis (hx) and of a vertical gain (vy).  Every class: wc / hc, the decoded
                                   // source chroma plane, and x0 / y0 per picture, the source chroma sample ExportArgs::c points at
  int32_t cls;                     // kFmt*
  int32_t vgain, vloss;            // the vertical axis gains / loses samples (neither: it stays)
  int32_t dv0, dv[3];              // vertical loss: the first row relative to 2j (-1 / 0) and the weights of rows dv0, dv0 + 1, dv0 + 2
  int32_t dh[3];                   // kFmtDown: the weights of source columns 2j - 1, 2j, 2j + 1
  int32_t constant;                // kFmtConst: the sample at the chroma output depth
};
void launch_export_fmt(const ExportArgs& a, const FmtConv& f, hipStream_t s);
// packed YUV export (k_export_yuvpack.hip, hmgpu_pictures_export_yuvpack; include/hmgpu.h "packed YUV"): Y, Cb and Cr of the format
// export at 4:2:2 or 4:4:4, interleaved into words of the one destination dst[0] / pitch[0] / bstride[0].  ExportArgs as
// launch_export_fmt takes it (w / h the output size in pixels; cw / ch are not read) and the conversion's FmtConv: kFmtConst for a
// 4:0:0 source, kFmtVert without gain or loss where the source has the words' own chroma format.  A family per shape of the word
// unit, what tells its members apart uniform:
enum {
  kPack422x8 = 0,                  // UYVY, YUY2: 4 bytes per 2 pixels, a lane 8 pixels
  kPack422x16 = 1,                 // Y210, Y216: 4 uint16 per 2 pixels, a lane 4 pixels
  kPackV210 = 2,                   // V210: 4 uint32 per 6 pixels, a lane one group
  kPackAYUV = 3,                   // 4 bytes per pixel, a lane 4 pixels
  kPackY410 = 4,                   // a uint32 per pixel, a lane 4 pixels
  kPackY416 = 5                    // 4 uint16 per pixel, a lane 2 pixels
};
struct YuvPackArgs {
  int32_t fam;                     // kPack*
  int32_t yfirst;                  // kPack422x8: Y before its chroma sample (YUY2), else behind it (UYVY)
  int32_t shift;                   // kPack422x16: every element shifted left (Y210: 6, Y216: 0)
  uint32_t alpha;                  // the 4:4:4 families: A
};
void launch_export_yuvpack(const ExportArgs& a, const FmtConv& f, const YuvPackArgs& p, hipStream_t s);
// scaled device export (k_export_scale.hip, hmgpu_picture_export_scaled).  One resampling table per axis of a plane class, in device
// memory of the context: first[n], count[n], span[tiles][2] (the source samples [lo, hi) a tile of outputs reads), then the Q14 weights
// tap-major (w[tap * n + i], zero beyond count[i])
struct ScaleTable {
  const int32_t* first;
  const int32_t* count;
  const int32_t* span;
  const int16_t* w;
  int32_t n;                       // output samples along the axis
};
constexpr int kScaleLdsBytes = 40960;   // LDS of one workgroup: four share a CU
struct ScaleClass {                // one plane class: 0 = luma (YUV) or RGB, 1 = the chroma pair (YUV)
  ScaleTable tx, ty;
  int32_t tw, th;                  // tile: output columns (4 .. 128, a power of two) x output rows, tw / 4 * th <= 256
  int32_t rows;                    // source rows per pass through LDS (<= 1024 / tw)
  int32_t span_cap;                // LDS samples per row and channel: the widest source span of a tile in 16-byte groups
  int32_t tiles_x, blocks;         // tiles per row, workgroups of the class
  int32_t x0, y0;                  // crop origin in the class's plane (samples)
  int32_t pitch;                   // int16 elements
};
struct ScaleArgs {
  ScaleClass cls[2];               // the classes of every picture; with pic_cls: tw, th, tiles_x and blocks, common to the call (one grid)
  const ScaleClass* pic_cls;       // null, or per picture and class ([grid y][2], device memory beside the tables): windows that differ
  const int16_t* src[kMaxExportBatch][2];   // per picture (grid y): sample (0, 0) of the luma plane and of the pair plane (Cb)
  int32_t pitch_c;                 // RGB: rows of the pair plane
  int32_t mono, csx, csy;
  int32_t sh[2], maxv[2], msb[2];  // bit-depth rule per channel type (as ExportArgs); RGB: maxv[0] = coef[9]
  int32_t e;                       // fractional bits kept between the passes (hmgpu_export_plan.coef[11])
  int32_t vec;                     // every group of 4 output samples may be one 4- or 8-byte store (alignment of dst and pitches)
  uint32_t flip;                   // bit i: picture i is mirrored (every output row reversed)
  uint8_t* dst[3];
  int64_t pitch[3];                // bytes
  int64_t bstride[3];              // bytes between the planes of consecutive pictures
  float scale[3], bias[3];         // float elements: per output plane
  int32_t coef[16];                // hmgpu_export_plan.coef
  PxOrder px;                      // packed pixels (nch below): dst[0] / pitch[0] / bstride[0] the one destination, vec = px.vst
};
// n pictures; elem: kElem*; nch: 0, or (RGB) 3 / 4 elements per packed pixel; cs / lut: null, or (RGB) the chroma stage in the stage
// step / the colour stage in the epilogue
void launch_export_scaled(const ScaleArgs& a, int layout, int elem, int n, int nch, const ChromaSite* cs, const ColourLut* lut, hipStream_t s);
// affine warp export (k_export_warp.hip, hmgpu_pictures_export_warp; include/hmgpu.h "affine warp export"): the RGB layout, planes or
// packed pixels, each picture through its own inverse map.  Per picture (grid y), in device memory of the window ring: the Q16 map
// and the source window in plane coordinates
struct WarpPic { int32_t m[6]; int32_t x0, y0, ws, hs; int32_t pad_[2]; };
constexpr int kWarpTileW = 64, kWarpTileH = 16;   // outputs of one workgroup: a lane has four adjacent columns of one row
struct WarpArgs {
  const WarpPic* pics;             // [grid y]
  const int16_t* src[kMaxExportBatch][2];   // per picture: sample (0, 0) of the luma plane and of the pair plane (Cb)
  int32_t pitch_y, pitch_c;        // int16 elements
  int32_t mono, csx, csy;
  int32_t w, h, tiles_x;           // the output of every picture; 64-column tiles per tile row
  int32_t filter, border;          // HMGPU_WARP_*
  uint32_t fill[3];                // HMGPU_WARP_FILL: R, G, B
  int32_t sh[2], maxv[2], msb[2];  // bit-depth rule per channel type (as ExportArgs)
  int32_t vec;                     // every group of 4 output samples may be one store (alignment of dst and pitches; packed: px.vst)
  uint32_t flip;                   // bit i: picture i is mirrored (every output row reversed)
  uint8_t* dst[3];
  int64_t pitch[3];                // bytes
  int64_t bstride[3];              // bytes between the planes of consecutive pictures
  float scale[3], bias[3];         // float elements: per output plane
  int32_t coef[16];                // hmgpu_export_plan.coef
  PxOrder px;                      // packed pixels (nch below): dst[0] / pitch[0] / bstride[0] the one destination
};
// n pictures; elem: kElem*; nch: 0, or 3 / 4 elements per packed pixel; cs: null, or the chroma stage; lut: null, or the colour stage
void launch_export_warp(const WarpArgs& a, int elem, int n, int nch, const ChromaSite* cs, const ColourLut* lut, hipStream_t s);
// motion and block export (k_motion.hip, hmgpu_pictures_export_motion): everything by value, validated on the host.  The raw HM
// arrays of every picture of the call (PicDev's own pointers: fixed for the life of a picture) and, per slot, the source window of the
// dense form.  Destination slots: 0 / 1 the vectors, 2 ref_poc, 3 block (HMGPU_MOTION_DST_*); a null destination is not written.
struct MotionSrc {
  const uint8_t* depth; const int8_t* part_size; const int8_t* pred_mode; const int8_t* qp;
  const int16_t* mv[2]; const int8_t* ref_idx[2];
  const uint16_t* slice_idx;
  const SliceDev* slices;
};
struct SideWin { int32_t left, top, w, h; };                   // dense forms: a picture's window in luma samples
struct MotionWin : SideWin { float kx, ky; };                  // ... and quarter samples -> output samples
struct MotionArgs {
  MotionSrc src[kMaxExportBatch];
  MotionWin win[kMaxExportBatch];
  int32_t n, lists, nlists;        // pictures; the lists mask; selected lists
  int32_t log2ctu, ctus_w, parts;  // geometry of the context
  int32_t x4, y4, w4, h4;          // blocks form: first block and size of the cropped grid
  int32_t W, H;                    // dense form: output size
  uint32_t flip;                   // dense form: bit i: slot i is mirrored
  int32_t vec;                     // blocks form: a group of four blocks may be one store per plane (alignment of crop, dst and strides)
  uint8_t* dst[4];
  int64_t pitch[4], pstride[4], bstride[4];   // bytes: row to row, plane to plane, picture to picture
};
void launch_motion_blocks(const MotionArgs& a, hipStream_t s);
void launch_motion_dense(const MotionArgs& a, int elem, hipStream_t s);   // elem: kElemF16 / kElemBF16 / kElemF32
// residual export (k_residual.hip, hmgpu_pictures_export_residual): everything by value, validated on the host.  The residual tiles
// of every picture of the call (PicDev::resid) and the HM arrays that say which samples a coded transform block covers; `gate` is what
// the host knows was staged for the picture: the arrays of a group that did not travel are never read.
enum { kResidIntra = 1, kResidFlags = 2 };      // ResidSrc::gate: intra CUs carry a residual (intra_dir[] was given); the flag group (ipcm) was staged
struct ResidSrc {
  const uint8_t* depth; const int8_t* part_size; const int8_t* pred_mode; const uint8_t* tr_idx;
  const uint8_t* cbf[3]; const uint8_t* ipcm;
  const int16_t* resid[3];
  int32_t gate, pad_;
};
struct ResidArgs {
  ResidSrc src[kMaxExportBatch];
  SideWin win[kMaxExportBatch];    // dense form
  int32_t n, comps, mono;          // pictures; the component mask (bit c; chroma bits cleared for 4:0:0 pictures); 4:0:0
  int32_t log2ctu, ctus_w, parts;  // geometry of the context
  int32_t rtw[3];                  // residual tiles per tile row of the component
  int32_t x0, y0, w, h;            // planes form: first luma sample and size of the cropped picture (multiples of 8)
  int32_t W, H;                    // dense form: output size
  uint32_t flip;                   // dense form: bit i: slot i is mirrored
  int32_t vec;                     // bit k: destination k may take 16-byte stores (alignment of crop, dst and strides)
  int32_t chan[3];                 // dense form: the plane of component c in dst[0]
  float scale[3];                  // dense form, float elements: per component
  uint8_t* dst[3];                 // planes form: per component; dense form: dst[0]
  int64_t pitch[3], pstride[3], bstride[3];   // bytes: row to row, plane to plane (dense), picture to picture
};
void launch_residual_planes(const ResidArgs& a, hipStream_t s);
void launch_residual_dense(const ResidArgs& a, int elem, hipStream_t s);   // elem: kElemU16 (int16) / kElemF16 / kElemBF16 / kElemF32
// transform export (k_transform.hip, hmgpu_pictures_export_transform): everything by value, validated on the host.  The levels of every
// picture of the call (PicDev::coef: HM's dense layout, or compact behind coef_start), the HM arrays that say where a coded block lies
// and how it is de-quantised, the slice table (chroma QP offsets) and the scaling-list matrices.  `gate` as in ResidSrc: the flag group
// is read only where it was staged; kTransDir: every call of the picture came with intra_dir[] (info channels 4 / 5).
// Destination slots: 0 .. 2 the component planes, 3 the info grid (HMGPU_TRANSFORM_DST_INFO).
enum { kTransDir = 1, kTransFlags = 2 };
struct TransformSrc {
  const uint8_t* depth; const int8_t* part_size; const int8_t* pred_mode; const int8_t* qp; const uint8_t* tr_idx;
  const uint8_t* cbf[3]; const uint8_t* tskip[3]; const uint8_t* bypass; const uint8_t* ipcm;
  const uint8_t* intra_dir[2];
  const uint16_t* slice_idx; const SliceDev* slices;
  const int16_t* coef[3];
  const uint32_t* coef_start[3];   // compact levels: the CTUs' starts, else null
  const uint8_t* sl_m;             // PicDev::sl_m, or null (flat scaling)
  int32_t gate, pad_;
};
struct TransformArgs {
  TransformSrc src[kMaxExportBatch];
  int32_t n, comps;                // pictures; the component mask (chroma bits cleared for 4:0:0 pictures)
  int32_t mono, fmt, csx, csy;     // 4:0:0; chroma_format_idc (0 kept as 1) and its subsampling
  int32_t log2ctu, ctus_w, parts;  // geometry of the context
  int32_t width, height, bd[3];    // luma samples; bit depth per component
  int32_t vec;                     // bit k: plane k may take 16-byte stores (alignment of dst and strides)
  float scale[3];                  // float elements: per component
  uint8_t* dst[4];
  int64_t pitch[4], pstride[4], bstride[4];   // bytes: row to row, channel to channel (info), picture to picture
};
// coeffs: HMGPU_TRANSFORM_COEFFS (else the levels); elem: kElemU16 (int16) / kElemF16 / kElemBF16 / kElemF32
void launch_transform(const TransformArgs& a, bool coeffs, int elem, int num_ctus, hipStream_t s);
// loop-filter export (k_lfinfo.hip, hmgpu_pictures_export_loopfilter): everything by value, validated on the host.  The edge-unit records
// k_prep derived for the picture (PicDev::edges), the slice table behind the per-CTU slice index, and the SAO parameters the last filter
// call resolved.  `gate` is what the host knows about those: without kLfSao the parameter buffer is never read (no filter call with an
// SAO stage on the handle's current picture) and every CTB is exported as off.
// Destination slots: 0 the edge grid, 1 the SAO grid, 2 the dense form (HMGPU_LOOPFILTER_DST_*).
enum { kLfSao = 1 };
struct LfSrc {
  const EdgeRec* edges; const SaoDev* saoprm;
  const uint16_t* slice_idx; const SliceDev* slices;
  int32_t gate, pad_;
};
struct LfArgs {
  LfSrc src[kMaxExportBatch];
  SideWin win[kMaxExportBatch];    // dense form
  int32_t n, mono, fmt, csx, csy;  // pictures; 4:0:0; chroma_format_idc (0 kept as 1) and its subsampling
  int32_t log2ctu, ctus_w, ctus_h; // geometry of the context
  int32_t ew;                      // EdgeRec records per row of the grid (grid_w / 2)
  int32_t width, height, bd[2];    // luma samples; bit depth of luma / chroma
  int32_t x8, y8, w8, h8;          // grids form: first 8x8 area and size of the cropped edge grid in areas
  int32_t W, H;                    // dense form: output size
  uint32_t flip;                   // dense form: bit i: slot i is mirrored
  int32_t vec;                     // bit k: destination k may take dword stores (alignment of dst and strides)
  float scale[3];                  // dense form, float elements: per channel
  uint8_t* dst[3];
  int64_t pitch[3], pstride[3], bstride[3];   // bytes: row to row, plane to plane, picture to picture
};
void launch_lfinfo_grids(const LfArgs& a, hipStream_t s);
void launch_lfinfo_dense(const LfArgs& a, int elem, hipStream_t s);   // elem: kElemU8 / kElemF16 / kElemBF16 / kElemF32
// picture metrics (k_metrics.hip, hmgpu_pictures_metrics): everything by value, validated on the host.  Plane class 0 is luma, class 1
// the chroma pair (Cb and Cr from one load of the pair plane); a class with no selected component has no tiles.  Work items are
// (picture, class, tile) in that order; workgroup g walks items [g * per, (g + 1) * per).  A tile is 2048 samples: 64 x 32 with SSIM (the
// 4-sample apron right and below costs least on a squarish tile), 256 x 8 without (rows of 512 contiguous bytes).
constexpr int kMetricsTileW = 64, kMetricsTileH = 32, kMetricsRowTileW = 256, kMetricsRowTileH = 8;
// workgroups of a call: four per CU without SSIM (all resident at once), eight with (its barriers want more waves to hide behind)
constexpr int kMetricsGrid = 1024, kMetricsGridSsim = 2048;
struct MetricsArgs {
  const int16_t* a[kMaxExportBatch][2];   // per picture: luma sample (crop left, crop top); Cb of the same chroma sample in the pair plane
  const int16_t* bp[kMaxExportBatch][2];  // REF_PICTURES: the same of the reference picture
  const uint8_t* bq[3];                   // REF_PLANES: per component (null: not compared), uint8 or uint16 elements
  int64_t bpitch[3], bstride[3];          // bytes: row to row, picture to picture
  uint8_t* results;                       // record (i, c) at results + i * rstride + c * 64, zeroed before the launch
  int64_t rstride;
  int64_t c1[2], c2[2];                   // SSIM constants per channel type
  int32_t n, comps;                       // pictures; the component mask (only components the format has)
  int32_t w[2], h[2], pitch[2];           // per class: the cropped plane in samples; the source pitch in int16 elements
  int32_t tiles_x[2], tiles[2];           // per class: tiles per tile row, tiles per picture (0: class not selected)
  int32_t per, total;                     // items per workgroup, items of the call
  uint32_t avec[2];                       // per class, bit i: the groups of 4 samples of picture i (and of its reference picture) are aligned for one load
  uint32_t bvec;                          // REF_PLANES, bit c: the same for the planes of component c
};
void launch_metrics(const MetricsArgs& a, int ref_kind, bool ssim, hipStream_t s);   // ref_kind: 0 pictures, 1 uint8 planes, 2 uint16 planes
// picture metric maps (k_metrics_map.hip, hmgpu_pictures_metrics_map): everything by value, validated on the host.  Classes as in
// MetricsArgs.  A workgroup owns one region of one class of one picture: 64 x 64 luma samples from the crop origin, or the matching
// (64 >> csx) x (64 >> csy) positions of the pair plane -- (64 / B)^2 whole blocks of either class; work item = (picture, class, region).
constexpr int kMapRegion = 64;              // luma samples: one block of the largest size
constexpr int kMapFields = 6;               // HMGPU_METRICS_MAP_FIELDS
struct MetricsMapArgs {
  const int16_t* a[kMaxExportBatch][2];   // as MetricsArgs
  const int16_t* bp[kMaxExportBatch][2];
  const uint8_t* bq[3];
  int64_t bpitch[3], bstride[3];
  uint8_t* maps[3];                       // per component (null: not compared): element (i, f, by, bx) at maps + i * mbstride + f * mfstride + by * mpitch + bx * 8
  int64_t mpitch[3], mfstride[3], mbstride[3];
  int64_t c1[2], c2[2];                   // SSIM constants per channel type
  int32_t n, comps;                       // pictures; the component mask (only components the format has)
  int32_t w[2], h[2], pitch[2];           // per class: the cropped plane in samples; the source pitch in int16 elements
  int32_t regions_x[2], regions[2];       // per class: regions per row of them, regions per picture (0: class not selected)
  int32_t log2_rw[2], log2_rh[2];         // per class: the region in samples, 64 or 32 a side
  int32_t log2_bw[2], log2_bh[2];         // per class: the block in samples, 4 .. 64 a side
  int32_t log2_nb;                        // blocks per side of a region: 6 - log2_block
  int32_t blocks_x, blocks_y;             // the map
  uint32_t avec[2];                       // as MetricsArgs
  uint32_t bvec;
};
void launch_metrics_map(const MetricsMapArgs& a, int ref_kind, bool ssim, hipStream_t s);   // ref_kind as launch_metrics
// picture histograms (k_histogram.hip, hmgpu_pictures_histogram): everything by value, validated on the host.  Plane class 0 walks the
// cropped luma plane and counts Y (channel 0) and maxRGB (channel 3) of a sample together, class 1 the chroma pair plane (channels 1
// and 2 from one load); a class with no selected channel has no tiles.  Work items and tiles as in MetricsArgs without SSIM.
constexpr int kHistTileW = 256, kHistTileH = 8;
constexpr int kHistMaxBins = 4096;          // 2^12: a channel's bins in the LDS, two channels per class
constexpr int kHistGrid = 1024;             // four workgroups per CU: what 32 KB of LDS each leaves room for
struct HistogramArgs {
  const int16_t* y[kMaxExportBatch];      // per picture: luma sample (crop left, crop top)
  const int16_t* c[kMaxExportBatch];      // Cb of the same chroma sample in the pair plane
  uint8_t* hist[4];                       // per channel: histogram of picture i at hist[c] + i * hstride[c], zeroed before the launch
  int64_t hstride[4];
  uint8_t* records;                       // record (i, c) at records + i * rstride + c * 64, zeroed before the launch
  int64_t rstride;
  int32_t n, chans;                       // pictures; the channel mask (only channels that are computed)
  int32_t do_hist;                        // 0: records only
  int32_t w[2], h[2], pitch[2];           // per class: the cropped plane in samples; the source pitch in int16 elements
  int32_t tiles_x[2], tiles[2];           // per class: tiles per tile row, tiles per picture (0: class not selected)
  int32_t per, total;                     // items per workgroup, items of the call
  int32_t shift[4], log2_bins[4];         // per channel: D_c - b_c, b_c
  uint32_t yvec, cvec, rvec;              // bit i: picture i takes whole loads of 4 luma samples / of 4 chroma pairs / of the chroma of 4 luma samples
  int32_t csx, csy, mono;                 // maxRGB: chroma subsampling; 4:0:0
  int32_t coef[16], sh[2], maxv[2];       // maxRGB: hmgpu_export_plan.coef and the depth rule of the identity, as ExportArgs
};
void launch_histogram(const HistogramArgs& a, hipStream_t s);
// picture import (k_import.hip, hmgpu_pictures_import; include/hmgpu.h "picture import"): the way in from device memory.  A chroma
// sample (jx, jy) of the picture is clamped to the converted source (ccw x cch, the padding rule) and then read through up to 3 x 3
// taps of the source's chroma plane (scw x sch; RGB: Cb / Cr at every pixel): column ((jx << hl) >> hr) + h0 + t with weight hw[t],
// rows likewise, weights in quarters, (sum + 8) >> 4 -- the sample itself, sample j >> 1, sample 2j and the decimation taps of the
// format export are all of this shape.
struct ImportArgs {
  int16_t* y[kMaxExportBatch];     // per picture: luma sample (0, 0) of the reconstruction planes
  int16_t* c[kMaxExportBatch];     // Cb of chroma sample (0, 0) in the pair plane (Cr one element on)
  int32_t pitch_y, pitch_c;        // int16 elements
  int32_t n;                       // pictures
  int32_t layout, elem;            // HMGPU_EXPORT_* of the source; element: 0 uint8, 1 uint16, 2 float16, 3 bfloat16, 4 float32;
                                   // packed YUV words in src[0] (layout planar): 5 of 1-byte, 6 of 2-byte elements, 7 of dwords
  int32_t nch, pos[3];             // RGB: 0 three planes, else 3 / 4 elements per packed pixel and where R, G, B stand in it
  int32_t w, h, sw, sh;            // the coded picture and the source, luma samples
  int32_t mono, psx, psy;          // the picture: no chroma (then psx = psy = 0); chroma subsampling
  int32_t smono, same, drop;       // the source: 4:0:0; its chroma planes have the picture's shape; no tap but one of weight 4 per axis
  int32_t ccw, cch, scw, sch;      // converted chroma size (sw >> psx, sh >> psy); the source's chroma plane
  int32_t hl, hr, h0, hw[3];       // horizontal taps
  int32_t vl, vr, v0, vw[3];       // vertical taps
  int32_t dsh[2], maxv[2];         // bit-depth rule per channel type: coding - source depth, 2^coding - 1
  int32_t smax[2], msb[2];        // 2^source depth - 1; container shift (msb_aligned: 16 - source depth)
  int32_t cconst;                  // 4:0:0 source: 1 << (source chroma depth - 1)
  uint32_t vec;                    // bit k: rows of source plane k start on multiples of eight elements; bit 8: rows of both
                                   // destination planes on multiples of 16 bytes
  const uint8_t* src[3];
  int64_t pitch[3];                // bytes
  int64_t bstride[3];              // bytes between the planes of consecutive pictures
  float scale[3], bias[3];         // float elements: per source plane / colour
  int32_t coef[16];                // hmgpu_import_plan.coef
  int32_t pk_ls, pk_lo;            // packed YUV, elements 5 / 6: luma sample x is element pk_ls * x + pk_lo of its row,
  int32_t pk_cs, pk_co[2];         // chroma sample x of Cb / Cr element pk_cs * x + pk_co[0 / 1] (msb: the shift of Y210)
  int32_t pk_v210;                 // element 7: V210 (else Y410)
};
void launch_import(const ImportArgs& a, hipStream_t s);
// chroma of 4:2:2 / 4:4:4 pictures (k_cfmt.hip): cross-component prediction on the residual tiles, motion compensation of every inter
// cell, chroma deblocking on the format's own grid; fmt = chroma_format_idc
void launch_ccp(const PicDev* pics, const Batch& b, int max_ctus, hipStream_t s);
void launch_mc_chroma_fmt(const PicDev* pics, const PlaneSet* finals, const Batch& b, int max_ctus, int log2ctu, int fmt, bool wp, hipStream_t s);
void launch_deblock_chroma_fmt(const PicDev* pics, const Batch& b, int dir, int width, int height, hipStream_t s);
void launch_intra_chroma_422(const PicDev* pics, const Batch& b, hipStream_t s);
void launch_deblock(const PicDev* pics, const Batch& b, int dir, int width, int height, hipStream_t s);
void launch_sao(const PicDev* pics, const Batch& b, int width, int height, int csx, int csy, hipStream_t s);
void launch_extend(const PicDev* pics, const Batch& b, int width, int height, int mx, int my, int csx, int csy, hipStream_t s);
// error concealment (k_conceal.hip, hmgpu_pictures_conceal; include/hmgpu.h "error concealment"): everything by value, validated on the
// host.  Per picture the FINAL planes of the destination and of the source (null: fill), the CTU mask in device memory, and -- motion
// copy -- the source's HM arrays and slice table, read only where `side` says decompress calls staged them for the whole picture.
struct ConcealPic {
  int16_t* dst_y; int16_t* dst_c;              // sample (0, 0) of the luma plane / Cb of the pair plane
  const int16_t* src_y; const int16_t* src_c;  // the same of the source; null: fill
  const uint8_t* mask;                         // (num_ctus + 7) / 8 bytes, bit (a & 7) of byte a >> 3 = CTU a
  const int8_t* part_size; const int8_t* pred_mode;
  const int16_t* mv[2]; const int8_t* ref_idx[2];
  const uint16_t* slice_idx; const SliceDev* slices;
  int32_t mode, side;                          // HMGPU_CONCEAL_*; the source has side information
  int32_t dst_poc, src_poc;
  uint32_t fill_y, fill_c;                     // the luma sample; Cb | Cr << 16
};
struct ConcealArgs {
  ConcealPic pic[kMaxBatch];
  int32_t n, mono;                             // pictures; 4:0:0 (no chroma plane is written)
  int32_t width, height, log2ctu, ctus_w, num_ctus, parts;
  int32_t pitch_y, pitch_c;                    // int16 elements
  int32_t csx, csy;
};
void launch_conceal(const ConcealArgs& a, hipStream_t s);
// kernel-level seams for tests
void launch_itx_flat(int log2size, int bit_depth, int n, const int16_t* levels, const int8_t* per, const int8_t* rem,
                     const uint8_t* flags, int16_t* resid, hipStream_t s);
void launch_mc_flat(int is_chroma, int bit_depth, const int16_t* ref, int ref_stride, int ref_w, int ref_h, int n,
                    const int32_t* blocks, const int32_t* out_off, int bi, int16_t* dst, hipStream_t s);

}  // namespace hmgpu
