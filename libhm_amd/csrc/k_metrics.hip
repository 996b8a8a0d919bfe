// k_metrics.hip -- finished pictures compared with other pictures or with caller-owned planes (hmgpu_pictures_metrics,
// include/hmgpu.h "picture metrics"): per picture and component SSE, SAD, differing samples, the first difference,
// max |d| and the 8x8 / stride-4 integer SSIM of x264, all exact integers.
// One pass, bound by its reads: 2 bytes of the picture per sample and 1 or 2 of the reference.  A workgroup walks a contiguous run of
// tiles of 2048 samples (MetricsArgs) with one lane per group of 4 samples of a row -- the 8-byte loads of the export kernels, 16-byte ones
// on the chroma pair plane, which gives Cb and Cr of a group at once, so the pair plane is read once for both components.  It keeps its
// sums in registers across the tiles of a (picture, plane class) and hands them over once: wave reduction by __shfl_xor, the four
// waves through LDS, then one set of 64-bit integer atomics per workgroup and record (k_prep's notes: ~11 ns per atomic on one word;
// a set per tile would cost more than the reads).  The sums are integers, so the arrival order does not show in the result.
// A lane's first difference is the least index it has seen, in 32 bits (metrics_plan bounds the plane).  first_diff travels as
// ~index through atomicMax on the zeroed record; the last workgroup to arrive at a record (a ticket in its reserved word, which it
// leaves 0) turns it back, which makes "none" UINT64_MAX.
// SSIM instance: the lanes are laid out by 4x4 block -- lanes 4k .. 4k + 3 hold the four rows of block k of the tile and its 4-sample
// apron right and below (17 x 9 blocks) -- so two __shfl_xor steps give the block's sums (a, b, a^2 + b^2, ab), written once to LDS;
// a window is the sum of a 2x2 group of blocks.  The apron is left out of the distortion terms.  desc->ssim == 0 is an instance of its
// own: row-major lanes on 256 x 8 tiles (a wave's load is one run of 512 bytes of a luma row), no apron, no LDS staging.
#include "hmgpu_dev.h"
#include "metrics_core.h"

namespace hmgpu {

namespace {

constexpr int kBlocksX = kMetricsTileW / 4 + 1, kBlocksY = kMetricsTileH / 4 + 1;   // 4x4 blocks of a tile and its apron: 17 x 9
constexpr int kUnitsSsim = kBlocksX * kBlocksY * 4;                                  // groups of 4 samples, block-major: 612
constexpr int kUnitsPlain = kMetricsRowTileW / 4 * kMetricsRowTileH;                 // row-major: 512
constexpr int kWindows = (kMetricsTileW / 4) * (kMetricsTileH / 4);                 // windows that start in a tile: 128

struct Acc {                      // what one lane has seen of one component since the last hand-over
  u64 sse, sad; long long ssim;
  uint32_t samples, differing, windows, max_abs, first;   // first: y * w + x, below 2^32 - 1 (metrics_plan); ~0u: none
};

__device__ inline void acc_clear(Acc& c) { c.sse = c.sad = 0; c.first = ~0u; c.ssim = 0; c.samples = c.differing = c.windows = c.max_abs = 0; }

__device__ inline u64 wave_sum(u64 v) { for (int m = 32; m; m >>= 1) v += xor64(v, m); return v; }
__device__ inline u64 wave_min(u64 v) { for (int m = 32; m; m >>= 1) { const u64 o = xor64(v, m); v = o < v ? o : v; } return v; }
__device__ inline uint32_t wave_max(uint32_t v) { for (int m = 32; m; m >>= 1) v = max(v, xor32(v, m)); return v; }

// One tile of plane class CLS of picture `pic`: NC = 1 + CLS components at once.  blk: the block sums of the SSIM instance.
template <int REF, bool SSIM, int CLS>
__device__ inline void tile_pass(const MetricsArgs& a, int pic, int tile, Acc acc[2], BlockSum (*blk)[kBlocksX * kBlocksY]) {
  constexpr int NC = CLS + 1;
  const int w = a.w[CLS], h = a.h[CLS], pitch = a.pitch[CLS];
  constexpr int TW = SSIM ? kMetricsTileW : kMetricsRowTileW, TH = SSIM ? kMetricsTileH : kMetricsRowTileH;
  const int tx0 = (tile % a.tiles_x[CLS]) * TW, ty0 = (tile / a.tiles_x[CLS]) * TH;
  const int16_t* const pa = a.a[pic][CLS];
  const int16_t* const pb = a.bp[pic][CLS];
  const bool avec = (a.avec[CLS] >> pic) & 1;
  const int tid = threadIdx.x;
  constexpr int PASSES = ((SSIM ? kUnitsSsim : kUnitsPlain) + 255) / 256;
#pragma unroll
  for (int pass = 0; pass < PASSES; pass++) {
    const int u = tid + 256 * pass;
    int x, y, b4 = 0;
    bool core = true, live;
    if (SSIM) {
      b4 = u >> 2;
      const int bx = b4 % kBlocksX, by = b4 / kBlocksX;
      x = tx0 + 4 * bx; y = ty0 + 4 * by + (u & 3);
      core = bx < kBlocksX - 1 && by < kBlocksY - 1;
      live = u < kUnitsSsim && x < w && y < h;
    } else {
      x = tx0 + 4 * (u & (TW / 4 - 1)); y = ty0 + u / (TW / 4);
      live = x < w && y < h;
    }
    int va[NC][4], vb[NC][4];
    for (int k = 0; k < NC; k++)
      for (int j = 0; j < 4; j++) va[k][j] = vb[k][j] = 0;
    const int nv = min(4, w - x);
    if (live) {
      const bool whole = nv == 4;
      load_pic<NC>(pa + (ptrdiff_t)y * pitch + NC * x, whole && avec, nv, va);
      if (REF == 0) {
        load_pic<NC>(pb + (ptrdiff_t)y * pitch + NC * x, whole && avec, nv, vb);
      } else {
        for (int k = 0; k < NC; k++) {
          const int c = CLS + k;
          const uint8_t* q = a.bq[c];
          if (q) load_plane<REF>(q + pic * a.bstride[c] + y * a.bpitch[c] + (int64_t)x * REF, whole && ((a.bvec >> c) & 1), nv, vb[k]);
        }
      }
    }
    if (live && core) {
      // per group of 4: |d| < 2^16, so the squares are 24-bit multiplies (full rate) and the group's SAD fits 32 bits.  A lane does not meet
      // its samples in index order -- it covers several rows of a tile, then rows above them in the tile to the right -- so its first
      // difference is the minimum over all it has seen
      for (int k = 0; k < NC; k++) {
        Acc& c = acc[k];
        c.samples += (uint32_t)nv;
        uint32_t ad[4], differ = 0, sad = 0, top = 0;
        for (int j = 0; j < 4; j++) {
          const int d = va[k][j] - vb[k][j];
          ad[j] = (uint32_t)(d < 0 ? -d : d);
          differ |= (ad[j] ? 1u : 0u) << j;
          sad += ad[j];
          top = max(top, ad[j]);
        }
        c.sse += ((u64)mul24(ad[0], ad[0]) + (u64)mul24(ad[1], ad[1])) + ((u64)mul24(ad[2], ad[2]) + (u64)mul24(ad[3], ad[3]));
        c.sad += sad;
        c.max_abs = max(c.max_abs, top);
        c.differing += (uint32_t)__popc(differ);
        if (differ) c.first = min(c.first, (uint32_t)y * (uint32_t)w + (uint32_t)(x + __ffs((int)differ) - 1));
      }
    }
    if (SSIM) {
      for (int k = 0; k < NC; k++) {
        const BlockSum sums = block_sums(va[k], vb[k]);
        if ((u & 3) == 0 && u < kUnitsSsim) blk[k][b4] = sums;
      }
    }
  }
  if (SSIM) {
    __syncthreads();
    if (tid < kWindows) {
      const int bx = tid & 15, by = tid >> 4;
      if (tx0 + 4 * bx + 8 <= w && ty0 + 4 * by + 8 <= h) {
        const long long c1 = a.c1[CLS], c2 = a.c2[CLS];
        for (int k = 0; k < NC; k++) {
          acc[k].ssim += window_q32(&blk[k][by * kBlocksX + bx], 1, kBlocksX, c1, c2);
          acc[k].windows++;
        }
      }
    }
    __syncthreads();                      // the next tile overwrites the block sums
  }
}

// the workgroup's sums of class `cls` of picture `pic` into the records, then the ticket: `last` workgroups hand over to this class
__device__ inline void hand_over(const MetricsArgs& a, int pic, int cls, Acc acc[2], u64 (*red)[8], int last) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int c = cls + k;
    if (k > cls || !((a.comps >> c) & 1)) continue;
    const Acc& v = acc[k];
    const u64 r[8] = {wave_sum(v.samples), wave_sum(v.sse), wave_sum(v.sad), wave_sum(v.differing), wave_min(v.first == ~0u ? ~0ull : (u64)v.first),
                      wave_sum((u64)v.ssim), wave_sum(v.windows), (u64)wave_max(v.max_abs)};
    __syncthreads();
    if (lane == 0)
      for (int f = 0; f < 8; f++) red[wave][f] = r[f];
    __syncthreads();
    if (tid == 0) {
      u64 t[8];
      for (int f = 0; f < 8; f++) t[f] = red[0][f];
      for (int q = 1; q < 4; q++) {
        for (int f = 0; f < 8; f++)
          if (f != 4 && f != 7) t[f] += red[q][f];
        t[4] = red[q][4] < t[4] ? red[q][4] : t[4];
        t[7] = red[q][7] > t[7] ? red[q][7] : t[7];
      }
      u64* rec = reinterpret_cast<u64*>(a.results + pic * a.rstride + c * 64);
      uint32_t* tail = reinterpret_cast<uint32_t*>(rec + 7);      // max_abs, then the reserved word: the ticket
      atomicAdd(rec + 0, t[0]); atomicAdd(rec + 1, t[1]); atomicAdd(rec + 2, t[2]); atomicAdd(rec + 3, t[3]);
      if (t[4] != ~0ull) atomicMax(rec + 4, ~t[4]);
      atomicAdd(rec + 5, t[5]); atomicAdd(rec + 6, t[6]);
      atomicMax(tail, (uint32_t)t[7]);
      __threadfence();
      if (atomicAdd(tail + 1, 1u) == (uint32_t)(last - 1)) {      // every other workgroup of this record has handed over
        __threadfence();
        const u64 key = atomicAdd(rec + 4, 0ull);
        atomicExch(rec + 4, ~key);
        atomicExch(tail + 1, 0u);
      }
    }
  }
}

}  // namespace

template <int REF, bool SSIM>
// the register counts lie at a step of the occupancy (72 / 96 VGPRs: 7 / 5 waves per SIMD), and which side an instance lands on moved
// with unrelated edits; the floor keeps each on the fast side (no vector register spills under it, no scratch)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SSIM ? 5 : 7))) k_metrics(const MetricsArgs a) {
  __shared__ BlockSum blk[SSIM ? 2 : 1][kBlocksX * kBlocksY];
  __shared__ u64 red[4][8];
  Acc acc[2];
  acc_clear(acc[0]); acc_clear(acc[1]);
  const int per_pic = a.tiles[0] + a.tiles[1];
  const int first = blockIdx.x * a.per, end = min(first + a.per, a.total);
  int cur = -1;                           // picture * 2 + class of the sums held
  for (int item = first; item < end; item++) {
    const int pic = item / per_pic, r = item - pic * per_pic;
    const int cls = r >= a.tiles[0] ? 1 : 0;
    const int key = pic * 2 + cls;
    if (key != cur) {
      if (cur >= 0) {
        // the workgroups whose runs meet the items of (picture, class) cur: every one of them computes the same count
        const int s = (cur >> 1) * per_pic + ((cur & 1) ? a.tiles[0] : 0), e = s + a.tiles[cur & 1];
        hand_over(a, cur >> 1, cur & 1, acc, red, (e - 1) / a.per - s / a.per + 1);
        acc_clear(acc[0]); acc_clear(acc[1]);
      }
      cur = key;
    }
    if (cls == 0) tile_pass<REF, SSIM, 0>(a, pic, r, acc, blk);
    else tile_pass<REF, SSIM, 1>(a, pic, r - a.tiles[0], acc, blk);
  }
  if (cur >= 0) {
    const int s = (cur >> 1) * per_pic + ((cur & 1) ? a.tiles[0] : 0), e = s + a.tiles[cur & 1];
    hand_over(a, cur >> 1, cur & 1, acc, red, (e - 1) / a.per - s / a.per + 1);
  }
}

void launch_metrics(const MetricsArgs& a, int ref_kind, bool ssim, hipStream_t s) {
  const dim3 grid((unsigned)((a.total + a.per - 1) / a.per)), block(256);
#define HMGPU_METRICS_CASE(R, S) \
  if (ref_kind == R && ssim == S) hipLaunchKernelGGL((k_metrics<R, S>), grid, block, 0, s, a);
  HMGPU_METRICS_CASE(0, false) HMGPU_METRICS_CASE(0, true)
  HMGPU_METRICS_CASE(1, false) HMGPU_METRICS_CASE(1, true)
  HMGPU_METRICS_CASE(2, false) HMGPU_METRICS_CASE(2, true)
#undef HMGPU_METRICS_CASE
}

}  // namespace hmgpu
