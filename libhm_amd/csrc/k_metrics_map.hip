// k_metrics_map.hip -- the sums of k_metrics.hip kept per block instead of per picture (hmgpu_pictures_metrics_map, include/hmgpu.h
// "picture metric maps"): per picture, component and block of B x B luma samples SSE, SAD, differing samples, max |d|
// and the SSIM windows that start in the block, all exact integers.
// One launch, no zeroing and no global atomics: a workgroup owns one region of 64 x 64 luma samples from the crop origin -- one block
// of the largest size, (64 / B)^2 whole blocks of any -- or the matching (64 >> csx) x (64 >> csy) positions of the pair plane, which
// gives Cb and Cr of a group from one 16-byte load.  It writes every map element of its region exactly once with plain stores, so the
// map is a function of the inputs alone and nothing between rows, fields and pictures of a padded destination is touched.
// Pass 1, the loads: lanes laid out by 4x4 cell as in k_metrics<R, true> -- lanes 4k .. 4k + 3 hold the four rows of cell k -- so two
// __shfl_xor steps give a cell's sums, written once to LDS: the distortion terms of the region's cells, and with SSIM the block sums
// (metrics_core.h) of the region and of its 4-sample apron right and below, which stays out of the distortion.
// Pass 2, one thread per cell, block-major: it adds the window that starts at its cell (the picture's own windows: their top-left at
// (4i, 4j) of the cropped plane, counted where that sample lies), then the cells of a block meet by __shfl_xor over log2(cells per
// block) steps -- blocks of more than 64 cells through LDS, once per wave -- and the first thread of each block stores its elements.
#include "hmgpu_dev.h"
#include "metrics_core.h"

namespace hmgpu {

namespace {

constexpr int kMaxCells = (kMapRegion / 4) * (kMapRegion / 4);                    // 4x4 cells of a region: 256, one per thread
constexpr int kMaxSums = (kMapRegion / 4 + 1) * (kMapRegion / 4 + 1);            // with the apron: 17 x 17

struct CellDist { u64 sse; uint32_t sad, dm; };      // of one 4x4 cell: sum d^2, sum |d|, max |d| << 16 | samples with d != 0
struct BlockAcc {                                    // what pass 2 reduces, per component
  u64 sse; long long ssim;
  uint32_t sad, max_abs, counts;                     // counts: differing << 16 | windows (4096 and 256 per region at most)
};

__device__ inline void acc_add(BlockAcc& v, int m) {
  v.sse += xor64(v.sse, m);
  v.ssim += (long long)xor64((u64)v.ssim, m);
  v.sad += xor32(v.sad, m);
  v.counts += xor32(v.counts, m);
  v.max_abs = max(v.max_abs, xor32(v.max_abs, m));
}

// cells per row of pass 1's layout: a constant divisor for each of the four widths
__device__ inline int cell_row(int b4, int nbx) { return nbx == 17 ? b4 / 17 : nbx == 9 ? b4 / 9 : nbx == 16 ? b4 >> 4 : b4 >> 3; }

template <int REF, bool SSIM, int CLS>
__device__ inline void region_pass(const MetricsMapArgs& a, int pic, int region, BlockSum* blk, CellDist (*dist)[kMaxCells],
                                   BlockAcc (*red)[2]) {
  constexpr int NC = CLS + 1;
  const int w = a.w[CLS], h = a.h[CLS], pitch = a.pitch[CLS];
  const int lrw = CLS ? a.log2_rw[1] : 6, lrh = CLS ? a.log2_rh[1] : 6;       // (the luma region is a constant: its passes unroll)
  const int cxn = 1 << (lrw - 2), cyn = 1 << (lrh - 2);                       // cells of the region
  const int nbx = cxn + (SSIM ? 1 : 0), nby = cyn + (SSIM ? 1 : 0);           // cells pass 1 loads
  const int units = nbx * nby * 4;
  const int rx0 = (region % a.regions_x[CLS]) << lrw, ry0 = (region / a.regions_x[CLS]) << lrh;
  const int16_t* const pa = a.a[pic][CLS];
  const int16_t* const pb = a.bp[pic][CLS];
  const bool avec = (a.avec[CLS] >> pic) & 1;
  const int tid = threadIdx.x;
#pragma unroll
  for (int pass = 0; pass * 256 < units; pass++) {
    const int u = tid + 256 * pass;
    const int b4 = u >> 2;
    const int cy = cell_row(b4, nbx), cx = b4 - cy * nbx;
    const int x = rx0 + 4 * cx, y = ry0 + 4 * cy + (u & 3);
    const bool core = cx < cxn && cy < cyn;
    const bool live = u < units && x < w && y < h;
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
    for (int k = 0; k < NC; k++) {
      // per group of 4: |d| < 2^16, so the squares are 24-bit multiplies and the sums of a cell fit 32 bits but for the squares.  The
      // rows outside the plane and the apron add nothing
      uint32_t sad = 0, top = 0, differ = 0;
      u64 sse = 0;
      if (core) {
        uint32_t ad[4];
        for (int j = 0; j < 4; j++) {
          const int d = va[k][j] - vb[k][j];
          ad[j] = (uint32_t)(d < 0 ? -d : d);
          differ += ad[j] ? 1u : 0u;
          sad += ad[j];
          top = max(top, ad[j]);
        }
        sse = ((u64)mul24(ad[0], ad[0]) + (u64)mul24(ad[1], ad[1])) + ((u64)mul24(ad[2], ad[2]) + (u64)mul24(ad[3], ad[3]));
      }
      for (int m = 1; m <= 2; m <<= 1) { sse += xor64(sse, m); sad += xor32(sad, m); differ += xor32(differ, m); top = max(top, xor32(top, m)); }
      if ((u & 3) == 0 && u < units && core) { CellDist& o = dist[k][(cy << (lrw - 2)) + cx]; o.sse = sse; o.sad = sad; o.dm = top << 16 | differ; }
      if (SSIM) {
        const BlockSum sums = block_sums(va[k], vb[k]);
        if ((u & 3) == 0 && u < units) blk[k * kMaxSums + cy * nbx + cx] = sums;
      }
    }
  }
  __syncthreads();
  // pass 2: thread t is cell (wx, wy) of block (bx, by) of the region, the cells of a block in consecutive threads
  const int lbx = a.log2_bw[CLS] - 2, lby = a.log2_bh[CLS] - 2, lcpb = lbx + lby, lnb = a.log2_nb;
  const int bl = tid >> lcpb, within = tid & ((1 << lcpb) - 1);
  const int bx = bl & ((1 << lnb) - 1), by = bl >> lnb;
  const int cx = (bx << lbx) + (within & ((1 << lbx) - 1)), cy = (by << lby) + (within >> lbx);
  const bool active = tid < cxn * cyn;
  BlockAcc acc[NC];
  for (int k = 0; k < NC; k++) {
    BlockAcc& v = acc[k];
    v.sse = 0; v.ssim = 0; v.sad = v.max_abs = v.counts = 0;
    if (!active) continue;
    const CellDist& d = dist[k][(cy << (lrw - 2)) + cx];
    v.sse = d.sse; v.sad = d.sad; v.max_abs = d.dm >> 16; v.counts = (d.dm & 0xffff) << 16;
    if (SSIM && rx0 + 4 * cx + 8 <= w && ry0 + 4 * cy + 8 <= h) {
      v.ssim = window_q32(&blk[k * kMaxSums + cy * nbx + cx], 1, nbx, a.c1[CLS], a.c2[CLS]);
      v.counts += 1;
    }
  }
  for (int s = 0; s < min(lcpb, 6); s++)
    for (int k = 0; k < NC; k++) acc_add(acc[k], 1 << s);
  if (lcpb > 6) {                          // a block of 2 or 4 waves (uniform over the workgroup)
    if ((tid & 63) == 0)
      for (int k = 0; k < NC; k++) red[tid >> 6][k] = acc[k];
    __syncthreads();
    if (within == 0)
      for (int q = 1; q < (1 << (lcpb - 6)); q++)
        for (int k = 0; k < NC; k++) {
          const BlockAcc& o = red[(tid >> 6) + q][k];
          acc[k].sse += o.sse; acc[k].ssim += o.ssim; acc[k].sad += o.sad; acc[k].counts += o.counts; acc[k].max_abs = max(acc[k].max_abs, o.max_abs);
        }
  }
  const int gbx = ((region % a.regions_x[CLS]) << lnb) + bx, gby = ((region / a.regions_x[CLS]) << lnb) + by;
  if (active && within == 0 && gbx < a.blocks_x && gby < a.blocks_y) {
    for (int k = 0; k < NC; k++) {
      const int c = CLS + k;
      if (!((a.comps >> c) & 1)) continue;
      uint8_t* const p = a.maps[c] + pic * a.mbstride[c] + gby * a.mpitch[c] + (int64_t)gbx * 8;
      const int64_t fs = a.mfstride[c];
      const BlockAcc& v = acc[k];
      *reinterpret_cast<long long*>(p) = (long long)v.sse;
      *reinterpret_cast<long long*>(p + fs) = (long long)v.sad;
      *reinterpret_cast<long long*>(p + 2 * fs) = (long long)(v.counts >> 16);
      *reinterpret_cast<long long*>(p + 3 * fs) = (long long)v.max_abs;
      if (SSIM) {
        *reinterpret_cast<long long*>(p + 4 * fs) = v.ssim;
        *reinterpret_cast<long long*>(p + 5 * fs) = (long long)(v.counts & 0xffff);
      }
    }
  }
}

}  // namespace

template <int REF, bool SSIM>
__global__ void __launch_bounds__(256) k_metrics_map(const MetricsMapArgs a) {
  __shared__ BlockSum blk[SSIM ? 2 * kMaxSums : 1];          // component k at k * kMaxSums
  __shared__ CellDist dist[2][kMaxCells];
  __shared__ BlockAcc red[4][2];
  const int per_pic = a.regions[0] + a.regions[1];
  const int item = blockIdx.x;
  const int pic = item / per_pic, r = item - pic * per_pic;
  if (r < a.regions[0]) region_pass<REF, SSIM, 0>(a, pic, r, blk, dist, red);
  else region_pass<REF, SSIM, 1>(a, pic, r - a.regions[0], blk, dist, red);
}

void launch_metrics_map(const MetricsMapArgs& a, int ref_kind, bool ssim, hipStream_t s) {
  const dim3 grid((unsigned)(a.n * (a.regions[0] + a.regions[1]))), block(256);
#define HMGPU_METRICS_MAP_CASE(R, S) \
  if (ref_kind == R && ssim == S) hipLaunchKernelGGL((k_metrics_map<R, S>), grid, block, 0, s, a);
  HMGPU_METRICS_MAP_CASE(0, false) HMGPU_METRICS_MAP_CASE(0, true)
  HMGPU_METRICS_MAP_CASE(1, false) HMGPU_METRICS_MAP_CASE(1, true)
  HMGPU_METRICS_MAP_CASE(2, false) HMGPU_METRICS_MAP_CASE(2, true)
#undef HMGPU_METRICS_MAP_CASE
}

}  // namespace hmgpu
