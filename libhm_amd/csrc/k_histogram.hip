// k_histogram.hip -- what finished pictures contain (hmgpu_pictures_histogram, include/hmgpu.h "picture histograms"): per
// picture and channel (Y, Cb, Cr, maxRGB) a histogram of the sample values and a record of samples, sum, sum of squares, min and max,
// all exact integers.
// One pass, bound by its reads and by the LDS atomics: the plain instance of k_metrics.hip over one picture.  A workgroup walks a
// contiguous run of 256 x 8 tiles (HistogramArgs) with one lane per group of 4 samples of a row -- 8-byte loads on luma, 16-byte ones
// on the chroma pair plane, which give Cb and Cr of a group at once; sample by sample where the crop leaves a group unaligned or the row
// ends inside it.  Plane class 0 counts Y and maxRGB of a luma sample together (one luma load for both; the maxRGB instance adds the
// chroma of the same samples and k_export's conversion, export_core.h export_rgb), class 1 Cb and Cr.
// The histogram of a workgroup's run lives in the LDS, 2^b_c counts per channel of the class (2 x 16 KB at 12 bits): zeroed once, filled
// with ds_add_u32, and its nonzero bins flushed -- global atomicAdd on uint32 -- once per workgroup and (picture, class), which zeroes
// them for the next.  Moments and extrema stay in registers across the tiles and go the way of k_metrics: wave reduction by __shfl_xor,
// the four waves through LDS, one set of atomics per workgroup and record.  All of it is integer sums, min and max, so the arrival
// order does not show.  min travels as ~v through atomicMax on the zeroed record; the last workgroup to arrive at a record (a ticket in
// its first reserved word, which it leaves 0) turns it back.
// Flat content sends all 64 lanes of a wave to one LDS word; a wave whose lanes all hold whole groups of one bin adds their count from
// one lane (count()).  Sixteen 2160p 4:2:0 10-bit pictures, Y + Cb + Cr, us per call: 299 natural-like / 292 flat with it, 264 / 1098
// without (DESIGN.md §9n has the table).
// gfx950, build.py's flags: k_histogram<false> 61 VGPRs, k_histogram<true> (maxRGB) 71; 32 928 bytes of LDS each (2 x 4096 bins and the
// hand-over), which leaves room for four workgroups per CU: kHistGrid; no vector register spills, no scratch.
#include "hmgpu_dev.h"
#include "export_core.h"

namespace hmgpu {

namespace {

typedef unsigned long long u64;

constexpr int kUnits = kHistTileW / 4 * kHistTileH;   // groups of 4 samples of a tile, row-major: 512

struct Acc {                      // what one lane has seen of one channel since the last hand-over
  u64 sum, sq;
  uint32_t samples, lo, hi;       // lo: ~0u: none
};

__device__ inline void acc_clear(Acc& c) { c.sum = c.sq = 0; c.samples = 0; c.lo = ~0u; c.hi = 0; }
__device__ inline uint32_t xor32(uint32_t v, int m) { return (uint32_t)__shfl_xor((int)v, m, 64); }
__device__ inline u64 xor64(u64 v, int m) { return ((u64)xor32((uint32_t)(v >> 32), m) << 32) | xor32((uint32_t)v, m); }
__device__ inline u64 wave_sum(u64 v) { for (int m = 32; m; m >>= 1) v += xor64(v, m); return v; }
__device__ inline uint32_t wave_min(uint32_t v) { for (int m = 32; m; m >>= 1) v = min(v, xor32(v, m)); return v; }
__device__ inline uint32_t wave_max(uint32_t v) { for (int m = 32; m; m >>= 1) v = max(v, xor32(v, m)); return v; }

// the channel of slot k of a class: Y, maxRGB; Cb, Cr
__device__ inline int channel_of(int cls, int k) { return cls ? 1 + k : 3 * k; }

// nv values of channel c into the lane's sums and the workgroup's bins.  Where every lane of the wave has a whole group and all
// of their values fall into one bin -- flat content: black frames, letterbox bars --, one lane adds the count of all of them; 64 lanes
// adding to one LDS word take 64 turns.
__device__ inline void count(const HistogramArgs& a, int c, const int v[4], int nv, Acc& acc, uint32_t* bins) {
  const int sh = a.shift[c];
  uint32_t s = 0, q = 0, b[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint32_t x = (uint32_t)v[j];
    b[j] = (x >> sh) & (kHistMaxBins - 1);                            // (the mask: a sample outside its depth stays inside the LDS)
    if (j >= nv) continue;
    s += x; q += x * x;                                              // x < 2^12: a group's sums fit 32 bits
    acc.lo = min(acc.lo, x); acc.hi = max(acc.hi, x);
  }
  acc.sum += s; acc.sq += q; acc.samples += (uint32_t)nv;
  if (!a.do_hist) return;
  {
    const bool same = nv == 4 && b[0] == b[1] && b[1] == b[2] && b[2] == b[3] && b[0] == (uint32_t)__builtin_amdgcn_readfirstlane((int)b[0]);
    if (__all(same)) {
      const unsigned long long active = __ballot(1);
      if ((int)(threadIdx.x & 63) == __ffsll(active) - 1) atomicAdd(&bins[b[0]], 4u * (uint32_t)__popcll(active));
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (j < nv) atomicAdd(&bins[b[j]], 1u);
}

// the samples of one group at (x, y) of picture `pic`, nv of them, as they lie in memory.  y: four luma samples (class 0).  p: four
// Cb | Cr << 16 pairs -- the group's own (class 1), or in the maxRGB instance the chroma of the group's four luma samples, replicated as
// the export does (one pair for two of them when csx = 1).  A pair is 4-byte aligned wherever the crop starts.  Sample by sample, the
// entries beyond nv repeat the last sample of the row (nothing is read beyond it) and are not counted.
struct Group { int y[4]; uint32_t p[4]; };
// (every branch assigns plain values and the group is put together once at the end: with stores into the arrays under the branches the
// compiler merged them into one store at a run-time address, which put the arrays into scratch)
template <bool RGB, int CLS>
__device__ inline Group load_group(const HistogramArgs& a, int pic, int x, int y, int nv, uint32_t mid) {
  const bool whole = nv == 4;
  const int j1 = min(1, nv - 1), j2 = min(2, nv - 1), j3 = min(3, nv - 1);
  int y0 = 0, y1 = 0, y2 = 0, y3 = 0;
  uint32_t p0 = mid, p1 = mid, p2 = mid, p3 = mid;
  if (CLS == 1) {
    const int16_t* p = a.c[pic] + (ptrdiff_t)y * a.pitch[1] + kCStep * x;
    if (whole && ((a.cvec >> pic) & 1)) {
      const u32x4 q = ldg4(p);
      p0 = q.x; p1 = q.y; p2 = q.z; p3 = q.w;
    } else {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
      p0 = ldg(q); p1 = ldg(q + j1); p2 = ldg(q + j2); p3 = ldg(q + j3);
    }
  } else {
    const int16_t* p = a.y[pic] + (ptrdiff_t)y * a.pitch[0] + x;
    if (whole && ((a.yvec >> pic) & 1)) {
      const u32x2 q = ldg2(p);
      y0 = (int16_t)(q.x & 0xffff); y1 = (int16_t)(q.x >> 16); y2 = (int16_t)(q.y & 0xffff); y3 = (int16_t)(q.y >> 16);
    } else {
      y0 = ldg(p); y1 = ldg(p + j1); y2 = ldg(p + j2); y3 = ldg(p + j3);
    }
    if (RGB && !a.mono) {
      const uint32_t* cp = reinterpret_cast<const uint32_t*>(a.c[pic] + (ptrdiff_t)(y >> a.csy) * a.pitch[1] + kCStep * (x >> a.csx));
      if (whole && ((a.rvec >> pic) & 1)) {
        if (a.csx) {
          const u32x2 q = ldg2(cp);
          p0 = p1 = q.x; p2 = p3 = q.y;
        } else {
          const u32x4 q = ldg4(cp);
          p0 = q.x; p1 = q.y; p2 = q.z; p3 = q.w;
        }
      } else {
        p0 = ldg(cp); p1 = ldg(cp + (j1 >> a.csx)); p2 = ldg(cp + (j2 >> a.csx)); p3 = ldg(cp + (j3 >> a.csx));
      }
    }
  }
  const Group g = {{y0, y1, y2, y3}, {p0, p1, p2, p3}};
  return g;
}

// One tile of plane class CLS of picture `pic`: the loads of a lane's two groups are issued before either is counted
template <bool RGB, int CLS>
__device__ inline void tile_pass(const HistogramArgs& a, int pic, int tile, Acc acc[2], uint32_t (*bins)[kHistMaxBins]) {
  constexpr int PASSES = kUnits / 256;
  const int w = a.w[CLS], h = a.h[CLS];
  const int tx0 = (tile % a.tiles_x[CLS]) * kHistTileW, ty0 = (tile / a.tiles_x[CLS]) * kHistTileH;
  const int tid = threadIdx.x;
  const uint32_t mid = (uint32_t)a.coef[3] * 0x10001u;                 // 4:0:0: Cb = Cr = mid
  int nv[PASSES];
  Group g[PASSES];
#pragma unroll
  for (int pass = 0; pass < PASSES; pass++) {
    const int u = tid + 256 * pass;
    const int x = tx0 + 4 * (u & (kHistTileW / 4 - 1)), y = ty0 + u / (kHistTileW / 4);
    nv[pass] = x < w && y < h ? min(4, w - x) : 0;                     // 0: the group lies outside the plane
    if (nv[pass]) g[pass] = load_group<RGB, CLS>(a, pic, x, y, nv[pass], mid);
  }
#pragma unroll
  for (int pass = 0; pass < PASSES; pass++) {
    if (!nv[pass]) continue;
    int v[4];
    if (CLS == 1) {
      if (a.chans & 2) {
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = (int16_t)(g[pass].p[j] & 0xffff);
        count(a, 1, v, nv[pass], acc[0], bins[0]);
      }
      if (a.chans & 4) {
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = (int16_t)(g[pass].p[j] >> 16);
        count(a, 2, v, nv[pass], acc[1], bins[1]);
      }
    } else {
      if (RGB) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          uint32_t R, G, B;
          const int u = (int16_t)(g[pass].p[j] & 0xffff), w = (int16_t)(g[pass].p[j] >> 16);
          export_rgb<1>(a, &g[pass].y[j], &u, &w, &R, &G, &B);
          v[j] = (int)max(R, max(G, B));
        }
        count(a, 3, v, nv[pass], acc[1], bins[1]);
      }
      if (a.chans & 1) count(a, 0, g[pass].y, nv[pass], acc[0], bins[0]);
    }
  }
}

// the workgroup's bins and sums of class `cls` of picture `pic` into the histograms and records, then the ticket: `last` workgroups
// hand over to this class.  Leaves the bins zero.
__device__ inline void hand_over(const HistogramArgs& a, int pic, int cls, Acc acc[2], uint32_t (*bins)[kHistMaxBins], u64 (*red)[5], int last) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __syncthreads();                                                   // every lane's counts are in the bins
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int c = channel_of(cls, k);
    if (!((a.chans >> c) & 1)) continue;
    if (a.do_hist) {
      uint32_t* g = reinterpret_cast<uint32_t*>(a.hist[c] + pic * a.hstride[c]);
      const int nb = 1 << a.log2_bins[c];
      for (int b = tid; b < nb; b += 256) {
        const uint32_t cnt = bins[k][b];
        if (cnt) { atomicAdd(g + b, cnt); bins[k][b] = 0; }
      }
    }
    const Acc& v = acc[k];
    const u64 r[5] = {wave_sum(v.samples), wave_sum(v.sum), wave_sum(v.sq), (u64)wave_min(v.lo), (u64)wave_max(v.hi)};
    __syncthreads();
    if (lane == 0)
      for (int f = 0; f < 5; f++) red[wave][f] = r[f];
    __syncthreads();
    if (tid == 0) {
      u64 t[5];
      for (int f = 0; f < 5; f++) t[f] = red[0][f];
      for (int q = 1; q < 4; q++) {
        for (int f = 0; f < 3; f++) t[f] += red[q][f];
        t[3] = red[q][3] < t[3] ? red[q][3] : t[3];
        t[4] = red[q][4] > t[4] ? red[q][4] : t[4];
      }
      u64* rec = reinterpret_cast<u64*>(a.records + pic * a.rstride + c * 64);
      uint32_t* tail = reinterpret_cast<uint32_t*>(rec + 3);        // min, max, then the reserved words: the first is the ticket
      atomicAdd(rec + 0, t[0]); atomicAdd(rec + 1, t[1]); atomicAdd(rec + 2, t[2]);
      atomicMax(tail + 0, ~(uint32_t)t[3]);
      atomicMax(tail + 1, (uint32_t)t[4]);
      __threadfence();
      if (atomicAdd(tail + 2, 1u) == (uint32_t)(last - 1)) {        // every other workgroup of this record has handed over
        __threadfence();
        const uint32_t key = atomicAdd(tail + 0, 0u);
        atomicExch(tail + 0, ~key);
        atomicExch(tail + 2, 0u);
      }
    }
  }
  __syncthreads();                                                   // the bins are zero before the next tile counts
}

}  // namespace

template <bool RGB>
__global__ void __launch_bounds__(256) k_histogram(const HistogramArgs a) {
  __shared__ uint32_t bins[2][kHistMaxBins];
  __shared__ u64 red[4][5];
  for (int b = threadIdx.x; b < 2 * kHistMaxBins; b += 256) (&bins[0][0])[b] = 0;
  Acc acc[2];
  acc_clear(acc[0]); acc_clear(acc[1]);
  const int per_pic = a.tiles[0] + a.tiles[1];
  const int first = blockIdx.x * a.per, end = min(first + a.per, a.total);
  int cur = -1;                           // picture * 2 + class of the sums held
  __syncthreads();
  for (int item = first; item < end; item++) {
    const int pic = item / per_pic, r = item - pic * per_pic;
    const int cls = r >= a.tiles[0] ? 1 : 0;
    const int key = pic * 2 + cls;
    if (key != cur) {
      if (cur >= 0) {
        // the workgroups whose runs meet the items of (picture, class) cur: every one of them computes the same count
        const int s = (cur >> 1) * per_pic + ((cur & 1) ? a.tiles[0] : 0), e = s + a.tiles[cur & 1];
        hand_over(a, cur >> 1, cur & 1, acc, bins, red, (e - 1) / a.per - s / a.per + 1);
        acc_clear(acc[0]); acc_clear(acc[1]);
      }
      cur = key;
    }
    if (cls == 0) tile_pass<RGB, 0>(a, pic, r, acc, bins);
    else tile_pass<RGB, 1>(a, pic, r - a.tiles[0], acc, bins);
  }
  if (cur >= 0) {
    const int s = (cur >> 1) * per_pic + ((cur & 1) ? a.tiles[0] : 0), e = s + a.tiles[cur & 1];
    hand_over(a, cur >> 1, cur & 1, acc, bins, red, (e - 1) / a.per - s / a.per + 1);
  }
}

void launch_histogram(const HistogramArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)((a.total + a.per - 1) / a.per)), block(256);
  if (a.chans & 8) hipLaunchKernelGGL((k_histogram<true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_histogram<false>), grid, block, 0, s, a);
}

}  // namespace hmgpu
