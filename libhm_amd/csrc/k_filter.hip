// k_filter.hip -- deblocking of both edge directions and SAO in ONE pass over the picture
// (TComLoopFilter::loopFilterPic + TComSampleAdaptiveOffset::SAOProcess, TDecGop.cpp:165-173).
//
// The stand-alone kernels (k_dbk.hip x 2, k_sao.hip) each stream the whole picture through HBM: ~1.0 GB of real traffic per
// batch of eight 2160p pictures, at 85-100 % of the achievable bandwidth -- the remaining lever is to move fewer bytes.
// Here a workgroup owns a 64x64 luma tile (+ the 32x32 tiles of Cb and Cr), loads it ONCE with the halo the filters reach
// through, runs vertical-edge deblocking, horizontal-edge deblocking and SAO on the copy in LDS, and writes only the SAO
// planes: read ~1.5 x picture + BlkInfo, write 1 x picture.  The deblocked picture itself is never stored (with SAO on, the
// SAO planes are the picture's final planes; pictures without SAO take the stand-alone path).  A tile on the picture's edge also
// writes the margins beside it (TComPicYuv::extendPicBorder, step 5 of the kernel): the finished picture needs no pass of k_extend.
//
// Halo arithmetic (luma; chroma is the same at half scale with a 1-sample filter): SAO of the tile needs deblocked samples
// one sample around it; a deblocked sample belongs to exactly one edge per direction (edges lie on the 8x8 grid, an edge
// rewrites 3 samples on each side and reads 4); so the horizontal edges y0, y0+8 .. y0+64 must be filtered over the columns
// [x0-4, x0+68), on input that has seen the vertical edges x0 .. x0+64 over the rows [y0-4, y0+68), which read the
// unfiltered columns [x0-4, x0+68).  Edge units on a tile border are computed by both neighbours, from the same unfiltered
// samples, hence identically.  Every decision and every filter is the code of the stand-alone kernels (filter_core.h).
#include "hmgpu_dev.h"
#include "filter_core.h"
#include <type_traits>

namespace hmgpu {

namespace {
constexpr int kTW = 64, kTH = 64;                 // luma tile
constexpr int kYC = kTW + 16, kYH = kTH + 8;      // luma copy: columns [x0-8, x0+72) (16-byte aligned rows), rows [y0-4, y0+68)
constexpr int kCC = kTW / 2 + 16, kCH = kTH / 2 + 4;   // chroma copy: columns [cx0-8, cx0+40), rows [cy0-2, cy0+34)
constexpr int kYW = kYC + 8, kCW = kCC + 8;       // row pitch in LDS: an odd number of 16-byte units (conflict-free 16-byte row accesses)

constexpr int kUnits = 9 * 18;                     // edge units of one direction per tile (see k_filter_fused)
struct FilterLds {
  __attribute__((aligned(16))) int16_t y[kYH][kYW];
  __attribute__((aligned(16))) int16_t c[2][kCH][kCW];
  // the edge units that really filter (Bs > 0), compacted per classifying wave: [direction][wave][slot] and their counts
  uint32_t unit[2][3][64];
  int32_t units[2][4];
};

// What the kernel reads of a picture's PicDev and of its slice 0, fetched ONCE at kernel entry through the constant address space: the
// descriptor is the same for the whole workgroup, so these are scalar loads (merged by the struct's layout) issued together and waited
// for once, before the first vector address is formed; from then on the values sit in SGPRs and no branch fetches a field again.
// (Nothing on the device writes a PicDev or the slice table while the filter runs.)
struct SliceLf { int tc_off, beta_off, cb_off, cr_off; };     // the deblocking constants of one slice
struct FPic {
  static constexpr int csx = 1, csy = 1;                      // the fused kernel runs on 4:2:0-shaped pictures only (run_filter)
  int width, height, bd0, bd1, bd2, log2ctu, ctus_w, pitch[2], mx, my, grid_w, any_nofilt, mono;   // mx, my: the luma margins (border tiles)
  __device__ inline int bd(int comp) const { return comp == 0 ? bd0 : comp == 1 ? bd1 : bd2; }   // (no array: a lane's component is a run-time value)
  const int16_t* rec[2];
  int16_t* sao[2];
  const uint16_t* slice_idx;
  const SliceDev* slices;
  const BlkInfo* blk;
  const EdgeRec* edges;
  const SaoDev* saoprm;
  SliceLf s0;
};
template <typename T> __device__ inline T ldc(const T* p) { return *(const T __attribute__((address_space(4)))*)p; }
__device__ inline FPic pic_state(const PicDev* p) {
  FPic f;
  f.width = ldc(&p->width); f.height = ldc(&p->height);
  f.bd0 = ldc(&p->bd[0]); f.bd1 = ldc(&p->bd[1]); f.bd2 = ldc(&p->bd[2]);
  f.log2ctu = ldc(&p->log2ctu); f.ctus_w = ldc(&p->ctus_w);
  f.pitch[0] = ldc(&p->pitch[0]); f.pitch[1] = ldc(&p->pitch[1]);
  f.mx = ldc(&p->mx[0]); f.my = ldc(&p->my[0]);
  f.grid_w = ldc(&p->grid_w);
  f.rec[0] = ldc(&p->rec[0]); f.rec[1] = ldc(&p->rec[1]);
  f.sao[0] = ldc(&p->sao[0]); f.sao[1] = ldc(&p->sao[1]);
  f.any_nofilt = ldc(&p->any_nofilt); f.mono = ldc(&p->mono);
  f.slice_idx = ldc(&p->slice_idx); f.slices = ldc(&p->slices);
  f.blk = ldc(&p->blk); f.edges = ldc(&p->edges); f.saoprm = ldc(&p->saoprm);
  const SliceDev* s = f.slices;
  f.s0 = {ldc(&s->tc_offset_div2), ldc(&s->beta_offset_div2), ldc(&s->pps_cb_qp_offset), ldc(&s->pps_cr_qp_offset)};
  return f;
}

// Per-lane memory accesses go through buffer descriptors: a 64-bit base that is the same for the whole workgroup (the tile's first
// row of a plane, the tile's first cell of a grid; SGPRs) plus a 32-bit byte offset per lane, bounded by the tile's own extent, so no
// picture size limit arises.  The descriptor's size is exactly what the tile may touch: a lane with nothing to fetch asks at that
// offset -- the range check answers with zeros and nothing goes to memory (as k_mc.hip does for idle lanes), so no load is predicated
// and all of a thread's loads can be in flight together.
struct Span {
  __amdgpu_buffer_rsrc_t rs;
  uint32_t bytes;                                              // the offset of "nowhere"
  __device__ inline Span(const void* base, uint32_t n) : rs(__builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, n, 0x00020000)), bytes(n) {}
  __device__ inline uint32_t at(bool valid, uint32_t off) const { return valid ? off : bytes; }
  __device__ inline u32x4 load4(uint32_t off) const { return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0)); }
  __device__ inline uint32_t load_u16(uint32_t off) const { return (uint16_t)__builtin_amdgcn_raw_buffer_load_b16(rs, off, 0, 0); }
  __device__ inline void store4(uint32_t off, u32x4 v) const { __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(decltype(__builtin_amdgcn_raw_buffer_load_b128(rs, 0, 0, 0)), v), rs, off, 0, 0); }
};

// SaoDev as three dwords
struct SaoPrm { uint32_t w0, off_lo, off_hi; };
__device__ inline SaoPrm sao_fetch(const Span& sp, uint32_t off) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b96(sp.rs, off, 0, 0);
  return {(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]};
}

// SAO of one group of 8 samples at (x, row) of component comp, reading the deblocked copy; (ox, oy) = picture coordinates
// of copy element [0][0]
// returns the group's eight output samples (the caller stores them: luma as they are, chroma paired with the other component's)
template <int W, bool NF>
__device__ inline u32x4 sao_group(const FPic& P, int comp, const int16_t (*t)[W], int ox, int oy, int x, int row, const SaoPrm& prm) {
  const int cs = comp ? 1 : 0;
  const int w = P.width >> cs, h = P.height >> cs;
  const int log2ctb = P.log2ctu - cs;
  const int cx = x >> log2ctb, cy = row >> log2ctb;
  const uint32_t w0 = prm.w0;
  const int type = (int)(int8_t)(w0 & 0xff);
  const int16_t* line = &t[row - oy][x - ox];
  const u32x4 cur = *reinterpret_cast<const u32x4*>(line);
  if (type < 0) return cur;
  const uint32_t off_lo = prm.off_lo, off_hi = prm.off_hi;
  const int bd = P.bd(comp), maxv = (1 << bd) - 1;
  uint32_t out[4];
  if (type == HMGPU_SAO_BO) {
    const int shift = bd - 5, band0 = (w0 >> 8) & 0xff;
    const uint32_t c[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t lo = c[j] & 0xffffu, hi = c[j] >> 16;
      const uint32_t k0 = min(((lo >> shift) - band0) & 31u, 4u), k1 = min(((hi >> shift) - band0) & 31u, 4u);
      const s16x2 off = lut_offsets(k0 | (k1 << 16), off_lo, 0u);
      out[j] = as_u32(__builtin_elementwise_min(__builtin_elementwise_max(as_s16x2(c[j]) + off, splat(0)), splat(maxv)));
    }
  } else {
    const int ctb = 1 << log2ctb;
    const int x0 = cx << log2ctb, y0 = cy << log2ctb;
    const int x1 = min(x0 + ctb, w) - 1, y1 = min(y0 + ctb, h) - 1;
    const unsigned av = w0 >> 16;
    // neighbour rows straight from the copy (its halo holds the deblocked samples around the tile; positions outside the
    // picture hold margin samples, which the availability mask never lets through)
    auto run = [&](auto dxc, auto dyc) {
      constexpr int DX = decltype(dxc)::value, DY = decltype(dyc)::value;
      const int16_t* ra = line + DY * W;
      const int16_t* rb = line - DY * W;
      const u32x4 ea = *reinterpret_cast<const u32x4*>(ra), eb = *reinterpret_cast<const u32x4*>(rb);
      uint32_t na[4], nb[4];
      uint32_t la = 0, raa = 0, lb = 0, rbb = 0;
      if constexpr (DX < 0) { la = (uint16_t)ra[-1]; rbb = (uint16_t)rb[8]; }
      if constexpr (DX > 0) { raa = (uint16_t)ra[8]; lb = (uint16_t)rb[-1]; }
      shifted<DX>(ea, la, raa, na);
      shifted<-DX>(eb, lb, rbb, nb);
      sao_eo_core<DX, DY>(x, row, cur, na, nb, off_lo, off_hi, av, x0, y0, x1, y1, maxv, out);
    };
    switch (type) {
      case HMGPU_SAO_EO_0:   run(std::integral_constant<int, -1>{}, std::integral_constant<int, 0>{}); break;
      case HMGPU_SAO_EO_90:  run(std::integral_constant<int, 0>{}, std::integral_constant<int, -1>{}); break;
      case HMGPU_SAO_EO_135: run(std::integral_constant<int, -1>{}, std::integral_constant<int, -1>{}); break;
      default:               run(std::integral_constant<int, 1>{}, std::integral_constant<int, -1>{}); break;
    }
  }
  if (NF && P.any_nofilt) {
    uint32_t m[4];
    sao_exempt_mask(P, comp, x, row, m);
    const uint32_t c[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
    for (int j = 0; j < 4; j++) out[j] = (c[j] & m[j]) | (out[j] & ~m[j]);
  }
  return u32x4{out[0], out[1], out[2], out[3]};
}

// Deblocking runs in two steps so that lanes are spent on real work only: every edge unit of the tile is CLASSIFIED by its
// own thread (edge flags, Bs; most units of large blocks stop here), the units that filter are compacted into a list in LDS
// and APPLIED by the first threads of the block -- a tile of 32x32 CUs keeps one wave busy with the filter arithmetic instead
// of three.  A list entry: unit index | Bs << 8 | P side unfiltered << 10 | Q side unfiltered << 11 | (QP + 64) << 12 |
// Q side's slice << 20.
__device__ inline SliceLf slice_lf(const SliceDev* s) {
  return {ldg(&s->tc_offset_div2), ldg(&s->beta_offset_div2), ldg(&s->pps_cb_qp_offset), ldg(&s->pps_cr_qp_offset)};
}
static_assert(HMGPU_MAX_SLICES <= 4096, "slice index must fit the 12 bits of a list entry");

// unit u of the tile with EdgeRec unit `rec` (0: not filtered; k_prep: Bs, mean QP, exemptions) -> list entry.  slice: the one whose
// deblocking constants apply, that of the Q side's CTU (TComLoopFilter.cpp:565-566).  Both were requested at kernel entry: nothing is
// fetched here
template <bool NF>
__device__ inline uint32_t edge_classify(uint32_t rec, uint32_t slice, int u) {
  const uint32_t bs = rec & 3u, qp = (rec >> 2) & 127u;                 // QP + 32
  const uint32_t p_nf = NF ? (rec >> 9) & 1u : 0u, q_nf = NF ? (rec >> 10) & 1u : 0u;
  const uint32_t e = (uint32_t)u | (bs << 8) | (p_nf << 10) | (q_nf << 11) | ((qp + 32u) << 12) | (slice << 20);
  return bs ? e : 0u;
}

// append the wave's active units to its list; called by the three waves that classify
__device__ inline void push_units(uint32_t (&list)[3][64], int32_t (&count)[4], uint32_t rec, int t) {
  const unsigned long long m = __ballot(rec != 0u);
  const int wave = t >> 6, lane = t & 63;
  if (rec != 0u) list[wave][__popcll(m & ((1ull << lane) - 1ull))] = rec;
  if (lane == 0) count[wave] = __popcll(m);
}
__device__ inline uint32_t pop_unit(const uint32_t (&list)[3][64], const int32_t (&count)[4], int t) {
  const int c0 = count[0], c1 = count[1], c2 = count[2];
  if (t < c0) return list[0][t];
  if (t < c0 + c1) return list[1][t - c0];
  if (t < c0 + c1 + c2) return list[2][t - c0 - c1];
  return 0u;
}

// one classified edge unit of direction DIR, filtered on the copies
template <int DIR, bool NF>
__device__ inline void edge_apply(const FPic& P, FilterLds& L, int x0, int y0, uint32_t rec) {
  if (rec == 0u) return;
  const int u = rec & 0xff, bs = (rec >> 8) & 3, qp = (int)((rec >> 12) & 0xff) - 64, slice = rec >> 20;
  const bool p_nf = NF && ((rec >> 10) & 1), q_nf = NF && ((rec >> 11) & 1);
  const int x = DIR == 0 ? x0 + 8 * (u % 9) : x0 - 4 + 4 * (u % 18);
  const int y = DIR == 0 ? y0 - 4 + 4 * (u / 9) : y0 + 8 * (u / 18);
  // offsets come from the Q side's slice (TComLoopFilter.cpp:565-566); slice 0's were fetched at kernel entry
  const SliceLf sl = slice == 0 ? P.s0 : slice_lf(P.slices + slice);
  const int tc_off = sl.tc_off, beta_off = sl.beta_off;
  int16_t* base = &L.y[y - (y0 - 4)][x - (x0 - 8)];
  // the unit as line pairs (filter_core.h): a = lines 0|1, b = lines 2|3, index = position across the edge
  uint32_t a[8], b[8];
  if (DIR == 0) {
    // a line = 8 contiguous samples starting 4 before the edge: 8-byte aligned in the copy
    uint32_t r[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const u32x2 lo = *reinterpret_cast<const u32x2*>(base + i * kYW - 4), hi = *reinterpret_cast<const u32x2*>(base + i * kYW);
      r[i][0] = lo.x; r[i][1] = lo.y; r[i][2] = hi.x; r[i][3] = hi.y;
    }
    rows_to_pairs(r[0], r[1], a);
    rows_to_pairs(r[2], r[3], b);
  } else {
    // position k across the edge = 4 contiguous samples (the four lines): one 8-byte access
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const u32x2 v = *reinterpret_cast<const u32x2*>(base + (k - 4) * kYW);
      a[k] = v.x; b[k] = v.y;
    }
  }
  filter_luma_unit(a, b, bs, qp, tc_off, beta_off, P.bd(0), p_nf, q_nf);
  if (DIR == 0) {
    uint32_t r[4][4];
    pairs_to_rows(a, r[0], r[1]);
    pairs_to_rows(b, r[2], r[3]);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      *reinterpret_cast<u32x2*>(base + i * kYW - 4) = (u32x2){r[i][0], r[i][1]};
      *reinterpret_cast<u32x2*>(base + i * kYW) = (u32x2){r[i][2], r[i][3]};
    }
  } else {
#pragma unroll
    for (int k = 1; k < 7; k++) *reinterpret_cast<u32x2*>(base + (k - 4) * kYW) = (u32x2){a[k], b[k]};
  }
  // chroma: Bs 2 only, edges on the 8-sample chroma grid (TComLoopFilter.cpp:225-229, 684-692, 727)
  if (bs == 2 && ((DIR == 0 ? x : y) & 15) == 0 && !P.mono) {      // (4:0:0: the chroma planes are left alone)
    const int maxc = (1 << P.bd(1)) - 1;
#pragma unroll
    for (int comp = 1; comp < 3; comp++) {
      const int tc = chroma_tc(qp, comp == 1 ? sl.cb_off : sl.cr_off, tc_off, P.bd(comp));
      int16_t* cb = &L.c[comp - 1][(y >> 1) - ((y0 >> 1) - 2)][(x >> 1) - ((x0 >> 1) - 8)];
#pragma unroll
      for (int i = 0; i < 2; i++) {
        int16_t* s = DIR == 0 ? cb + i * kCW : cb + i;
        const int o = DIR == 0 ? 1 : kCW;
        const int m2 = (uint16_t)s[-2 * o], m3 = (uint16_t)s[-o], m4 = (uint16_t)s[0], m5 = (uint16_t)s[o];
        const int delta = clip3(-tc, tc, ((((m4 - m3) << 2) + m2 - m5 + 4) >> 3));
        if (!p_nf) s[-o] = (int16_t)clip3(0, maxc, m3 + delta);              // xPelFilterChroma :883-890
        if (!q_nf) s[0] = (int16_t)clip3(0, maxc, m4 - delta);
      }
    }
  }
}

// The margins a border tile owns (TComPicYuv::extendPicBorder for the SAO planes, byte for byte what extend_plane of k_sao.hip writes):
// `out` is the tile's FINAL samples in LDS (vw x vh valid elements, rows `opitch` int16 apart), `org` the tile's first element in the
// plane.  el / er / et / eb: the tile holds the picture's first / last column, first / last row.  The tile's valid rectangle grows by
// mx columns on the sides it is an edge of and by my rows likewise; every element of the grown rectangle outside the valid one is the
// nearest valid element, and no other tile writes it (left and right bands over the tile's rows, bands above and below over its
// columns, the corner blocks with the corner tiles).  E = int16 elements per picture element (1 luma, kCStep chroma: the (Cb, Cr) pair).
// All 256 threads store 16-byte pieces: 16 lanes along a row of the side bands, 8 along a row of the bands above and below.
template <int E>
__device__ inline void put_margins(const int16_t* out, int opitch, int16_t* org, int pitch, int vw, int vh, bool el, bool er, bool et, bool eb,
                                   int mx, int my, int t) {
  constexpr int VE = 8 / E;                                   // elements per 16-byte vector
  const int xl = el ? mx : 0, yt = et ? my : 0;               // margin columns / rows in front of the tile's first
  const int rows = yt + vh + (eb ? my : 0);
  const Span sm(org - ((ptrdiff_t)yt * pitch + E * xl), (uint32_t)(((rows - 1) * pitch + E * (xl + vw + (er ? mx : 0))) * 2));
  // side bands, corner blocks included: rows of the grown rectangle, every vector a replica of the row's first / last valid element
  const int nl = xl / VE, ns = nl + (er ? mx / VE : 0);
  for (int r = t >> 4; r < rows; r += 16) {
    const int16_t* line = out + clip3(0, vh - 1, r - yt) * opitch;
    for (int k = t & 15; k < ns; k += 16) {
      const bool right = k >= nl;
      const int16_t* e = line + E * (right ? vw - 1 : 0);
      uint32_t v;
      if constexpr (E == 1) v = (uint16_t)e[0] * 0x10001u;
      else v = *reinterpret_cast<const uint32_t*>(e);
      const int x = right ? xl + vw + (k - nl) * VE : k * VE;
      sm.store4((uint32_t)((r * pitch + E * x) * 2), u32x4{v, v, v, v});
    }
  }
  // bands above and below the tile's columns: replicas of its first / last valid row
  const int nt = yt, nb = nt + (eb ? my : 0);
  const int k = t & 7;
  if (k * VE < vw)
    for (int r = t >> 3; r < nb; r += 32) {
      const bool below = r >= nt;
      const u32x4 v = *reinterpret_cast<const u32x4*>(out + (below ? vh - 1 : 0) * opitch + 8 * k);
      sm.store4((uint32_t)(((below ? vh + r : r) * pitch + E * xl + 8 * k) * 2), v);
    }
}

}  // namespace

// NF: the variant for batches in which some picture holds lossless / unfiltered PCM CUs (chosen on the host)
template <bool NF>
__global__ void __launch_bounds__(256) k_filter_fused(const PicDev* __restrict__ pics, Batch b, int tiles_x, int tiles) {
  __shared__ FilterLds L;
  // XCD-aware tile order (xcd_remap): the tiles of one picture (band) run on one XCD in raster order, so that the halo a tile
  // shares with its neighbours -- whole 128-byte lines to the left and right, rows above and below -- is found in that XCD's
  // L2 instead of being fetched from memory once per neighbour (measured: 0.9 GB of reads per batch without)
  int slot, lb;
  if (!xcd_remap(blockIdx.x, b.n, tiles, slot, lb)) return;
  const FPic P = pic_state(pics + b.pic[slot]);
  __builtin_amdgcn_sched_barrier(0);
  const int x0 = (lb % tiles_x) * kTW, y0 = (lb / tiles_x) * kTH;
  const int t = threadIdx.x;
  const int l2 = P.log2ctu, p0 = P.pitch[0], p1 = P.pitch[1];
  // ---- 1. everything the thread reads from memory is requested here, back to back: its edge records with the slice of their Q side's
  // CTU, the tile and its halo before any filtering (pictures carry margins: every address is inside the allocation), the parameters
  // of its SAO groups.  The edge units are classified while the tile flies, then the copy is written.
  // edge units of this thread: vertical edges x0, x0+8 .. x0+64 over the rows [y0-4, y0+68) (9 edges x 18 units), horizontal
  // edges y0 .. y0+64 over the columns [x0-4, x0+68); cells and CTUs are counted from those of (x0-8, y0-8)
  const int vx = x0 + 8 * (t % 9), vy = y0 - 4 + 4 * (t / 9), hx = x0 - 4 + 4 * (t % 18), hy = y0 + 8 * (t / 18);
  const bool vin = t < kUnits && vy >= 0 && vx < P.width && vy < P.height, hin = t < kUnits && hx >= 0 && hx < P.width && hy < P.height;
  const int ecw = P.grid_w >> 1, ex0 = (x0 >> 3) - 1, ey0 = (y0 >> 3) - 1;
  const Span se(reinterpret_cast<const char*>(P.edges) + ((ptrdiff_t)ey0 * ecw + ex0) * (ptrdiff_t)sizeof(EdgeRec), (uint32_t)((9 * ecw + 10) * (int)sizeof(EdgeRec)));
  const uint32_t ev = se.load_u16(se.at(vin, (uint32_t)((((vy >> 3) - ey0) * ecw + (vx >> 3) - ex0) * 8 + ((vy >> 2) & 1) * 2)));
  const uint32_t eh = se.load_u16(se.at(hin, (uint32_t)((((hy >> 3) - ey0) * ecw + (hx >> 3) - ex0) * 8 + 4 + ((hx >> 2) & 1) * 2)));
  // (P.slice_idx == nullptr: an empty span, every answer is slice 0)
  const int sx0 = (x0 - 8) >> l2, sy0 = (y0 - 8) >> l2;
  const Span ss(reinterpret_cast<const char*>(P.slice_idx) + ((ptrdiff_t)sy0 * P.ctus_w + sx0) * 2,
                P.slice_idx ? (uint32_t)(((((y0 + 64) >> l2) - sy0) * P.ctus_w + ((x0 + 64) >> l2) - sx0 + 1) * 2) : 0u);
  uint32_t sv = ss.load_u16(ss.at(vin, (uint32_t)((((vy >> l2) - sy0) * P.ctus_w + (vx >> l2) - sx0) * 2)));
  uint32_t sh = ss.load_u16(ss.at(hin, (uint32_t)((((hy >> l2) - sy0) * P.ctus_w + (hx >> l2) - sx0) * 2)));
  // the copies: luma 72 rows of 10 vectors (8 samples), chroma 36 rows of 12 vectors (the (Cb, Cr) pairs of four positions), dealt to the
  // threads in turn; the last round of each is short
  constexpr int VPR = kYC / 8, VPC = 2 * kCC / 8;
  static_assert(kYH * VPR > 512 && kYH * VPR <= 768 && kCH * VPC > 256 && kCH * VPC <= 512, "three rounds of luma vectors, two of chroma");
  const int yr0 = t / VPR, yv0 = t % VPR, yr1 = (t + 256) / VPR, yv1 = (t + 256) % VPR, yr2 = (t + 512) / VPR, yv2 = (t + 512) % VPR;
  const int ur0 = t / VPC, uv0 = t % VPC, ur1 = (t + 256) / VPC, uv1 = (t + 256) % VPC;
  const bool yin2 = t + 512 < kYH * VPR, uin1 = t + 256 < kCH * VPC;
  const Span sy(P.rec[0] + ((ptrdiff_t)(y0 - 4) * p0 + (x0 - 8)), (uint32_t)(((kYH - 1) * p0 + kYC) * 2));
  const Span sc(P.rec[1] + ((ptrdiff_t)((y0 >> 1) - 2) * p1 + kCStep * ((x0 >> 1) - 8)), (uint32_t)(((kCH - 1) * p1 + kCStep * kCC) * 2));
  const u32x4 ty0 = sy.load4((uint32_t)((yr0 * p0 + 8 * yv0) * 2));
  const u32x4 ty1 = sy.load4((uint32_t)((yr1 * p0 + 8 * yv1) * 2));
  const u32x4 ty2 = sy.load4(sy.at(yin2, (uint32_t)((yr2 * p0 + 8 * yv2) * 2)));
  const u32x4 tc0 = sc.load4((uint32_t)((ur0 * p1 + 8 * uv0) * 2));
  const u32x4 tc1 = sc.load4(sc.at(uin1, (uint32_t)((ur1 * p1 + 8 * uv1) * 2)));
  // SAO groups of this thread (8 samples each): two of luma (64 rows x 8 groups), one of Cb or Cr (32 rows x 4 groups each; neighbouring
  // lanes hold Cb and Cr of the same group: the plane wants them pair by pair, hmgpu_dev.h "chroma planes")
  const int gx = (t & 7) * 8, gy = t >> 3;                          // luma group k at (gx, gy + 32 k) of the tile
  const int lx = x0 + gx, ly[2] = {y0 + gy, y0 + gy + 32};
  const int ccomp = 1 + (t & 1), ccx = (x0 >> 1) + ((t >> 1) & 3) * 8, ccy = (y0 >> 1) + gy;
  const bool lin[2] = {lx < P.width && ly[0] < P.height, lx < P.width && ly[1] < P.height}, cin = ccx < (P.width >> 1) && ccy < (P.height >> 1);
  const int n64 = 63 >> l2;                                         // the tile's CTUs: (n64 + 1) x (n64 + 1), counted from that of (x0, y0)
  const Span sp(P.saoprm + ((ptrdiff_t)(y0 >> l2) * P.ctus_w + (x0 >> l2)) * 3, (uint32_t)(((n64 * P.ctus_w + n64) * 3 + 3) * (int)sizeof(SaoDev)));
  const uint32_t prow = (uint32_t)(3 * (int)sizeof(SaoDev)) * (uint32_t)P.ctus_w;
  const SaoPrm sl0 = sao_fetch(sp, sp.at(lin[0], (uint32_t)(gy >> l2) * prow + (uint32_t)((gx >> l2) * 3 * (int)sizeof(SaoDev))));
  const SaoPrm sl1 = sao_fetch(sp, sp.at(lin[1], (uint32_t)((gy + 32) >> l2) * prow + (uint32_t)((gx >> l2) * 3 * (int)sizeof(SaoDev))));
  const SaoPrm sc0 = sao_fetch(sp, sp.at(cin, (uint32_t)((2 * gy) >> l2) * prow + (uint32_t)(((((t >> 1) & 3) * 16) >> l2) * 3 + ccomp) * (uint32_t)sizeof(SaoDev)));
  // (a slice index is only looked at for units that filter: left alone, the compiler moves its request into that branch, behind the
  // tile's loads, and the classification waits for all of them.  The empty statement takes the two values here, where they are due.)
  asm volatile("" : "+v"(sv), "+v"(sh));
  if (t < 192) {
    push_units(L.unit[0], L.units[0], edge_classify<NF>(ev, sv, t), t);
    push_units(L.unit[1], L.units[1], edge_classify<NF>(eh, sh, t), t);
  }
  *reinterpret_cast<u32x4*>(&L.y[yr0][8 * yv0]) = ty0;
  *reinterpret_cast<u32x4*>(&L.y[yr1][8 * yv1]) = ty1;
  if (yin2) *reinterpret_cast<u32x4*>(&L.y[yr2][8 * yv2]) = ty2;
  // the copies in LDS are one per component: the filters run on them as they did on separate planes
  auto put_chroma = [&](int r, int v, const u32x4 c) {
    *reinterpret_cast<u32x2*>(&L.c[0][r][4 * v]) = u32x2{__builtin_amdgcn_perm(c.y, c.x, 0x05040100u), __builtin_amdgcn_perm(c.w, c.z, 0x05040100u)};
    *reinterpret_cast<u32x2*>(&L.c[1][r][4 * v]) = u32x2{__builtin_amdgcn_perm(c.y, c.x, 0x07060302u), __builtin_amdgcn_perm(c.w, c.z, 0x07060302u)};
  };
  put_chroma(ur0, uv0, tc0);
  if (uin1) put_chroma(ur1, uv1, tc1);
  __syncthreads();
  // ---- 2. vertical edges
  edge_apply<0, NF>(P, L, x0, y0, pop_unit(L.unit[0], L.units[0], t));
  __syncthreads();
  // ---- 3. horizontal edges
  edge_apply<1, NF>(P, L, x0, y0, pop_unit(L.unit[1], L.units[1], t));
  __syncthreads();
  // ---- 4. SAO of the tile from the deblocked copy, stored relative to the tile's first sample in the SAO planes
  const Span oy(P.sao[0] + ((ptrdiff_t)y0 * p0 + x0), (uint32_t)(((kTH - 1) * p0 + kTW) * 2));
  // the thread's final samples: border tiles use them again below.  (Threads without a group never look at theirs: any value serves, so
  // the empty statement stands for one, and no instruction of the interior tiles' path sets it.)
  u32x4 fy0, fy1, fc;
  asm("" : "=v"(fy0), "=v"(fy1), "=v"(fc));
  if (lin[0]) { fy0 = sao_group<kYW, NF>(P, 0, L.y, x0 - 8, y0 - 4, lx, ly[0], sl0); oy.store4((uint32_t)((gy * p0 + gx) * 2), fy0); }
  if (lin[1]) { fy1 = sao_group<kYW, NF>(P, 0, L.y, x0 - 8, y0 - 4, lx, ly[1], sl1); oy.store4((uint32_t)(((gy + 32) * p0 + gx) * 2), fy1); }
  if (cin) {
    const u32x4 own = sao_group<kCW, NF>(P, ccomp, L.c[ccomp - 1], (x0 >> 1) - 8, (y0 >> 1) - 2, ccx, ccy, sc0);
    // the even lane (Cb) writes positions 0..3 of the group, the odd lane (Cr) positions 4..7: each hands the other the half it does not write
    const bool odd = t & 1;
    const uint32_t r0 = (uint32_t)__shfl_xor((int)(odd ? own.x : own.z), 1, 64), r1 = (uint32_t)__shfl_xor((int)(odd ? own.y : own.w), 1, 64);
    const uint32_t cb0 = odd ? r0 : own.x, cb1 = odd ? r1 : own.y, cr0 = odd ? own.z : r0, cr1 = odd ? own.w : r1;
    fc = u32x4{__builtin_amdgcn_perm(cr0, cb0, 0x05040100u), __builtin_amdgcn_perm(cr0, cb0, 0x07060302u),
               __builtin_amdgcn_perm(cr1, cb1, 0x05040100u), __builtin_amdgcn_perm(cr1, cb1, 0x07060302u)};
    const Span oc(P.sao[1] + ((ptrdiff_t)(y0 >> 1) * p1 + kCStep * (x0 >> 1)), (uint32_t)(((kTH / 2 - 1) * p1 + kCStep * kTW / 2) * 2));
    oc.store4((uint32_t)((gy * p1 + kCStep * (((t >> 1) & 3) * 8 + (odd ? 4 : 0))) * 2), fc);
  }
  // ---- 5. a tile on the picture's edge writes the margins beside it (put_margins), so that no pass over the finished picture is needed
  // before it serves as a reference.  One scalar branch for every other tile.  The final samples go where the copies were (the SAO phase
  // has read them: barrier), luma as 64 rows of the luma copy's pitch, chroma as 32 rows of 32 (Cb, Cr) pairs, and all threads write from there.
  const bool el = x0 == 0, er = x0 + kTW >= P.width, et = y0 == 0, eb = y0 + kTH >= P.height;
  if (!(el || er || et || eb)) return;
  constexpr int kFC = kCStep * kTW / 2;                             // row pitch of the final chroma pairs in LDS
  static_assert(kTH <= kYH && kTW <= kYW && kTH / 2 * kFC * 2 <= (int)sizeof(L.c), "the final samples fit the copies' space");
  int16_t* const fcs = &L.c[0][0][0];
  // (the thread index as this path's own value: what is derived from it here is computed here, not hoisted in front of the branch)
  int tb = t;
  asm volatile("" : "+v"(tb));
  const int by = tb >> 3, bx = (tb & 7) * 8;                        // the thread's groups again: luma (bx, by), (bx, by + 32); chroma pairs from bp
  const int bp = ((tb >> 1) & 3) * 8 + (tb & 1) * 4;
  __syncthreads();
  if (lin[0]) *reinterpret_cast<u32x4*>(&L.y[by][bx]) = fy0;
  if (lin[1]) *reinterpret_cast<u32x4*>(&L.y[by + 32][bx]) = fy1;
  if (cin) *reinterpret_cast<u32x4*>(fcs + by * kFC + kCStep * bp) = fc;
  __syncthreads();
  const int vw = min(kTW, P.width - x0), vh = min(kTH, P.height - y0);
  put_margins<1>(&L.y[0][0], kYW, P.sao[0] + ((ptrdiff_t)y0 * p0 + x0), p0, vw, vh, el, er, et, eb, P.mx, P.my, tb);
  if (!P.mono)                                                      // (4:0:0: the chroma planes are left alone)
    put_margins<kCStep>(fcs, kFC, P.sao[1] + ((ptrdiff_t)(y0 >> 1) * p1 + kCStep * (x0 >> 1)), p1, vw >> 1, vh >> 1, el, er, et, eb, P.mx >> 1, P.my >> 1, tb);
}

void launch_filter_fused(const PicDev* pics, const Batch& b, int width, int height, bool nofilt, hipStream_t s) {
  const int tiles_x = (width + kTW - 1) / kTW, tiles = tiles_x * ((height + kTH - 1) / kTH);
  dim3 grid((unsigned)xcd_grid(b.n, tiles));
  if (nofilt) hipLaunchKernelGGL(k_filter_fused<true>, grid, dim3(256), 0, s, pics, b, tiles_x, tiles);
  else hipLaunchKernelGGL(k_filter_fused<false>, grid, dim3(256), 0, s, pics, b, tiles_x, tiles);
}

}  // namespace hmgpu
