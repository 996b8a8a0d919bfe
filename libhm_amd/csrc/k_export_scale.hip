// k_export_scale.hip -- scaled device export (hmgpu_picture_export_scaled / hmgpu_pictures_export, include/hmgpu.h "scaled export"):
// finished pictures converted as k_export.hip converts them and resized in the same pass, horizontally then vertically, with the
// host's Q14 tables.  The pictures of a batch lie along the grid's y and share the tiling; they share the tables too, unless the call
// gives each picture a source window of its own (hmgpu_pictures_export_windows: ScaleArgs::pic_cls), and each may be mirrored.
//
// One workgroup of 256 lanes owns a tile of tw x th outputs of one plane class (RGB: R, G and B together; YUV: Y, or Cb and Cr
// together).  It walks the tile's source rows in passes of `rows` rows through LDS:
//   1. the pass's source rows, over the tile's source span, are read once with 16-byte loads (8 luma samples or 4 CbCr pairs) and
//      converted to output code values (the bit-depth rule, or the RGB matrix) into LDS as 16-bit samples;
//   2. the horizontal taps turn them into t values, one tile column per lane and up to four rows per lane (a weight is loaded once for
//      its rows), into LDS as 32-bit values;
//   3. each lane adds the rows of the pass that fall in the vertical windows of its four outputs (four adjacent columns of one row)
//      to sums it keeps in registers.
// After the last pass the sums are rounded, clipped and stored, 4 or 8 bytes per plane and lane where aligned.  No intermediate
// leaves the workgroup.  One instance per layout and output element (hmgpu_dev.h export_store4); the class, and the channels with
// it, is uniform per workgroup.  Packed pixels (hmgpu_pictures_export_pixels): an instance family of the RGB layout whose epilogue
// writes the lane's four columns x 3 or 4 elements as one run of bytes (hmgpu_dev.h export_store_px).  The colour stage
// (hmgpu_pictures_export_colour): k_export_scale_colour, the RGB layout with colour_core.h's colour_map4 between the clip and the store.
// The chroma stage (hmgpu_pictures_export_chroma): k_export_scale_chroma, whose stage step interpolates the chroma of a 16-byte group
// (chroma_core.h) where the others replicate it; one pair left and right of the group's four come from neighbouring groups' lines.
// The depth rule and the 16-byte unpack are export_core.h's, and so is the dispatch of launch_export_scaled.  The stage step keeps its
// own 8-sample text of the chroma fetches, the conversion and the store choice, and the three __global__ wrappers stay: with those
// taken from export_core.h (export_chroma_replicated<8> / export_chroma_sited<8>, export_rgb<8>, export_store_rgb, one __global__ over
// a stage pack) no instance had scratch or lost occupancy, but scaled 1080p bicubic uint8 planes measured 0.2 - 0.3 % slower than the
// parent in two jobs (profiles/EXPERIMENTS.md), and sharing the fetches alone already changes 15 to 45 instances' instructions.  As
// it stands every instance's instructions are those from before the shared core.  A change to the matrix or to the sited fetch is
// made here as well as in export_core.h.
// Source loads may reach up to 7 samples left and right of the crop window (16-byte groups): the planes keep 64 or more samples of
// margin on both sides, and the tables never point at them.
#include "hmgpu_dev.h"
#include "export_core.h"

namespace hmgpu {

namespace {

// C channels: 3 = RGB from the luma grid, 1 = Y, 2 = Cb and Cr from the pair plane; NCH: 0, or (C = 3) the elements of a packed pixel;
// COL (C = 3): the colour stage (colour_core.h) between the final clip and the store; CHR (C = 3): the chroma stage (chroma_core.h)
// in place of the replicated chroma of the stage step
template <int LAYOUT, int ELEM, int C, int NCH = 0, bool COL = false, bool CHR = false>
__device__ void scale_tile(const ScaleArgs& a, const ScaleClass& k, int blk, int32_t* lds, const ColourLut* lut = nullptr,
                           const ChromaSite* site = nullptr) {
  constexpr int BYTES = elem_bytes<ELEM>();
  constexpr int G = C == 2 ? 4 : 8;                       // samples per 16-byte group
  const int pic = blockIdx.y;
  const int16_t* const src = a.src[pic][C == 2 ? 1 : 0];  // the class's plane of this picture
  const int16_t* const csrc = a.src[pic][1];              // RGB: its chroma
  const int chan = C == 2 ? 1 : 0;                        // channel type of the bit-depth rule
  const int tid = threadIdx.x;
  const int tyi = blk / k.tiles_x, txi = blk - tyi * k.tiles_x;
  const int ox0 = txi * k.tw, oy0 = tyi * k.th;
  const int nx = min(k.tw, k.tx.n - ox0), ny = min(k.th, k.ty.n - oy0);
  const int sx_lo = ldg(k.tx.span + 2 * txi), sx_hi = ldg(k.tx.span + 2 * txi + 1);
  const int sy_lo = ldg(k.ty.span + 2 * tyi), sy_hi = ldg(k.ty.span + 2 * tyi + 1);
  const int ax = (k.x0 + sx_lo) & ~(G - 1);               // first sample (plane coordinates) of the staged span, 16-byte aligned
  const int groups = (k.x0 + sx_hi - ax + G - 1) / G;
  const int cap = k.span_cap, R = k.rows, TW = k.tw;
  uint16_t* sbuf = reinterpret_cast<uint16_t*>(lds);      // [C][R][cap]
  int32_t* tbuf = lds + (C * R * cap) / 2;                // [C][R][tw]
  // horizontal pass: column hx of the tile, rows hr + q * hstep (q < 4)
  const int hx = tid & (TW - 1), hr = tid / TW, hstep = 256 / TW;
  const bool hval = hx < nx;
  const int hf = hval ? ldg(k.tx.first + ox0 + hx) : 0, hn = hval ? ldg(k.tx.count + ox0 + hx) : 0;
  const int hbase = k.x0 + hf - ax;
  const int hsh = 14 - a.e, hrnd = 1 << (13 - a.e);
  // vertical sums: columns vx .. vx + 3, row vy of the tile
  const int vx = 4 * (tid % (TW / 4)), vy = tid / (TW / 4);
  const bool vval = vy < ny && vx < nx;
  const int vf = vval ? ldg(k.ty.first + oy0 + vy) : 0, vn = vval ? ldg(k.ty.count + oy0 + vy) : 0;
  int acc[C][4];
  for (int c = 0; c < C; c++)
    for (int j = 0; j < 4; j++) acc[c][j] = 0;

  for (int r0 = sy_lo; r0 < sy_hi; r0 += R) {
    const int nr = min(R, sy_hi - r0);
    // 1. stage: nr rows x `groups` 16-byte groups, converted
    for (int i = tid; i < nr * groups; i += 256) {
      const int r = i / groups, g = i - r * groups;
      const int x = ax + g * G, y = k.y0 + r0 + r;
      uint32_t o[C][8];
      if constexpr (C == 2) {
        int p[8];
        unpack8(ldg4(src + (ptrdiff_t)y * k.pitch + kCStep * x), p);
        for (int s = 0; s < 4; s++) {
          o[0][s] = (uint32_t)depth_conv(p[2 * s], a.sh[1], a.maxv[1]);
          o[C - 1][s] = (uint32_t)depth_conv(p[2 * s + 1], a.sh[1], a.maxv[1]);
        }
      } else {
        int yv[8];
        unpack8(ldg4(src + (ptrdiff_t)y * k.pitch + x), yv);
        if constexpr (C == 1) {
          for (int s = 0; s < 8; s++) o[0][s] = (uint32_t)depth_conv(yv[s], a.sh[0], a.maxv[0]);
        } else {
          int u[8], v[8];
          if constexpr (CHR) {
            // the chroma stage (csx = 1): pairs J - 1 .. J + 4 of two rows, six loads none of which waits for another
            int ia, ib, wv;
            chroma_rows(*site, y, a.csy, &ia, &ib, &wv);
            const int16_t* pa = csrc + (ptrdiff_t)ia * a.pitch_c + kCStep * (x >> 1);
            const int16_t* pb = csrc + (ptrdiff_t)ib * a.pitch_c + kCStep * (x >> 1);
            int ma[8], mb[8], ua[6], ub[6], va[6], vb[6];
            unpack8(ldg4(pa), ma);
            unpack8(ldg4(pb), mb);
            chroma_pair(pa - kCStep, &ua[0], &va[0]);
            chroma_pair(pb - kCStep, &ub[0], &vb[0]);
            chroma_pair(pa + 4 * kCStep, &ua[5], &va[5]);
            chroma_pair(pb + 4 * kCStep, &ub[5], &vb[5]);
            for (int s = 0; s < 4; s++) { ua[1 + s] = ma[2 * s]; va[1 + s] = ma[2 * s + 1]; ub[1 + s] = mb[2 * s]; vb[1 + s] = mb[2 * s + 1]; }
            chroma_line<4>(*site, x >> 1, wv, ua, ub, u);
            chroma_line<4>(*site, x >> 1, wv, va, vb, v);
          } else if (a.mono) {
            for (int s = 0; s < 8; s++) u[s] = v[s] = a.coef[3];
          } else {
            const int16_t* cp = csrc + (ptrdiff_t)(y >> a.csy) * a.pitch_c + kCStep * (x >> a.csx);
            int p[16];
            unpack8(ldg4(cp), p);
            if (a.csx) {
              for (int s = 0; s < 8; s++) { u[s] = p[2 * (s >> 1)]; v[s] = p[2 * (s >> 1) + 1]; }
            } else {
              unpack8(ldg4(cp + 8), p + 8);
              for (int s = 0; s < 8; s++) { u[s] = p[2 * s]; v[s] = p[2 * s + 1]; }
            }
          }
          if (a.coef[10]) {                   // identity (GBR)
            for (int s = 0; s < 8; s++) {
              o[0][s] = (uint32_t)depth_conv(v[s], a.sh[1], a.maxv[1]);
              o[1][s] = (uint32_t)depth_conv(yv[s], a.sh[0], a.maxv[0]);
              o[C - 1][s] = (uint32_t)depth_conv(u[s], a.sh[1], a.maxv[1]);
            }
          } else {
            const int S = a.coef[0], M = a.coef[9];
            for (int s = 0; s < 8; s++) {
              const int t = a.coef[4] * (yv[s] - a.coef[2]) + a.coef[1];
              const int cu = u[s] - a.coef[3], cv = v[s] - a.coef[3];
              o[0][s] = (uint32_t)min(M, max(0, (t + a.coef[5] * cv) >> S));
              o[1][s] = (uint32_t)min(M, max(0, (t + a.coef[6] * cu + a.coef[7] * cv) >> S));
              o[C - 1][s] = (uint32_t)min(M, max(0, (t + a.coef[8] * cu) >> S));
            }
          }
        }
      }
      for (int c = 0; c < C; c++) {
        uint16_t* d = sbuf + (c * R + r) * cap + g * G;
        if constexpr (G == 8) {
          u32x4 w;
          for (int s = 0; s < 4; s++) w[s] = o[c][2 * s] | o[c][2 * s + 1] << 16;
          *reinterpret_cast<u32x4*>(d) = w;
        } else {
          u32x2 w;
          w.x = o[c][0] | o[c][1] << 16; w.y = o[c][2] | o[c][3] << 16;
          *reinterpret_cast<u32x2*>(d) = w;
        }
      }
    }
    __syncthreads();
    // 2. horizontal taps
    if (hval && hr < nr) {
      int h[C][4];
      for (int c = 0; c < C; c++)
        for (int q = 0; q < 4; q++) h[c][q] = 0;
      const int16_t* wp = k.tx.w + ox0 + hx;
      for (int j = 0; j < hn; j++) {
        const int w = ldg(wp + (ptrdiff_t)j * k.tx.n);
        for (int q = 0; q < 4; q++) {
          const int r = hr + q * hstep;
          if (r < nr)
            for (int c = 0; c < C; c++) h[c][q] += w * (int)sbuf[(c * R + r) * cap + hbase + j];
        }
      }
      for (int q = 0; q < 4; q++) {
        const int r = hr + q * hstep;
        if (r < nr)
          for (int c = 0; c < C; c++) tbuf[(c * R + r) * TW + hx] = (h[c][q] + hrnd) >> hsh;
      }
    }
    __syncthreads();
    // 3. vertical taps of the rows of this pass
    if (vval) {
      const int j0 = max(r0, vf), j1 = min(r0 + nr, vf + vn);
      const int16_t* wp = k.ty.w + oy0 + vy;
      for (int j = j0; j < j1; j++) {
        const int w = ldg(wp + (ptrdiff_t)(j - vf) * k.ty.n);
        for (int c = 0; c < C; c++) {
          const u32x4 t = *reinterpret_cast<const u32x4*>(tbuf + (c * R + j - r0) * TW + vx);
          for (int q = 0; q < 4; q++) acc[c][q] += w * (int)t[q];
        }
      }
    }
  }
  if (!vval) return;
  const int vsh = 14 + a.e, vrnd = 1 << (13 + a.e);
  const int M = a.maxv[chan], msb = a.msb[chan];
  uint32_t o[C][4];
  for (int c = 0; c < C; c++)
    for (int q = 0; q < 4; q++) o[c][q] = (uint32_t)min(M, max(0, (acc[c][q] + vrnd) >> vsh));
  if constexpr (COL) colour_map4(*lut, o[0], o[1], o[C - 1]);
  const int x = ox0 + vx, y = oy0 + vy, n = min(4, k.tx.n - x);
  const bool vec = a.vec != 0, flip = (a.flip >> pic) & 1;    // the mirror: columns x .. x + 3 reversed to W - 1 - x ..
  const int W = k.tx.n;
  if constexpr (NCH != 0) {                   // packed pixels: the lane's four columns as one run of bytes
    export_store_px<ELEM, NCH>(a.dst[0] + pic * a.bstride[0] + y * a.pitch[0], x, W, o[0], o[1], o[C - 1], n, vec, flip, msb, msb,
                               a.scale, a.bias, a.px);
  } else if constexpr (C != 2) {
    for (int c = 0; c < C; c++)
      export_store_row<ELEM>(a.dst[c] + pic * a.bstride[c] + y * a.pitch[c], x, W, o[c], n, vec, flip, msb, a.scale[c], a.bias[c]);
  } else if (LAYOUT == HMGPU_EXPORT_PLANAR) {
    export_store_row<ELEM>(a.dst[1] + pic * a.bstride[1] + y * a.pitch[1], x, W, o[0], n, vec, flip, msb, a.scale[1], a.bias[1]);
    export_store_row<ELEM>(a.dst[2] + pic * a.bstride[2] + y * a.pitch[2], x, W, o[C - 1], n, vec, flip, msb, a.scale[2], a.bias[2]);
  } else if constexpr (ELEM <= kElemU16) {    // semi-planar (integer elements only): the pairs interleaved
    const uint32_t p[8] = {o[0][0], o[C - 1][0], o[0][1], o[C - 1][1], o[0][2], o[C - 1][2], o[0][3], o[C - 1][3]};
    export_store_pairs<ELEM>(a.dst[1] + pic * a.bstride[1] + y * a.pitch[1], x, W, p, n, vec, flip, msb);
  }
}

}  // namespace

template <int LAYOUT, int ELEM, int NCH = 0>
__global__ void __launch_bounds__(256) k_export_scale(const ScaleArgs a) {
  __shared__ __attribute__((aligned(16))) int32_t lds[kScaleLdsBytes / 4];
  const int b = blockIdx.x;
  const int c = LAYOUT == HMGPU_EXPORT_RGB || b < a.cls[0].blocks ? 0 : 1;
  // the class as this picture sees it: the call's own, or (windows that differ) the picture's from device memory, a wave-uniform load
  ScaleClass k = a.cls[c];
  if (a.pic_cls) k = a.pic_cls[2 * blockIdx.y + c];
  if (LAYOUT == HMGPU_EXPORT_RGB) scale_tile<LAYOUT, ELEM, 3, NCH>(a, k, b, lds);
  else if (c == 0) scale_tile<LAYOUT, ELEM, 1>(a, k, b, lds);
  else scale_tile<LAYOUT, ELEM, 2>(a, k, b - a.cls[0].blocks, lds);
}

// the RGB layout with the colour stage: planes (NCH 0) or packed pixels
template <int ELEM, int NCH>
__global__ void __launch_bounds__(256) k_export_scale_colour(const ScaleArgs a, const ColourLut lut) {
  __shared__ __attribute__((aligned(16))) int32_t lds[kScaleLdsBytes / 4];
  ScaleClass k = a.cls[0];
  if (a.pic_cls) k = a.pic_cls[2 * blockIdx.y];
  scale_tile<HMGPU_EXPORT_RGB, ELEM, 3, NCH, true>(a, k, blockIdx.x, lds, &lut);
}

// the RGB layout with the chroma stage, and (COL) the colour stage as well: planes (NCH 0) or packed pixels
template <int ELEM, int NCH, bool COL>
__global__ void __launch_bounds__(256) k_export_scale_chroma(const ScaleArgs a, const ChromaSite site, const ColourLut lut) {
  __shared__ __attribute__((aligned(16))) int32_t lds[kScaleLdsBytes / 4];
  ScaleClass k = a.cls[0];
  if (a.pic_cls) k = a.pic_cls[2 * blockIdx.y];
  scale_tile<HMGPU_EXPORT_RGB, ELEM, 3, NCH, COL, true>(a, k, blockIdx.x, lds, &lut, &site);
}

// n pictures; nch: 0, or (RGB) 3 / 4 elements per packed pixel (a.px); cs / lut: null, or the stage (RGB only)
void launch_export_scaled(const ScaleArgs& a, int layout, int elem, int n, int nch, const ChromaSite* cs, const ColourLut* lut, hipStream_t s) {
  const bool rgb = layout == HMGPU_EXPORT_RGB;
  const dim3 grid((unsigned)(a.cls[0].blocks + (rgb ? 0 : a.cls[1].blocks)), (unsigned)n), block(256);
  if (!rgb) {
    export_yuv_instance(layout, elem, [&](auto l, auto e) { hipLaunchKernelGGL((k_export_scale<l(), e()>), grid, block, 0, s, a); });
    return;
  }
  // (the chroma kernel has one signature for both of its instance families: without the colour stage it is given an empty table)
  export_rgb_instance(elem, nch, cs, lut, [&](auto e, auto c, const auto&... st) {
    if constexpr (pack_has<ChromaSite, std::decay_t<decltype(st)>...>) {
      if constexpr (sizeof...(st) == 2) hipLaunchKernelGGL((k_export_scale_chroma<e(), c(), true>), grid, block, 0, s, a, st...);
      else hipLaunchKernelGGL((k_export_scale_chroma<e(), c(), false>), grid, block, 0, s, a, st..., ColourLut{});
    } else if constexpr (sizeof...(st) == 1) {
      hipLaunchKernelGGL((k_export_scale_colour<e(), c()>), grid, block, 0, s, a, st...);
    } else {
      hipLaunchKernelGGL((k_export_scale<HMGPU_EXPORT_RGB, e(), c()>), grid, block, 0, s, a);
    }
  });
}

}  // namespace hmgpu
