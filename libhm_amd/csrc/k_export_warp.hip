// k_export_warp.hip -- affine warp export (hmgpu_pictures_export_warp, include/hmgpu.h "affine warp export"): finished pictures
// converted as k_export.hip converts them for the RGB layout and sampled through one inverse affine map per picture, in the same pass.
// A plain gather, no LDS and no barrier: one workgroup of 256 lanes owns a tile of 64 x 16 outputs, a lane four adjacent columns of
// one row, so the epilogues of the other exports (hmgpu_dev.h export_store_row / export_store_px, colour_core.h colour_map4) are the
// ones used here; the pictures of a batch lie along the grid's y, each with its map and window (WarpPic) in device memory.  Neighbouring
// lanes read neighbouring samples for any map that does not shrink much, and the caches do the rest.
//
// Coordinates: X and Y of the lane's first column from two 64-bit multiply-adds each, m0 / m3 added per column; the tap indices are
// clamped to the window (EDGE) or tested against it (FILL) as 64-bit values, and only the clamped values are narrowed and turned into
// addresses.  NO LOAD EVER USES AN UNCLAMPED INDEX: under FILL an outside tap still loads the clamped sample and a select replaces it.
// A tap is one 2-byte luma load and one dword (Cb, Cr) load of the pair plane -- with the chroma stage (chroma_core.h's ChromaSite
// weights) the 2 x 2 pairs of its two rows and two columns, clamped to the decoded plane -- then the matrix and the clip of
// hmgpu_export_plan.coef; the four results are blended with weights that sum to 65536.  Filter and border are launch-uniform branches.
// One instance per output element, planes / packed pixel size, colour stage and chroma stage.
// The depth rule and the dispatch of launch_export_warp are export_core.h's.  The tap keeps its own one-sample text of the replicated
// chroma and of the conversion, and the epilogue its own store choice: with those taken from export_core.h
// (export_chroma_replicated<1>, export_rgb<1>, export_store_rgb, the stages as a pack) the bilinear uint8 planes case at 2160p measured
// slower than the parent by more than the parent's own spread in two whole jobs (+1.0 and +4.7 us in 1316; profiles/EXPERIMENTS.md),
// and sharing either piece alone changes most instances' instructions.  As it stands every instance's instructions are those from
// before the shared core.  A change to the matrix is made here as well as in export_core.h.
#include "hmgpu_dev.h"
#include "export_core.h"

namespace hmgpu {

namespace {

// v clamped to 0 .. hi, still 64 bits wide
__device__ inline long long clamp64(long long v, long long hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// S at the sample (px, py) of the decoded picture (plane coordinates, inside the window: the caller has clamped them): R, G, B
template <bool CHR>
__device__ inline void warp_tap(const WarpArgs& a, const ChromaSite& site, const int16_t* ys, const int16_t* cs, int px, int py, uint32_t o[3]) {
  const int yv = ldg(ys + (ptrdiff_t)py * a.pitch_y + px);
  int u, v;
  if constexpr (CHR) {
    // the chroma stage (csx = 1): the two columns of this parity that carry weight, of two rows, every index clamped to the plane
    int ia, ib, wv;
    chroma_rows(site, py, a.csy, &ia, &ib, &wv);
    const int J = px >> 1, par = px & 1, left = site.hx[par][0];
    const int c0 = left ? J - 1 : J, w0 = left ? left : site.hx[par][1];
    const int ca = min(site.wc - 1, max(0, c0)), cb = min(site.wc - 1, max(0, c0 + 1));
    const int16_t* ra = cs + (ptrdiff_t)ia * a.pitch_c;
    const int16_t* rb = cs + (ptrdiff_t)ib * a.pitch_c;
    int uaa, vaa, uab, vab, uba, vba, ubb, vbb;
    chroma_pair(ra + kCStep * ca, &uaa, &vaa);
    chroma_pair(ra + kCStep * cb, &uab, &vab);
    chroma_pair(rb + kCStep * ca, &uba, &vba);
    chroma_pair(rb + kCStep * cb, &ubb, &vbb);
    u = (w0 * (wv * uaa + (4 - wv) * uba) + (4 - w0) * (wv * uab + (4 - wv) * ubb) + 8) >> 4;
    v = (w0 * (wv * vaa + (4 - wv) * vba) + (4 - w0) * (wv * vab + (4 - wv) * vbb) + 8) >> 4;
  } else if (a.mono) {
    u = v = a.coef[3];
  } else {
    chroma_pair(cs + (ptrdiff_t)(py >> a.csy) * a.pitch_c + kCStep * (px >> a.csx), &u, &v);
  }
  if (a.coef[10]) {                       // identity (GBR): the YUV bit-depth rule per channel type
    o[0] = (uint32_t)depth_conv(v, a.sh[1], a.maxv[1]);
    o[1] = (uint32_t)depth_conv(yv, a.sh[0], a.maxv[0]);
    o[2] = (uint32_t)depth_conv(u, a.sh[1], a.maxv[1]);
  } else {
    const int S = a.coef[0], M = a.coef[9];
    const int t = a.coef[4] * (yv - a.coef[2]) + a.coef[1];
    const int cu = u - a.coef[3], cv = v - a.coef[3];
    o[0] = (uint32_t)min(M, max(0, (t + a.coef[5] * cv) >> S));
    o[1] = (uint32_t)min(M, max(0, (t + a.coef[6] * cu + a.coef[7] * cv) >> S));
    o[2] = (uint32_t)min(M, max(0, (t + a.coef[8] * cu) >> S));
  }
}

}  // namespace

// NCH: 0 (three planes), or the elements of a packed pixel; COL: the colour stage between the blend and the store; CHR: the chroma
// stage in the tap
template <int ELEM, int NCH, bool COL, bool CHR>
__global__ void __launch_bounds__(256) k_export_warp(const WarpArgs a, const ChromaSite site, const ColourLut lut) {
  const int pic = blockIdx.y;
  const int tyi = blockIdx.x / a.tiles_x, txi = blockIdx.x - tyi * a.tiles_x;
  const int ox = txi * kWarpTileW + 4 * (threadIdx.x & 15), oy = tyi * kWarpTileH + (threadIdx.x >> 4);
  if (ox >= a.w || oy >= a.h) return;
  const WarpPic k = a.pics[pic];          // wave-uniform
  const int16_t* const ys = a.src[pic][0];
  const int16_t* const cs = a.src[pic][1];
  const bool bilinear = a.filter == HMGPU_WARP_BILINEAR, fillb = a.border == HMGPU_WARP_FILL;
  const long long rnd = bilinear ? 128 : 32768;
  long long X = (long long)k.m[0] * ox + (long long)k.m[1] * oy + k.m[2] + rnd;
  long long Y = (long long)k.m[3] * ox + (long long)k.m[4] * oy + k.m[5] + rnd;
  const long long xmax = k.ws - 1, ymax = k.hs - 1;
  uint32_t R[4], G[4], B[4];
  for (int i = 0; i < 4; i++, X += k.m[0], Y += k.m[3]) {
    const long long ix = X >> 16, iy = Y >> 16;
    // (the clamped values fit 32 bits: 0 .. ws - 1, 0 .. hs - 1)
    const int x0 = (int)clamp64(ix, xmax), y0 = (int)clamp64(iy, ymax);
    if (!bilinear) {
      uint32_t t[3];
      warp_tap<CHR>(a, site, ys, cs, k.x0 + x0, k.y0 + y0, t);
      const bool outside = fillb && (ix != x0 || iy != y0);
      R[i] = outside ? a.fill[0] : t[0]; G[i] = outside ? a.fill[1] : t[1]; B[i] = outside ? a.fill[2] : t[2];
      continue;
    }
    const int x1 = (int)clamp64(ix + 1, xmax), y1 = (int)clamp64(iy + 1, ymax);
    const bool ex0 = ix != x0, ex1 = ix + 1 != x1, ey0 = iy != y0, ey1 = iy + 1 != y1;   // the tap's column / row lies outside
    const uint32_t fx = (uint32_t)(X >> 8) & 255u, fy = (uint32_t)(Y >> 8) & 255u;
    uint32_t t[4][3];
    warp_tap<CHR>(a, site, ys, cs, k.x0 + x0, k.y0 + y0, t[0]);
    warp_tap<CHR>(a, site, ys, cs, k.x0 + x1, k.y0 + y0, t[1]);
    warp_tap<CHR>(a, site, ys, cs, k.x0 + x0, k.y0 + y1, t[2]);
    warp_tap<CHR>(a, site, ys, cs, k.x0 + x1, k.y0 + y1, t[3]);
    const bool outside[4] = {fillb && (ex0 || ey0), fillb && (ex1 || ey0), fillb && (ex0 || ey1), fillb && (ex1 || ey1)};
    const uint32_t w[4] = {(256u - fx) * (256u - fy), fx * (256u - fy), (256u - fx) * fy, fx * fy};
    uint32_t s[3] = {32768u, 32768u, 32768u};
    for (int q = 0; q < 4; q++)
      for (int c = 0; c < 3; c++) s[c] += w[q] * (outside[q] ? a.fill[c] : t[q][c]);
    R[i] = s[0] >> 16; G[i] = s[1] >> 16; B[i] = s[2] >> 16;
  }
  if constexpr (COL) colour_map4(lut, R, G, B);
  const int n = min(4, a.w - ox);
  const bool vec = a.vec != 0, flip = (a.flip >> pic) & 1;
  // (identity: G carries the luma container shift, B and R the chroma one; the matrix: all three the luma one)
  const int mc = a.coef[10] ? a.msb[1] : a.msb[0];
  if constexpr (NCH != 0) {
    export_store_px<ELEM, NCH>(a.dst[0] + pic * a.bstride[0] + oy * a.pitch[0], ox, a.w, R, G, B, n, vec, flip, mc, a.msb[0], a.scale,
                               a.bias, a.px);
  } else {
    export_store_row<ELEM>(a.dst[0] + pic * a.bstride[0] + oy * a.pitch[0], ox, a.w, R, n, vec, flip, mc, a.scale[0], a.bias[0]);
    export_store_row<ELEM>(a.dst[1] + pic * a.bstride[1] + oy * a.pitch[1], ox, a.w, G, n, vec, flip, a.msb[0], a.scale[1], a.bias[1]);
    export_store_row<ELEM>(a.dst[2] + pic * a.bstride[2] + oy * a.pitch[2], ox, a.w, B, n, vec, flip, mc, a.scale[2], a.bias[2]);
  }
}

void launch_export_warp(const WarpArgs& a, int elem, int n, int nch, const ChromaSite* cs, const ColourLut* lut, hipStream_t s) {
  const dim3 grid((unsigned)(a.tiles_x * ((a.h + kWarpTileH - 1) / kWarpTileH)), (unsigned)n), block(256);
  // (the kernel has one signature for its four instance families: a stage it does not have is given an empty record)
  export_rgb_instance(elem, nch, cs, lut, [&](auto e, auto c, const auto&... st) {
    constexpr bool chr = pack_has<ChromaSite, std::decay_t<decltype(st)>...>, col = pack_has<ColourLut, std::decay_t<decltype(st)>...>;
    hipLaunchKernelGGL((k_export_warp<e(), c(), col, chr>), grid, block, 0, s, a, cs ? *cs : ChromaSite{}, lut ? *lut : ColourLut{});
  });
}

}  // namespace hmgpu
