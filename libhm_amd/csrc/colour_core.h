// colour_core.h -- the colour stage of the RGB exports (hmgpu_pictures_export_colour, include/hmgpu.h "colour export"): a lane's four
// (R, G, B) triples through the per-channel shaper and the 3D lattice with tetrahedral interpolation, between the final clip and the
// store: the first half of export_core.h's export_store_rgb, the epilogue of k_export.hip, and of the epilogues of k_export_scale.hip and
// k_export_warp.hip.
// Only the LUT stage lives here; the conversion to R'G'B' is export_core.h's export_rgb.  Integer arithmetic only, unsigned 32-bit; the
// table's nodes are 8 bytes {R | G << 16, B} in device memory, so a vertex is one load, and the sixteen vertex loads of a lane's four
// pixels are issued before the first is consumed.  Never indexes past node L - 1: the cell index is at most L - 2
// (u <= 65535, so u * (L - 1) >> 16 <= L - 2).
#pragma once
#include "hmgpu_dev.h"

namespace hmgpu {

// position 0 .. 65535 of the code value v of channel c.  A lane converts four columns even where the row ends sooner; what it read
// beyond the row is margin of any content, so v is bounded here before it indexes anything.
__device__ inline uint32_t colour_pos(const ColourLut& l, int c, uint32_t v) {
  v = min(v, (1u << l.depth) - 1u);
  if (l.shaper) return ldg(l.shaper + ((size_t)c << l.depth) + v);
  return ((v << (16 - l.depth)) | (v >> (2 * l.depth - 16))) & 0xffffu;       // bit replication
}

__device__ inline void colour_map4(const ColourLut& l, uint32_t R[4], uint32_t G[4], uint32_t B[4]) {
  uint32_t u[4][3];
  for (int i = 0; i < 4; i++) {
    u[i][0] = colour_pos(l, 0, R[i]); u[i][1] = colour_pos(l, 1, G[i]); u[i][2] = colour_pos(l, 2, B[i]);
  }
  if (!l.size) {                                            // shaper only (launch-uniform)
    for (int i = 0; i < 4; i++) { R[i] = u[i][0]; G[i] = u[i][1]; B[i] = u[i][2]; }
    return;
  }
  const uint32_t L = (uint32_t)l.size, L1 = L - 1;
  uint32_t w[4][4];
  u32x2 v[4][4];
  for (int i = 0; i < 4; i++) {
    const uint32_t tr = u[i][0] * L1, tg = u[i][1] * L1, tb = u[i][2] * L1;
    const uint32_t base = (tr >> 16) + L * ((tg >> 16) + L * (tb >> 16));
    // the fractions in descending order with the step each axis takes (a tie: the differing vertex gets weight 0)
    uint32_t fa = tr & 0xffffu, fb = tg & 0xffffu, fc = tb & 0xffffu, sa = 1, sb = L, sc = L * L;
    if (fa < fb) { uint32_t t = fa; fa = fb; fb = t; t = sa; sa = sb; sb = t; }
    if (fb < fc) { uint32_t t = fb; fb = fc; fc = t; t = sb; sb = sc; sc = t; }
    if (fa < fb) { uint32_t t = fa; fa = fb; fb = t; t = sa; sa = sb; sb = t; }
    w[i][0] = 65536u - fa; w[i][1] = fa - fb; w[i][2] = fb - fc; w[i][3] = fc;
    v[i][0] = ldg2(l.nodes + base);
    v[i][1] = ldg2(l.nodes + base + sa);
    v[i][2] = ldg2(l.nodes + base + sa + sb);
    v[i][3] = ldg2(l.nodes + base + sa + sb + sc);
  }
  for (int i = 0; i < 4; i++) {
    uint32_t r = 32768u, g = 32768u, b = 32768u;
    for (int k = 0; k < 4; k++) {
      r += w[i][k] * (v[i][k].x & 0xffffu);
      g += w[i][k] * (v[i][k].x >> 16);
      b += w[i][k] * (v[i][k].y & 0xffffu);
    }
    R[i] = r >> 16; G[i] = g >> 16; B[i] = b >> 16;
  }
}

}  // namespace hmgpu
