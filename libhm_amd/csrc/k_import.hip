// k_import.hip -- picture import (hmgpu_pictures_import, include/hmgpu.h "picture import"): planar / semi-planar YUV
// or RGB (planes or packed pixels) in caller-owned device memory into the sample planes of up to 16 pictures, one launch.
//
// A lane owns eight luma samples of a row -- of both rows of a pair where the picture's chroma is subsampled vertically -- and the
// (Cb, Cr) pairs beneath them: it forms every value in registers first, so that all its source loads are issued before any store, and
// then writes 16 bytes of luma per row and 16 (4:2:0, 4:2:2) or 32 (4:4:4) bytes of the pair plane; eight lanes write 128 contiguous
// bytes of a plane row.  A run of eight source elements -- of eight packed pixels -- that lies inside the source and whose plane
// is aligned to eight elements (ImportArgs::vec) is read with whole 8- or 16-byte loads; every other element -- unaligned planes, the
// ragged last group, the columns and rows the padding rule repeats, the taps of a chroma conversion -- is loaded on its own with its
// index clamped to the source.  Packed YUV words (hmgpu_pictures_import_yuvpack) are three more element kinds of the YUV instance: a
// sample is fetched from its word by a per-format accessor (pk_raw), element by element with the same clamped indices, and everything
// behind the fetch is the code of the planar source.  The kernel writes the coded w x h samples of each plane and nothing else: no margin, no other picture.  No LDS, no scratch.
#include "hmgpu_dev.h"

namespace hmgpu {
namespace {

enum { kImpU8 = 0, kImpU16 = 1, kImpF16 = 2, kImpBF16 = 3, kImpF32 = 4, kImpPk8 = 5, kImpPk16 = 6, kImpPk32 = 7 };
template <int EL> constexpr int kElemBytes = EL == kImpU8 ? 1 : EL == kImpF32 ? 4 : 2;

// element idx of a row, as its bits
template <int EL>
__device__ inline uint32_t raw_at(const uint8_t* row, int idx) {
  if constexpr (EL == kImpU8) return ldg(row + idx);
  else if constexpr (EL == kImpF32) return ldg(reinterpret_cast<const uint32_t*>(row) + idx);
  else return ldg(reinterpret_cast<const uint16_t*>(row) + idx);
}

// eight elements from idx on, the address a multiple of eight elements: one load
template <int EL>
__device__ inline void raw8(const uint8_t* row, int idx, uint32_t r[8]) {
  if constexpr (EL == kImpU8) {
    const u32x2 v = ldg2(row + idx);
    for (int i = 0; i < 4; i++) { r[i] = (v.x >> (8 * i)) & 0xff; r[4 + i] = (v.y >> (8 * i)) & 0xff; }
  } else if constexpr (EL == kImpF32) {
    const u32x4 a = ldg4(row + 4 * (size_t)idx), b = ldg4(row + 4 * (size_t)idx + 16);
    r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
  } else {
    const u32x4 a = ldg4(row + 2 * (size_t)idx);
    r[0] = a.x & 0xffff; r[1] = a.x >> 16; r[2] = a.y & 0xffff; r[3] = a.y >> 16;
    r[4] = a.z & 0xffff; r[5] = a.z >> 16; r[6] = a.w & 0xffff; r[7] = a.w >> 16;
  }
}

// Eight packed pixels of NCH elements from element idx on, the row's start a multiple of eight elements and idx a multiple of 8 * NCH:
// 24 .. 128 consecutive bytes as whole loads (8-byte pieces for three uint8 channels, else 16-byte ones), then the elements that
// stand where R, G and B do (pos: uniform) picked out with selects.  Every index into d[] is a constant: no scratch.
template <int EL, int NCH>
__device__ inline void raw8_px(const uint8_t* row, int idx, const int32_t pos[3], uint32_t r[3][8]) {
  constexpr int ES = kElemBytes<EL>, DW = 8 * NCH * ES / 4;
  const uint8_t* p = row + (size_t)idx * ES;
  uint32_t d[DW];
  if constexpr (EL == kImpU8 && NCH == 3) {
#pragma unroll
    for (int j = 0; j < DW; j += 2) { const u32x2 v = ldg2(p + 4 * j); d[j] = v.x; d[j + 1] = v.y; }
  } else {
#pragma unroll
    for (int j = 0; j < DW; j += 4) {
      const u32x4 v = EL == kImpU8 ? ldg4_a8(p + 4 * j) : ldg4(p + 4 * j);
      d[j] = v.x; d[j + 1] = v.y; d[j + 2] = v.z; d[j + 3] = v.w;
    }
  }
#pragma unroll
  for (int i = 0; i < 8; i++) {
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      const int e = i * NCH + c;
      uint32_t v;
      if constexpr (ES == 1) v = (d[e / 4] >> (8 * (e % 4))) & 0xff;
      else if constexpr (ES == 2) v = (d[e / 2] >> (16 * (e % 2))) & 0xffff;
      else v = d[e];
      for (int k = 0; k < 3; k++) if (pos[k] == c) r[k][i] = v;
    }
  }
}

// packed YUV: sample x of component comp (0 Y, 1 Cb, 2 Cr; x in that component's plane) of a row of words, as its bits.  Elements:
// at a uniform stride and offset.  V210: field p of the group's twelve (Y i: 2 i + 1, Cb m: 4 m, Cr m: 4 m + 2), three to a dword
// from bit 0.  Y410: Cb, Y, Cr from bits 0, 10, 20 of the pixel's dword
template <int EL>
__device__ inline uint32_t pk_raw(const ImportArgs& a, const uint8_t* row, int x, int comp) {
  if constexpr (EL == kImpPk32) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(row);
    if (a.pk_v210) {
      const int per = comp ? 3 : 6, g = x / per, i = x - g * per, p = comp ? 4 * i + 2 * (comp - 1) : 2 * i + 1;
      return (ldg(w + 4 * g + p / 3) >> (10 * (p % 3))) & 0x3ff;
    }
    return (ldg(w + x) >> (comp == 0 ? 10 : comp == 1 ? 0 : 20)) & 0x3ff;
  } else {
    const int idx = comp ? a.pk_cs * x + a.pk_co[comp - 1] : a.pk_ls * x + a.pk_lo;
    if constexpr (EL == kImpPk8) return ldg(row + idx);
    else return ldg(reinterpret_cast<const uint16_t*>(row) + idx);
  }
}

// the integer of an element at the source depth of channel type t; k: the plane (colour) whose scale and bias a float element takes
template <int EL>
__device__ inline int code_of(const ImportArgs& a, uint32_t raw, int t, int k) {
  if constexpr (EL == kImpU8 || EL == kImpU16 || EL >= kImpPk8) {
    return min((int)(raw >> a.msb[t]), a.smax[t]);
  } else {
    float f;
    if constexpr (EL == kImpF16) f = (float)__builtin_bit_cast(_Float16, (uint16_t)raw);
    else if constexpr (EL == kImpBF16) f = __builtin_bit_cast(float, raw << 16);
    else f = __builtin_bit_cast(float, raw);
    const float r = rintf(__fadd_rn(__fmul_rn(f, a.scale[k]), a.bias[k]));      // two roundings, never one fma
    return r == r ? (int)fminf(fmaxf(r, 0.0f), (float)a.smax[t]) : 0;            // NaN: 0
  }
}

// the bit-depth rule of channel type t (TVideoIOYuv.cpp:70-87, scalePlane)
__device__ inline int to_coding(const ImportArgs& a, int v, int t) {
  const int s = a.dsh[t];
  return s >= 0 ? v << s : min(a.maxv[t], (v + (1 << (-s - 1))) >> -s);
}

__device__ inline const uint8_t* src_row(const ImportArgs& a, int k, int pic, int y) {
  return a.src[k] + (int64_t)pic * a.bstride[k] + (int64_t)y * a.pitch[k];
}

// ---- YUV sources
// luma sample (x, y) of the source, both inside it
template <int EL>
__device__ inline int yuv_luma(const ImportArgs& a, int pic, int x, int y) {
  if constexpr (EL >= kImpPk8) return to_coding(a, code_of<EL>(a, pk_raw<EL>(a, src_row(a, 0, pic, y), x, 0), 0, 0), 0);
  else return to_coding(a, code_of<EL>(a, raw_at<EL>(src_row(a, 0, pic, y), x), 0, 0), 0);
}
// chroma sample (x, y) of component comp (1 / 2) of the source's own format, both inside its plane, at the source depth
template <int EL>
__device__ inline int yuv_chroma_src(const ImportArgs& a, int pic, int comp, int x, int y) {
  if constexpr (EL >= kImpPk8) {
    return code_of<EL>(a, pk_raw<EL>(a, src_row(a, 0, pic, y), x, comp), 1, comp);
  } else {
    const bool semi = a.layout == HMGPU_EXPORT_SEMIPLANAR;
    const uint8_t* row = src_row(a, semi ? 1 : comp, pic, y);
    return code_of<EL>(a, raw_at<EL>(row, semi ? 2 * x + comp - 1 : x), 1, comp);
  }
}

// ---- RGB sources
struct Ycc { int y, cb, cr; };
__device__ inline Ycc rgb_matrix(const ImportArgs& a, int r, int g, int b) {
  Ycc o;
  if (a.coef[14]) { o.y = to_coding(a, g, 0); o.cb = to_coding(a, b, 1); o.cr = to_coding(a, r, 1); return o; }
  const int S = a.coef[0], half = a.coef[1];
  o.y = min(a.maxv[0], max(0, ((a.coef[4] * r + a.coef[5] * g + a.coef[6] * b + half) >> S) + a.coef[2]));
  o.cb = min(a.maxv[1], max(0, ((a.coef[7] * r + a.coef[8] * g + a.coef[9] * b + half) >> S) + a.coef[3]));
  o.cr = min(a.maxv[1], max(0, ((a.coef[10] * r + a.coef[11] * g + a.coef[12] * b + half) >> S) + a.coef[3]));
  return o;
}
// pixel (x, y) of the source, both inside it
template <int EL>
__device__ inline Ycc rgb_at(const ImportArgs& a, int pic, int x, int y) {
  int v[3];
  if (a.nch) {
    const uint8_t* row = src_row(a, 0, pic, y);
    for (int k = 0; k < 3; k++) v[k] = code_of<EL>(a, raw_at<EL>(row, x * a.nch + a.pos[k]), 0, k);
  } else {
    for (int k = 0; k < 3; k++) v[k] = code_of<EL>(a, raw_at<EL>(src_row(a, k, pic, y), x), 0, k);
  }
  return rgb_matrix(a, v[0], v[1], v[2]);
}

// One chroma pair of the picture, (jx, jy) in its chroma plane: the index clamped to the converted source (the padding rule), then
// the taps of each axis (ImportArgs::hw / vw from hbase / vbase on) clamped to the source's plane.  A tap of weight 0 is not loaded
// (the weights are uniform).  RGB: the source plane is Cb / Cr formed at every pixel.
template <int EL, bool RGB>
__device__ inline void chroma_taps(const ImportArgs& a, int pic, int jx, int jy, int* cb, int* cr) {
  if (!RGB && a.smono) { *cb = *cr = to_coding(a, a.cconst, 1); return; }
  jx = min(jx, a.ccw - 1); jy = min(jy, a.cch - 1);
  const int bx = ((jx << a.hl) >> a.hr) + a.h0, by = ((jy << a.vl) >> a.vr) + a.v0;
  int su = 0, sv = 0;
#pragma unroll
  for (int ty = 0; ty < 3; ty++) {
    if (!a.vw[ty]) continue;
    const int y = min(a.sch - 1, max(0, by + ty));
#pragma unroll
    for (int tx = 0; tx < 3; tx++) {
      if (!a.hw[tx]) continue;
      const int x = min(a.scw - 1, max(0, bx + tx)), w = a.vw[ty] * a.hw[tx];
      if constexpr (RGB) {
        const Ycc p = rgb_at<EL>(a, pic, x, y);
        su += w * p.cb; sv += w * p.cr;
      } else {
        su += w * yuv_chroma_src<EL>(a, pic, 1, x, y);
        sv += w * yuv_chroma_src<EL>(a, pic, 2, x, y);
      }
    }
  }
  su = (su + 8) >> 4; sv = (sv + 8) >> 4;
  if constexpr (RGB) { *cb = su; *cr = sv; }                   // (already at the coding depth)
  else { *cb = to_coding(a, su, 1); *cr = to_coding(a, sv, 1); }
}

// eight int16 from x on of a destination row, w the row's samples
__device__ inline void store8(int16_t* row, int x, int w, const int v[8], bool vec) {
  if (vec && x + 8 <= w) {
    u32x4 q;
    q.x = (uint32_t)(uint16_t)v[0] | (uint32_t)v[1] << 16; q.y = (uint32_t)(uint16_t)v[2] | (uint32_t)v[3] << 16;
    q.z = (uint32_t)(uint16_t)v[4] | (uint32_t)v[5] << 16; q.w = (uint32_t)(uint16_t)v[6] | (uint32_t)v[7] << 16;
    stg4(row + x, q);
    return;
  }
  for (int i = 0; i < 8; i++) if (x + i < w) stg(row + x + i, (int16_t)v[i]);
}

// PX: RGB as packed pixels (an instance of its own: the whole-group loads of packed pixels take registers the planes do not need)
template <int EL, bool RGB, bool PX>
__global__ __launch_bounds__(256) void k_import(const ImportArgs a) {
  const int X0 = 8 * (blockIdx.x * blockDim.x + threadIdx.x), unit = blockIdx.y * blockDim.y + threadIdx.y, pic = blockIdx.z;
  const int R = 1 << a.psy, Y0 = unit << a.psy;
  if (X0 >= a.w || Y0 >= a.h) return;
  const bool inside = X0 + 8 <= a.sw && Y0 + R <= a.sh;       // the lane's samples all come from their own source positions
  int yv[2][8], cv[16];
  // ---- luma (RGB: and Cb / Cr at every pixel of the lane, for the DROP rule)
  int fcb[2][8], fcr[2][8];
#pragma unroll
  for (int r = 0; r < 2; r++) {
    if (r >= R) break;
    const int ys = min(Y0 + r, a.sh - 1);
    if constexpr (RGB) {
      if (inside && (PX ? (a.vec & 1) : (a.vec & 7) == 7)) {
        uint32_t q[3][8];
        if constexpr (PX) {
          if (a.nch == 3) raw8_px<EL, 3>(src_row(a, 0, pic, ys), 3 * X0, a.pos, q);
          else raw8_px<EL, 4>(src_row(a, 0, pic, ys), 4 * X0, a.pos, q);
        } else {
          for (int k = 0; k < 3; k++) raw8<EL>(src_row(a, k, pic, ys), X0, q[k]);
        }
        for (int i = 0; i < 8; i++) {
          const Ycc p = rgb_matrix(a, code_of<EL>(a, q[0][i], 0, 0), code_of<EL>(a, q[1][i], 0, 1), code_of<EL>(a, q[2][i], 0, 2));
          yv[r][i] = p.y; fcb[r][i] = p.cb; fcr[r][i] = p.cr;
        }
      } else {
        for (int i = 0; i < 8; i++) {
          const Ycc p = rgb_at<EL>(a, pic, min(X0 + i, a.sw - 1), ys);
          yv[r][i] = p.y; fcb[r][i] = p.cb; fcr[r][i] = p.cr;
        }
      }
    } else {
      if (EL < kImpPk8 && inside && (a.vec & 1)) {
        uint32_t q[8];
        raw8<EL>(src_row(a, 0, pic, ys), X0, q);
        for (int i = 0; i < 8; i++) yv[r][i] = to_coding(a, code_of<EL>(a, q[i], 0, 0), 0);
      } else {
        for (int i = 0; i < 8; i++) yv[r][i] = yuv_luma<EL>(a, pic, min(X0 + i, a.sw - 1), ys);
      }
    }
  }
  // ---- the pairs beneath: 8 >> psx of them on chroma row `unit`
  const int np = 8 >> a.psx, J0 = X0 >> a.psx;
  if (!a.mono) {
    if (RGB && inside && a.drop) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        if (j >= np) break;
        cv[2 * j] = fcb[0][j << a.psx]; cv[2 * j + 1] = fcr[0][j << a.psx];
      }
    } else if (!RGB && EL < kImpPk8 && inside && a.same && a.layout == HMGPU_EXPORT_SEMIPLANAR && (a.vec & 2)) {
      // the source's pair plane has the picture's shape: np pairs are 2 * np consecutive elements
#pragma unroll
      for (int g = 0; g < 2; g++) {
        if (8 * g >= 2 * np) break;
        uint32_t q[8];
        raw8<EL>(src_row(a, 1, pic, unit), 2 * J0 + 8 * g, q);
        for (int i = 0; i < 8; i++) cv[8 * g + i] = to_coding(a, code_of<EL>(a, q[i], 1, 1 + (i & 1)), 1);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        if (j >= np) break;
        chroma_taps<EL, RGB>(a, pic, J0 + j, unit, &cv[2 * j], &cv[2 * j + 1]);
      }
    }
  }
  // ---- stores
  const bool vst = (a.vec >> 8) & 1;
#pragma unroll
  for (int r = 0; r < 2; r++) {
    if (r >= R) break;
    store8(a.y[pic] + (int64_t)(Y0 + r) * a.pitch_y, X0, a.w, yv[r], vst);
  }
  if (!a.mono) {
    int16_t* row = a.c[pic] + (int64_t)unit * a.pitch_c;
    const int cw2 = 2 * (a.w >> a.psx);
    store8(row, 2 * J0, cw2, cv, vst);
    if (np == 8) store8(row, 2 * J0 + 8, cw2, cv + 8, vst);
  }
}

template <bool RGB, bool PX>
void launch_elem(const ImportArgs& a, dim3 grid, dim3 block, hipStream_t s) {
  switch (a.elem) {
    case kImpU8: hipLaunchKernelGGL((k_import<kImpU8, RGB, PX>), grid, block, 0, s, a); break;
    case kImpU16: hipLaunchKernelGGL((k_import<kImpU16, RGB, PX>), grid, block, 0, s, a); break;
    case kImpF16: hipLaunchKernelGGL((k_import<kImpF16, RGB, PX>), grid, block, 0, s, a); break;
    case kImpBF16: hipLaunchKernelGGL((k_import<kImpBF16, RGB, PX>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((k_import<kImpF32, RGB, PX>), grid, block, 0, s, a); break;
  }
}

}  // namespace

void launch_import(const ImportArgs& a, hipStream_t s) {
  const dim3 block(32, 8);
  const int groups = (a.w + 7) / 8, units = a.h >> a.psy;
  const dim3 grid((groups + 31) / 32, (units + 7) / 8, a.n);
  if (a.elem == kImpPk8) hipLaunchKernelGGL((k_import<kImpPk8, false, false>), grid, block, 0, s, a);
  else if (a.elem == kImpPk16) hipLaunchKernelGGL((k_import<kImpPk16, false, false>), grid, block, 0, s, a);
  else if (a.elem == kImpPk32) hipLaunchKernelGGL((k_import<kImpPk32, false, false>), grid, block, 0, s, a);
  else if (a.layout != HMGPU_EXPORT_RGB) launch_elem<false, false>(a, grid, block, s);
  else if (a.nch) launch_elem<true, true>(a, grid, block, s);
  else launch_elem<true, false>(a, grid, block, s);
}

}  // namespace hmgpu
