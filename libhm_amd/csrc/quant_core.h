// quant_core.h -- what the flattener and the side-information exports share of the quantiser: QpParam of a block (k_prep.hip lists it
// with every transform unit, k_transform.hip de-quantises with it) and the output element of an int16 value (k_residual.hip,
// k_transform.hip).
#pragma once
#include "hmgpu_dev.h"

namespace hmgpu {

static __constant__ uint8_t c_chroma_scale_420[58] = {   // HM g_aucChromaScale[CHROMA_420], TComRom.cpp:503
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
    29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51};

// QpParam (TComTrQuant.cpp:71-100); fmt: chroma_format_idc -- the 4:2:0 table, min(qPi, 51) otherwise (g_aucChromaScale, TComRom.cpp:499-506)
__device__ inline void qp_param(int qp_y, int comp, int bd, int chroma_off, int fmt, int8_t& per, int8_t& rem) {
  const int bdo = 6 * (bd - 8);
  int base;
  if (comp == 0) base = qp_y + bdo;
  else {
    base = clip3(-bdo, 57, qp_y + chroma_off);
    base = base < 0 ? base + bdo : (fmt == 1 ? c_chroma_scale_420[base] : min(base, 51)) + bdo;
  }
  per = (int8_t)(base / 6);
  rem = (int8_t)(base % 6);
}

// the output element of the int16 value r: as it is, or convert((float)r * sc) -- one binary32 product, then the conversion of the
// batched tensor export (float16 / bfloat16: nearest even)
template <int ELEM> __device__ inline uint32_t resid_elem(int r, float sc) {
  if constexpr (ELEM == kElemU16) return (uint32_t)r & 0xffffu;
  else {
    float f = (float)r * sc;
    // the product is rounded to binary32 and keeps its sign when it is zero: without this fence the compiler folds product and
    // conversion into one mixed-precision fma with a +0 addend, which turns -0 (r = 0, sc < 0) into +0
    if constexpr (ELEM == kElemF16) asm("" : "+v"(f));
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    if constexpr (ELEM == kElemF32) return u;
    else if constexpr (ELEM == kElemF16) return __builtin_bit_cast(uint16_t, (_Float16)f);
    else return ((u + 0x7fffu + ((u >> 16) & 1u)) >> 16) & 0xffffu;       // (f is never a NaN: r and sc are finite)
  }
}

}  // namespace hmgpu
