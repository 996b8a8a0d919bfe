// hmgpu_import.hip -- picture import of the host runtime (include/hmgpu.h "picture import", k_import.hip): the rules of the
// descriptor and the plan, the forward RGB coefficients, the taps of a chroma conversion, the source check and the one launch with
// the picture state of an upload and the stream bracket of the exports.
#include "hmgpu_host.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace {

long long round_half_away(double v) { return v < 0 ? -(long long)std::floor(-v + 0.5) : (long long)std::floor(v + 0.5); }

bool matrix_kr_kb(int matrix, double* kr, double* kb) {       // H.273 Table 4, the codes of the exports
  switch (matrix) {
    case 1: *kr = 0.2126; *kb = 0.0722; return true;
    case 5: case 6: *kr = 0.299; *kb = 0.114; return true;
    case 9: *kr = 0.2627; *kb = 0.0593; return true;
    default: return false;
  }
}

// what a validated descriptor means for a sequence
struct ImportRules {
  int W, H, sw, sh;            // coded size, source size
  int fs, fp;                  // source / picture chroma format (RGB source: 3)
  int D[2];                    // source depth per channel type
  int ES, nch;                 // element bytes; packed pixels: elements per pixel (else 0)
  int elem;                    // ImportArgs::elem
  bool rgb, mono, smono, flt;
};

// the forward matrix in integers (include/hmgpu.h has the formula); false: no shift fits
bool rgb_coef(const hmgpu_seq_params* seq, const hmgpu_import_desc* d, int D, double kr, double kb, int32_t coef[16]) {
  const int bdY = seq->bit_depth_luma, bdC = seq->bit_depth_chroma;
  const double M = (double)((1 << D) - 1);
  const double ys = d->full_range ? (double)((1 << bdY) - 1) : (double)(219 << (bdY - 8));
  const double cs = d->full_range ? (double)((1 << bdC) - 1) : (double)(224 << (bdC - 8));
  for (int S = 30; S >= 1; S--) {
    const double q = (double)(1LL << S);
    long long c[9];
    c[0] = round_half_away(kr * ys / M * q); c[2] = round_half_away(kb * ys / M * q); c[1] = round_half_away(ys / M * q) - c[0] - c[2];
    c[5] = round_half_away(cs / (2 * M) * q); c[3] = round_half_away(-kr / (1 - kb) * cs / (2 * M) * q); c[4] = -(c[3] + c[5]);
    c[6] = round_half_away(cs / (2 * M) * q); c[8] = round_half_away(-kb / (1 - kr) * cs / (2 * M) * q); c[7] = -(c[6] + c[8]);
    long long bound = 0;
    for (int r = 0; r < 3; r++) {
      long long pos = 0, neg = 0;
      for (int k = 0; k < 3; k++) (c[3 * r + k] > 0 ? pos : neg) += std::llabs(c[3 * r + k]);
      bound = std::max(bound, std::max(pos, neg) * (long long)M + (1LL << (S - 1)));
    }
    if (bound > INT32_MAX) continue;
    coef[0] = S; coef[1] = 1 << (S - 1); coef[2] = d->full_range ? 0 : 16 << (bdY - 8); coef[3] = 1 << (bdC - 1);
    for (int k = 0; k < 9; k++) coef[4 + k] = (int32_t)c[k];
    return true;
  }
  return false;
}

// steps 1 and 2 of the validation, the plan, and the rules the launch needs
hmgpu_status import_rules(const hmgpu_seq_params* seq, const hmgpu_import_desc* d, hmgpu_import_plan* out, ImportRules* r) {
  if (out) memset(out, 0, sizeof(*out));                      // (a refused plan is all zero)
  if (!seq || !d || !out) return HMGPU_EINVAL;
  const int fp = seq->chroma_format, bdY = seq->bit_depth_luma, bdC = seq->bit_depth_chroma;
  if (fp < 0 || fp > 3 || bdY < 8 || bdY > 12 || bdC < 8 || bdC > 12 || seq->width <= 0 || seq->height <= 0) return HMGPU_EINVAL;
  // ---- 1
  for (int k = 0; k < 8; k++) if (d->reserved[k]) return HMGPU_EINVAL;
  if (d->layout < HMGPU_EXPORT_PLANAR || d->layout > HMGPU_EXPORT_RGB) return HMGPU_EINVAL;
  const bool rgb = d->layout == HMGPU_EXPORT_RGB;
  if (d->order < -1 || d->order > HMGPU_PIXEL_ABGR || (!rgb && d->order != -1)) return HMGPU_EINVAL;
  const bool flt = d->sample_type != HMGPU_SAMPLE_UINT;
  const int fs = rgb ? 3 : d->chroma_format;
  if (!rgb && (fs < 0 || fs > 3)) return HMGPU_EINVAL;
  const bool mono = fp == 0, smono = fs == 0;
  int D[2] = {d->bit_depth[0] ? d->bit_depth[0] : bdY, rgb ? 0 : d->bit_depth[1] ? d->bit_depth[1] : bdC};
  if (rgb) D[1] = D[0];
  if (d->bytes_per_sample != 1 && d->bytes_per_sample != 2) return HMGPU_EINVAL;
  if ((d->msb_aligned != 0 && d->msb_aligned != 1) || (d->msb_aligned && (d->bytes_per_sample != 2 || flt))) return HMGPU_EINVAL;
  const int types = !rgb && mono ? 1 : 2;                     // (a 4:0:0 picture reads no chroma: its depth is not looked at)
  int dmax = 0;
  for (int t = 0; t < types; t++) {
    if (D[t] < 1 || D[t] > 16 || (!flt && d->bytes_per_sample == 1 && D[t] > 8)) return HMGPU_EINVAL;
    dmax = std::max(dmax, D[t]);
  }
  if (flt) {
    if (d->bytes_per_sample != (dmax > 8 ? 2 : 1)) return HMGPU_EINVAL;
    for (int k = 0; k < 3; k++) if (!std::isfinite(d->scale[k]) || !std::isfinite(d->bias[k])) return HMGPU_EINVAL;
  }
  const int W = seq->width, H = seq->height, sw = d->width ? d->width : W, sh = d->height ? d->height : H;
  if (sw < 1 || sh < 1 || sw > W || sh > H) return HMGPU_EINVAL;
  int ssx = 0, ssy = 0, psx = 0, psy = 0;
  if (!smono) chroma_shifts(fs, &ssx, &ssy);
  if (!mono) chroma_shifts(fp, &psx, &psy);
  if (((sw & ((1 << ssx) - 1)) | (sw & ((1 << psx) - 1)) | (sh & ((1 << ssy) - 1)) | (sh & ((1 << psy) - 1))) != 0) return HMGPU_EINVAL;
  if (d->loc < 0 || d->loc > 5) return HMGPU_EINVAL;
  if (rgb && ((d->full_range != 0 && d->full_range != 1) || (d->matrix == 0 && fp != 3))) return HMGPU_EINVAL;
  // ---- 2
  double kr = 0, kb = 0;
  if (rgb && d->matrix != 0 && !matrix_kr_kb(d->matrix, &kr, &kb)) return HMGPU_EUNSUPPORTED;
  if (d->down != HMGPU_DOWN_DROP && d->down != HMGPU_DOWN_LINEAR) return HMGPU_EUNSUPPORTED;
  if (d->sample_type < HMGPU_SAMPLE_UINT || d->sample_type > HMGPU_SAMPLE_F32) return HMGPU_EUNSUPPORTED;
  if (flt && d->layout == HMGPU_EXPORT_SEMIPLANAR) return HMGPU_EUNSUPPORTED;
  // ---- the plan
  const int ES = d->sample_type == HMGPU_SAMPLE_UINT ? d->bytes_per_sample : d->sample_type == HMGPU_SAMPLE_F32 ? 4 : 2;
  const int nch = !rgb || d->order < 0 ? 0 : d->order <= HMGPU_PIXEL_BGR ? 3 : 4;
  if (rgb) {
    out->planes = nch ? 1 : 3;
    for (int k = 0; k < out->planes; k++) { out->width[k] = sw; out->height[k] = sh; out->row_bytes[k] = sw * (nch ? nch : 1) * ES; }
    out->coef[13] = (1 << D[0]) - 1;
    if (d->matrix == 0) out->coef[14] = 1;
    else if (!rgb_coef(seq, d, D[0], kr, kb, out->coef)) { memset(out, 0, sizeof(*out)); return HMGPU_EUNSUPPORTED; }
  } else {
    out->planes = smono || mono ? 1 : d->layout == HMGPU_EXPORT_PLANAR ? 3 : 2;
    out->width[0] = sw; out->height[0] = sh; out->row_bytes[0] = sw * ES;
    for (int k = 1; k < out->planes; k++) {
      out->width[k] = sw >> ssx; out->height[k] = sh >> ssy;
      out->row_bytes[k] = (d->layout == HMGPU_EXPORT_PLANAR ? 1 : 2) * out->width[k] * ES;
    }
  }
  if (r) {
    r->W = W; r->H = H; r->sw = sw; r->sh = sh; r->fs = fs; r->fp = fp; r->D[0] = D[0]; r->D[1] = types == 2 ? D[1] : D[0];
    r->ES = ES; r->nch = nch; r->rgb = rgb; r->mono = mono; r->smono = smono; r->flt = flt;
    r->elem = !flt ? d->bytes_per_sample - 1 : 1 + d->sample_type;
  }
  return HMGPU_OK;
}

// steps 3 and 5: n, then the planes of the plan as device memory of the context's GPU.  *vec: ImportArgs::vec bits 0 .. 2
hmgpu_status source_ok(const hmgpu_ctx* c, int32_t n, const hmgpu_import_plan& plan, int ES, const void* const src[3],
                       const int64_t pitch[3], const int64_t bstride[3], uint32_t* vec) {
  if (n < 1 || n > HMGPU_EXPORT_MAX_BATCH) return HMGPU_EINVAL;
  if (!src || !pitch || !bstride) return HMGPU_EINVAL;
  hipSetDevice(c->device);
  *vec = 0;
  for (int k = 0; k < plan.planes; k++) {
    if (!src[k]) return HMGPU_EINVAL;
    if ((uintptr_t)src[k] % ES || pitch[k] % ES || bstride[k] % ES) return HMGPU_EINVAL;
    if (pitch[k] < plan.row_bytes[k] || pitch[k] > ((int64_t)1 << 40)) return HMGPU_EINVAL;
    const int64_t plane = pitch[k] * (plan.height[k] - 1) + plan.row_bytes[k];
    if (bstride[k] < plane || bstride[k] > ((int64_t)1 << 56)) return HMGPU_EINVAL;
    if (!device_span_ok(src[k], (size_t)((n - 1) * bstride[k] + plane), c->device)) return HMGPU_EINVAL;
    const int64_t g = 8 * ES;
    if ((uintptr_t)src[k] % g == 0 && pitch[k] % g == 0 && bstride[k] % g == 0) *vec |= 1u << k;
  }
  return HMGPU_OK;
}

// the taps of one axis (ImportArgs): gain > 0 the picture has more samples on it, < 0 fewer; siting: 0 co-sited, 1 centred, 2 bottom
void axis_taps(int gain, bool linear, int siting, int32_t* l, int32_t* r, int32_t* first, int32_t w[3]) {
  *l = gain < 0; *r = gain > 0; *first = 0;
  w[0] = 4; w[1] = w[2] = 0;                                  // the sample itself, j >> 1, 2j
  if (gain < 0 && linear) {
    if (siting == 0) { *first = -1; w[0] = 1; w[1] = 2; w[2] = 1; }
    else if (siting == 1) { w[0] = 2; w[1] = 2; }
    else { w[0] = 1; w[1] = 2; w[2] = 1; }
  }
}

// Steps 1 and 2 of a packed YUV import (include/hmgpu.h), in front of the steps of the planar import that defines it; *dd: the
// descriptor of that import, *pf: the word format
hmgpu_status import_yuvpack_rules(const hmgpu_import_desc* d, const hmgpu_import_yuvpack* pack, hmgpu_import_desc* dd, YuvPackFormat* pf) {
  if (!pack) return HMGPU_EINVAL;
  for (int k = 0; k < 7; k++) if (pack->reserved[k]) return HMGPU_EINVAL;
  if (!yuvpack_format(pack->format, pf)) return HMGPU_EUNSUPPORTED;
  const int B = pf->depth <= 8 ? 1 : 2;
  if (!d || d->layout != HMGPU_EXPORT_PLANAR || d->order != -1 || d->chroma_format != pf->cf) return HMGPU_EINVAL;
  for (int k = 0; k < 2; k++) if (d->bit_depth[k] != 0 && d->bit_depth[k] != pf->depth) return HMGPU_EINVAL;
  if ((d->bytes_per_sample != 0 && d->bytes_per_sample != B) || d->sample_type != HMGPU_SAMPLE_UINT || d->msb_aligned != 0) return HMGPU_EINVAL;
  *dd = *d;
  dd->bit_depth[0] = dd->bit_depth[1] = pf->depth;
  dd->bytes_per_sample = B;
  return HMGPU_OK;
}

// import_rules of a packed YUV source: the planar plan becomes the one plane of words
hmgpu_status import_yuvpack_plan(const hmgpu_seq_params* seq, const hmgpu_import_desc* d, const hmgpu_import_yuvpack* pack,
                                 hmgpu_import_plan* out, ImportRules* r, hmgpu_import_desc* dd, YuvPackFormat* pf) {
  if (out) memset(out, 0, sizeof(*out));
  if (!seq || !out) return HMGPU_EINVAL;
  { const hmgpu_status st = import_yuvpack_rules(d, pack, dd, pf); if (st != HMGPU_OK) return st; }
  { const hmgpu_status st = import_rules(seq, dd, out, r); if (st != HMGPU_OK) return st; }
  const int sw = out->width[0], sh = out->height[0];
  memset(out, 0, sizeof(*out));
  out->planes = 1;
  out->width[0] = sw; out->height[0] = sh; out->row_bytes[0] = yuvpack_row_bytes(*pf, sw);
  return HMGPU_OK;
}

// the unused planes of a packed source
bool only_plane_0(const void* const src[3]) { return !src || (!src[1] && !src[2]); }

}  // namespace

extern "C" {

static hmgpu_status import_impl(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_import_desc* d, const hmgpu_import_yuvpack* pack,
                                bool packed, const void* const src[3], const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3],
                                int32_t on_stream, void* stream);

hmgpu_status hmgpu_import_yuvpack_plan_for(const hmgpu_seq_params* seq, const hmgpu_import_desc* d, const hmgpu_import_yuvpack* pack,
                                           hmgpu_import_plan* out) {
  ImportRules r;
  hmgpu_import_desc dd;
  YuvPackFormat pf;
  return import_yuvpack_plan(seq, d, pack, out, &r, &dd, &pf);
}

hmgpu_status hmgpu_import_yuvpack_source_check(hmgpu_ctx* c, int32_t n, const hmgpu_import_desc* d, const hmgpu_import_yuvpack* pack,
                                               const void* const src[3], const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3]) {
  if (!c) return HMGPU_EINVAL;
  hmgpu_import_plan plan;
  ImportRules r;
  hmgpu_import_desc dd;
  YuvPackFormat pf;
  { const hmgpu_status st = import_yuvpack_plan(&c->seq, d, pack, &plan, &r, &dd, &pf); if (st != HMGPU_OK) return st; }
  uint32_t vec;
  { const hmgpu_status st = source_ok(c, n, plan, pf.align, src, pitch_bytes, batch_stride_bytes, &vec); if (st != HMGPU_OK) return st; }
  return only_plane_0(src) ? HMGPU_OK : HMGPU_EINVAL;
}

hmgpu_status hmgpu_pictures_import_yuvpack(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_import_desc* d,
                                           const hmgpu_import_yuvpack* pack, const void* const src[3], const int64_t pitch_bytes[3],
                                           const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream) {
  return import_impl(c, n, pics, d, pack, true, src, pitch_bytes, batch_stride_bytes, on_stream, stream);
}

hmgpu_status hmgpu_import_plan_for(const hmgpu_seq_params* seq, const hmgpu_import_desc* d, hmgpu_import_plan* out) {
  return import_rules(seq, d, out, nullptr);
}

hmgpu_status hmgpu_import_source_check(hmgpu_ctx* c, int32_t n, const hmgpu_import_desc* d, const void* const src[3],
                                       const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3]) {
  if (!c) return HMGPU_EINVAL;
  hmgpu_import_plan plan;
  ImportRules r;
  { const hmgpu_status st = import_rules(&c->seq, d, &plan, &r); if (st != HMGPU_OK) return st; }
  uint32_t vec;
  return source_ok(c, n, plan, r.ES, src, pitch_bytes, batch_stride_bytes, &vec);
}

hmgpu_status hmgpu_pictures_import(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_import_desc* d, const void* const src[3],
                                   const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream) {
  return import_impl(c, n, pics, d, nullptr, false, src, pitch_bytes, batch_stride_bytes, on_stream, stream);
}

// both imports: planes (packed false), or the words of `pack` in src[0], which are the planar source of the descriptor dd
static hmgpu_status import_impl(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_import_desc* d, const hmgpu_import_yuvpack* pack,
                                bool packed, const void* const src[3], const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3],
                                int32_t on_stream, void* stream) {
  if (!c) return HMGPU_EINVAL;
  hmgpu_import_plan plan;
  ImportRules r;
  hmgpu_import_desc dd;
  YuvPackFormat pf;
  if (packed) {
    const hmgpu_status st = import_yuvpack_plan(&c->seq, d, pack, &plan, &r, &dd, &pf);
    if (st != HMGPU_OK) return st;
    d = &dd;
    r.ES = pf.align;
  } else {
    const hmgpu_status st = import_rules(&c->seq, d, &plan, &r);
    if (st != HMGPU_OK) return st;
  }
  if (n < 1 || n > HMGPU_EXPORT_MAX_BATCH || !pics) return HMGPU_EINVAL;
  for (int i = 0; i < n; i++) {
    if (!valid_pic(c, pics[i])) return HMGPU_EINVAL;
    for (int j = 0; j < i; j++) if (pics[j] == pics[i]) return HMGPU_EINVAL;       // two writers of one picture
  }
  uint32_t vec = 0;
  { const hmgpu_status st = source_ok(c, n, plan, r.ES, src, pitch_bytes, batch_stride_bytes, &vec); if (st != HMGPU_OK) return st; }
  if (packed && !only_plane_0(src)) return HMGPU_EINVAL;
  if (on_stream != 0 && on_stream != 1) return HMGPU_EINVAL;
  if (on_stream && stream) {                                   // (export_open makes the same check, behind the picture state)
    hipDevice_t dev = -1;
    if (hipStreamGetDevice((hipStream_t)stream, &dev) != hipSuccess) { (void)hipGetLastError(); return HMGPU_EINVAL; }
    if ((int)dev != c->device) return HMGPU_EINVAL;
  }

  ImportArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n; a.layout = d->layout; a.elem = r.elem; a.nch = r.nch;
  if (r.nch) {
    static const int8_t kPos[6][3] = {{0, 1, 2}, {2, 1, 0}, {0, 1, 2}, {2, 1, 0}, {1, 2, 3}, {3, 2, 1}};   // R, G, B in RGB BGR RGBA BGRA ARGB ABGR
    for (int k = 0; k < 3; k++) a.pos[k] = kPos[d->order][k];
  }
  a.w = r.W; a.h = r.H; a.sw = r.sw; a.sh = r.sh;
  a.mono = r.mono; a.smono = r.smono;
  int ssx = 0, ssy = 0;
  if (!r.mono) chroma_shifts(r.fp, &a.psx, &a.psy);
  if (!r.smono) chroma_shifts(r.fs, &ssx, &ssy);
  a.same = !r.rgb && !r.smono && !r.mono && ssx == a.psx && ssy == a.psy;
  a.ccw = r.sw >> a.psx; a.cch = r.sh >> a.psy; a.scw = r.sw >> ssx; a.sch = r.sh >> ssy;
  const bool lin = d->down == HMGPU_DOWN_LINEAR;
  axis_taps(ssx - a.psx, lin, r.fp == 1 && (d->loc & 1) ? 1 : 0, &a.hl, &a.hr, &a.h0, a.hw);
  axis_taps(ssy - a.psy, lin, d->loc < 2 ? 1 : d->loc < 4 ? 0 : 2, &a.vl, &a.vr, &a.v0, a.vw);
  a.drop = a.hw[0] == 4 && a.vw[0] == 4;
  const int bd[2] = {c->seq.bit_depth_luma, c->seq.bit_depth_chroma};
  for (int t = 0; t < 2; t++) {
    a.dsh[t] = bd[t] - r.D[t]; a.maxv[t] = (1 << bd[t]) - 1; a.smax[t] = (1 << r.D[t]) - 1;
    a.msb[t] = d->msb_aligned ? 16 - r.D[t] : 0;
  }
  a.cconst = 1 << (r.D[1] - 1);
  if (packed) {                                                // the accessor of the words; no whole-group loads of planes
    // per format: luma stride and offset, chroma stride, Cb and Cr offsets, in elements
    static const int8_t kAt[8][5] = {{2, 1, 4, 0, 2}, {2, 0, 4, 1, 3}, {2, 0, 4, 1, 3}, {2, 0, 4, 1, 3}, {0, 0, 0, 0, 0},
                                     {4, 2, 4, 1, 0}, {0, 0, 0, 0, 0}, {4, 1, 4, 0, 2}};
    const int8_t* at = kAt[pack->format];
    a.elem = pf.align == 1 ? 5 : pf.align == 2 ? 6 : 7;
    a.pk_ls = at[0]; a.pk_lo = at[1]; a.pk_cs = at[2]; a.pk_co[0] = at[3]; a.pk_co[1] = at[4];
    a.pk_v210 = pack->format == HMGPU_YUVPACK_V210;
    a.msb[0] = a.msb[1] = pf.shift;
    vec = 0;
  }
  for (int k = 0; k < 3; k++) {
    a.scale[k] = d->scale[k]; a.bias[k] = d->bias[k];
    if (k < plan.planes) { a.src[k] = (const uint8_t*)src[k]; a.pitch[k] = pitch_bytes[k]; a.bstride[k] = batch_stride_bytes[k]; }
  }
  memcpy(a.coef, plan.coef, sizeof(a.coef));
  a.pitch_y = c->pitch[0]; a.pitch_c = c->pitch[1];
  bool vst = a.pitch_y % 8 == 0 && a.pitch_c % 8 == 0;

  // the state an upload leaves: the samples ARE the picture, in the reconstruction planes, without side information
  for (int i = 0; i < n; i++) {
    Picture& p = c->pics[pics[i]];
    coverage_clear(p);
    filter_forget(p);
    if (p.sao_applied) {
      p.sao_applied = false; p.dev.sao_applied = 0;
      hmgpu_status st = push_final(c, pics[i], c->stream);
      if (st == HMGPU_OK) st = push_picdev(c, pics[i]);
      if (st != HMGPU_OK) return st;
    }
    p.extended = false;
    a.y[i] = p.dev.rec[0]; a.c[i] = p.dev.rec[1];
    vst = vst && (uintptr_t)a.y[i] % 16 == 0 && (uintptr_t)a.c[i] % 16 == 0;
  }
  a.vec = vec | (vst ? 1u << 8 : 0);
  hipStream_t hs = c->stream;
  { const hmgpu_status st = export_open(c, on_stream, stream, &hs); if (st != HMGPU_OK) return st; }
  launch_import(a, hs);
  return export_end(c, n, pics, on_stream, hs);
}

}  // extern "C"
