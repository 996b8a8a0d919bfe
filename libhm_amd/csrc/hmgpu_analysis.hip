// hmgpu_analysis.hip -- picture analysis of the host runtime: the picture metrics, the picture metric maps and the picture histograms.
// Per family one plan and one *_resolve under the check and the launching entry (k_metrics.hip, k_metrics_map.hip, k_histogram.hip).
#include "hmgpu_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>

// what MetricsArgs and MetricsMapArgs share: the SSIM constants, per plane class the cropped plane, per picture the first sample of
// both sides and whether its groups of 4 take one load, the caller's planes
template <class Args>
static void metrics_sources(hmgpu_ctx* c, int n, const hmgpu_pic* pics, const hmgpu_metrics_desc* d, const hmgpu_pic* ref_pics,
                            const void* const* ref, const int64_t* ref_pitch, const int64_t* ref_bstride, const hmgpu_metrics_plan& plan, int vec,
                            Args* out) {
  Args& a = *out;
  const bool planes = d->reference == HMGPU_METRICS_REF_PLANES;
  a.n = n;
  const int bd[2] = {c->seq.bit_depth_luma, c->seq.bit_depth_chroma};
  for (int k = 0; k < 2; k++) {
    const double maxv = (double)((1 << bd[k]) - 1);
    a.c1[k] = (int64_t)(.01 * .01 * maxv * maxv * 64 + .5);
    a.c2[k] = (int64_t)(.03 * .03 * maxv * maxv * 64 * 63 + .5);
    const int comp = k ? (plan.channels[1] ? 1 : 2) : 0;             // a component of the class that is compared, if any
    if (!plan.channels[comp]) continue;
    a.w[k] = plan.width[comp]; a.h[k] = plan.height[comp]; a.pitch[k] = c->pitch[k];
  }
  for (int k = 0; k < 3; k++) {
    if (!plan.channels[k]) continue;
    a.comps |= 1 << k;
    if (planes) { a.bq[k] = static_cast<const uint8_t*>(ref[k]); a.bpitch[k] = ref_pitch[k]; a.bstride[k] = ref_bstride[k]; }
  }
  a.bvec = (uint32_t)vec;
  const int x0 = d->crop[0], y0 = d->crop[2];
  for (int i = 0; i < n; i++) {
    for (int side = 0; side < (planes ? 1 : 2); side++) {
      const Picture& p = c->pics[side ? ref_pics[i] : pics[i]];
      int16_t* const* src = p.sao_applied ? p.dev.sao : p.dev.rec;
      const int16_t* org[2] = {src[0] + (ptrdiff_t)y0 * c->pitch[0] + x0, src[1] + (ptrdiff_t)(y0 >> c->csy) * c->pitch[1] + kCStep * (x0 >> c->csx)};
      for (int k = 0; k < 2; k++) {
        (side ? a.bp : a.a)[i][k] = org[k];
        const size_t g = k ? 16 : 8;                                   // a group of 4 samples, of 4 pairs
        if (side == 0) a.avec[k] |= 1u << i;
        if ((uintptr_t)org[k] % g || ((size_t)c->pitch[k] * 2) % g) a.avec[k] &= ~(1u << i);
      }
    }
  }
}

extern "C" {

// ------------------------------------------------------------------------------------------------ picture metrics (k_metrics.hip)
// hmgpu_metrics_plan_for; the plan's channels / elem_bytes / row_bytes / height describe the reference planes to strided_dst_ok
static hmgpu_status metrics_plan(const hmgpu_seq_params* seq, const hmgpu_metrics_desc* d, hmgpu_metrics_plan* out) {
  if (!seq || !d || !out) return HMGPU_EINVAL;
  memset(out, 0, sizeof(*out));
  const int fmt = seq->chroma_format, bd[2] = {seq->bit_depth_luma, seq->bit_depth_chroma};
  if (fmt < 0 || fmt > 3 || bd[0] < 8 || bd[0] > 12 || bd[1] < 8 || bd[1] > 12 || seq->width <= 0 || seq->height <= 0) return HMGPU_EINVAL;
  for (int k = 0; k < 7; k++) if (d->reserved[k]) return HMGPU_EINVAL;
  if (d->reference != HMGPU_METRICS_REF_PICTURES && d->reference != HMGPU_METRICS_REF_PLANES) return HMGPU_EINVAL;
  if (d->components < 1 || d->components > 7 || (d->ssim != 0 && d->ssim != 1)) return HMGPU_EINVAL;
  const bool planes = d->reference == HMGPU_METRICS_REF_PLANES;
  const int B = d->ref_bytes_per_sample;
  if (planes ? (B != 1 && B != 2) : B != 0) return HMGPU_EINVAL;
  const int comps = fmt == 0 ? d->components & 1 : d->components;
  if (!comps) return HMGPU_EINVAL;                                    // (4:0:0: the chroma bits alone select nothing)
  int W, H, csx, csy;
  { const hmgpu_status st = crop_ok(seq, d->crop, nullptr, &W, &H); if (st != HMGPU_OK) return st; }
  chroma_shifts(fmt, &csx, &csy);
  for (int k = 0; k < 3; k++) {
    if (!((comps >> k) & 1)) continue;
    if (B == 1 && bd[k ? 1 : 0] > 8) return HMGPU_EINVAL;
    const int w = k ? W >> csx : W, h = k ? H >> csy : H;
    if ((int64_t)w * h >= 0xffffffffll) return HMGPU_EUNSUPPORTED;     // a lane of k_metrics keeps y * w + x in 32 bits, all ones: none
    out->channels[k] = 1; out->width[k] = w; out->height[k] = h;
    out->elem_bytes[k] = B; out->row_bytes[k] = w * B;
    out->ssim_windows[k] = d->ssim && w >= 8 && h >= 8 ? (int64_t)((w >> 2) - 1) * ((h >> 2) - 1) : 0;
  }
  out->result_bytes = 3 * (int)sizeof(hmgpu_metrics_result);
  return HMGPU_OK;
}

hmgpu_status hmgpu_metrics_plan_for(const hmgpu_seq_params* seq, const hmgpu_metrics_desc* d, hmgpu_metrics_plan* out) {
  const hmgpu_status st = metrics_plan(seq, d, out);
  if (st != HMGPU_OK && out) memset(out, 0, sizeof(*out));
  return st;
}

double hmgpu_metrics_psnr(const hmgpu_metrics_result* r, int32_t bit_depth) {
  if (!r || bit_depth < 8 || bit_depth > 16) return NAN;
  if (!r->sse) return 999.99;
  const int maxval = 255 << (bit_depth - 8);
  const double ref = (double)maxval * maxval * (double)r->samples;     // (fRefValue of TEncGOP::xCalculateAddPSNR)
  return 10.0 * std::log10(ref / (double)r->sse);
}

// what hmgpu_pictures_metrics and hmgpu_pictures_metrics_map check of their pictures and of the reference, behind the description's plan;
// vec: bit c: the planes of component c take whole loads of 4 elements
static hmgpu_status metrics_inputs_ok(hmgpu_ctx* c, int32_t n, const hmgpu_pic* pics, const hmgpu_metrics_desc* d, const hmgpu_pic* ref_pics,
                                      const void* const* ref, const int64_t* ref_pitch, const int64_t* ref_bstride, const hmgpu_metrics_plan* plan,
                                      int* vec) {
  for (int i = 0; i < n; i++) if (!valid_pic(c, pics[i])) return HMGPU_EINVAL;
  *vec = 0;
  if (d->reference == HMGPU_METRICS_REF_PICTURES) {
    if (!ref_pics || ref || ref_pitch || ref_bstride) return HMGPU_EINVAL;
    for (int i = 0; i < n; i++) if (!valid_pic(c, ref_pics[i])) return HMGPU_EINVAL;
    hipSetDevice(c->device);
  } else {
    if (ref_pics || !ref || !ref_pitch || !ref_bstride) return HMGPU_EINVAL;
    for (int k = 0; k < 3; k++) if (plan->channels[k] && !ref[k]) return HMGPU_EINVAL;   // (one that is not compared: strided_dst_ok refuses it)
    const hmgpu_status st = strided_dst_ok(c, *plan, 3, n, const_cast<void* const*>(ref), ref_pitch, nullptr, ref_bstride, 0, vec);
    if (st != HMGPU_OK) return st;
  }
  return HMGPU_OK;
}

// everything hmgpu_pictures_metrics checks
static hmgpu_status metrics_resolve(hmgpu_ctx* c, int32_t n, const hmgpu_pic* pics, const hmgpu_metrics_desc* d, const hmgpu_pic* ref_pics,
                                    const void* const* ref, const int64_t* ref_pitch, const int64_t* ref_bstride, void* results, int64_t rstride,
                                    hmgpu_metrics_plan* plan, int* vec) {
  if (!c || !pics || !d || n < 1 || n > HMGPU_EXPORT_MAX_BATCH) return HMGPU_EINVAL;
  { const hmgpu_status st = metrics_plan(&c->seq, d, plan); if (st != HMGPU_OK) return st; }
  { const hmgpu_status st = metrics_inputs_ok(c, n, pics, d, ref_pics, ref, ref_pitch, ref_bstride, plan, vec); if (st != HMGPU_OK) return st; }
  const int64_t rec = plan->result_bytes;
  if (!results || (uintptr_t)results % 8 || rstride < rec || rstride % 8 || rstride > ((int64_t)1 << 40)) return HMGPU_EINVAL;
  if (!device_span_ok(results, (size_t)((n - 1) * rstride + rec), c->device)) return HMGPU_EINVAL;
  return HMGPU_OK;
}

hmgpu_status hmgpu_metrics_check(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_metrics_desc* d, const hmgpu_pic ref_pics[],
                                 const void* const ref[3], const int64_t ref_pitch_bytes[3], const int64_t ref_batch_stride_bytes[3],
                                 void* results, int64_t results_batch_stride_bytes) {
  hmgpu_metrics_plan plan;
  int vec = 0;
  return metrics_resolve(c, n, pics, d, ref_pics, ref, ref_pitch_bytes, ref_batch_stride_bytes, results, results_batch_stride_bytes, &plan, &vec);
}

hmgpu_status hmgpu_pictures_metrics(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_metrics_desc* d, const hmgpu_pic ref_pics[],
                                    const void* const ref[3], const int64_t ref_pitch_bytes[3], const int64_t ref_batch_stride_bytes[3],
                                    void* results, int64_t results_batch_stride_bytes, int32_t on_stream, void* stream) {
  if (on_stream != 0 && on_stream != 1) return HMGPU_EINVAL;
  hmgpu_metrics_plan plan;
  int vec = 0;
  { const hmgpu_status st = metrics_resolve(c, n, pics, d, ref_pics, ref, ref_pitch_bytes, ref_batch_stride_bytes, results, results_batch_stride_bytes, &plan, &vec);
    if (st != HMGPU_OK) return st; }
  hipStream_t hs = c->stream;
  { const hmgpu_status st = export_open(c, on_stream, stream, &hs); if (st != HMGPU_OK) return st; }
  const bool planes = d->reference == HMGPU_METRICS_REF_PLANES;
  MetricsArgs a;
  memset(&a, 0, sizeof(a));
  a.results = static_cast<uint8_t*>(results); a.rstride = results_batch_stride_bytes;
  metrics_sources(c, n, pics, d, ref_pics, ref, ref_pitch_bytes, ref_batch_stride_bytes, plan, vec, &a);
  for (int k = 0; k < 2; k++) {
    if (!a.w[k]) continue;
    const int tw = d->ssim ? kMetricsTileW : kMetricsRowTileW, th = d->ssim ? kMetricsTileH : kMetricsRowTileH;
    a.tiles_x[k] = (a.w[k] + tw - 1) / tw;
    a.tiles[k] = a.tiles_x[k] * ((a.h[k] + th - 1) / th);
  }
  a.total = n * (a.tiles[0] + a.tiles[1]);
  const int grid = d->ssim ? kMetricsGridSsim : kMetricsGrid;
  a.per = (a.total + grid - 1) / grid;
  const int64_t rec = plan.result_bytes;
  if (n == 1 || a.rstride == rec) HIP_TRY(c, hipMemsetAsync(results, 0, (size_t)(n * rec), hs));
  else HIP_TRY(c, hipMemset2DAsync(results, (size_t)a.rstride, 0, (size_t)rec, (size_t)n, hs));
  launch_metrics(a, planes ? d->ref_bytes_per_sample : 0, d->ssim != 0, hs);
  if (!planes) for (int i = 0; i < n; i++) touch(c, ref_pics[i]);      // (the reference pictures are read too)
  return export_end(c, n, pics, on_stream, hs);
}

// ------------------------------------------------------------------------------------------------ picture metric maps (k_metrics_map.hip)
// what strided_dst_ok needs to know of the maps: per component `fields` planes of blocks_y rows of blocks_x int64 elements
struct MapDstPlan { int32_t channels[3], height[3], elem_bytes[3], row_bytes[3]; };

// hmgpu_metrics_map_plan_for: the refusals of the metrics description first (mp: its plan), then those of the map's own
static hmgpu_status metrics_map_plan(const hmgpu_seq_params* seq, const hmgpu_metrics_desc* d, const hmgpu_metrics_map_desc* md,
                                     hmgpu_metrics_plan* mp, hmgpu_metrics_map_plan* out) {
  if (!out) return HMGPU_EINVAL;
  memset(out, 0, sizeof(*out));
  { const hmgpu_status st = metrics_plan(seq, d, mp); if (st != HMGPU_OK) return st; }
  if (!md || md->log2_block < 3 || md->log2_block > 6) return HMGPU_EINVAL;
  for (int k = 0; k < 7; k++) if (md->reserved[k]) return HMGPU_EINVAL;
  int W, H, csx, csy;
  { const hmgpu_status st = crop_ok(seq, d->crop, nullptr, &W, &H); if (st != HMGPU_OK) return st; }
  chroma_shifts(seq->chroma_format, &csx, &csy);
  const int B = 1 << md->log2_block;
  out->blocks_x = (W + B - 1) / B; out->blocks_y = (H + B - 1) / B;
  for (int k = 0; k < 3; k++) {
    if (!mp->channels[k]) continue;
    out->channels[k] = 1; out->width[k] = mp->width[k]; out->height[k] = mp->height[k];
    out->block_w[k] = k ? B >> csx : B; out->block_h[k] = k ? B >> csy : B;
  }
  out->fields = d->ssim ? HMGPU_METRICS_MAP_FIELDS : 4;
  out->row_bytes = out->blocks_x * 8;
  return HMGPU_OK;
}

hmgpu_status hmgpu_metrics_map_plan_for(const hmgpu_seq_params* seq, const hmgpu_metrics_desc* d, const hmgpu_metrics_map_desc* md,
                                        hmgpu_metrics_map_plan* out) {
  hmgpu_metrics_plan mp;
  const hmgpu_status st = metrics_map_plan(seq, d, md, &mp, out);
  if (st != HMGPU_OK && out) memset(out, 0, sizeof(*out));
  return st;
}

// everything hmgpu_pictures_metrics_map checks
static hmgpu_status metrics_map_resolve(hmgpu_ctx* c, int32_t n, const hmgpu_pic* pics, const hmgpu_metrics_desc* d, const hmgpu_metrics_map_desc* md,
                                        const hmgpu_pic* ref_pics, const void* const* ref, const int64_t* ref_pitch, const int64_t* ref_bstride,
                                        void* const* maps, const int64_t* pitch, const int64_t* fstride, const int64_t* bstride,
                                        hmgpu_metrics_plan* mp, hmgpu_metrics_map_plan* plan, int* vec) {
  if (!c || !pics || !d || n < 1 || n > HMGPU_EXPORT_MAX_BATCH) return HMGPU_EINVAL;
  { const hmgpu_status st = metrics_map_plan(&c->seq, d, md, mp, plan); if (st != HMGPU_OK) return st; }
  { const hmgpu_status st = metrics_inputs_ok(c, n, pics, d, ref_pics, ref, ref_pitch, ref_bstride, mp, vec); if (st != HMGPU_OK) return st; }
  if (!maps || !pitch || !fstride || !bstride) return HMGPU_EINVAL;
  MapDstPlan dp;
  memset(&dp, 0, sizeof(dp));
  for (int k = 0; k < 3; k++) {
    if (!plan->channels[k]) continue;                                  // (a map of a component that is not compared: strided_dst_ok refuses it)
    if (!maps[k]) return HMGPU_EINVAL;
    dp.channels[k] = plan->fields; dp.height[k] = plan->blocks_y; dp.elem_bytes[k] = 8; dp.row_bytes[k] = plan->row_bytes;
  }
  int mvec = 0;
  return strided_dst_ok(c, dp, 3, n, maps, pitch, fstride, bstride, 8, &mvec);
}

hmgpu_status hmgpu_metrics_map_check(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_metrics_desc* d, const hmgpu_metrics_map_desc* md,
                                     const hmgpu_pic ref_pics[], const void* const ref[3], const int64_t ref_pitch_bytes[3],
                                     const int64_t ref_batch_stride_bytes[3], void* const maps[3], const int64_t map_pitch_bytes[3],
                                     const int64_t map_field_stride_bytes[3], const int64_t map_batch_stride_bytes[3]) {
  hmgpu_metrics_plan mp;
  hmgpu_metrics_map_plan plan;
  int vec = 0;
  return metrics_map_resolve(c, n, pics, d, md, ref_pics, ref, ref_pitch_bytes, ref_batch_stride_bytes, maps, map_pitch_bytes, map_field_stride_bytes,
                             map_batch_stride_bytes, &mp, &plan, &vec);
}

hmgpu_status hmgpu_pictures_metrics_map(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_metrics_desc* d, const hmgpu_metrics_map_desc* md,
                                        const hmgpu_pic ref_pics[], const void* const ref[3], const int64_t ref_pitch_bytes[3],
                                        const int64_t ref_batch_stride_bytes[3], void* const maps[3], const int64_t map_pitch_bytes[3],
                                        const int64_t map_field_stride_bytes[3], const int64_t map_batch_stride_bytes[3], int32_t on_stream,
                                        void* stream) {
  if (on_stream != 0 && on_stream != 1) return HMGPU_EINVAL;
  hmgpu_metrics_plan mp;
  hmgpu_metrics_map_plan plan;
  int vec = 0;
  { const hmgpu_status st = metrics_map_resolve(c, n, pics, d, md, ref_pics, ref, ref_pitch_bytes, ref_batch_stride_bytes, maps, map_pitch_bytes,
                                                map_field_stride_bytes, map_batch_stride_bytes, &mp, &plan, &vec);
    if (st != HMGPU_OK) return st; }
  hipStream_t hs = c->stream;
  { const hmgpu_status st = export_open(c, on_stream, stream, &hs); if (st != HMGPU_OK) return st; }
  MetricsMapArgs a;
  memset(&a, 0, sizeof(a));
  metrics_sources(c, n, pics, d, ref_pics, ref, ref_pitch_bytes, ref_batch_stride_bytes, mp, vec, &a);
  for (int k = 0; k < 3; k++) {
    if (!plan.channels[k]) continue;
    a.maps[k] = static_cast<uint8_t*>(maps[k]);
    a.mpitch[k] = map_pitch_bytes[k]; a.mfstride[k] = map_field_stride_bytes[k]; a.mbstride[k] = map_batch_stride_bytes[k];
  }
  for (int k = 0; k < 2; k++) {
    a.log2_rw[k] = 6 - (k ? c->csx : 0); a.log2_rh[k] = 6 - (k ? c->csy : 0);
    a.log2_bw[k] = md->log2_block - (k ? c->csx : 0); a.log2_bh[k] = md->log2_block - (k ? c->csy : 0);
    if (!a.w[k]) continue;
    const int rw = 1 << a.log2_rw[k], rh = 1 << a.log2_rh[k];
    a.regions_x[k] = (a.w[k] + rw - 1) / rw;
    a.regions[k] = a.regions_x[k] * ((a.h[k] + rh - 1) / rh);
  }
  a.log2_nb = 6 - md->log2_block;
  a.blocks_x = plan.blocks_x; a.blocks_y = plan.blocks_y;
  const bool planes = d->reference == HMGPU_METRICS_REF_PLANES;
  launch_metrics_map(a, planes ? d->ref_bytes_per_sample : 0, d->ssim != 0, hs);
  if (!planes) for (int i = 0; i < n; i++) touch(c, ref_pics[i]);      // (the reference pictures are read too)
  return export_end(c, n, pics, on_stream, hs);
}

// ------------------------------------------------------------------------------------------------ picture histograms (k_histogram.hip)
static hmgpu_status histogram_plan(const hmgpu_seq_params* seq, const hmgpu_histogram_desc* d, hmgpu_histogram_plan* out) {
  if (!seq || !d || !out) return HMGPU_EINVAL;
  memset(out, 0, sizeof(*out));
  const int fmt = seq->chroma_format, bd[2] = {seq->bit_depth_luma, seq->bit_depth_chroma};
  if (fmt < 0 || fmt > 3 || bd[0] < 8 || bd[0] > 12 || bd[1] < 8 || bd[1] > 12 || seq->width <= 0 || seq->height <= 0) return HMGPU_EINVAL;
  for (int k = 0; k < 6; k++) if (d->reserved[k]) return HMGPU_EINVAL;
  if (d->channels < 1 || d->channels > 15 || (d->histogram != 0 && d->histogram != 1)) return HMGPU_EINVAL;
  if (d->log2_bins != 0 && (d->log2_bins < 4 || d->log2_bins > 12)) return HMGPU_EINVAL;
  const int chans = fmt == 0 ? d->channels & 9 : d->channels;
  if (!chans) return HMGPU_EINVAL;                                    // (4:0:0: the chroma bits alone select nothing)
  int W, H, csx, csy;
  { const hmgpu_status st = crop_ok(seq, d->crop, nullptr, &W, &H); if (st != HMGPU_OK) return st; }
  if ((int64_t)W * H >= ((int64_t)1 << 31)) return HMGPU_EUNSUPPORTED;  // every count, and an int32 view of it, stays below 2^31
  chroma_shifts(fmt, &csx, &csy);
  int depth[4] = {bd[0], bd[1], bd[1], bd[0]};
  if (chans & 8) {
    if (d->rgb_bit_depth) {
      if (d->rgb_bit_depth < 8) return HMGPU_EINVAL;
      if (d->rgb_bit_depth > 12) return HMGPU_EUNSUPPORTED;            // the bins of a channel fit the LDS up to 2^12
      depth[3] = d->rgb_bit_depth;
    }
    // the RGB export whose samples these are: its rules for matrix and full_range, and its constants
    hmgpu_export_desc e;
    memset(&e, 0, sizeof(e));
    e.layout = HMGPU_EXPORT_RGB; e.bit_depth[0] = depth[3]; e.bytes_per_sample = 2;
    memcpy(e.crop, d->crop, sizeof(e.crop));
    e.matrix = d->matrix; e.full_range = d->full_range;
    hmgpu_export_plan ep;
    const hmgpu_status st = hmgpu_export_plan_for(seq, &e, &ep);
    if (st != HMGPU_OK) return st;
    memcpy(out->coef, ep.coef, sizeof(out->coef));
  }
  for (int k = 0; k < 4; k++) {
    if (!((chans >> k) & 1)) continue;
    const bool chroma = k == 1 || k == 2;
    out->channels[k] = 1;
    out->width[k] = chroma ? W >> csx : W; out->height[k] = chroma ? H >> csy : H;
    out->depth[k] = depth[k];
    out->log2_bins[k] = d->log2_bins ? std::min(d->log2_bins, depth[k]) : depth[k];
    out->hist_bytes[k] = d->histogram ? 4 << out->log2_bins[k] : 0;
  }
  out->record_bytes = 4 * (int)sizeof(hmgpu_histogram_result);
  return HMGPU_OK;
}

hmgpu_status hmgpu_histogram_plan_for(const hmgpu_seq_params* seq, const hmgpu_histogram_desc* d, hmgpu_histogram_plan* out) {
  const hmgpu_status st = histogram_plan(seq, d, out);
  if (st != HMGPU_OK && out) memset(out, 0, sizeof(*out));
  return st;
}

// everything hmgpu_pictures_histogram checks
static hmgpu_status histogram_resolve(hmgpu_ctx* c, int32_t n, const hmgpu_pic* pics, const hmgpu_histogram_desc* d, void* const* hist,
                                      const int64_t* hstride, void* records, int64_t rstride, hmgpu_histogram_plan* plan) {
  if (!c || !pics || !d || n < 1 || n > HMGPU_EXPORT_MAX_BATCH) return HMGPU_EINVAL;
  { const hmgpu_status st = histogram_plan(&c->seq, d, plan); if (st != HMGPU_OK) return st; }
  for (int i = 0; i < n; i++) if (!valid_pic(c, pics[i])) return HMGPU_EINVAL;
  hipSetDevice(c->device);
  if (d->histogram && (!hist || !hstride)) return HMGPU_EINVAL;
  for (int k = 0; k < 4; k++) {
    void* const p = hist ? hist[k] : nullptr;
    if (!d->histogram || !plan->channels[k]) {
      if (p) return HMGPU_EINVAL;                                      // a histogram this call does not compute
      continue;
    }
    const int64_t bytes = plan->hist_bytes[k], s = hstride[k];
    if (!p || (uintptr_t)p % 4 || s < bytes || s % 4 || s > ((int64_t)1 << 40)) return HMGPU_EINVAL;
    if (!device_span_ok(p, (size_t)((n - 1) * s + bytes), c->device)) return HMGPU_EINVAL;
  }
  const int64_t rec = plan->record_bytes;
  if (!records || (uintptr_t)records % 8 || rstride < rec || rstride % 8 || rstride > ((int64_t)1 << 40)) return HMGPU_EINVAL;
  if (!device_span_ok(records, (size_t)((n - 1) * rstride + rec), c->device)) return HMGPU_EINVAL;
  return HMGPU_OK;
}

hmgpu_status hmgpu_histogram_check(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_histogram_desc* d, void* const hist[4],
                                   const int64_t hist_batch_stride_bytes[4], void* records, int64_t records_batch_stride_bytes) {
  hmgpu_histogram_plan plan;
  return histogram_resolve(c, n, pics, d, hist, hist_batch_stride_bytes, records, records_batch_stride_bytes, &plan);
}

hmgpu_status hmgpu_pictures_histogram(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_histogram_desc* d, void* const hist[4],
                                      const int64_t hist_batch_stride_bytes[4], void* records, int64_t records_batch_stride_bytes,
                                      int32_t on_stream, void* stream) {
  if (on_stream != 0 && on_stream != 1) return HMGPU_EINVAL;
  hmgpu_histogram_plan plan;
  { const hmgpu_status st = histogram_resolve(c, n, pics, d, hist, hist_batch_stride_bytes, records, records_batch_stride_bytes, &plan);
    if (st != HMGPU_OK) return st; }
  hipStream_t hs = c->stream;
  { const hmgpu_status st = export_open(c, on_stream, stream, &hs); if (st != HMGPU_OK) return st; }
  HistogramArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n; a.do_hist = d->histogram;
  a.records = static_cast<uint8_t*>(records); a.rstride = records_batch_stride_bytes;
  for (int k = 0; k < 4; k++) {
    if (!plan.channels[k]) continue;
    a.chans |= 1 << k;
    a.shift[k] = plan.depth[k] - plan.log2_bins[k]; a.log2_bins[k] = plan.log2_bins[k];
    if (d->histogram) { a.hist[k] = static_cast<uint8_t*>(hist[k]); a.hstride[k] = hist_batch_stride_bytes[k]; }
  }
  for (int k = 0; k < 2; k++) {
    const int ch = k ? (plan.channels[1] ? 1 : 2) : (plan.channels[0] ? 0 : 3);   // a channel of the class that is computed, if any
    a.pitch[k] = c->pitch[k];
    if (!plan.channels[ch]) continue;
    a.w[k] = plan.width[ch]; a.h[k] = plan.height[ch];
    a.tiles_x[k] = (a.w[k] + kHistTileW - 1) / kHistTileW;
    a.tiles[k] = a.tiles_x[k] * ((a.h[k] + kHistTileH - 1) / kHistTileH);
  }
  a.csx = c->csx; a.csy = c->csy; a.mono = c->seq.chroma_format == 0;
  memcpy(a.coef, plan.coef, sizeof(a.coef));
  for (int k = 0; k < 2; k++) {                                        // maxRGB: the depth rule of the export's identity, both types at D_3
    a.sh[k] = plan.depth[3] - (k ? c->seq.bit_depth_chroma : c->seq.bit_depth_luma);
    a.maxv[k] = (1 << plan.depth[3]) - 1;
  }
  const int x0 = d->crop[0], y0 = d->crop[2];
  const size_t rg = c->csx ? 8 : 16;                                   // the chroma of 4 luma samples: 2 pairs or 4
  for (int i = 0; i < n; i++) {
    const Picture& p = c->pics[pics[i]];
    int16_t* const* src = p.sao_applied ? p.dev.sao : p.dev.rec;
    a.y[i] = src[0] + (ptrdiff_t)y0 * c->pitch[0] + x0;
    a.c[i] = a.mono ? nullptr : src[1] + (ptrdiff_t)(y0 >> c->csy) * c->pitch[1] + kCStep * (x0 >> c->csx);
    if ((uintptr_t)a.y[i] % 8 == 0 && ((size_t)c->pitch[0] * 2) % 8 == 0) a.yvec |= 1u << i;
    if (a.mono) continue;
    if ((uintptr_t)a.c[i] % 16 == 0 && ((size_t)c->pitch[1] * 2) % 16 == 0) a.cvec |= 1u << i;
    if ((uintptr_t)a.c[i] % rg == 0 && ((size_t)c->pitch[1] * 2) % rg == 0) a.rvec |= 1u << i;
  }
  a.total = n * (a.tiles[0] + a.tiles[1]);
  a.per = (a.total + kHistGrid - 1) / kHistGrid;
  const int64_t rec = plan.record_bytes;
  if (n == 1 || a.rstride == rec) HIP_TRY(c, hipMemsetAsync(records, 0, (size_t)(n * rec), hs));
  else HIP_TRY(c, hipMemset2DAsync(records, (size_t)a.rstride, 0, (size_t)rec, (size_t)n, hs));
  for (int k = 0; k < 4; k++) {
    if (!a.hist[k]) continue;
    const int64_t bytes = plan.hist_bytes[k];
    if (n == 1 || a.hstride[k] == bytes) HIP_TRY(c, hipMemsetAsync(a.hist[k], 0, (size_t)(n * bytes), hs));
    else HIP_TRY(c, hipMemset2DAsync(a.hist[k], (size_t)a.hstride[k], 0, (size_t)bytes, (size_t)n, hs));
  }
  launch_histogram(a, hs);
  return export_end(c, n, pics, on_stream, hs);
}

}  // extern "C"
