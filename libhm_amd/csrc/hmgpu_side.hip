// hmgpu_side.hip -- side-information export of the host runtime: the motion / block, residual, transform and loop-filter exports.  Per
// family one plan, one *_resolve under the destination check and the launching entry, and the kernel's arguments (k_motion / k_residual /
// k_transform / k_lfinfo.hip).
#include "hmgpu_host.h"

#include <cmath>
#include <cstring>

// ------------------------------------------------------------------------------------------------ what the families share
// the preamble of every plan: *out zeroed (a plan writes it only behind its last refusal: a refused plan is all zero); the sequence's
// geometry (sizes whole in size_mask + 1 samples), n, reserved[]
template <class Desc, class Plan>
static bool side_plan_open(const hmgpu_seq_params* seq, const Desc* d, int size_mask, int n, Plan* out) {
  if (out) memset(out, 0, sizeof(*out));
  if (!seq || !d || !out) return false;
  const int fmt = seq->chroma_format;
  if (fmt < 0 || fmt > 3 || seq->width <= 0 || seq->height <= 0 || (seq->width & size_mask) || (seq->height & size_mask)) return false;
  if (n < 1 || n > HMGPU_EXPORT_MAX_BATCH) return false;
  for (int32_t r : d->reserved) if (r) return false;
  return true;
}

// the output element of a sample_type: kElem* (kElemU16 stands for the integer type, taken where `integer`), -1 for any other one
static int side_elem(int sample_type, bool integer) {
  if (sample_type == HMGPU_SAMPLE_UINT) return integer ? kElemU16 : -1;
  return sample_type == HMGPU_SAMPLE_F16 ? kElemF16 : sample_type == HMGPU_SAMPLE_BF16 ? kElemBF16 : sample_type == HMGPU_SAMPLE_F32 ? kElemF32 : -1;
}

// ... and of a float element, that the scale of every selected component is finite
static bool side_scale_ok(int elem, int components, const float* scale) {
  if (elem != kElemU16)
    for (int k = 0; k < 3; k++) if (((components >> k) & 1) && !std::isfinite(scale[k])) return false;
  return true;
}

// what the plan of a dense form asks beyond its element: no crop of the description's (the window is the crop), of a scale that has
// passed scale_desc_ok the nearest filter (side information is not interpolated), and the windows, in order (the first failure is the
// call's status); w x h: the output -- sc's size, or (unscaled) the one size every window has
static hmgpu_status dense_form_ok(const hmgpu_seq_params* seq, const int32_t crop[4], const hmgpu_export_scale* sc, int n, const hmgpu_export_window* win,
                                  int* w, int* h) {
  if (!win || crop[0] || crop[1] || crop[2] || crop[3]) return HMGPU_EINVAL;
  if (sc && sc->filter != HMGPU_SCALE_NEAREST) return HMGPU_EUNSUPPORTED;
  for (int i = 0; i < n; i++) {
    int ww, wh;
    { const hmgpu_status st = window_ok(seq, win[i], sc, &ww, &wh); if (st != HMGPU_OK) return st; }
    if (sc) continue;
    if (!i) { *w = ww; *h = wh; }
    if (ww != *w || wh != *h) return HMGPU_EINVAL;
    if (ww > 16384 || wh > 16384) return HMGPU_EUNSUPPORTED;
  }
  if (sc) { *w = sc->width; *h = sc->height; }
  return HMGPU_OK;
}

// ... and picture i's as a dense kernel takes it, with its bit of the mirror mask
static void dense_window(const hmgpu_seq_params& seq, const hmgpu_export_window* windows, int i, SideWin* w, uint32_t* flip) {
  const int* cr = windows[i].crop;
  w->left = cr[0]; w->top = cr[2]; w->w = seq.width - cr[0] - cr[1]; w->h = seq.height - cr[2] - cr[3];
  *flip |= (uint32_t)(windows[i].flip & 1) << i;
}

// the pictures of a call: valid handles with side information
static hmgpu_status side_pictures_ok(hmgpu_ctx* c, int32_t n, const hmgpu_pic* pics) {
  if (!c || !pics || n < 1 || n > HMGPU_EXPORT_MAX_BATCH) return HMGPU_EINVAL;
  for (int i = 0; i < n; i++) {
    if (!valid_pic(c, pics[i])) return HMGPU_EINVAL;
    if (c->pics[pics[i]].covered_ctus != c->num_ctus) return HMGPU_EINVAL;       // no side information (uploaded, received, partly decoded)
  }
  return HMGPU_OK;
}

// intra CUs carry a residual, and the intra modes are the picture's, only when EVERY call that covers the picture came with intra_dir[]:
// a picture whose slice calls disagree exports its intra CUs as 0 (k_prep listed no TU for those of the calls without the modes: their
// tiles are stale)
static bool all_calls_had_intra_dir(const Picture& pic) {
  bool dir = !pic.calls.empty();
  for (const SliceCall& sc : pic.calls) dir = dir && sc.dir;
  return dir;
}

// the first `slots` destinations of a call in its kernel's arguments: a null one is not written (pstride null: one plane per slot)
template <class Args>
static void side_destinations(Args* a, int slots, void* const* dst, const int64_t* pitch, const int64_t* pstride, const int64_t* bstride) {
  for (int k = 0; k < slots; k++) {
    if (!dst[k]) continue;
    a->dst[k] = static_cast<uint8_t*>(dst[k]);
    a->pitch[k] = pitch[k]; a->pstride[k] = pstride ? pstride[k] : 0; a->bstride[k] = bstride[k];
  }
}

extern "C" {

// (the same record for all three: every CTU covered by decompress calls)
hmgpu_status hmgpu_pictures_motion_check(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[]) { return side_pictures_ok(c, n, pics); }
hmgpu_status hmgpu_pictures_residual_check(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[]) { return side_pictures_ok(c, n, pics); }
hmgpu_status hmgpu_pictures_transform_check(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[]) { return side_pictures_ok(c, n, pics); }

// ------------------------------------------------------------------------------------------------ motion and block export (k_motion.hip)
hmgpu_status hmgpu_motion_plan_for(const hmgpu_seq_params* seq, const hmgpu_motion_desc* d, const hmgpu_export_scale* sc, int32_t n,
                                   const hmgpu_export_window win[], hmgpu_motion_plan* out) {
  if (!side_plan_open(seq, d, 3, n, out)) return HMGPU_EINVAL;
  if (d->form != HMGPU_MOTION_BLOCKS && d->form != HMGPU_MOTION_DENSE) return HMGPU_EINVAL;
  if (d->lists < 1 || d->lists > 3) return HMGPU_EINVAL;
  const int L = (d->lists & 1) + (d->lists >> 1);
  int w = 0, h = 0;
  if (d->form == HMGPU_MOTION_BLOCKS) {
    if (sc || win || d->sample_type != HMGPU_SAMPLE_UINT) return HMGPU_EINVAL;
    if ((d->crop[0] | d->crop[1] | d->crop[2] | d->crop[3]) & 3) return HMGPU_EINVAL;         // whole blocks (a negative crop: crop_ok)
    if (crop_ok(seq, d->crop, nullptr, &w, &h) != HMGPU_OK) return HMGPU_EINVAL;
    w /= 4; h /= 4;
    out->channels[HMGPU_MOTION_DST_MV0] = 2 * L;
    out->elem_bytes[HMGPU_MOTION_DST_MV0] = 2;
  } else {
    const int elem = side_elem(d->sample_type, false);
    if (elem < 0) return HMGPU_EINVAL;
    if (sc) { const hmgpu_status st = scale_desc_ok(sc); if (st != HMGPU_OK) return st; }
    { const hmgpu_status st = dense_form_ok(seq, d->crop, sc, n, win, &w, &h); if (st != HMGPU_OK) return st; }
    const int es = elem == kElemF32 ? 4 : 2;
    for (int l = 0; l < 2; l++) if ((d->lists >> l) & 1) { out->channels[l] = 2; out->elem_bytes[l] = es; }
  }
  out->lists = L;
  out->channels[HMGPU_MOTION_DST_REF] = L; out->elem_bytes[HMGPU_MOTION_DST_REF] = 4;
  out->channels[HMGPU_MOTION_DST_BLOCK] = 4; out->elem_bytes[HMGPU_MOTION_DST_BLOCK] = 1;
  for (int k = 0; k < HMGPU_MOTION_DSTS; k++) {
    if (!out->channels[k]) { out->elem_bytes[k] = 0; continue; }
    out->width[k] = w; out->height[k] = h; out->row_bytes[k] = w * out->elem_bytes[k];
  }
  return HMGPU_OK;
}

// everything hmgpu_pictures_export_motion checks, the pictures first (pics null: hmgpu_motion_destination_check, which has none), and
// what the destinations give the kernel: *a zero but for its four slots, in HMGPU_MOTION_DST_* order, and vec
static hmgpu_status motion_resolve(hmgpu_ctx* c, int32_t n, const hmgpu_pic* pics, const hmgpu_motion_desc* d, const hmgpu_export_scale* sc,
                                   const hmgpu_export_window* windows, void* const dst_mv[2], void* dst_ref, void* dst_block, const int64_t* pitch,
                                   const int64_t* pstride, const int64_t* bstride, hmgpu_motion_plan* plan, MotionArgs* a) {
  if (!c || !d || !dst_mv || !pitch || !pstride || !bstride) return HMGPU_EINVAL;
  if (pics) { const hmgpu_status st = side_pictures_ok(c, n, pics); if (st != HMGPU_OK) return st; }
  { const hmgpu_status st = hmgpu_motion_plan_for(&c->seq, d, sc, n, windows, plan); if (st != HMGPU_OK) return st; }
  void* const dst[4] = {dst_mv[0], dst_mv[1], dst_ref, dst_block};
  memset(a, 0, sizeof(*a));
  { const hmgpu_status st = strided_dst_ok(c, *plan, HMGPU_MOTION_DSTS, n, dst, pitch, pstride, bstride, 0, &a->vec); if (st != HMGPU_OK) return st; }
  side_destinations(a, HMGPU_MOTION_DSTS, dst, pitch, pstride, bstride);
  return HMGPU_OK;
}

hmgpu_status hmgpu_motion_destination_check(hmgpu_ctx* c, int32_t n, const hmgpu_motion_desc* d, const hmgpu_export_scale* sc,
                                            const hmgpu_export_window windows[], void* const dst_mv[2], void* dst_ref, void* dst_block,
                                            const int64_t pitch_bytes[4], const int64_t plane_stride_bytes[4],
                                            const int64_t batch_stride_bytes[4]) {
  hmgpu_motion_plan plan;
  MotionArgs a;
  return motion_resolve(c, n, nullptr, d, sc, windows, dst_mv, dst_ref, dst_block, pitch_bytes, plane_stride_bytes, batch_stride_bytes, &plan, &a);
}

hmgpu_status hmgpu_pictures_export_motion(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_motion_desc* d,
                                          const hmgpu_export_scale* sc, const hmgpu_export_window windows[], void* const dst_mv[2],
                                          void* dst_ref, void* dst_block, const int64_t pitch_bytes[4],
                                          const int64_t plane_stride_bytes[4], const int64_t batch_stride_bytes[4], int32_t on_stream,
                                          void* stream) {
  if (!pics || (on_stream != 0 && on_stream != 1)) return HMGPU_EINVAL;
  hmgpu_motion_plan plan;
  MotionArgs a;
  { const hmgpu_status st = motion_resolve(c, n, pics, d, sc, windows, dst_mv, dst_ref, dst_block, pitch_bytes, plane_stride_bytes, batch_stride_bytes, &plan, &a);
    if (st != HMGPU_OK) return st; }
  hipStream_t hs = c->stream;
  { const hmgpu_status st = export_open(c, on_stream, stream, &hs); if (st != HMGPU_OK) return st; }
  a.n = n; a.lists = d->lists; a.nlists = plan.lists;
  a.log2ctu = c->seq.log2_ctu_size; a.ctus_w = c->ctus_w; a.parts = c->parts;
  for (int i = 0; i < n; i++) {
    const PicDev& p = c->pics[pics[i]].dev;
    MotionSrc& s = a.src[i];
    s.depth = p.depth; s.part_size = p.part_size; s.pred_mode = p.pred_mode; s.qp = p.qp;
    for (int l = 0; l < 2; l++) { s.mv[l] = p.mv[l]; s.ref_idx[l] = p.ref_idx[l]; }
    s.slice_idx = p.slice_idx; s.slices = p.slices;
  }
  if (d->form == HMGPU_MOTION_BLOCKS) {
    a.x4 = d->crop[0] / 4; a.y4 = d->crop[2] / 4; a.w4 = plan.width[HMGPU_MOTION_DST_REF]; a.h4 = plan.height[HMGPU_MOTION_DST_REF];
    if (a.x4 & 3) a.vec = 0;                         // a lane's four blocks are aligned in the picture, not in the crop
    launch_motion_blocks(a, hs);
  } else {
    a.W = plan.width[HMGPU_MOTION_DST_REF]; a.H = plan.height[HMGPU_MOTION_DST_REF];
    for (int i = 0; i < n; i++) {
      MotionWin& w = a.win[i];
      dense_window(c->seq, windows, i, &w, &a.flip);
      w.kx = (float)((double)a.W / (4.0 * w.w)); w.ky = (float)((double)a.H / (4.0 * w.h));     // quarter luma samples -> output samples
    }
    launch_motion_dense(a, side_elem(d->sample_type, false), hs);
  }
  return export_end(c, n, pics, on_stream, hs);
}

// ------------------------------------------------------------------------------------------------ residual export (k_residual.hip)
hmgpu_status hmgpu_residual_plan_for(const hmgpu_seq_params* seq, const hmgpu_residual_desc* d, const hmgpu_export_scale* sc, int32_t n,
                                     const hmgpu_export_window win[], hmgpu_residual_plan* out) {
  if (!side_plan_open(seq, d, 7, n, out)) return HMGPU_EINVAL;
  if (d->form != HMGPU_RESIDUAL_PLANES && d->form != HMGPU_RESIDUAL_DENSE) return HMGPU_EINVAL;
  if (d->components < 1 || d->components > 7) return HMGPU_EINVAL;
  if (sc) { const hmgpu_status st = scale_desc_ok(sc); if (st != HMGPU_OK) return st; }   // (before the format's refusal)
  const int fmt = seq->chroma_format;
  if (fmt >= 2) return HMGPU_EUNSUPPORTED;          // k_ccp rewrites their chroma tiles in place; 4:2:2 blocks are two squares
  const bool mono = fmt == 0;
  if (d->form == HMGPU_RESIDUAL_PLANES) {
    if (sc || win || d->sample_type != HMGPU_SAMPLE_UINT) return HMGPU_EINVAL;
    if ((d->crop[0] | d->crop[1] | d->crop[2] | d->crop[3]) & 7) return HMGPU_EINVAL;         // whole 8x8 tiles (a negative crop: crop_ok)
    int w, h;
    if (crop_ok(seq, d->crop, nullptr, &w, &h) != HMGPU_OK) return HMGPU_EINVAL;
    for (int k = 0; k < 3; k++) {
      if (!((d->components >> k) & 1) || (k && mono)) continue;
      out->channels[k] = 1; out->elem_bytes[k] = 2;
      out->width[k] = k ? w / 2 : w; out->height[k] = k ? h / 2 : h; out->row_bytes[k] = out->width[k] * 2;
    }
    return HMGPU_OK;
  }
  const int elem = side_elem(d->sample_type, true);
  if (elem < 0 || !side_scale_ok(elem, d->components, d->scale)) return HMGPU_EINVAL;
  int w = 0, h = 0;
  { const hmgpu_status st = dense_form_ok(seq, d->crop, sc, n, win, &w, &h); if (st != HMGPU_OK) return st; }
  out->channels[0] = (d->components & 1) + ((d->components >> 1) & 1) + ((d->components >> 2) & 1);
  out->elem_bytes[0] = elem == kElemF32 ? 4 : 2;
  out->width[0] = w; out->height[0] = h; out->row_bytes[0] = w * out->elem_bytes[0];
  return HMGPU_OK;
}

// everything hmgpu_pictures_export_residual checks: the plan (the format's refusal comes first: it does not depend on the pictures),
// the pictures (pics null: hmgpu_residual_destination_check, which has none), the destinations; and what these give the kernel: *a
// zero but for its slots and vec
static hmgpu_status residual_resolve(hmgpu_ctx* c, int32_t n, const hmgpu_pic* pics, const hmgpu_residual_desc* d, const hmgpu_export_scale* sc,
                                     const hmgpu_export_window* windows, void* const dst[3], const int64_t* pitch, const int64_t* pstride,
                                     const int64_t* bstride, hmgpu_residual_plan* plan, ResidArgs* a) {
  if (!c || !d || !dst || !pitch || !pstride || !bstride) return HMGPU_EINVAL;
  { const hmgpu_status st = hmgpu_residual_plan_for(&c->seq, d, sc, n, windows, plan); if (st != HMGPU_OK) return st; }
  if (pics) { const hmgpu_status st = side_pictures_ok(c, n, pics); if (st != HMGPU_OK) return st; }
  const bool planes = d->form == HMGPU_RESIDUAL_PLANES;
  const int slots = planes && c->seq.chroma_format == 0 ? 1 : 3;       // (the chroma destinations of a 4:0:0 picture's planes are ignored)
  if (planes) pstride = nullptr;                                       // (... and the plane strides of planes: one plane per slot)
  memset(a, 0, sizeof(*a));
  { const hmgpu_status st = strided_dst_ok(c, *plan, slots, n, dst, pitch, pstride, bstride, 16, &a->vec); if (st != HMGPU_OK) return st; }
  side_destinations(a, slots, dst, pitch, pstride, bstride);
  return HMGPU_OK;
}

hmgpu_status hmgpu_residual_destination_check(hmgpu_ctx* c, int32_t n, const hmgpu_residual_desc* d, const hmgpu_export_scale* sc,
                                              const hmgpu_export_window windows[], void* const dst[3], const int64_t pitch_bytes[3],
                                              const int64_t plane_stride_bytes[3], const int64_t batch_stride_bytes[3]) {
  hmgpu_residual_plan plan;
  ResidArgs a;
  return residual_resolve(c, n, nullptr, d, sc, windows, dst, pitch_bytes, plane_stride_bytes, batch_stride_bytes, &plan, &a);
}

hmgpu_status hmgpu_pictures_export_residual(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_residual_desc* d,
                                            const hmgpu_export_scale* sc, const hmgpu_export_window windows[], void* const dst[3],
                                            const int64_t pitch_bytes[3], const int64_t plane_stride_bytes[3],
                                            const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream) {
  if (!pics || (on_stream != 0 && on_stream != 1)) return HMGPU_EINVAL;
  hmgpu_residual_plan plan;
  ResidArgs a;
  { const hmgpu_status st = residual_resolve(c, n, pics, d, sc, windows, dst, pitch_bytes, plane_stride_bytes, batch_stride_bytes, &plan, &a);
    if (st != HMGPU_OK) return st; }
  hipStream_t hs = c->stream;
  { const hmgpu_status st = export_open(c, on_stream, stream, &hs); if (st != HMGPU_OK) return st; }
  const bool mono = c->seq.chroma_format == 0;
  a.n = n; a.mono = mono; a.comps = mono ? d->components & 1 : d->components;
  a.log2ctu = c->seq.log2_ctu_size; a.ctus_w = c->ctus_w; a.parts = c->parts;
  for (int k = 0; k < 3; k++) a.rtw[k] = (c->grid_w / 2) >> (k ? c->csx : 0);
  for (int i = 0; i < n; i++) {
    const Picture& pic = c->pics[pics[i]];
    const PicDev& p = pic.dev;
    ResidSrc& s = a.src[i];
    s.depth = p.depth; s.part_size = p.part_size; s.pred_mode = p.pred_mode; s.tr_idx = p.tr_idx; s.ipcm = p.ipcm;
    for (int k = 0; k < 3; k++) { s.cbf[k] = p.cbf[k]; s.resid[k] = p.resid[k]; }
    s.gate = (all_calls_had_intra_dir(pic) ? kResidIntra : 0) | (pic.flags_staged ? kResidFlags : 0);
  }
  if (d->form == HMGPU_RESIDUAL_PLANES) {
    a.x0 = d->crop[0]; a.y0 = d->crop[2]; a.w = c->seq.width - d->crop[0] - d->crop[1]; a.h = c->seq.height - d->crop[2] - d->crop[3];
    if (a.x0 & 15) a.vec &= 1;                       // a chroma lane's eight samples are aligned in the picture, not in the crop
    launch_residual_planes(a, hs);
  } else {
    a.W = plan.width[0]; a.H = plan.height[0];
    int ch = 0;
    for (int k = 0; k < 3; k++) { a.chan[k] = ch; if ((d->components >> k) & 1) ch++; a.scale[k] = d->scale[k]; }
    for (int i = 0; i < n; i++) dense_window(c->seq, windows, i, &a.win[i], &a.flip);
    launch_residual_dense(a, side_elem(d->sample_type, true), hs);
  }
  return export_end(c, n, pics, on_stream, hs);
}

// ------------------------------------------------------------------------------------------------ transform export (k_transform.hip)
hmgpu_status hmgpu_transform_plan_for(const hmgpu_seq_params* seq, const hmgpu_transform_desc* d, int32_t n, hmgpu_transform_plan* out) {
  if (!side_plan_open(seq, d, 7, n, out)) return HMGPU_EINVAL;
  if (d->value != HMGPU_TRANSFORM_LEVELS && d->value != HMGPU_TRANSFORM_COEFFS) return HMGPU_EINVAL;
  if (d->components < 1 || d->components > 7) return HMGPU_EINVAL;
  const int elem = side_elem(d->sample_type, true);
  if (elem < 0) return HMGPU_EUNSUPPORTED;
  if (!side_scale_ok(elem, d->components, d->scale)) return HMGPU_EINVAL;
  const int fmt = seq->chroma_format;
  const int csx = (fmt == 1 || fmt == 2) ? 1 : 0, csy = fmt == 1 ? 1 : 0, es = elem == kElemF32 ? 4 : 2;
  for (int k = 0; k < 3; k++) {
    if (!((d->components >> k) & 1) || (k && fmt == 0)) continue;
    out->channels[k] = 1; out->elem_bytes[k] = es;
    out->width[k] = k ? seq->width >> csx : seq->width; out->height[k] = k ? seq->height >> csy : seq->height;
    out->row_bytes[k] = out->width[k] * es;
  }
  const int I = HMGPU_TRANSFORM_DST_INFO;
  out->channels[I] = HMGPU_TRANSFORM_INFO_CHANNELS; out->elem_bytes[I] = 1;
  out->width[I] = seq->width / 4; out->height[I] = seq->height / 4; out->row_bytes[I] = out->width[I];
  return HMGPU_OK;
}

// everything hmgpu_pictures_export_transform checks: the plan, the pictures (pics null: hmgpu_transform_destination_check, which has
// none), the destinations: the planes as the residual export's (one plane per slot, 16-byte stores where aligned; the chroma
// destinations of a 4:0:0 picture are ignored), the info grid with its channel stride; at least one of the four.  And what these give
// the kernel: *a zero but for its slots and vec
struct TransformInfoPlan { int32_t channels[1], height[1], elem_bytes[1], row_bytes[1]; };
static hmgpu_status transform_resolve(hmgpu_ctx* c, int32_t n, const hmgpu_pic* pics, const hmgpu_transform_desc* d, void* const dst[3],
                                      void* dst_info, const int64_t* pitch, const int64_t* pstride, const int64_t* bstride,
                                      hmgpu_transform_plan* plan, TransformArgs* a) {
  if (!c || !d || !dst || !pitch || !pstride || !bstride) return HMGPU_EINVAL;
  { const hmgpu_status st = hmgpu_transform_plan_for(&c->seq, d, n, plan); if (st != HMGPU_OK) return st; }
  if (pics) { const hmgpu_status st = side_pictures_ok(c, n, pics); if (st != HMGPU_OK) return st; }
  const int slots = c->seq.chroma_format == 0 ? 1 : 3, I = HMGPU_TRANSFORM_DST_INFO;
  bool planes = false;
  for (int k = 0; k < slots; k++) planes = planes || dst[k];
  memset(a, 0, sizeof(*a));
  if (!planes && !dst_info) return HMGPU_EINVAL;
  if (planes) { const hmgpu_status st = strided_dst_ok(c, *plan, slots, n, dst, pitch, nullptr, bstride, 16, &a->vec); if (st != HMGPU_OK) return st; }
  if (dst_info) {
    const TransformInfoPlan ip = {{plan->channels[I]}, {plan->height[I]}, {plan->elem_bytes[I]}, {plan->row_bytes[I]}};
    void* const di[1] = {dst_info};
    int v = 0;
    const hmgpu_status st = strided_dst_ok(c, ip, 1, n, di, pitch + I, pstride + I, bstride + I, 0, &v);
    if (st != HMGPU_OK) return st;
    a->dst[I] = static_cast<uint8_t*>(dst_info);
    a->pitch[I] = pitch[I]; a->pstride[I] = pstride[I]; a->bstride[I] = bstride[I];
  }
  side_destinations(a, slots, dst, pitch, nullptr, bstride);
  return HMGPU_OK;
}

hmgpu_status hmgpu_transform_destination_check(hmgpu_ctx* c, int32_t n, const hmgpu_transform_desc* d, void* const dst[3], void* dst_info,
                                               const int64_t pitch_bytes[4], const int64_t plane_stride_bytes[4],
                                               const int64_t batch_stride_bytes[4]) {
  hmgpu_transform_plan plan;
  TransformArgs a;
  return transform_resolve(c, n, nullptr, d, dst, dst_info, pitch_bytes, plane_stride_bytes, batch_stride_bytes, &plan, &a);
}

hmgpu_status hmgpu_pictures_export_transform(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_transform_desc* d,
                                             void* const dst[3], void* dst_info, const int64_t pitch_bytes[4],
                                             const int64_t plane_stride_bytes[4], const int64_t batch_stride_bytes[4], int32_t on_stream,
                                             void* stream) {
  if (!pics || (on_stream != 0 && on_stream != 1)) return HMGPU_EINVAL;
  hmgpu_transform_plan plan;
  TransformArgs a;
  { const hmgpu_status st = transform_resolve(c, n, pics, d, dst, dst_info, pitch_bytes, plane_stride_bytes, batch_stride_bytes, &plan, &a);
    if (st != HMGPU_OK) return st; }
  hipStream_t hs = c->stream;
  { const hmgpu_status st = export_open(c, on_stream, stream, &hs); if (st != HMGPU_OK) return st; }
  const bool mono = c->seq.chroma_format == 0;
  a.n = n; a.mono = mono; a.comps = mono ? d->components & 1 : d->components;
  a.fmt = c->fmt; a.csx = c->csx; a.csy = c->csy;
  a.log2ctu = c->seq.log2_ctu_size; a.ctus_w = c->ctus_w; a.parts = c->parts;
  a.width = c->seq.width; a.height = c->seq.height;
  a.bd[0] = c->seq.bit_depth_luma; a.bd[1] = a.bd[2] = c->seq.bit_depth_chroma;
  for (int i = 0; i < n; i++) {
    const Picture& pic = c->pics[pics[i]];
    const PicDev& p = pic.dev;
    TransformSrc& s = a.src[i];
    s.depth = p.depth; s.part_size = p.part_size; s.pred_mode = p.pred_mode; s.qp = p.qp; s.tr_idx = p.tr_idx;
    for (int k = 0; k < 3; k++) { s.cbf[k] = p.cbf[k]; s.tskip[k] = p.tskip[k]; s.coef[k] = p.coef[k]; s.coef_start[k] = p.coef_start[k]; }
    s.bypass = p.bypass; s.ipcm = p.ipcm;
    s.intra_dir[0] = p.intra_dir[0]; s.intra_dir[1] = p.intra_dir[1];
    s.slice_idx = p.slice_idx; s.slices = p.slices; s.sl_m = p.sl_m;
    s.gate = (all_calls_had_intra_dir(pic) ? kTransDir : 0) | (pic.flags_staged ? kTransFlags : 0);
  }
  for (int k = 0; k < (mono ? 1 : 3); k++) if (dst[k]) a.scale[k] = d->scale[k];
  launch_transform(a, d->value == HMGPU_TRANSFORM_COEFFS, side_elem(d->sample_type, true), c->num_ctus, hs);
  return export_end(c, n, pics, on_stream, hs);
}


// ------------------------------------------------------------------------------------------------ loop-filter export (k_lfinfo.hip)
hmgpu_status hmgpu_loopfilter_plan_for(const hmgpu_seq_params* seq, const hmgpu_loopfilter_desc* d, const hmgpu_export_scale* sc, int32_t n,
                                       const hmgpu_export_window win[], hmgpu_loopfilter_plan* out) {
  if (!side_plan_open(seq, d, 7, n, out)) return HMGPU_EINVAL;
  if (d->form != HMGPU_LOOPFILTER_GRIDS && d->form != HMGPU_LOOPFILTER_DENSE) return HMGPU_EINVAL;
  if (d->form == HMGPU_LOOPFILTER_GRIDS) {
    if (sc || win || d->sample_type != HMGPU_SAMPLE_UINT) return HMGPU_EINVAL;
    if ((d->crop[0] | d->crop[1] | d->crop[2] | d->crop[3]) & 7) return HMGPU_EINVAL;         // whole 8x8 areas (a negative crop: crop_ok)
    int w, h;
    if (crop_ok(seq, d->crop, nullptr, &w, &h) != HMGPU_OK) return HMGPU_EINVAL;
    const int E = HMGPU_LOOPFILTER_DST_EDGE, S = HMGPU_LOOPFILTER_DST_SAO, ctu = 1 << seq->log2_ctu_size;
    out->channels[E] = HMGPU_LOOPFILTER_EDGE_CHANNELS; out->elem_bytes[E] = 2;
    out->width[E] = w / 4; out->height[E] = h / 4; out->row_bytes[E] = out->width[E] * 2;
    out->channels[S] = 3 * HMGPU_LOOPFILTER_SAO_CHANNELS; out->elem_bytes[S] = 1;               // the CTBs of the whole picture
    out->width[S] = (seq->width + ctu - 1) / ctu; out->height[S] = (seq->height + ctu - 1) / ctu; out->row_bytes[S] = out->width[S];
    return HMGPU_OK;
  }
  const int elem = side_elem(d->sample_type, true);                                            // (the integer element is uint8 here)
  if (elem < 0 || !side_scale_ok(elem, 7, d->scale)) return HMGPU_EINVAL;
  if (sc) { const hmgpu_status st = scale_desc_ok(sc); if (st != HMGPU_OK) return st; }
  int w = 0, h = 0;
  { const hmgpu_status st = dense_form_ok(seq, d->crop, sc, n, win, &w, &h); if (st != HMGPU_OK) return st; }
  const int D = HMGPU_LOOPFILTER_DST_DENSE;
  out->channels[D] = 3; out->elem_bytes[D] = elem == kElemU16 ? 1 : elem == kElemF32 ? 4 : 2;
  out->width[D] = w; out->height[D] = h; out->row_bytes[D] = w * out->elem_bytes[D];
  return HMGPU_OK;
}

// the pictures of a call: covered like every side-information export's; need_filter (the SAO grid, the dense form): a filter call has
// run on the handle's current picture, so that what the SAO parameters are -- resolved by that call, or known to be off -- is on record
static hmgpu_status loopfilter_pictures_ok(hmgpu_ctx* c, int32_t n, const hmgpu_pic* pics, bool need_filter) {
  { const hmgpu_status st = side_pictures_ok(c, n, pics); if (st != HMGPU_OK) return st; }
  for (int i = 0; i < n && need_filter; i++) if (!c->pics[pics[i]].lf_called) return HMGPU_EINVAL;
  return HMGPU_OK;
}

hmgpu_status hmgpu_pictures_loopfilter_check(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], int32_t need_filter) {
  return loopfilter_pictures_ok(c, n, pics, need_filter != 0);
}

// everything hmgpu_pictures_export_loopfilter checks: the plan, the pictures (pics null: hmgpu_loopfilter_destination_check, which has
// none), the destinations -- those of the other form must be null --; and what these give the kernel: *a zero but for its slots and vec
static hmgpu_status loopfilter_resolve(hmgpu_ctx* c, int32_t n, const hmgpu_pic* pics, const hmgpu_loopfilter_desc* d, const hmgpu_export_scale* sc,
                                       const hmgpu_export_window* windows, void* const dst[3], const int64_t* pitch, const int64_t* pstride,
                                       const int64_t* bstride, hmgpu_loopfilter_plan* plan, LfArgs* a) {
  if (!c || !d || !dst || !pitch || !pstride || !bstride) return HMGPU_EINVAL;
  { const hmgpu_status st = hmgpu_loopfilter_plan_for(&c->seq, d, sc, n, windows, plan); if (st != HMGPU_OK) return st; }
  const bool dense = d->form == HMGPU_LOOPFILTER_DENSE;
  if (pics) {
    const hmgpu_status st = loopfilter_pictures_ok(c, n, pics, dense || dst[HMGPU_LOOPFILTER_DST_SAO] != nullptr);
    if (st != HMGPU_OK) return st;
  }
  memset(a, 0, sizeof(*a));
  // dword stores: two int16 of the edge grid, four elements of the dense form
  { const hmgpu_status st = strided_dst_ok(c, *plan, HMGPU_LOOPFILTER_DSTS, n, dst, pitch, pstride, bstride, dense ? 0 : 4, &a->vec);
    if (st != HMGPU_OK) return st; }
  side_destinations(a, HMGPU_LOOPFILTER_DSTS, dst, pitch, pstride, bstride);
  return HMGPU_OK;
}

hmgpu_status hmgpu_loopfilter_destination_check(hmgpu_ctx* c, int32_t n, const hmgpu_loopfilter_desc* d, const hmgpu_export_scale* sc,
                                                const hmgpu_export_window windows[], void* const dst[3], const int64_t pitch_bytes[3],
                                                const int64_t plane_stride_bytes[3], const int64_t batch_stride_bytes[3]) {
  hmgpu_loopfilter_plan plan;
  LfArgs a;
  return loopfilter_resolve(c, n, nullptr, d, sc, windows, dst, pitch_bytes, plane_stride_bytes, batch_stride_bytes, &plan, &a);
}

hmgpu_status hmgpu_pictures_export_loopfilter(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_loopfilter_desc* d,
                                              const hmgpu_export_scale* sc, const hmgpu_export_window windows[], void* const dst[3],
                                              const int64_t pitch_bytes[3], const int64_t plane_stride_bytes[3],
                                              const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream) {
  if (!pics || (on_stream != 0 && on_stream != 1)) return HMGPU_EINVAL;
  hmgpu_loopfilter_plan plan;
  LfArgs a;
  { const hmgpu_status st = loopfilter_resolve(c, n, pics, d, sc, windows, dst, pitch_bytes, plane_stride_bytes, batch_stride_bytes, &plan, &a);
    if (st != HMGPU_OK) return st; }
  hipStream_t hs = c->stream;
  { const hmgpu_status st = export_open(c, on_stream, stream, &hs); if (st != HMGPU_OK) return st; }
  a.n = n; a.mono = c->seq.chroma_format == 0; a.fmt = c->fmt; a.csx = c->csx; a.csy = c->csy;
  a.log2ctu = c->seq.log2_ctu_size; a.ctus_w = c->ctus_w; a.ctus_h = c->ctus_h; a.ew = c->grid_w / 2;
  a.width = c->seq.width; a.height = c->seq.height;
  a.bd[0] = c->seq.bit_depth_luma; a.bd[1] = c->seq.bit_depth_chroma;
  for (int i = 0; i < n; i++) {
    const Picture& pic = c->pics[pics[i]];
    const PicDev& p = pic.dev;
    LfSrc& s = a.src[i];
    s.edges = p.edges; s.saoprm = p.saoprm; s.slice_idx = p.slice_idx; s.slices = p.slices;
    s.gate = pic.lf_sao ? kLfSao : 0;               // (the parameter buffer of a picture filtered without an SAO stage is stale: never read)
  }
  if (d->form == HMGPU_LOOPFILTER_GRIDS) {
    a.x8 = d->crop[0] / 8; a.y8 = d->crop[2] / 8;
    a.w8 = plan.width[HMGPU_LOOPFILTER_DST_EDGE] / 2; a.h8 = plan.height[HMGPU_LOOPFILTER_DST_EDGE] / 2;
    launch_lfinfo_grids(a, hs);
  } else {
    const int D = HMGPU_LOOPFILTER_DST_DENSE;
    a.W = plan.width[D]; a.H = plan.height[D];
    for (int k = 0; k < 3; k++) a.scale[k] = d->scale[k];
    for (int i = 0; i < n; i++) dense_window(c->seq, windows, i, &a.win[i], &a.flip);
    const int elem = side_elem(d->sample_type, true);
    launch_lfinfo_dense(a, elem == kElemU16 ? kElemU8 : elem, hs);
  }
  return export_end(c, n, pics, on_stream, hs);
}

}  // extern "C"
