// hmgpu_conceal.hip -- error concealment of the host runtime (include/hmgpu.h "error concealment", k_conceal.hip): the rules of a
// call, the masks on their way to the device, the one launch and the margin pass behind it.
#include "hmgpu_host.h"

namespace {

// everything hmgpu_pictures_conceal checks; host code
hmgpu_status conceal_rules(const hmgpu_ctx* c, int32_t n, const hmgpu_conceal_job* jobs) {
  if (!c || !jobs || n < 1 || n > HMGPU_EXPORT_MAX_BATCH) return HMGPU_EINVAL;
  const bool mono = c->seq.chroma_format == 0;
  const int bd[3] = {c->seq.bit_depth_luma, c->seq.bit_depth_chroma, c->seq.bit_depth_chroma};
  for (int i = 0; i < n; i++) {
    const hmgpu_conceal_job& j = jobs[i];
    for (int k = 0; k < 4; k++) if (j.reserved[k]) return HMGPU_EINVAL;
    if (!valid_pic(c, j.dst) || (j.src != HMGPU_NO_PIC && !valid_pic(c, j.src)) || j.dst == j.src) return HMGPU_EINVAL;
    if (j.mode != HMGPU_CONCEAL_COPY && j.mode != HMGPU_CONCEAL_MOTION) return HMGPU_EINVAL;
    for (int k = 0; k < (mono ? 1 : 3); k++) if (j.fill[k] > (1 << bd[k]) - 1) return HMGPU_EINVAL;
    if (j.ctu_mask && (c->num_ctus & 7) && (j.ctu_mask[c->num_ctus >> 3] >> (c->num_ctus & 7))) return HMGPU_EINVAL;
    for (int q = 0; q < n; q++)                                  // one writer per picture, and nobody reads what the call writes
      if (q != i && (jobs[q].dst == j.dst || jobs[q].src == j.dst)) return HMGPU_EINVAL;
  }
  return HMGPU_OK;
}

}  // namespace

extern "C" {

hmgpu_status hmgpu_conceal_check(hmgpu_ctx* c, int32_t n, const hmgpu_conceal_job jobs[]) { return conceal_rules(c, n, jobs); }

hmgpu_status hmgpu_picture_concealed_ctus(hmgpu_ctx* c, hmgpu_pic pic, int32_t* out) {
  if (!c || !out || !valid_pic(c, pic)) return HMGPU_EINVAL;
  *out = c->pics[pic].concealed_ctus;
  return HMGPU_OK;
}

hmgpu_status hmgpu_pictures_conceal(hmgpu_ctx* c, int32_t n, const hmgpu_conceal_job jobs[]) {
  { const hmgpu_status st = conceal_rules(c, n, jobs); if (st != HMGPU_OK) return st; }
  hipSetDevice(c->device);
  const size_t mb = align_up((size_t)(c->num_ctus + 7) / 8, 64);
  if (!c->conceal_masks) HIP_TRY(c, hipMalloc((void**)&c->conceal_masks, mb * kMaxBatch));
  // the masks of the call, one copy: a job without a mask names every CTU
  std::vector<uint8_t> masks(mb * n, 0);
  for (int i = 0; i < n; i++) {
    uint8_t* m = masks.data() + mb * i;
    if (jobs[i].ctu_mask) memcpy(m, jobs[i].ctu_mask, (size_t)(c->num_ctus + 7) / 8);
    else for (int a = 0; a < c->num_ctus; a++) m[a >> 3] |= (uint8_t)(1u << (a & 7));
  }
  bool staged = false;
  HIP_TRY(c, h2d_small(c, c->conceal_masks, masks.data(), masks.size(), c->stream, &staged));
  if (!staged) HIP_TRY(c, hipStreamSynchronize(c->stream));   // (not through the page-locked ring: `masks` goes with this call)

  ConcealArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n; a.mono = c->seq.chroma_format == 0;
  a.width = c->seq.width; a.height = c->seq.height; a.log2ctu = c->seq.log2_ctu_size;
  a.ctus_w = c->ctus_w; a.num_ctus = c->num_ctus; a.parts = c->parts;
  a.pitch_y = c->pitch[0]; a.pitch_c = c->pitch[1]; a.csx = c->csx; a.csy = c->csy;
  const int bd[3] = {c->seq.bit_depth_luma, c->seq.bit_depth_chroma, c->seq.bit_depth_chroma};
  Batch b;
  memset(&b, 0, sizeof(b));
  b.n = n;
  for (int i = 0; i < n; i++) {
    const hmgpu_conceal_job& j = jobs[i];
    ConcealPic& q = a.pic[i];
    Picture& d = c->pics[j.dst];
    q.dst_y = d.sao_applied ? d.dev.sao[0] : d.dev.rec[0];
    q.dst_c = d.sao_applied ? d.dev.sao[1] : d.dev.rec[1];
    if (j.src != HMGPU_NO_PIC) {
      const Picture& s = c->pics[j.src];
      q.src_y = s.sao_applied ? s.dev.sao[0] : s.dev.rec[0];
      q.src_c = s.sao_applied ? s.dev.sao[1] : s.dev.rec[1];
      q.part_size = s.dev.part_size; q.pred_mode = s.dev.pred_mode;
      for (int l = 0; l < 2; l++) { q.mv[l] = s.dev.mv[l]; q.ref_idx[l] = s.dev.ref_idx[l]; }
      q.slice_idx = s.dev.slice_idx; q.slices = s.dev.slices;
      q.side = s.covered_ctus == c->num_ctus;
      touch(c, j.src);
    }
    q.mask = c->conceal_masks + mb * i;
    q.mode = j.mode; q.dst_poc = j.dst_poc; q.src_poc = j.src_poc;
    uint32_t f[3];
    for (int k = 0; k < 3; k++) f[k] = (uint32_t)(j.fill[k] < 0 ? 1 << (bd[k] - 1) : j.fill[k]) & 0xffffu;
    q.fill_y = f[0] * 0x10001u; q.fill_c = f[1] | (f[2] << 16);
    b.pic[i] = j.dst;
    touch(c, j.dst);
  }
  launch_conceal(a, c->stream);
  // the margins of the concealed pictures: the border of their final planes again
  launch_extend(c->d_pics, b, c->seq.width, c->seq.height, c->mx[0], c->my[0], c->csx, c->csy, c->stream);
  HIP_TRY(c, hipGetLastError());
  for (int i = 0; i < n; i++) {
    Picture& d = c->pics[jobs[i].dst];
    d.extended = true;
    if (d.concealed.empty()) d.concealed.assign((size_t)c->num_ctus, false);
    const uint8_t* m = masks.data() + mb * i;
    for (int t = 0; t < c->num_ctus; t++)
      if (((m[t >> 3] >> (t & 7)) & 1) && !d.concealed[(size_t)t]) { d.concealed[(size_t)t] = true; d.concealed_ctus++; }
  }
  commit_use(c);
  return HMGPU_OK;
}

}  // extern "C"
