// hmgpu_export.hip -- picture export of the host runtime: the shared validation rules under the export plans, scale tables and their
// slots, window tables, colour LUTs, the rules and weights of the chroma stage, the weights and rules of the format export and the
// rules of the warp and of the packed YUV words; ExportReq, the stages of one
// picture export as a record, with export_plan under every plan function and export_resolve under export_impl and every picture
// destination check; export_impl's three argument builders (unscaled, scaled, warp with its per-call maps) (k_export.hip,
// k_export_scale.hip, k_export_warp.hip, k_export_fmt.hip, k_export_yuvpack.hip).  Also the rules and the stream bracket that the
// side-information exports (hmgpu_side.hip) and the picture analyses (hmgpu_analysis.hip) take from here: hmgpu_host.h.
#include "hmgpu_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

// ------------------------------------------------------------------------------------------------ shared with hmgpu_side.hip and hmgpu_analysis.hip (hmgpu_host.h)
namespace hmgpu_host __attribute__((visibility("hidden"))) {

// the chroma subsampling of a chroma_format_idc
void chroma_shifts(int fmt, int* csx, int* csy) { *csx = fmt == 3 ? 0 : 1; *csy = fmt == 1 || fmt == 0 ? 1 : 0; }

hmgpu_status scale_desc_ok(const hmgpu_export_scale* sc) {
  for (int k = 0; k < 5; k++) if (sc->reserved[k]) return HMGPU_EINVAL;
  if (sc->filter < HMGPU_SCALE_NEAREST || sc->filter > HMGPU_SCALE_AREA || sc->width <= 0 || sc->height <= 0) return HMGPU_EINVAL;
  return HMGPU_OK;
}

// the scaling limits of one axis: 16384 outputs, 32x down, 8x up
static bool scale_ratio_ok(long long in, long long out) { return out <= 16384 && in <= 32 * out && out <= 8 * in; }

// a crop of the coded picture, w x h: nothing negative, not empty, whole chroma samples, and (sc) within the limits of scaling to sc
hmgpu_status crop_ok(const hmgpu_seq_params* seq, const int32_t cr[4], const hmgpu_export_scale* sc, int* w, int* h) {
  if (cr[0] < 0 || cr[1] < 0 || cr[2] < 0 || cr[3] < 0) return HMGPU_EINVAL;
  *w = seq->width - cr[0] - cr[1]; *h = seq->height - cr[2] - cr[3];
  if (*w <= 0 || *h <= 0) return HMGPU_EINVAL;
  int csx, csy;
  chroma_shifts(seq->chroma_format, &csx, &csy);
  if (seq->chroma_format != 0 && (((cr[0] | cr[1]) & ((1 << csx) - 1)) || ((cr[2] | cr[3]) & ((1 << csy) - 1)))) return HMGPU_EINVAL;
  if (sc && !(scale_ratio_ok(*w, sc->width) && scale_ratio_ok(*h, sc->height))) return HMGPU_EUNSUPPORTED;
  return HMGPU_OK;
}

// a window: its own fields, then its crop
static bool window_fields_ok(const hmgpu_export_window& win) { return !((win.flip & ~1) || win.reserved[0] || win.reserved[1] || win.reserved[2]); }
hmgpu_status window_ok(const hmgpu_seq_params* seq, const hmgpu_export_window& win, const hmgpu_export_scale* sc, int* w, int* h) {
  return window_fields_ok(win) ? crop_ok(seq, win.crop, sc, w, h) : HMGPU_EINVAL;
}

// true if [p, p + bytes) lies inside one device allocation of `device`
bool device_span_ok(const void* p, size_t bytes, int device) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (at.type != hipMemoryTypeDevice || at.device != device) return false;
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return false; }
  const uintptr_t b = (uintptr_t)base, q = (uintptr_t)p;
  return q >= b && q - b + bytes <= size;
}

// the stream an export runs on: the context's (on_stream 0) or the caller's, which must belong to the context's device and then waits
// for everything enqueued for the pictures
hmgpu_status export_open(hmgpu_ctx* c, int32_t on_stream, void* stream, hipStream_t* hs) {
  *hs = c->stream;
  if (!on_stream) return HMGPU_OK;
  *hs = (hipStream_t)stream;
  if (*hs) {
    hipDevice_t dev = -1;
    if (hipStreamGetDevice(*hs, &dev) != hipSuccess) { (void)hipGetLastError(); return HMGPU_EINVAL; }
    if ((int)dev != c->device) return HMGPU_EINVAL;
  }
  for (int k = 0; k < 2; k++) if (!c->exp_ev[k]) HIP_TRY(c, hipEventCreateWithFlags(&c->exp_ev[k], hipEventDisableTiming));
  HIP_TRY(c, hipEventRecord(c->exp_ev[0], c->stream));                   // behind everything enqueued for the picture ...
  HIP_TRY(c, hipStreamWaitEvent(*hs, c->exp_ev[0], 0));                  // ... and behind what is already on the caller's stream
  return HMGPU_OK;
}

// after the export's launch
hmgpu_status export_end(hmgpu_ctx* c, int n, const hmgpu_pic* pics, int32_t on_stream, hipStream_t hs) {
  HIP_TRY(c, hipGetLastError());
  if (on_stream) {
    HIP_TRY(c, hipEventRecord(c->exp_ev[1], hs));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->exp_ev[1], 0));          // whatever the context does next with the picture waits for the export
  }
  for (int i = 0; i < n; i++) touch(c, pics[i]);
  commit_use(c);
  return HMGPU_OK;
}

// packed YUV: the table of the word formats (hmgpu_host.h)
bool yuvpack_format(int format, YuvPackFormat* p) {
  static const YuvPackFormat tab[8] = {
    {2, 8, 1, kPack422x8, 0, 0, 0}, {2, 8, 1, kPack422x8, 1, 0, 0}, {2, 10, 2, kPack422x16, 0, 6, 0}, {2, 16, 2, kPack422x16, 0, 0, 0},
    {2, 10, 4, kPackV210, 0, 0, 0}, {3, 8, 1, kPackAYUV, 0, 0, 255}, {3, 10, 4, kPackY410, 0, 0, 3}, {3, 16, 2, kPackY416, 0, 0, 65535}};
  if (format < HMGPU_YUVPACK_UYVY || format > HMGPU_YUVPACK_Y416) return false;
  *p = tab[format];
  return true;
}
int yuvpack_row_bytes(const YuvPackFormat& p, int w) {
  return p.fam == kPackV210 ? (w + 5) / 6 * 16 : p.fam == kPack422x8 ? 2 * w : p.fam == kPackY416 ? 8 * w : 4 * w;
}

}  // namespace hmgpu_host

extern "C" {

// ------------------------------------------------------------------------------------------------ device export (k_export.hip)
static long long round_half_away(double v) { return v < 0 ? -(long long)std::floor(-v + 0.5) : (long long)std::floor(v + 0.5); }

// the output depth per channel type (a 0 of the descriptor: the coding depth); RGB: the first one for both
static void out_depths(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, int ob[2]) {
  ob[0] = d->bit_depth[0] ? d->bit_depth[0] : seq->bit_depth_luma;
  ob[1] = d->layout == HMGPU_EXPORT_RGB ? ob[0] : d->bit_depth[1] ? d->bit_depth[1] : seq->bit_depth_chroma;
}

// H.273 Kr / Kb of the matrix_coefficients codes the export takes (Table 4): false for any other code
static bool matrix_kr_kb(int matrix, double* kr, double* kb) {
  switch (matrix) {
    case 1: *kr = 0.2126; *kb = 0.0722; return true;            // BT.709
    case 5: case 6: *kr = 0.299; *kb = 0.114; return true;      // BT.601 (625 / 525)
    case 9: *kr = 0.2627; *kb = 0.0593; return true;            // BT.2020 non-constant luminance
    default: return false;
  }
}

hmgpu_status hmgpu_export_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, hmgpu_export_plan* out) {
  if (!seq || !d || !out) return HMGPU_EINVAL;
  memset(out, 0, sizeof(*out));
  const int fmt = seq->chroma_format, bdY = seq->bit_depth_luma, bdC = seq->bit_depth_chroma;
  if (fmt < 0 || fmt > 3 || bdY < 8 || bdY > 12 || bdC < 8 || bdC > 12 || seq->width <= 0 || seq->height <= 0) return HMGPU_EINVAL;
  if (d->layout < HMGPU_EXPORT_PLANAR || d->layout > HMGPU_EXPORT_RGB) return HMGPU_EINVAL;
  if (d->bytes_per_sample != 1 && d->bytes_per_sample != 2) return HMGPU_EINVAL;
  if ((d->msb_aligned != 0 && d->msb_aligned != 1) || (d->msb_aligned && d->bytes_per_sample != 2)) return HMGPU_EINVAL;
  for (int k = 0; k < 6; k++) if (d->reserved[k]) return HMGPU_EINVAL;
  const bool rgb = d->layout == HMGPU_EXPORT_RGB, mono = fmt == 0;
  int csx, csy, ob[2], W, H;
  chroma_shifts(fmt, &csx, &csy);
  out_depths(seq, d, ob);
  const int lo = rgb ? 8 : 1;
  for (int t = 0; t < (mono && !rgb ? 1 : 2); t++)
    if (ob[t] < lo || ob[t] > 16 || (d->bytes_per_sample == 1 && ob[t] > 8)) return HMGPU_EINVAL;
  { const hmgpu_status st = crop_ok(seq, d->crop, nullptr, &W, &H); if (st != HMGPU_OK) return st; }
  const int B = d->bytes_per_sample;
  if (rgb) {
    if (d->full_range != 0 && d->full_range != 1) return HMGPU_EINVAL;
    double kr = 0, kb = 0;
    if (d->matrix == 0) {
      if (fmt != 3) return HMGPU_EINVAL;                         // identity: 4:4:4 only
    } else if (!matrix_kr_kb(d->matrix, &kr, &kb)) {
      return HMGPU_EUNSUPPORTED;
    }
    out->planes = 3;
    for (int k = 0; k < 3; k++) { out->width[k] = W; out->height[k] = H; out->row_bytes[k] = W * B; }
    const int M = (1 << ob[0]) - 1;
    out->coef[9] = M;
    if (d->matrix == 0) { out->coef[10] = 1; return HMGPU_OK; }
    const double kg = 1.0 - kr - kb;
    const int yo = d->full_range ? 0 : 16 << (bdY - 8), co = 1 << (bdC - 1);
    const double ys = d->full_range ? (double)((1 << bdY) - 1) : (double)(219 << (bdY - 8));
    const double cs = d->full_range ? (double)((1 << bdC) - 1) : (double)(224 << (bdC - 8));
    const double r[5] = {M / ys, M * 2.0 * (1.0 - kr) / cs, -M * 2.0 * kb * (1.0 - kb) / kg / cs, -M * 2.0 * kr * (1.0 - kr) / kg / cs, M * 2.0 * (1.0 - kb) / cs};
    const long long maxdy = std::max(yo, (1 << bdY) - 1 - yo), maxdc = co;
    for (int S = 30; S >= 1; S--) {
      long long c[5];
      for (int i = 0; i < 5; i++) c[i] = round_half_away(r[i] * (double)(1LL << S));
      const long long t = std::llabs(c[0]) * maxdy + (1LL << (S - 1));
      const long long bound = std::max({t + std::llabs(c[1]) * maxdc, t + (std::llabs(c[2]) + std::llabs(c[3])) * maxdc, t + std::llabs(c[4]) * maxdc});
      if (bound > INT32_MAX) continue;
      out->coef[0] = S; out->coef[1] = 1 << (S - 1); out->coef[2] = yo; out->coef[3] = co;
      for (int i = 0; i < 5; i++) out->coef[4 + i] = (int32_t)c[i];
      return HMGPU_OK;
    }
    return HMGPU_EUNSUPPORTED;
  }
  out->planes = mono ? 1 : d->layout == HMGPU_EXPORT_PLANAR ? 3 : 2;
  out->width[0] = W; out->height[0] = H; out->row_bytes[0] = W * B;
  for (int k = 1; k < out->planes; k++) {
    out->width[k] = W >> csx; out->height[k] = H >> csy;
    out->row_bytes[k] = (d->layout == HMGPU_EXPORT_PLANAR ? 1 : 2) * out->width[k] * B;
  }
  return HMGPU_OK;
}

// ------------------------------------------------------------------------------------------------ scaled export (k_export_scale.hip)
namespace {

// one resampling table: `in` source samples to `out` outputs (include/hmgpu.h "scaled export")
struct ScaleTab {
  int taps = 0;                        // widest row
  std::vector<int32_t> first, count;
  std::vector<int16_t> w;              // [out][taps]
  long long pos = 0, neg = 0;          // the largest sum of the positive / of the magnitudes of the negative weights of a row
};

double scale_filter(int filter, double x) {
  x = std::fabs(x);
  if (filter == HMGPU_SCALE_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
  const double a = -0.5;                                         // Keys, as PIL and torch's antialiased bicubic
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
  if (x < 2.0) return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a;
  return 0.0;
}

std::shared_ptr<const ScaleTab> build_scale_tab(int in, int out, int filter) {
  auto t = std::make_shared<ScaleTab>();
  std::vector<std::vector<int>> rows((size_t)out);
  t->first.resize((size_t)out);
  t->count.resize((size_t)out);
  std::vector<double> w;
  for (int i = 0; i < out; i++) {
    int lo = 0;
    w.clear();
    if (filter == HMGPU_SCALE_NEAREST) {                         // nearest-exact, the source index exact (no rounding at ties)
      lo = (int)std::min((2LL * i + 1) * in / (2LL * out), (long long)in - 1);
      w.push_back(1.0);
    } else if (filter == HMGPU_SCALE_AREA) {                     // adaptive average pooling
      lo = (int)((long long)i * in / out);
      const int hi = (int)(((long long)(i + 1) * in + out - 1) / out);
      w.assign((size_t)(hi - lo), 1.0 / (hi - lo));
    } else {                                                     // torch's antialiased interpolation (PIL's weights)
      const double scale = (double)in / out, support = (filter == HMGPU_SCALE_BILINEAR ? 1.0 : 2.0) * (scale >= 1.0 ? scale : 1.0);
      const double centre = scale * (i + 0.5), inv = scale >= 1.0 ? 1.0 / scale : 1.0;
      lo = (int)std::max((long long)(centre - support + 0.5), 0LL);
      const int hi = (int)std::min((long long)(centre + support + 0.5), (long long)in);
      double total = 0;
      for (int j = lo; j < hi; j++) { w.push_back(scale_filter(filter, (j - centre + 0.5) * inv)); total += w.back(); }
      if (total != 0.0) for (double& v : w) v /= total;
    }
    // Q14 by largest remainders: every weight rounded down, then one unit each to the largest remainders (lower index first on a tie)
    // until the row sums to 16384, so that every weight is within one unit of its exact value
    std::vector<int>& q = rows[(size_t)i];
    std::vector<std::pair<double, int>> rem;
    int sum = 0;
    for (size_t j = 0; j < w.size(); j++) {
      const double v = w[j] * 16384.0, f = std::floor(v);
      q.push_back((int)f);
      sum += q.back();
      rem.emplace_back(-(v - f), (int)j);
    }
    std::sort(rem.begin(), rem.end());
    for (int u = 0; u < 16384 - sum; u++) q[(size_t)rem[(size_t)u % rem.size()].second] += 1;
    size_t b = 0, e = q.size();
    while (q[b] == 0) b++;
    while (q[e - 1] == 0) e--;
    q = std::vector<int>(q.begin() + (ptrdiff_t)b, q.begin() + (ptrdiff_t)e);
    t->first[(size_t)i] = lo + (int)b;
    t->count[(size_t)i] = (int)q.size();
    t->taps = std::max(t->taps, (int)q.size());
    long long p = 0, n = 0;
    for (int v : q) (v > 0 ? p : n) += std::llabs(v);
    t->pos = std::max(t->pos, p);
    t->neg = std::max(t->neg, n);
  }
  t->w.assign((size_t)out * t->taps, 0);
  for (int i = 0; i < out; i++)
    for (size_t j = 0; j < rows[(size_t)i].size(); j++) t->w[(size_t)i * t->taps + j] = (int16_t)rows[(size_t)i][j];
  return t;
}

// the tables of one call whose windows differ (hmgpu_pictures_export_windows), keyed by (in, out, filter): windows that share them on
// an axis share a table.  Random windows never repeat, so these stay out of the process-wide map below, which would only be emptied by
// them.  The tables of the most recent such call are kept (call_tabs_recent), because one export validates the same windows more than
// once -- the plan for the caller's allocation, the destination check of libhmdec, then the export itself, per run of slots -- and
// each of these would derive every table again.
typedef std::map<std::tuple<int, int, int>, std::shared_ptr<const ScaleTab>> CallTabs;
std::mutex call_tabs_mu;
CallTabs call_tabs_recent;

std::shared_ptr<const ScaleTab> call_tab(CallTabs& tabs, int in, int out, int filter) {
  const auto key = std::make_tuple(in, out, filter);
  auto& t = tabs[key];
  if (t) return t;
  {
    std::lock_guard<std::mutex> g(call_tabs_mu);
    auto it = call_tabs_recent.find(key);
    if (it != call_tabs_recent.end()) t = it->second;
  }
  if (!t) t = build_scale_tab(in, out, filter);
  return t;
}

// after a windows call has been validated: its tables replace the kept ones
void call_tabs_keep(const CallTabs& tabs) {
  if (tabs.empty()) return;
  std::lock_guard<std::mutex> g(call_tabs_mu);
  call_tabs_recent = tabs;
}

// process-wide: the tables of recent shapes (a plan or an export of a repeated shape derives nothing)
std::shared_ptr<const ScaleTab> scale_tab(int in, int out, int filter) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, int>, std::shared_ptr<const ScaleTab>> tabs;
  const auto key = std::make_tuple(in, out, filter);
  {
    std::lock_guard<std::mutex> g(mu);
    auto it = tabs.find(key);
    if (it != tabs.end()) return it->second;
  }
  auto t = build_scale_tab(in, out, filter);
  std::lock_guard<std::mutex> g(mu);
  if (tabs.size() >= 64) tabs.clear();
  tabs[key] = t;
  return t;
}

// everything a scaled export of one shape needs on the host: the plan, per plane class its tables
struct ScaleShape {
  int classes = 1;                                              // 2: YUV with chroma
  int in[2][2] = {}, out[2][2] = {};                             // [class][axis]
  std::shared_ptr<const ScaleTab> tab[2][2];
  int depth[2] = {8, 8};                                         // output depth per class
};

// t = (h + 2^(13-E)) >> (14-E), o = (sum wy t + 2^(13+E)) >> (14+E): no 32-bit sum overflows for samples 0 .. 2^D - 1
bool scale_sums_fit(const ScaleTab& x, const ScaleTab& y, int D, int E) {
  const long long V = (1LL << D) - 1, r1 = 1LL << (13 - E), r2 = 1LL << (13 + E);
  const long long hmax = x.pos * V + r1, hmin = -x.neg * V + r1;
  if (hmax > INT32_MAX || hmin < INT32_MIN) return false;
  const long long tmax = hmax >> (14 - E), tmin = hmin >> (14 - E);       // (arithmetic shifts: floor)
  const long long vmax = y.pos * tmax + y.neg * std::max(-tmin, 0LL) + r2;
  const long long vmin = -(y.pos * std::max(-tmin, 0LL) + y.neg * tmax) + r2;
  return vmax <= INT32_MAX && vmin >= INT32_MIN;
}

// a YUV plan at the output chroma format fo of a format export: the chroma planes and their sizes from plane 0's
void plan_set_format(const hmgpu_export_desc* d, int fo, hmgpu_export_plan* out) {
  int osx, osy;
  chroma_shifts(fo, &osx, &osy);
  const int W = out->width[0], H = out->height[0], B = d->bytes_per_sample;
  out->planes = fo == 0 ? 1 : d->layout == HMGPU_EXPORT_PLANAR ? 3 : 2;
  for (int k = 1; k < 3; k++) {
    const bool has = k < out->planes;
    out->width[k] = has ? W >> osx : 0; out->height[k] = has ? H >> osy : 0;
    out->row_bytes[k] = has ? (d->layout == HMGPU_EXPORT_PLANAR ? 1 : 2) * out->width[k] * B : 0;
  }
}

// fmt_out: -1, or the output chroma format of a format export (YUV layouts): plane class 1 then goes from the cropped source chroma
// plane to the chroma size of that format
hmgpu_status scaled_plan(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, const hmgpu_export_scale* sc, hmgpu_export_plan* out,
                         ScaleShape* shape, CallTabs* call_tabs = nullptr, int fmt_out = -1) {
  if (!seq || !d || !sc || !out) return HMGPU_EINVAL;
  memset(out, 0, sizeof(*out));
  { const hmgpu_status st = scale_desc_ok(sc); if (st != HMGPU_OK) return st; }
  hmgpu_export_plan base;
  { const hmgpu_status st = hmgpu_export_plan_for(seq, d, &base); if (st != HMGPU_OK) return st; }
  if (fmt_out >= 0) plan_set_format(d, fmt_out, &base);
  const bool rgb = d->layout == HMGPU_EXPORT_RGB, chroma = !rgb && base.planes > 1 && seq->chroma_format != 0;
  int csx, csy, osx, osy;
  chroma_shifts(seq->chroma_format, &csx, &csy);
  chroma_shifts(fmt_out >= 0 ? fmt_out : seq->chroma_format, &osx, &osy);
  if (chroma && ((sc->width & ((1 << osx) - 1)) || (sc->height & ((1 << osy) - 1)))) return HMGPU_EINVAL;   // whole chroma samples
  ScaleShape s;
  s.classes = chroma ? 2 : 1;
  const int W = base.width[0], H = base.height[0];
  out_depths(seq, d, s.depth);
  for (int k = 0; k < s.classes; k++) {
    const int sx = k ? csx : 0, sy = k ? csy : 0;
    s.in[k][0] = W >> sx; s.in[k][1] = H >> sy;
    s.out[k][0] = sc->width >> (k ? osx : 0); s.out[k][1] = sc->height >> (k ? osy : 0);
    for (int ax = 0; ax < 2; ax++) if (!scale_ratio_ok(s.in[k][ax], s.out[k][ax])) return HMGPU_EUNSUPPORTED;
  }
  const int D = std::max(s.depth[0], s.depth[chroma ? 1 : 0]);
  const int E = 16 - D;
  int taps[2] = {0, 0};
  for (int k = 0; k < s.classes; k++) {
    for (int ax = 0; ax < 2; ax++) {
      if (call_tabs) {
        s.tab[k][ax] = call_tab(*call_tabs, s.in[k][ax], s.out[k][ax], sc->filter);
      } else {
        s.tab[k][ax] = scale_tab(s.in[k][ax], s.out[k][ax], sc->filter);
      }
      taps[ax] = std::max(taps[ax], s.tab[k][ax]->taps);
    }
    if (!scale_sums_fit(*s.tab[k][0], *s.tab[k][1], s.depth[k], E)) return HMGPU_EUNSUPPORTED;
  }
  *out = base;
  for (int p = 0; p < out->planes; p++) {
    const int k = rgb || p == 0 ? 0 : 1;
    const int w = k ? sc->width >> osx : sc->width, h = k ? sc->height >> osy : sc->height;
    out->row_bytes[p] = out->row_bytes[p] / out->width[p] * w;
    out->width[p] = w; out->height[p] = h;
  }
  out->coef[11] = E; out->coef[12] = taps[0]; out->coef[13] = taps[1];
  if (shape) *shape = s;
  return HMGPU_OK;
}

}  // namespace

hmgpu_status hmgpu_export_scale_taps(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, const hmgpu_export_scale* sc, int32_t chroma,
                                     int32_t axis, int32_t max_taps, int32_t* first, int32_t* count, int16_t* weights) {
  if (!first || !count || !weights || (chroma != 0 && chroma != 1) || (axis != 0 && axis != 1)) return HMGPU_EINVAL;
  hmgpu_export_plan plan;
  ScaleShape s;
  { const hmgpu_status st = scaled_plan(seq, d, sc, &plan, &s); if (st != HMGPU_OK) return st; }
  if (chroma >= s.classes) return HMGPU_EINVAL;
  const ScaleTab& t = *s.tab[chroma][axis];
  if (max_taps < t.taps) return HMGPU_EINVAL;
  const int n = s.out[chroma][axis];
  memcpy(first, t.first.data(), sizeof(int32_t) * (size_t)n);
  memcpy(count, t.count.data(), sizeof(int32_t) * (size_t)n);
  for (int i = 0; i < n; i++) {
    memset(weights + (size_t)i * max_taps, 0, sizeof(int16_t) * (size_t)max_taps);
    memcpy(weights + (size_t)i * max_taps, t.w.data() + (size_t)i * t.taps, sizeof(int16_t) * (size_t)t.taps);
  }
  return HMGPU_OK;
}

namespace {

// tile of one plane class (ScaleClass): wide enough to share source samples, small enough to give the GPU work for every CU, and the
// LDS of a pass (C channels: 16-bit staged samples + 32-bit horizontal sums) within kScaleLdsBytes
struct ScaleTiles { int tw, th, rows, cap, tiles_x, tiles_y; std::vector<int32_t> span[2]; };

std::vector<int32_t> scale_spans(const ScaleTab& t, int n, int tile) {
  std::vector<int32_t> sp;
  for (int i0 = 0; i0 < n; i0 += tile) {
    int lo = INT32_MAX, hi = 0;
    for (int i = i0; i < std::min(n, i0 + tile); i++) { lo = std::min(lo, t.first[(size_t)i]); hi = std::max(hi, t.first[(size_t)i] + t.count[(size_t)i]); }
    sp.push_back(lo); sp.push_back(hi);
  }
  return sp;
}

// the tile a class starts from: wide for sharing source samples, shrunk towards 64 outputs while the n pictures of a call bring fewer
// than ~1000 workgroups (large reductions: or a few workgroups would do all the work)
void scale_tile_start(int outw, int outh, int n, int* tw_out, int* th_out) {
  int tw = 128;
  while (tw > 4 && tw / 2 >= outw) tw /= 2;
  int th = 1024 / tw;
  while (th > 1 && th / 2 >= outh) th /= 2;
  auto blocks = [&]() { return (long long)((outw + tw - 1) / tw) * ((outh + th - 1) / th); };
  while (blocks() * n < 1024 && tw * th > 64) {
    if (th >= tw / 4 && th > 2) th /= 2;
    else if (tw > 16) tw /= 2;
    else break;
  }
  *tw_out = tw; *th_out = th;
}

ScaleTiles scale_tiles(const ScaleTab& tx, const ScaleTab& ty, int outw, int outh, int x0, int C, int tw, int th) {
  const int G = C == 2 ? 4 : 8;
  ScaleTiles z;
  z.tw = tw; z.th = th;
  for (;;) {
    z.span[0] = scale_spans(tx, outw, z.tw);
    z.cap = 0;
    for (size_t i = 0; i < z.span[0].size(); i += 2) {
      const int a = (x0 + z.span[0][i]) & ~(G - 1), b = (x0 + z.span[0][i + 1] + G - 1) & ~(G - 1);
      z.cap = std::max(z.cap, b - a);
    }
    z.cap = (z.cap + 7) & ~7;
    z.rows = std::min(1024 / z.tw, kScaleLdsBytes / (C * (2 * z.cap + 4 * z.tw)));
    if ((z.rows >= 4 || z.tw <= 16) && z.rows >= 1) break;
    z.tw /= 2;
  }
  z.span[1] = scale_spans(ty, outh, z.th);
  z.tiles_x = (outw + z.tw - 1) / z.tw;
  z.tiles_y = (outh + z.th - 1) / z.th;
  return z;
}

// a table buffer nobody reads any more, with room for `bytes`: waits for the export that read it last; too small, the device and host
// pair is allocated again with `grow` bytes
static hmgpu_status table_room(hmgpu_ctx* c, hmgpu_ctx::TableBuf* b, size_t bytes, size_t grow) {
  if (b->pending) HIP_TRY(c, hipEventSynchronize(b->done));
  b->pending = false;
  if (bytes > b->cap) {
    if (b->dev) HIP_TRY(c, hipFree(b->dev));
    if (b->host) HIP_TRY(c, hipHostFree(b->host));
    b->dev = b->host = nullptr;
    b->cap = 0;
    HIP_TRY(c, hipMalloc(&b->dev, grow));
    HIP_TRY(c, hipHostMalloc(&b->host, grow, hipHostMallocDefault));
    b->cap = grow;
  }
  if (!b->done) HIP_TRY(c, hipEventCreateWithFlags(&b->done, hipEventDisableTiming));
  return HMGPU_OK;
}

// the slot that holds the tables of `key`: found, or filled (least recently used slot) with a copy enqueued on hs
hmgpu_status scale_slot(hmgpu_ctx* c, const int32_t key[8], const ScaleShape& s, bool rgb, int x0c[2], const int tile[2][2], hipStream_t hs, hmgpu_ctx::ScaleSlot** out) {
  hmgpu_ctx::ScaleSlot* slot = nullptr;
  for (auto& sl : c->scale_slot)
    if (sl.valid && !memcmp(sl.key, key, sizeof(sl.key))) { slot = &sl; break; }
  if (!slot) {
    slot = &c->scale_slot[0];
    for (auto& sl : c->scale_slot) {
      if (!sl.valid) { slot = &sl; break; }
      if (sl.used < slot->used) slot = &sl;
    }
    slot->valid = false;
    // layout: per class and axis first, count, span, weights (tap-major), each 256-byte aligned
    ScaleTiles z[2];
    size_t off[2][2][4], bytes = 0;
    for (int k = 0; k < s.classes; k++) {
      const int C = rgb ? 3 : k ? 2 : 1;
      z[k] = scale_tiles(*s.tab[k][0], *s.tab[k][1], s.out[k][0], s.out[k][1], x0c[k], C, tile[k][0], tile[k][1]);
      for (int ax = 0; ax < 2; ax++) {
        const size_t n = (size_t)s.out[k][ax], sizes[4] = {4 * n, 4 * n, 4 * z[k].span[ax].size(), 2 * n * (size_t)s.tab[k][ax]->taps};
        for (int f = 0; f < 4; f++) { off[k][ax][f] = bytes; bytes += align_up(sizes[f], 256); }
      }
    }
    { const hmgpu_status st = table_room(c, slot, bytes, bytes); if (st != HMGPU_OK) return st; }   // (an export in flight may still read it)
    for (int k = 0; k < s.classes; k++) {
      ScaleClass& cl = slot->cls[k];
      memset(&cl, 0, sizeof(cl));
      for (int ax = 0; ax < 2; ax++) {
        const ScaleTab& t = *s.tab[k][ax];
        const int n = s.out[k][ax];
        memcpy(slot->host + off[k][ax][0], t.first.data(), 4 * (size_t)n);
        memcpy(slot->host + off[k][ax][1], t.count.data(), 4 * (size_t)n);
        memcpy(slot->host + off[k][ax][2], z[k].span[ax].data(), 4 * z[k].span[ax].size());
        int16_t* w = reinterpret_cast<int16_t*>(slot->host + off[k][ax][3]);
        for (int j = 0; j < t.taps; j++)
          for (int i = 0; i < n; i++) w[(size_t)j * n + i] = t.w[(size_t)i * t.taps + j];
        ScaleTable& d = ax ? cl.ty : cl.tx;
        d.first = reinterpret_cast<const int32_t*>(slot->dev + off[k][ax][0]);
        d.count = reinterpret_cast<const int32_t*>(slot->dev + off[k][ax][1]);
        d.span = reinterpret_cast<const int32_t*>(slot->dev + off[k][ax][2]);
        d.w = reinterpret_cast<const int16_t*>(slot->dev + off[k][ax][3]);
        d.n = n;
      }
      cl.tw = z[k].tw; cl.th = z[k].th; cl.rows = z[k].rows; cl.span_cap = z[k].cap;
      cl.tiles_x = z[k].tiles_x; cl.blocks = z[k].tiles_x * z[k].tiles_y;
    }
    HIP_TRY(c, hipMemcpyAsync(slot->dev, slot->host, bytes, hipMemcpyHostToDevice, hs));
    memcpy(slot->key, key, sizeof(slot->key));
    slot->valid = true;
  }
  slot->used = ++c->scale_tick;
  *out = slot;
  return HMGPU_OK;
}

// hmgpu_pictures_export_windows, windows that differ: the blob of one call -- the per-picture classes ([n][2] ScaleClass), then every
// distinct table (first, count, weights tap-major) and every distinct span list, each 256-byte aligned -- built in the next buffer of
// the ring and sent in one copy on hs.  tile: where the classes' tiles start (scale_tile_start); tw shrinks until the LDS of a pass
// fits the most demanding window.  cls: tw, th, tiles_x and blocks of the call; *pic_cls: the classes in device memory.
hmgpu_status window_tables(hmgpu_ctx* c, int n, const std::vector<ScaleShape>& shapes, const hmgpu_export_window* win, bool rgb,
                           const int tile[2][2], hipStream_t hs, ScaleClass cls[2], const ScaleClass** pic_cls, hmgpu_ctx::TableBuf** out) {
  const int classes = shapes[0].classes;
  std::vector<ScaleTiles> z((size_t)n * 2);
  for (int k = 0; k < classes; k++) {
    const int C = rgb ? 3 : k ? 2 : 1;
    for (int tw = tile[k][0];;) {
      int least = tw;
      for (int i = 0; i < n; i++) {
        const ScaleShape& s = shapes[(size_t)i];
        z[(size_t)i * 2 + k] = scale_tiles(*s.tab[k][0], *s.tab[k][1], s.out[k][0], s.out[k][1], k ? win[i].crop[0] >> c->csx : win[i].crop[0], C, tw, tile[k][1]);
        least = std::min(least, z[(size_t)i * 2 + k].tw);
      }
      if (least == tw) break;
      tw = least;
    }
  }
  std::vector<char> blob(align_up((size_t)n * 2 * sizeof(ScaleClass), 256), 0);
  auto place = [&](const void* src, size_t bytes) {
    const size_t off = blob.size();
    blob.resize(off + align_up(bytes, 256), 0);
    memcpy(blob.data() + off, src, bytes);
    return off;
  };
  std::map<const ScaleTab*, size_t> tab_at;                                // first; count and the weights follow
  std::map<std::pair<const ScaleTab*, int>, size_t> span_at;               // (table, tile size)
  struct TabOff { size_t first, count, w, span; };
  std::vector<TabOff> offs((size_t)n * 4);
  std::vector<int16_t> w;
  for (int i = 0; i < n; i++) {
    for (int k = 0; k < classes; k++) {
      const ScaleTiles& zt = z[(size_t)i * 2 + k];
      for (int ax = 0; ax < 2; ax++) {
        const ScaleTab* t = shapes[(size_t)i].tab[k][ax].get();
        const int no = shapes[(size_t)i].out[k][ax];
        TabOff& o = offs[(size_t)i * 4 + k * 2 + ax];
        auto it = tab_at.find(t);
        if (it == tab_at.end()) {
          const size_t at = place(t->first.data(), 4 * (size_t)no);
          place(t->count.data(), 4 * (size_t)no);
          w.assign((size_t)no * t->taps, 0);
          for (int j = 0; j < t->taps; j++)
            for (int q = 0; q < no; q++) w[(size_t)j * no + q] = t->w[(size_t)q * t->taps + j];
          place(w.data(), 2 * w.size());
          it = tab_at.emplace(t, at).first;
        }
        o.first = it->second;
        o.count = o.first + align_up(4 * (size_t)no, 256);
        o.w = o.count + align_up(4 * (size_t)no, 256);
        const auto skey = std::make_pair(t, ax ? zt.th : zt.tw);
        auto sp = span_at.find(skey);
        if (sp == span_at.end()) sp = span_at.emplace(skey, place(zt.span[ax].data(), 4 * zt.span[ax].size())).first;
        o.span = sp->second;
      }
    }
  }
  hmgpu_ctx::TableBuf* wb = &c->window_buf[c->window_next];
  c->window_next = (c->window_next + 1) % hmgpu_ctx::kWindowBufs;
  // (the export that read the buffer last may still be in flight; head room: the next call's windows differ)
  { const hmgpu_status st = table_room(c, wb, blob.size(), align_up(blob.size() + blob.size() / 2, 4096)); if (st != HMGPU_OK) return st; }
  ScaleClass* pc = reinterpret_cast<ScaleClass*>(blob.data());
  for (int i = 0; i < n; i++) {
    for (int k = 0; k < classes; k++) {
      const ScaleTiles& zt = z[(size_t)i * 2 + k];
      ScaleClass& cl = pc[i * 2 + k];
      for (int ax = 0; ax < 2; ax++) {
        const TabOff& o = offs[(size_t)i * 4 + k * 2 + ax];
        ScaleTable& d = ax ? cl.ty : cl.tx;
        d.first = reinterpret_cast<const int32_t*>(wb->dev + o.first);
        d.count = reinterpret_cast<const int32_t*>(wb->dev + o.count);
        d.span = reinterpret_cast<const int32_t*>(wb->dev + o.span);
        d.w = reinterpret_cast<const int16_t*>(wb->dev + o.w);
        d.n = shapes[(size_t)i].out[k][ax];
      }
      cl.tw = zt.tw; cl.th = zt.th; cl.rows = zt.rows; cl.span_cap = zt.cap;
      cl.tiles_x = zt.tiles_x; cl.blocks = zt.tiles_x * zt.tiles_y;
      cl.x0 = k ? win[i].crop[0] >> c->csx : win[i].crop[0];
      cl.y0 = k ? win[i].crop[2] >> c->csy : win[i].crop[2];
      cl.pitch = c->pitch[k];
      if (!i) cls[k] = cl;
    }
  }
  memcpy(wb->host, blob.data(), blob.size());
  HIP_TRY(c, hipMemcpyAsync(wb->dev, wb->host, blob.size(), hipMemcpyHostToDevice, hs));
  *pic_cls = reinterpret_cast<const ScaleClass*>(wb->dev);
  *out = wb;
  return HMGPU_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ the export entry points
// the output element (kElem*) of a descriptor already validated by its plan function, and of `t` (null: unsigned)
static hmgpu_status export_elem(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, const hmgpu_export_tensor* t, int* elem) {
  *elem = d->bytes_per_sample == 1 ? kElemU8 : kElemU16;
  if (!t) return HMGPU_OK;
  for (int k = 0; k < 5; k++) if (t->reserved[k]) return HMGPU_EINVAL;
  if (t->sample_type < HMGPU_SAMPLE_UINT || t->sample_type > HMGPU_SAMPLE_F32) return HMGPU_EINVAL;
  if (t->sample_type == HMGPU_SAMPLE_UINT) return HMGPU_OK;
  if (d->msb_aligned) return HMGPU_EINVAL;
  for (int k = 0; k < 3; k++) if (!std::isfinite(t->scale[k]) || !std::isfinite(t->bias[k])) return HMGPU_EINVAL;
  int ob[2];
  out_depths(seq, d, ob);
  const int D = seq->chroma_format != 0 ? std::max(ob[0], ob[1]) : ob[0];
  if (d->bytes_per_sample != (D <= 8 ? 1 : 2)) return HMGPU_EINVAL;      // the container an unsigned export of that depth needs
  if (d->layout == HMGPU_EXPORT_SEMIPLANAR) return HMGPU_EUNSUPPORTED;
  *elem = t->sample_type == HMGPU_SAMPLE_F16 ? kElemF16 : t->sample_type == HMGPU_SAMPLE_BF16 ? kElemBF16 : kElemF32;
  return HMGPU_OK;
}

static int elem_size(int elem) { return elem == kElemU8 ? 1 : elem == kElemF32 ? 4 : 2; }

static hmgpu_status tensor_plan(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                const hmgpu_export_tensor* t, hmgpu_export_plan* out, ScaleShape* shape, int* elem, CallTabs* call_tabs = nullptr,
                                int fmt_out = -1) {
  if (!seq || !d || !out) return HMGPU_EINVAL;
  { const hmgpu_status st = sc ? scaled_plan(seq, d, sc, out, shape, call_tabs, fmt_out) : hmgpu_export_plan_for(seq, d, out); if (st != HMGPU_OK) return st; }
  if (!sc && fmt_out >= 0) plan_set_format(d, fmt_out, out);
  const hmgpu_status st = export_elem(seq, d, t, elem);
  if (st != HMGPU_OK) { memset(out, 0, sizeof(*out)); return st; }
  if (*elem >= kElemF16)
    for (int k = 0; k < out->planes; k++) out->row_bytes[k] = out->width[k] * elem_size(*elem);
  return HMGPU_OK;
}

// hmgpu_pictures_export_windows: every window validated as the single call validates its crop, in order (the first failure is the
// call's status).  differ: the windows are not all equal; shapes (scaled): one per window then, else one for all.
static hmgpu_status windows_plan(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, const hmgpu_export_scale* sc, const hmgpu_export_tensor* t,
                                 int n, const hmgpu_export_window* win, hmgpu_export_plan* out, std::vector<ScaleShape>* shapes, int* elem,
                                 bool* differ, bool any_size = false, int fmt_out = -1) {
  if (!seq || !d || !out) return HMGPU_EINVAL;
  memset(out, 0, sizeof(*out));
  if (!win || n < 1 || n > HMGPU_EXPORT_MAX_BATCH) return HMGPU_EINVAL;
  if (d->crop[0] || d->crop[1] || d->crop[2] || d->crop[3]) return HMGPU_EINVAL;          // the window is the crop
  *differ = false;
  for (int i = 1; i < n; i++) if (memcmp(win[i].crop, win[0].crop, sizeof(win[0].crop))) *differ = true;
  CallTabs tabs;
  hmgpu_export_plan plan;
  if (shapes) shapes->clear();
  for (int i = 0; i < n; i++) {
    if (!window_fields_ok(win[i])) { memset(out, 0, sizeof(*out)); return HMGPU_EINVAL; }
    if (i && !*differ) continue;
    hmgpu_export_desc dd = *d;
    memcpy(dd.crop, win[i].crop, sizeof(dd.crop));
    ScaleShape s;
    const hmgpu_status st = tensor_plan(seq, &dd, sc, t, &plan, &s, elem, *differ && sc ? &tabs : nullptr, fmt_out);
    if (st != HMGPU_OK) { memset(out, 0, sizeof(*out)); return st; }
    if (shapes && sc) shapes->push_back(s);
    if (!i) { *out = plan; continue; }
    // (unscaled; any_size: the warp export, whose output size is not the windows')
    if (!any_size && (plan.width[0] != out->width[0] || plan.height[0] != out->height[0])) { memset(out, 0, sizeof(*out)); return HMGPU_EINVAL; }
    out->coef[12] = std::max(out->coef[12], plan.coef[12]);
    out->coef[13] = std::max(out->coef[13], plan.coef[13]);
  }
  call_tabs_keep(tabs);
  return HMGPU_OK;
}

// every plane's destination, all n pictures of it, inside one allocation of the context's device (bstride null: one picture); vec is
// cleared unless every group of 4 samples of every picture may be one store; bs: the batch strides in use
static hmgpu_status export_dst_ok(const hmgpu_ctx* c, const hmgpu_export_plan& plan, int ES, int n, void* const dst[3],
                                  const int64_t pitch_bytes[3], const int64_t* bstride, bool* vec, int64_t bs[3]) {
  hipSetDevice(c->device);
  for (int k = 0; k < plan.planes; k++) {
    if (!dst[k] || pitch_bytes[k] < plan.row_bytes[k] || pitch_bytes[k] > ((int64_t)1 << 40)) return HMGPU_EINVAL;
    const int64_t extent = pitch_bytes[k] * (plan.height[k] - 1) + plan.row_bytes[k];
    if (bstride) {
      if (bstride[k] < extent || bstride[k] > ((int64_t)1 << 56)) return HMGPU_EINVAL;
      bs[k] = bstride[k];
    }
    if (!device_span_ok(dst[k], (size_t)((n - 1) * bs[k] + extent), c->device)) return HMGPU_EINVAL;
    *vec = *vec && ((uintptr_t)dst[k] % (4 * ES)) == 0 && pitch_bytes[k] % (4 * ES) == 0 && (n == 1 || bs[k] % (4 * ES) == 0);
  }
  return HMGPU_OK;
}

// packed pixels (include/hmgpu.h "packed pixel export"): `plan`, the planar RGB plan of the call already validated, becomes the
// one-plane plan of the packed destination; po: the channel order and the A element as the kernels take them
static hmgpu_status pixel_plan(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, int elem, const hmgpu_export_pixel* px,
                               hmgpu_export_plan* plan, PxOrder* po) {
  hmgpu_export_plan p = *plan;
  memset(plan, 0, sizeof(*plan));
  if (d->layout != HMGPU_EXPORT_RGB) return HMGPU_EINVAL;
  if (px->order < HMGPU_PIXEL_RGB || px->order > HMGPU_PIXEL_ABGR) return HMGPU_EINVAL;
  for (int k = 0; k < 5; k++) if (px->reserved[k]) return HMGPU_EINVAL;
  const int C = px->order <= HMGPU_PIXEL_BGR ? 3 : 4;
  memset(po, 0, sizeof(*po));
  po->swap = px->order == HMGPU_PIXEL_BGR || px->order == HMGPU_PIXEL_BGRA || px->order == HMGPU_PIXEL_ABGR;
  po->afirst = px->order == HMGPU_PIXEL_ARGB || px->order == HMGPU_PIXEL_ABGR;
  if (C == 4 && elem <= kElemU16) {
    int ob[2];
    out_depths(seq, d, ob);
    const int D = ob[0];
    if (px->alpha < -1 || px->alpha > (1 << D) - 1) return HMGPU_EINVAL;
    po->abits = (uint32_t)(px->alpha < 0 ? (1 << D) - 1 : px->alpha) << (d->msb_aligned ? 16 - D : 0);
  } else if (C == 4) {
    const float f = px->alpha_value;
    if (!std::isfinite(f)) return HMGPU_EINVAL;
    uint32_t u;
    memcpy(&u, &f, 4);
    if (elem == kElemF16) { const _Float16 h = (_Float16)f; uint16_t b; memcpy(&b, &h, 2); u = b; }
    else if (elem == kElemBF16) u = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    po->abits = u;
  }
  p.planes = 1;
  p.row_bytes[0] = p.width[0] * C * elem_size(elem);
  for (int k = 1; k < 3; k++) p.width[k] = p.height[k] = p.row_bytes[k] = 0;
  *plan = p;
  return HMGPU_OK;
}

// ------------------------------------------------------------------------------------------------ colour LUTs (colour_core.h)
// a LUT description by itself: the rules that need neither tables nor a context
static bool colour_desc_ok(const hmgpu_colour_lut_desc* ld) {
  if (!ld || ld->depth < 8 || ld->depth > 16 || (ld->size != 0 && (ld->size < 2 || ld->size > 65))) return false;
  if ((ld->has_shaper != 0 && ld->has_shaper != 1) || (!ld->has_shaper && !ld->size)) return false;
  for (int k = 0; k < 5; k++) if (ld->reserved[k]) return false;
  return true;
}

hmgpu_status hmgpu_colour_lut_check(const hmgpu_colour_lut_desc* ld, const uint16_t* shaper, const uint16_t* lattice) {
  if (!colour_desc_ok(ld) || (ld->has_shaper && !shaper) || (ld->size && !lattice)) return HMGPU_EINVAL;
  const uint32_t M = (1u << ld->depth) - 1u;
  const size_t nodes = (size_t)ld->size * ld->size * ld->size;
  for (size_t i = 0; i < 3 * nodes; i++) if (lattice[i] > M) return HMGPU_EINVAL;
  if (!ld->size)
    for (size_t i = 0; i < ((size_t)3 << ld->depth); i++) if (shaper[i] > M) return HMGPU_EINVAL;
  return HMGPU_OK;
}

hmgpu_status hmgpu_colour_lut_create(hmgpu_ctx* c, const hmgpu_colour_lut_desc* ld, const uint16_t* shaper, const uint16_t* lattice,
                                     hmgpu_lut* out) {
  if (!c || !out) return HMGPU_EINVAL;
  *out = 0;
  { const hmgpu_status st = hmgpu_colour_lut_check(ld, shaper, lattice); if (st != HMGPU_OK) return st; }
  hmgpu_ctx::ColourSlot* cs = nullptr;
  for (auto& sl : c->colour_slot) if (!sl.handle) { cs = &sl; break; }
  if (!cs) return HMGPU_ENOMEM;
  // device layout: the nodes, 8 bytes each {R | G << 16, B} (a vertex is one load), then the shaper as it is
  const size_t nodes = (size_t)ld->size * ld->size * ld->size, node_bytes = align_up(8 * nodes, 256);
  const size_t shaper_bytes = ld->has_shaper ? ((size_t)6 << ld->depth) : 0;
  std::vector<uint32_t> blob((node_bytes + shaper_bytes + 3) / 4, 0);
  for (size_t i = 0; i < nodes; i++) {
    blob[2 * i] = (uint32_t)lattice[3 * i] | (uint32_t)lattice[3 * i + 1] << 16;
    blob[2 * i + 1] = lattice[3 * i + 2];
  }
  if (shaper_bytes) memcpy(reinterpret_cast<char*>(blob.data()) + node_bytes, shaper, shaper_bytes);
  hipSetDevice(c->device);
  HIP_TRY(c, hipMalloc(&cs->dev, node_bytes + shaper_bytes));
  if (hipMemcpy(cs->dev, blob.data(), node_bytes + shaper_bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipEventCreateWithFlags(&cs->done, hipEventDisableTiming) != hipSuccess) {
    c->last_err = (int32_t)hipGetLastError();
    cs->release();
    return HMGPU_EDEVICE;
  }
  cs->lut.nodes = nodes ? reinterpret_cast<const u32x2*>(cs->dev) : nullptr;
  cs->lut.shaper = shaper_bytes ? reinterpret_cast<const uint16_t*>(cs->dev + node_bytes) : nullptr;
  cs->lut.size = ld->size; cs->lut.depth = ld->depth;
  // handles are unique in the process, so that one of another context never names a LUT of this one
  static std::atomic<int64_t> next{1};
  cs->handle = next.fetch_add(1);
  *out = cs->handle;
  return HMGPU_OK;
}

static hmgpu_ctx::ColourSlot* colour_find(hmgpu_ctx* c, hmgpu_lut lut) {
  if (lut <= 0) return nullptr;
  for (auto& sl : c->colour_slot) if (sl.handle == lut) return &sl;
  return nullptr;
}

hmgpu_status hmgpu_colour_lut_destroy(hmgpu_ctx* c, hmgpu_lut lut) {
  if (!c) return HMGPU_EINVAL;
  hmgpu_ctx::ColourSlot* cs = colour_find(c, lut);
  if (!cs) return HMGPU_EINVAL;
  hipSetDevice(c->device);
  if (cs->pending) HIP_TRY(c, hipEventSynchronize(cs->done));        // the last export that reads it
  cs->release();
  return HMGPU_OK;
}

// the rules a colour export adds behind the validation of the matching call: the layout, then the LUT's depth against the call's
static hmgpu_status colour_rules(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, int lut_depth) {
  if (d->layout != HMGPU_EXPORT_RGB) return HMGPU_EINVAL;
  int ob[2];
  out_depths(seq, d, ob);
  return lut_depth == ob[0] ? HMGPU_OK : HMGPU_EINVAL;
}

// ------------------------------------------------------------------------------------------------ chroma stage (chroma_core.h)
// the rules a chroma export adds behind the validation of the matching call, in the order include/hmgpu.h "chroma export" gives
static hmgpu_status chroma_rules(const hmgpu_export_desc* d, const hmgpu_export_chroma* ch) {
  if (d->layout != HMGPU_EXPORT_RGB) return HMGPU_EINVAL;
  if (!ch || ch->loc < 0 || ch->loc > 5) return HMGPU_EINVAL;
  for (int k = 0; k < 6; k++) if (ch->reserved[k]) return HMGPU_EINVAL;
  if (ch->filter != HMGPU_CHROMA_REPLICATE && ch->filter != HMGPU_CHROMA_LINEAR) return HMGPU_EUNSUPPORTED;
  return HMGPU_OK;
}

// the weights of a validated descriptor for a 4:2:0 or 4:2:2 sequence (H.265 figure E.1), in quarters
static void chroma_site(const hmgpu_seq_params& seq, const hmgpu_export_chroma& ch, ChromaSite* s) {
  memset(s, 0, sizeof(*s));
  const bool f420 = seq.chroma_format == 1;
  const bool centred = f420 && (ch.loc & 1);
  const int32_t hx[2][2][3] = {{{0, 4, 0}, {0, 2, 2}}, {{1, 3, 0}, {0, 3, 1}}};                  // co-sited, centred
  const int32_t vy[4][2][2] = {{{-1, 1}, {0, 3}}, {{0, 4}, {0, 2}}, {{-1, 2}, {0, 4}}, {{0, 4}, {0, 4}}};   // centred, co-sited, bottom, none
  memcpy(s->hx, hx[centred ? 1 : 0], sizeof(s->hx));
  memcpy(s->vy, vy[f420 ? ch.loc >> 1 : 3], sizeof(s->vy));
  s->wc = seq.width >> 1;
  s->hc = seq.height >> (f420 ? 1 : 0);
}

// ------------------------------------------------------------------------------------------------ format export (k_export_fmt.hip)
// the class and the weights of a validated conversion from the sequence's format to another one with chroma (include/hmgpu.h "format
// export"); ob1: the chroma output depth.  REPLICATE and DROP are a single weight 4 on the axis, which the rounding returns exactly.
static void fmt_conv(const hmgpu_seq_params& seq, const hmgpu_export_format& f, int ob1, FmtConv* v) {
  memset(v, 0, sizeof(*v));
  const int fs = seq.chroma_format, fo = f.chroma_format;
  int ssx, ssy, osx, osy;
  chroma_shifts(fs, &ssx, &ssy);
  chroma_shifts(fo, &osx, &osy);
  if (fs == 0) { v->cls = kFmtConst; v->constant = 1 << (ob1 - 1); return; }
  const int gx = ssx - osx, gy = ssy - osy;                      // per axis: 1 gains samples, -1 loses them
  if (gx > 0 || gy > 0) {
    hmgpu_export_chroma ch;
    memset(&ch, 0, sizeof(ch));
    ch.filter = HMGPU_CHROMA_LINEAR; ch.loc = f.loc;
    chroma_site(seq, ch, &v->cs);                                // the siting of the source, the 4:2:0 (or 4:2:2) side
    if (f.up == HMGPU_CHROMA_REPLICATE) {
      const int32_t hx[2][3] = {{0, 4, 0}, {0, 4, 0}}, vy[2][2] = {{0, 4}, {0, 4}};
      memcpy(v->cs.hx, hx, sizeof(hx));
      memcpy(v->cs.vy, vy, sizeof(vy));
    }
    v->vgain = gy > 0;
    v->cls = gx > 0 ? kFmtUp : kFmtVert;
  } else {
    const bool lin = f.down == HMGPU_DOWN_LINEAR;
    const int32_t dh[3][3] = {{0, 4, 0}, {1, 2, 1}, {0, 2, 2}};                   // drop, co-sited, centred
    const int32_t dv[4][4] = {{0, 4, 0, 0}, {0, 2, 2, 0}, {-1, 1, 2, 1}, {0, 1, 2, 1}};   // drop, centred, co-sited, bottom: first row, weights
    memcpy(v->dh, dh[!lin ? 0 : fo == 1 && (f.loc & 1) ? 2 : 1], sizeof(v->dh));
    const int32_t* w = dv[lin ? 1 + (f.loc >> 1) : 0];
    v->dv0 = w[0];
    memcpy(v->dv, w + 1, sizeof(v->dv));
    v->vloss = gy < 0;
    v->cls = gx < 0 ? kFmtDown : kFmtVert;
  }
  v->cs.wc = seq.width >> ssx;
  v->cs.hc = seq.height >> ssy;
}

// ------------------------------------------------------------------------------------------------ affine warp export (k_export_warp.hip)
// whether `wp` names an output size (the plan and the destination check need one before the warp rules have their turn)
static bool warp_sized(const hmgpu_export_warp* wp) {
  return wp && wp->width >= 1 && wp->width <= 16384 && wp->height >= 1 && wp->height <= 16384;
}

// the rules a warp export adds behind the validation of the matching call, in the order include/hmgpu.h "affine warp export" gives
static hmgpu_status warp_rules(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, int n, const hmgpu_export_warp* wp, const hmgpu_warp_map* maps) {
  if (!wp || !maps) return HMGPU_EINVAL;
  for (int k = 0; k < 5; k++) if (wp->reserved[k]) return HMGPU_EINVAL;
  for (int i = 0; i < n; i++) if (maps[i].reserved[0] || maps[i].reserved[1]) return HMGPU_EINVAL;
  if (!warp_sized(wp)) return HMGPU_EINVAL;
  if (d->layout != HMGPU_EXPORT_RGB) return HMGPU_EINVAL;
  if (wp->border == HMGPU_WARP_FILL) {
    int ob[2];
    out_depths(seq, d, ob);
    for (int k = 0; k < 3; k++) if (wp->fill[k] < 0 || wp->fill[k] > (1 << ob[0]) - 1) return HMGPU_EINVAL;
  }
  if (wp->filter != HMGPU_WARP_NEAREST && wp->filter != HMGPU_WARP_BILINEAR) return HMGPU_EUNSUPPORTED;
  if (wp->border != HMGPU_WARP_EDGE && wp->border != HMGPU_WARP_FILL) return HMGPU_EUNSUPPORTED;
  return HMGPU_OK;
}

// ------------------------------------------------------------------------------------------------ the request record: one plan, one resolver
namespace {
// The stages of one picture export, as every layer under the public entries takes them; a stage the call does not have is null
// (lut: 0).  The flags are everything the entries differ in: an entry fills the record and has no code of its own behind that.
struct ExportReq {
  ExportReq(const hmgpu_export_desc* d, const hmgpu_export_scale* sc, const hmgpu_export_tensor* t, const hmgpu_export_window* win = nullptr,
            const hmgpu_export_pixel* px = nullptr) : d(d), sc(sc), t(t), win(win), px(px) {}
  const hmgpu_export_desc* d;
  const hmgpu_export_scale* sc;
  const hmgpu_export_tensor* t;
  const hmgpu_export_window* win;                    // null: d->crop for every picture, no mirror
  const hmgpu_export_pixel* px;                      // packed pixels: dst[0] the one destination
  hmgpu_lut lut = 0;                                 // the LUT of a call or check ...
  const hmgpu_colour_lut_desc* ld = nullptr;         // ... and of a plan, which has no context to look a handle up in
  const hmgpu_export_chroma* chroma = nullptr;
  const hmgpu_export_warp* wp = nullptr;
  const hmgpu_warp_map* maps = nullptr;
  const hmgpu_export_format* fmt = nullptr;
  const hmgpu_export_yuvpack* pack = nullptr;        // packed YUV: validated by yuvpack_rules, d the planar call that defines its values
  bool format_stage = false;                         // the format entries: the format rules apply and the plan is the output format's
  bool need_sc = false, need_win = false, need_px = false;   // the entry is refused without that stage
  bool colour_stage = false;                         // the colour rules apply: the colour entries always, the wider ones with a LUT
  bool chroma_stage = false;                         // the chroma rules apply: the chroma entries always, the warp ones with a descriptor
  bool warp = false;                                 // the warp entries: n checked without windows too, windows of any size, every plane
                                                     // wp's size, the destination checked once wp names one, the warp rules
  bool single = false;                               // hmgpu_picture_export(_scaled): no batch stride
};

// what every picture export resolves its arguments to before anything is enqueued, and what the destination checks stop at: the
// plan, the element, the shapes of a scaled call, the pixel order, the destination checked against the plan, the LUT's slot
struct ExportCall {
  hmgpu_export_plan plan;
  hmgpu_export_desc d;                               // the descriptor; windows that are all equal: with that window as its crop
  int elem = 0, nch = 0;                             // nch: elements per packed pixel (0: planes)
  bool differ = false;                               // the windows are not all equal
  uint32_t flip = 0;
  ScaleShape s;                                      // scaled: the output size and the depths (those of every window)
  std::vector<ScaleShape> shapes;                    // windows that differ, scaled: one per picture
  PxOrder po;
  bool vec = true;
  int64_t bs[3] = {0, 0, 0};
  hmgpu_ctx::ColourSlot* cs = nullptr;               // the colour stage (null: none)
  int fmt_out = -1;                                  // a format export: the output chroma format (-1: the picture's own)
};

// the stages behind the pixels of the entries in which each of them is optional (the plans: ld, the calls and checks: lut)
void optional_stages(ExportReq* q, hmgpu_lut lut, const hmgpu_colour_lut_desc* ld, const hmgpu_export_chroma* ch, bool chroma_entry) {
  q->lut = lut; q->ld = ld; q->chroma = ch;
  q->colour_stage = lut || ld;
  q->chroma_stage = chroma_entry || ch;
}
}  // namespace

// Rules 1 and 2 of the order include/hmgpu.h documents: the base plan -- per window in order (windows_plan), else of the one crop
// (tensor_plan) -- then pixel_plan.  shapes: the export itself asks for the scale shapes (a plan or a check needs none).
static hmgpu_status base_plan(const hmgpu_seq_params* seq, int n, const ExportReq& q, hmgpu_export_plan* out, ExportCall* r, bool shapes) {
  if (q.win || q.need_win) {
    const hmgpu_status st = windows_plan(seq, q.d, q.sc, q.t, n, q.win, out, shapes ? &r->shapes : nullptr, &r->elem, &r->differ, q.warp,
                                         r->fmt_out);
    if (st != HMGPU_OK) return st;
    for (int i = 0; i < n; i++) r->flip |= (uint32_t)(q.win[i].flip & 1) << i;
    if (q.sc && shapes) r->s = r->shapes[0];
  } else {
    memset(out, 0, sizeof(*out));
    if (q.warp && (n < 1 || n > HMGPU_EXPORT_MAX_BATCH)) return HMGPU_EINVAL;
    const hmgpu_status st = tensor_plan(seq, q.d, q.sc, q.t, out, shapes ? &r->s : nullptr, &r->elem, nullptr, r->fmt_out);
    if (st != HMGPU_OK) return st;
  }
  return HMGPU_OK;
}

// The rules a format export adds behind the plan of the matching call (`out`, already made), in the order include/hmgpu.h "format
// export" gives; then the plan again, of the output format.  They stand in front of the destination check, which needs that plan.
static hmgpu_status format_rules(const hmgpu_seq_params* seq, int n, const ExportReq& q, hmgpu_export_plan* out, ExportCall* r, bool shapes) {
  const hmgpu_export_desc* d = q.d;
  const hmgpu_export_format* f = q.fmt;
  if (d->layout == HMGPU_EXPORT_RGB) return HMGPU_EINVAL;
  if (!f || f->chroma_format < 0 || f->chroma_format > 3 || f->loc < 0 || f->loc > 5) return HMGPU_EINVAL;
  for (int k = 0; k < 4; k++) if (f->reserved[k]) return HMGPU_EINVAL;
  if (seq->chroma_format == 0 && f->chroma_format != 0) {         // the chroma output depth, which the matching call did not look at
    int ob[2];
    out_depths(seq, d, ob);
    if (ob[1] < 1 || ob[1] > 16 || (d->bytes_per_sample == 1 && ob[1] > 8)) return HMGPU_EINVAL;
    if (r->elem >= kElemF16 && d->bytes_per_sample != (std::max(ob[0], ob[1]) <= 8 ? 1 : 2)) return HMGPU_EINVAL;
  }
  if (f->up != HMGPU_CHROMA_REPLICATE && f->up != HMGPU_CHROMA_LINEAR) return HMGPU_EUNSUPPORTED;
  if (f->down != HMGPU_DOWN_DROP && f->down != HMGPU_DOWN_LINEAR) return HMGPU_EUNSUPPORTED;
  int osx, osy;
  chroma_shifts(f->chroma_format, &osx, &osy);
  if (f->chroma_format != 0) {
    const int mx = (1 << osx) - 1, my = (1 << osy) - 1;
    for (int i = 0; i < (q.win ? n : 1); i++) {
      const int32_t* cr = q.win ? q.win[i].crop : d->crop;
      const int W = seq->width - cr[0] - cr[1], H = seq->height - cr[2] - cr[3];
      if (((cr[0] | W) & mx) || ((cr[2] | H) & my)) return HMGPU_EINVAL;
    }
    if (q.sc && ((q.sc->width & mx) || (q.sc->height & my))) return HMGPU_EINVAL;
  }
  r->fmt_out = f->chroma_format;
  return base_plan(seq, n, q, out, r, shapes);
}

// Rules 1 to 5 of a packed YUV export, in the order include/hmgpu.h "packed YUV" gives, in front of the rules of the format export
// that defines its values; *dd: the descriptor of that export (the planar layout at depth D in the container D needs)
static hmgpu_status yuvpack_rules(const hmgpu_export_desc* d, const hmgpu_export_scale* sc, const hmgpu_export_tensor* t,
                                  const hmgpu_export_format* f, const hmgpu_export_yuvpack* pack, hmgpu_export_desc* dd) {
  if (!pack) return HMGPU_EINVAL;
  for (int k = 0; k < 6; k++) if (pack->reserved[k]) return HMGPU_EINVAL;
  YuvPackFormat pf;
  if (!yuvpack_format(pack->format, &pf)) return HMGPU_EUNSUPPORTED;
  const int B = pf.depth <= 8 ? 1 : 2;
  if (!d || d->layout != HMGPU_EXPORT_PLANAR) return HMGPU_EINVAL;
  for (int k = 0; k < 2; k++) if (d->bit_depth[k] != 0 && d->bit_depth[k] != pf.depth) return HMGPU_EINVAL;
  if ((d->bytes_per_sample != 0 && d->bytes_per_sample != B) || d->msb_aligned != 0) return HMGPU_EINVAL;
  if (!f || f->chroma_format != pf.cf) return HMGPU_EINVAL;
  if (pack->alpha < 0 || pack->alpha > pf.amax) return HMGPU_EINVAL;
  if (sc) return HMGPU_EUNSUPPORTED;
  if (t && t->sample_type >= HMGPU_SAMPLE_F16 && t->sample_type <= HMGPU_SAMPLE_F32) return HMGPU_EUNSUPPORTED;
  *dd = *d;
  dd->bit_depth[0] = dd->bit_depth[1] = pf.depth;
  dd->bytes_per_sample = B;
  return HMGPU_OK;
}

static hmgpu_status export_plan(const hmgpu_seq_params* seq, int n, const ExportReq& q, hmgpu_export_plan* out, ExportCall* r, bool shapes) {
  if (!seq || !q.d || !out || (q.need_sc && !q.sc) || (q.need_px && !q.px)) return HMGPU_EINVAL;
  { const hmgpu_status st = base_plan(seq, n, q, out, r, shapes); if (st != HMGPU_OK) return st; }
  if (q.format_stage) {
    const hmgpu_status st = format_rules(seq, n, q, out, r, shapes);
    if (st != HMGPU_OK) { memset(out, 0, sizeof(*out)); return st; }
  }
  if (q.pack) {                                        // the planes of the format export become the one plane of words
    YuvPackFormat pf;
    yuvpack_format(q.pack->format, &pf);                // (accepted by yuvpack_rules in every entry: cannot fail)
    const int W = out->width[0], H = out->height[0];
    memset(out, 0, sizeof(*out));
    out->planes = 1;
    out->width[0] = W; out->height[0] = H; out->row_bytes[0] = yuvpack_row_bytes(pf, W);
  }
  if (q.warp && warp_sized(q.wp) && q.d->layout == HMGPU_EXPORT_RGB)
    for (int k = 0; k < out->planes; k++) {
      out->row_bytes[k] = out->row_bytes[k] / out->width[k] * q.wp->width;
      out->width[k] = q.wp->width; out->height[k] = q.wp->height;
    }
  if (!q.px) return HMGPU_OK;
  r->nch = q.px->order <= HMGPU_PIXEL_BGR ? 3 : 4;
  return pixel_plan(seq, q.d, r->elem, q.px, out, &r->po);
}

// Rules 4 to 6, behind the plan and (a call or check) the destination: colour -- the RGB layout, the LUT found, its depth --, then
// chroma, then warp.  c null: a plan function, which knows the LUT by its description.
static hmgpu_status stage_rules(hmgpu_ctx* c, const hmgpu_seq_params* seq, int n, const ExportReq& q, hmgpu_ctx::ColourSlot** cs) {
  if (q.colour_stage) {
    if (q.d->layout != HMGPU_EXPORT_RGB) return HMGPU_EINVAL;
    if (c) *cs = colour_find(c, q.lut);
    if (c ? !*cs : !colour_desc_ok(q.ld)) return HMGPU_EINVAL;
    const hmgpu_status st = colour_rules(seq, q.d, c ? (*cs)->lut.depth : q.ld->depth);
    if (st != HMGPU_OK) return st;
  }
  if (q.chroma_stage) { const hmgpu_status st = chroma_rules(q.d, q.chroma); if (st != HMGPU_OK) return st; }
  return q.warp ? warp_rules(seq, q.d, n, q.wp, q.maps) : HMGPU_OK;
}

// every plan function: export_plan, then the stage rules; a refused plan is all zero
static hmgpu_status plan_for(const hmgpu_seq_params* seq, int n, const ExportReq& q, hmgpu_export_plan* out) {
  ExportCall r;
  hmgpu_status st = export_plan(seq, n, q, out, &r, false);
  if (st == HMGPU_OK && (st = stage_rules(nullptr, seq, n, q, nullptr)) != HMGPU_OK) memset(out, 0, sizeof(*out));
  return st;
}

// every export and destination check: the plan, the destination against it (rule 3), the stage rules.  bstride null: one picture,
// no batch stride to check
static hmgpu_status export_resolve(hmgpu_ctx* c, int n, const ExportReq& q, void* const dst[3], const int64_t pitch_bytes[3],
                                   const int64_t* bstride, bool shapes, ExportCall* r) {
  { const hmgpu_status st = export_plan(&c->seq, n, q, &r->plan, r, shapes); if (st != HMGPU_OK) return st; }
  r->d = *q.d;
  if (q.win && !r->differ) memcpy(r->d.crop, q.win[0].crop, sizeof(r->d.crop));
  if (q.pack) {                                       // words: the unused planes, and the alignment of the format's element
    YuvPackFormat pf;
    yuvpack_format(q.pack->format, &pf);                // (accepted by yuvpack_rules in every entry: cannot fail)
    if (dst[1] || dst[2]) return HMGPU_EINVAL;
    if ((uintptr_t)dst[0] % pf.align || pitch_bytes[0] % pf.align || (bstride && bstride[0] % pf.align)) return HMGPU_EINVAL;
  }
  if (!q.warp || warp_sized(q.wp)) {                  // (a warp without a size: refused below, by the warp rules at the latest)
    const hmgpu_status st = export_dst_ok(c, r->plan, elem_size(r->elem), n, dst, pitch_bytes, bstride, &r->vec, r->bs);
    if (st != HMGPU_OK) return st;
  }
  // packed pixels: a full group is a run of dwords where the destination is dword aligned; the loads have their own condition
  if (q.px) r->po.vst = (uintptr_t)dst[0] % 4 == 0 && pitch_bytes[0] % 4 == 0 && (n == 1 || r->bs[0] % 4 == 0);
  return stage_rules(c, &c->seq, n, q, &r->cs);
}

static hmgpu_status destination_check(hmgpu_ctx* c, int n, const ExportReq& q, void* const dst[3], const int64_t pitch_bytes[3],
                                      const int64_t batch_stride_bytes[3]) {
  // (need_win: export_resolve would take null windows for a call without windows and check the wrong plan)
  if (!c || n < 1 || n > HMGPU_EXPORT_MAX_BATCH || !q.d || (q.need_win && !q.win) || (q.need_px && !q.px) || !dst || !pitch_bytes ||
      !batch_stride_bytes) return HMGPU_EINVAL;
  ExportCall r;
  return export_resolve(c, n, q, dst, pitch_bytes, batch_stride_bytes, false, &r);
}

hmgpu_status hmgpu_export_scaled_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                          hmgpu_export_plan* out) {
  ExportReq q(d, sc, nullptr);
  q.need_sc = true;
  return plan_for(seq, 1, q, out);
}

hmgpu_status hmgpu_export_tensor_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                          const hmgpu_export_tensor* t, hmgpu_export_plan* out) {
  return plan_for(seq, 1, ExportReq(d, sc, t), out);
}

hmgpu_status hmgpu_export_windows_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                           const hmgpu_export_tensor* t, int32_t n, const hmgpu_export_window windows[], hmgpu_export_plan* out) {
  ExportReq q(d, sc, t, windows);
  q.need_win = true;
  return plan_for(seq, n, q, out);
}

hmgpu_status hmgpu_export_pixels_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                          const hmgpu_export_tensor* t, int32_t n, const hmgpu_export_window win[],
                                          const hmgpu_export_pixel* px, hmgpu_export_plan* out) {
  ExportReq q(d, sc, t, win, px);
  q.need_px = true;
  return plan_for(seq, n, q, out);
}

hmgpu_status hmgpu_export_colour_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                          const hmgpu_export_tensor* t, int32_t n, const hmgpu_export_window win[],
                                          const hmgpu_export_pixel* px, const hmgpu_colour_lut_desc* ld, hmgpu_export_plan* out) {
  ExportReq q(d, sc, t, win, px);
  q.ld = ld;
  q.colour_stage = true;
  return plan_for(seq, n, q, out);
}

hmgpu_status hmgpu_export_chroma_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                          const hmgpu_export_tensor* t, int32_t n, const hmgpu_export_window win[],
                                          const hmgpu_export_pixel* px, const hmgpu_colour_lut_desc* ld, const hmgpu_export_chroma* ch,
                                          hmgpu_export_plan* out) {
  ExportReq q(d, sc, t, win, px);
  optional_stages(&q, 0, ld, ch, true);
  return plan_for(seq, n, q, out);
}

hmgpu_status hmgpu_export_warp_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, const hmgpu_export_tensor* t, int32_t n,
                                        const hmgpu_export_window win[], const hmgpu_export_pixel* px, const hmgpu_colour_lut_desc* ld,
                                        const hmgpu_export_chroma* ch, const hmgpu_export_warp* wp, const hmgpu_warp_map maps[],
                                        hmgpu_export_plan* out) {
  ExportReq q(d, nullptr, t, win, px);
  optional_stages(&q, 0, ld, ch, false);
  q.wp = wp; q.maps = maps; q.warp = true;
  return plan_for(seq, n, q, out);
}

hmgpu_status hmgpu_export_format_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                          const hmgpu_export_tensor* t, int32_t n, const hmgpu_export_window win[],
                                          const hmgpu_export_format* fmt, hmgpu_export_plan* out) {
  ExportReq q(d, sc, t, win);
  q.fmt = fmt; q.format_stage = true;
  return plan_for(seq, n, q, out);
}

hmgpu_status hmgpu_export_yuvpack_plan_for(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, const hmgpu_export_tensor* t, int32_t n,
                                           const hmgpu_export_window win[], const hmgpu_export_format* fmt,
                                           const hmgpu_export_yuvpack* pack, hmgpu_export_plan* out) {
  if (!seq || !out) return HMGPU_EINVAL;
  memset(out, 0, sizeof(*out));
  hmgpu_export_desc dd;
  { const hmgpu_status st = yuvpack_rules(d, nullptr, t, fmt, pack, &dd); if (st != HMGPU_OK) return st; }
  ExportReq q(&dd, nullptr, t, win);
  q.fmt = fmt; q.format_stage = true; q.pack = pack;
  return plan_for(seq, n, q, out);
}

hmgpu_status hmgpu_export_yuvpack_destination_check(hmgpu_ctx* c, int32_t n, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                                    const hmgpu_export_tensor* t, const hmgpu_export_window windows[],
                                                    const hmgpu_export_format* fmt, const hmgpu_export_yuvpack* pack, void* const dst[3],
                                                    const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3]) {
  hmgpu_export_desc dd;
  { const hmgpu_status st = yuvpack_rules(d, sc, t, fmt, pack, &dd); if (st != HMGPU_OK) return st; }
  ExportReq q(&dd, nullptr, t, windows);
  q.fmt = fmt; q.format_stage = true; q.pack = pack;
  return destination_check(c, n, q, dst, pitch_bytes, batch_stride_bytes);
}

hmgpu_status hmgpu_export_format_scale_taps(const hmgpu_seq_params* seq, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                            const hmgpu_export_format* fmt, int32_t chroma, int32_t axis, int32_t max_taps,
                                            int32_t* first, int32_t* count, int16_t* weights) {
  if (!first || !count || !weights || !sc || (chroma != 0 && chroma != 1) || (axis != 0 && axis != 1)) return HMGPU_EINVAL;
  ExportReq q(d, sc, nullptr);
  q.fmt = fmt; q.format_stage = true;
  hmgpu_export_plan plan;
  ExportCall r;
  { const hmgpu_status st = export_plan(seq, 1, q, &plan, &r, true); if (st != HMGPU_OK) return st; }
  if (chroma >= r.s.classes) return HMGPU_EINVAL;
  const ScaleTab& t = *r.s.tab[chroma][axis];
  if (max_taps < t.taps) return HMGPU_EINVAL;
  const int n = r.s.out[chroma][axis];
  memcpy(first, t.first.data(), sizeof(int32_t) * (size_t)n);
  memcpy(count, t.count.data(), sizeof(int32_t) * (size_t)n);
  for (int i = 0; i < n; i++) {
    memset(weights + (size_t)i * max_taps, 0, sizeof(int16_t) * (size_t)max_taps);
    memcpy(weights + (size_t)i * max_taps, t.w.data() + (size_t)i * t.taps, sizeof(int16_t) * (size_t)t.taps);
  }
  return HMGPU_OK;
}

hmgpu_status hmgpu_export_format_destination_check(hmgpu_ctx* c, int32_t n, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                                   const hmgpu_export_tensor* t, const hmgpu_export_window windows[],
                                                   const hmgpu_export_format* fmt, void* const dst[3], const int64_t pitch_bytes[3],
                                                   const int64_t batch_stride_bytes[3]) {
  ExportReq q(d, sc, t, windows);
  q.fmt = fmt; q.format_stage = true;
  return destination_check(c, n, q, dst, pitch_bytes, batch_stride_bytes);
}

hmgpu_status hmgpu_export_destination_check(hmgpu_ctx* c, int32_t n, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                            const hmgpu_export_tensor* t, void* const dst[3], const int64_t pitch_bytes[3],
                                            const int64_t batch_stride_bytes[3]) {
  return destination_check(c, n, ExportReq(d, sc, t), dst, pitch_bytes, batch_stride_bytes);
}

hmgpu_status hmgpu_export_windows_destination_check(hmgpu_ctx* c, int32_t n, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                                    const hmgpu_export_tensor* t, const hmgpu_export_window windows[], void* const dst[3],
                                                    const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3]) {
  ExportReq q(d, sc, t, windows);
  q.need_win = true;
  return destination_check(c, n, q, dst, pitch_bytes, batch_stride_bytes);
}

hmgpu_status hmgpu_export_pixels_destination_check(hmgpu_ctx* c, int32_t n, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                                   const hmgpu_export_tensor* t, const hmgpu_export_window windows[],
                                                   const hmgpu_export_pixel* px, void* dst, int64_t pitch_bytes, int64_t batch_stride_bytes) {
  void* const dst3[3] = {dst, nullptr, nullptr};
  const int64_t pitch3[3] = {pitch_bytes, 0, 0}, bstride3[3] = {batch_stride_bytes, 0, 0};
  ExportReq q(d, sc, t, windows, px);
  q.need_px = true;
  return destination_check(c, n, q, dst3, pitch3, bstride3);
}

hmgpu_status hmgpu_export_colour_destination_check(hmgpu_ctx* c, int32_t n, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                                   const hmgpu_export_tensor* t, const hmgpu_export_window windows[],
                                                   const hmgpu_export_pixel* px, hmgpu_lut lut, void* const dst[3],
                                                   const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3]) {
  ExportReq q(d, sc, t, windows, px);
  q.lut = lut;
  q.colour_stage = true;
  return destination_check(c, n, q, dst, pitch_bytes, batch_stride_bytes);
}

hmgpu_status hmgpu_export_chroma_destination_check(hmgpu_ctx* c, int32_t n, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                                   const hmgpu_export_tensor* t, const hmgpu_export_window windows[],
                                                   const hmgpu_export_pixel* px, hmgpu_lut lut, const hmgpu_export_chroma* ch,
                                                   void* const dst[3], const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3]) {
  ExportReq q(d, sc, t, windows, px);
  optional_stages(&q, lut, nullptr, ch, true);
  return destination_check(c, n, q, dst, pitch_bytes, batch_stride_bytes);
}

hmgpu_status hmgpu_export_warp_destination_check(hmgpu_ctx* c, int32_t n, const hmgpu_export_desc* d, const hmgpu_export_tensor* t,
                                                 const hmgpu_export_window windows[], const hmgpu_export_pixel* px, hmgpu_lut lut,
                                                 const hmgpu_export_chroma* ch, const hmgpu_export_warp* wp, const hmgpu_warp_map maps[],
                                                 void* const dst[3], const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3]) {
  ExportReq q(d, nullptr, t, windows, px);
  optional_stages(&q, lut, nullptr, ch, false);
  q.wp = wp; q.maps = maps; q.warp = true;
  return destination_check(c, n, q, dst, pitch_bytes, batch_stride_bytes);
}

}  // extern "C"

// what ExportArgs and ScaleArgs share behind their sources: the depth rule, the destination, the float conversion, the plan's constants
template <class Args>
static void export_args_tail(Args& a, const hmgpu_seq_params& seq, const ExportCall& r, const hmgpu_export_tensor* t, void* const dst[3],
                             const int64_t pitch_bytes[3]) {
  int ob[2];
  out_depths(&seq, &r.d, ob);
  a.flip = r.flip;
  a.sh[0] = ob[0] - seq.bit_depth_luma; a.sh[1] = ob[1] - seq.bit_depth_chroma;
  for (int k = 0; k < 2; k++) { a.maxv[k] = (1 << ob[k]) - 1; a.msb[k] = r.d.msb_aligned ? 16 - ob[k] : 0; }
  for (int k = 0; k < 3; k++) {
    a.dst[k] = k < r.plan.planes ? static_cast<uint8_t*>(dst[k]) : nullptr;
    a.pitch[k] = k < r.plan.planes ? pitch_bytes[k] : 0;
    a.bstride[k] = r.bs[k];
    if (r.elem >= kElemF16) { a.scale[k] = t->scale[k]; a.bias[k] = t->bias[k]; }
  }
  memcpy(a.coef, r.plan.coef, sizeof(a.coef));
}

extern "C" {

// The three argument builders of export_impl -- unscaled, scaled, warp -- each from the resolved call to its launch on hs.  site:
// the chroma stage's weights (null: the instances without it); *tables: the table buffer the launch reads, for export_impl to mark.
static void launch_unscaled(hmgpu_ctx* c, int n, const hmgpu_pic* pics, const ExportReq& q, const ExportCall& r, ChromaSite* site,
                            void* const dst[3], const int64_t pitch_bytes[3], hipStream_t hs) {
  const hmgpu_export_desc* d = &r.d;
  ExportArgs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < n; i++) {
    const Picture& p = c->pics[pics[i]];
    int16_t* const* src = p.sao_applied ? p.dev.sao : p.dev.rec;
    const int x0 = r.differ ? q.win[i].crop[0] : d->crop[0], y0 = r.differ ? q.win[i].crop[2] : d->crop[2];
    a.y[i] = src[0] + (ptrdiff_t)y0 * c->pitch[0] + x0;
    a.c[i] = src[1] + (ptrdiff_t)(y0 >> c->csy) * c->pitch[1] + kCStep * (x0 >> c->csx);
    if ((r.vec || q.px) && (x0 & 3) == 0) a.vec |= 1u << i;               // (a batch may mix aligned and unaligned left edges)
    if (site) { site->x0[i] = (int16_t)(x0 >> c->csx); site->y0[i] = (int16_t)(y0 >> c->csy); }
  }
  a.pitch_y = c->pitch[0]; a.pitch_c = c->pitch[1];
  a.n = n; a.layout = d->layout; a.elem = r.elem; a.mono = c->seq.chroma_format == 0; a.csx = c->csx; a.csy = c->csy;
  a.w = r.plan.width[0]; a.h = r.plan.height[0];
  a.cw = r.plan.width[0] >> c->csx; a.ch = r.plan.height[0] >> c->csy;
  export_args_tail(a, c->seq, r, q.t, dst, pitch_bytes);
  if (q.pack) {
    // packed YUV: the conversion of the format export (none: one row of weight 4 through kFmtVert), then the words
    YuvPackFormat pf;
    yuvpack_format(q.pack->format, &pf);                // (accepted by yuvpack_rules in every entry: cannot fail)
    FmtConv f;
    if (pf.cf == c->seq.chroma_format) {
      memset(&f, 0, sizeof(f));
      f.cls = kFmtVert;
      f.cs.wc = c->seq.width >> c->csx; f.cs.hc = c->seq.height >> c->csy;
    } else {
      fmt_conv(c->seq, *q.fmt, pf.depth, &f);
    }
    for (int i = 0; i < n; i++) {
      const int x0 = r.differ ? q.win[i].crop[0] : d->crop[0], y0 = r.differ ? q.win[i].crop[2] : d->crop[2];
      f.cs.x0[i] = (int16_t)(x0 >> c->csx); f.cs.y0[i] = (int16_t)(y0 >> c->csy);
    }
    YuvPackArgs pk;
    pk.fam = pf.fam; pk.yfirst = pf.yfirst; pk.shift = pf.shift; pk.alpha = (uint32_t)q.pack->alpha;
    launch_export_yuvpack(a, f, pk, hs);
    return;
  }
  if (r.fmt_out >= 0 && r.fmt_out != c->seq.chroma_format) {
    // a format export that converts: Y alone through the 4:0:0 path of k_export, else the chroma rows of the output format
    if (r.fmt_out == 0) { a.mono = 1; launch_export(a, nullptr, 0, nullptr, nullptr, hs); return; }
    FmtConv f;
    fmt_conv(c->seq, *q.fmt, a.sh[1] + c->seq.bit_depth_chroma, &f);
    for (int i = 0; i < n; i++) {
      const int x0 = r.differ ? q.win[i].crop[0] : d->crop[0], y0 = r.differ ? q.win[i].crop[2] : d->crop[2];
      f.cs.x0[i] = (int16_t)(x0 >> c->csx); f.cs.y0[i] = (int16_t)(y0 >> c->csy);
    }
    a.cw = r.plan.width[1]; a.ch = r.plan.height[1];
    launch_export_fmt(a, f, hs);
    return;
  }
  launch_export(a, q.px ? &r.po : nullptr, r.nch, site, r.cs ? &r.cs->lut : nullptr, hs);
}

static hmgpu_status launch_scaled(hmgpu_ctx* c, int n, const hmgpu_pic* pics, const ExportReq& q, const ExportCall& r, const ChromaSite* site,
                                  void* const dst[3], const int64_t pitch_bytes[3], hipStream_t hs, hmgpu_ctx::TableBuf** tables) {
  const hmgpu_export_desc* d = &r.d;
  const bool rgb = d->layout == HMGPU_EXPORT_RGB;
  const ScaleShape& s = r.s;
  // the tables' slot is keyed by the tiles the batch size leads to, not by the batch size: calls of varying n share a slot
  int tile[2][2] = {{0, 0}, {0, 0}};
  int32_t tkey = rgb ? 1 : 0;
  for (int k = 0; k < s.classes; k++) {
    scale_tile_start(s.out[k][0], s.out[k][1], n, &tile[k][0], &tile[k][1]);
    tkey |= (__builtin_ctz((unsigned)tile[k][0]) | __builtin_ctz((unsigned)tile[k][1]) << 3) << (1 + 7 * k);
  }
  tkey |= (r.fmt_out + 1) << 24;                      // (a format export: class 1 has the tables of its output format)
  ScaleArgs a;
  memset(&a, 0, sizeof(a));
  if (r.differ) {
    const hmgpu_status st = window_tables(c, n, r.shapes, q.win, rgb, tile, hs, a.cls, &a.pic_cls, tables);
    if (st != HMGPU_OK) return st;
  } else {
    const int32_t key[8] = {d->crop[0], d->crop[1], d->crop[2], d->crop[3], q.sc->width, q.sc->height, q.sc->filter, tkey};
    int x0c[2] = {d->crop[0], d->crop[0] >> c->csx};
    hmgpu_ctx::ScaleSlot* slot = nullptr;
    { const hmgpu_status st = scale_slot(c, key, s, rgb, x0c, tile, hs, &slot); if (st != HMGPU_OK) return st; }
    for (int k = 0; k < s.classes; k++) {
      a.cls[k] = slot->cls[k];
      a.cls[k].pitch = c->pitch[k];
      a.cls[k].x0 = x0c[k];
      a.cls[k].y0 = k ? d->crop[2] >> c->csy : d->crop[2];
    }
    *tables = slot;
  }
  for (int i = 0; i < n; i++) {
    const Picture& p = c->pics[pics[i]];
    int16_t* const* src = p.sao_applied ? p.dev.sao : p.dev.rec;
    a.src[i][0] = src[0]; a.src[i][1] = src[1];
  }
  a.pitch_c = c->pitch[1];
  a.mono = c->seq.chroma_format == 0; a.csx = c->csx; a.csy = c->csy;
  a.e = r.plan.coef[11];
  a.vec = q.px ? (int)r.po.vst : r.vec ? 1 : 0;
  if (q.px) a.px = r.po;
  export_args_tail(a, c->seq, r, q.t, dst, pitch_bytes);
  launch_export_scaled(a, d->layout, r.elem, n, r.nch, site, r.cs ? &r.cs->lut : nullptr, hs);
  if (r.fmt_out > 0 && c->seq.chroma_format == 0) {
    // a format export of a 4:0:0 picture with chroma planes: nothing to resample, the constant through k_export_fmt's chroma rows
    ExportArgs e;
    memset(&e, 0, sizeof(e));
    e.n = n; e.layout = d->layout; e.elem = r.elem;
    e.cw = r.plan.width[1]; e.ch = r.plan.height[1];
    e.vec = r.vec ? (n >= 32 ? ~0u : (1u << n) - 1) : 0;
    export_args_tail(e, c->seq, r, q.t, dst, pitch_bytes);
    FmtConv f;
    fmt_conv(c->seq, *q.fmt, e.sh[1] + c->seq.bit_depth_chroma, &f);
    launch_export_fmt(e, f, hs);
  }
  return HMGPU_OK;
}

// n pictures of the RGB layout, each through its own map: the maps and windows in one copy through the window ring
static hmgpu_status launch_warp(hmgpu_ctx* c, int n, const hmgpu_pic* pics, const ExportReq& q, const ExportCall& r, const ChromaSite* site,
                                void* const dst[3], const int64_t pitch_bytes[3], hipStream_t hs, hmgpu_ctx::TableBuf** tables) {
  hmgpu_ctx::TableBuf* wb = &c->window_buf[c->window_next];
  c->window_next = (c->window_next + 1) % hmgpu_ctx::kWindowBufs;
  // (the export that read the buffer last may still be in flight)
  const size_t bytes = (size_t)n * sizeof(WarpPic);
  { const hmgpu_status st = table_room(c, wb, bytes, 4096); if (st != HMGPU_OK) return st; }
  WarpArgs a;
  memset(&a, 0, sizeof(a));
  WarpPic* wpic = reinterpret_cast<WarpPic*>(wb->host);
  for (int i = 0; i < n; i++) {
    const Picture& p = c->pics[pics[i]];
    int16_t* const* src = p.sao_applied ? p.dev.sao : p.dev.rec;
    a.src[i][0] = src[0]; a.src[i][1] = src[1];
    const int32_t* cr = q.win ? q.win[i].crop : q.d->crop;
    WarpPic& k = wpic[i];
    memset(&k, 0, sizeof(k));
    memcpy(k.m, q.maps[i].m, sizeof(k.m));
    k.x0 = cr[0]; k.y0 = cr[2];
    k.ws = c->seq.width - cr[0] - cr[1]; k.hs = c->seq.height - cr[2] - cr[3];
  }
  HIP_TRY(c, hipMemcpyAsync(wb->dev, wb->host, bytes, hipMemcpyHostToDevice, hs));
  a.pics = reinterpret_cast<const WarpPic*>(wb->dev);
  a.pitch_y = c->pitch[0]; a.pitch_c = c->pitch[1];
  a.mono = c->seq.chroma_format == 0; a.csx = c->csx; a.csy = c->csy;
  a.w = q.wp->width; a.h = q.wp->height; a.tiles_x = (q.wp->width + kWarpTileW - 1) / kWarpTileW;
  a.filter = q.wp->filter; a.border = q.wp->border;
  for (int k = 0; k < 3; k++) a.fill[k] = q.wp->border == HMGPU_WARP_FILL ? (uint32_t)q.wp->fill[k] : 0;
  a.vec = q.px ? (int)r.po.vst : r.vec ? 1 : 0;
  if (q.px) a.px = r.po;
  export_args_tail(a, c->seq, r, q.t, dst, pitch_bytes);
  launch_export_warp(a, r.elem, n, r.nch, site, r.cs ? &r.cs->lut : nullptr, hs);
  *tables = wb;
  return HMGPU_OK;
}

// every export: n pictures of the request q, the destination as export_resolve takes it.  One launch, the stream ordering once.
static hmgpu_status export_impl(hmgpu_ctx* c, int32_t n, const hmgpu_pic* pics, const ExportReq& q, void* const dst[3],
                                const int64_t pitch_bytes[3], const int64_t* bstride, int32_t on_stream, void* stream) {
  if (!c || !pics || n < 1 || n > HMGPU_EXPORT_MAX_BATCH || !q.d || (q.need_sc && !q.sc) || (q.need_win && !q.win) || (q.need_px && !q.px) ||
      !dst || !pitch_bytes || (!q.single && !bstride) || (on_stream != 0 && on_stream != 1)) return HMGPU_EINVAL;
  for (int i = 0; i < n; i++) if (!valid_pic(c, pics[i])) return HMGPU_EINVAL;
  ExportCall r;
  { const hmgpu_status st = export_resolve(c, n, q, dst, pitch_bytes, bstride, true, &r); if (st != HMGPU_OK) return st; }
  // the chroma stage: 4:4:4 and 4:0:0, where it is the identity, and HMGPU_CHROMA_REPLICATE run the instances without it
  ChromaSite site;
  const bool linear = q.chroma && q.chroma->filter == HMGPU_CHROMA_LINEAR && (c->seq.chroma_format == 1 || c->seq.chroma_format == 2);
  if (linear) chroma_site(c->seq, *q.chroma, &site);
  hipStream_t hs = c->stream;
  { const hmgpu_status st = export_open(c, on_stream, stream, &hs); if (st != HMGPU_OK) return st; }
  hmgpu_ctx::TableBuf* tables = nullptr;
  hmgpu_status st = HMGPU_OK;
  if (q.warp) st = launch_warp(c, n, pics, q, r, linear ? &site : nullptr, dst, pitch_bytes, hs, &tables);
  else if (q.sc) st = launch_scaled(c, n, pics, q, r, linear ? &site : nullptr, dst, pitch_bytes, hs, &tables);
  else launch_unscaled(c, n, pics, q, r, linear ? &site : nullptr, dst, pitch_bytes, hs);
  if (st != HMGPU_OK) return st;
  if (r.cs) { HIP_TRY(c, hipEventRecord(r.cs->done, hs)); r.cs->pending = true; }
  if (tables) { HIP_TRY(c, hipEventRecord(tables->done, hs)); tables->pending = true; }
  return export_end(c, n, pics, on_stream, hs);
}

hmgpu_status hmgpu_picture_export(hmgpu_ctx* c, hmgpu_pic pic, const hmgpu_export_desc* d, void* const dst[3], const int64_t pitch_bytes[3],
                                  int32_t on_stream, void* stream) {
  ExportReq q(d, nullptr, nullptr);
  q.single = true;
  return export_impl(c, 1, &pic, q, dst, pitch_bytes, nullptr, on_stream, stream);
}

hmgpu_status hmgpu_picture_export_scaled(hmgpu_ctx* c, hmgpu_pic pic, const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                         void* const dst[3], const int64_t pitch_bytes[3], int32_t on_stream, void* stream) {
  ExportReq q(d, sc, nullptr);
  q.single = q.need_sc = true;
  return export_impl(c, 1, &pic, q, dst, pitch_bytes, nullptr, on_stream, stream);
}

hmgpu_status hmgpu_pictures_export(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                   const hmgpu_export_tensor* t, void* const dst[3], const int64_t pitch_bytes[3],
                                   const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream) {
  return export_impl(c, n, pics, ExportReq(d, sc, t), dst, pitch_bytes, batch_stride_bytes, on_stream, stream);
}

hmgpu_status hmgpu_pictures_export_windows(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                           const hmgpu_export_tensor* t, const hmgpu_export_window windows[], void* const dst[3],
                                           const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream) {
  ExportReq q(d, sc, t, windows);
  q.need_win = true;
  return export_impl(c, n, pics, q, dst, pitch_bytes, batch_stride_bytes, on_stream, stream);
}

hmgpu_status hmgpu_pictures_export_pixels(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                          const hmgpu_export_tensor* t, const hmgpu_export_window windows[], const hmgpu_export_pixel* px,
                                          void* dst, int64_t pitch_bytes, int64_t batch_stride_bytes, int32_t on_stream, void* stream) {
  void* const dst3[3] = {dst, nullptr, nullptr};
  const int64_t pitch3[3] = {pitch_bytes, 0, 0}, bstride3[3] = {batch_stride_bytes, 0, 0};
  ExportReq q(d, sc, t, windows, px);
  q.need_px = true;
  return export_impl(c, n, pics, q, dst3, pitch3, bstride3, on_stream, stream);
}

hmgpu_status hmgpu_pictures_export_colour(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                          const hmgpu_export_tensor* t, const hmgpu_export_window windows[], const hmgpu_export_pixel* px,
                                          hmgpu_lut lut, void* const dst[3], const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3],
                                          int32_t on_stream, void* stream) {
  ExportReq q(d, sc, t, windows, px);
  q.lut = lut;
  q.colour_stage = true;
  return export_impl(c, n, pics, q, dst, pitch_bytes, batch_stride_bytes, on_stream, stream);
}

hmgpu_status hmgpu_pictures_export_chroma(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                          const hmgpu_export_tensor* t, const hmgpu_export_window windows[], const hmgpu_export_pixel* px,
                                          hmgpu_lut lut, const hmgpu_export_chroma* chroma, void* const dst[3], const int64_t pitch_bytes[3],
                                          const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream) {
  ExportReq q(d, sc, t, windows, px);
  optional_stages(&q, lut, nullptr, chroma, true);
  return export_impl(c, n, pics, q, dst, pitch_bytes, batch_stride_bytes, on_stream, stream);
}

hmgpu_status hmgpu_pictures_export_format(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                          const hmgpu_export_tensor* t, const hmgpu_export_window windows[], const hmgpu_export_format* fmt,
                                          void* const dst[3], const int64_t pitch_bytes[3], const int64_t batch_stride_bytes[3],
                                          int32_t on_stream, void* stream) {
  ExportReq q(d, sc, t, windows);
  q.fmt = fmt; q.format_stage = true;
  return export_impl(c, n, pics, q, dst, pitch_bytes, batch_stride_bytes, on_stream, stream);
}

hmgpu_status hmgpu_pictures_export_yuvpack(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_export_desc* d, const hmgpu_export_scale* sc,
                                           const hmgpu_export_tensor* t, const hmgpu_export_window windows[], const hmgpu_export_format* fmt,
                                           const hmgpu_export_yuvpack* pack, void* const dst[3], const int64_t pitch_bytes[3],
                                           const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream) {
  hmgpu_export_desc dd;
  { const hmgpu_status st = yuvpack_rules(d, sc, t, fmt, pack, &dd); if (st != HMGPU_OK) return st; }
  ExportReq q(&dd, nullptr, t, windows);
  q.fmt = fmt; q.format_stage = true; q.pack = pack;
  return export_impl(c, n, pics, q, dst, pitch_bytes, batch_stride_bytes, on_stream, stream);
}

hmgpu_status hmgpu_pictures_export_warp(hmgpu_ctx* c, int32_t n, const hmgpu_pic pics[], const hmgpu_export_desc* d,
                                        const hmgpu_export_tensor* t, const hmgpu_export_window windows[], const hmgpu_export_pixel* px,
                                        hmgpu_lut lut, const hmgpu_export_chroma* chroma, const hmgpu_export_warp* wp,
                                        const hmgpu_warp_map maps[], void* const dst[3], const int64_t pitch_bytes[3],
                                        const int64_t batch_stride_bytes[3], int32_t on_stream, void* stream) {
  ExportReq q(d, nullptr, t, windows, px);
  optional_stages(&q, lut, nullptr, chroma, false);
  q.wp = wp; q.maps = maps; q.warp = true;
  return export_impl(c, n, pics, q, dst, pitch_bytes, batch_stride_bytes, on_stream, stream);
}

}  // extern "C"
