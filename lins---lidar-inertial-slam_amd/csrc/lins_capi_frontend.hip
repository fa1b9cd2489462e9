// lins_capi_frontend.hip — the stages either side of the update in the C ABI (include/lins_ieskf.h, lins_host.h):
// image_projection (lins_segment_batch), the feature front-end (lins_extract_features_batch), the device-resident
// streams (lins_streams_*) and updatePointCloud's re-projection (lins_transform_to_end_batch).
#include "lins_ctx.h"

using namespace lins;

namespace {
// slot layout (points): [flat 512 | sharp 256 | less flat LINS_CLOUD_MAX | less sharp 1920]; the less-sharp cloud
// follows the less-flat one so that the multi-resident kernel's sorted copy (positions 0 .. n_all) stays in the slot
constexpr long long kSlotFlat = 0, kSlotSharp = 512, kSlotLessFlat = 768, kSlotLessSharp = 768 + LINS_CLOUD_MAX;
constexpr long long kSlotSize = kSlotLessSharp + 1920;
inline long long slot_base(int stream, int slot) { return ((long long)stream * 2 + slot) * kSlotSize; }
}  // namespace

namespace lins {
void streams_free(lins_ctx* ctx) {
  auto& t = ctx->st;
  (void)hipFree(t.d_arena), (void)hipFree(t.d_sorted), (void)hipFree(t.d_desc), (void)hipFree(t.d_jobs), (void)hipFree(t.d_desc_next);
  t.d_desc_next = nullptr, t.index_ready = false;
  streams_filter_free(ctx);
  streams_boot_free(ctx);
  streams_slam_free(ctx);
  (void)hipFree(t.d_gsorted), (void)hipFree(t.d_gridtab), (void)hipFree(t.d_outl);
  t = lins_ctx::Streams{};
}

int streams_count(lins_ctx* ctx) { return ctx->st.failed ? 0 : ctx->st.n; }

int streams_map_clouds(lins_ctx* ctx, int stream, StreamMapClouds* v) {
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed) return LINS_E_STATE;
  if (stream < 0 || stream >= t.n) return LINS_E_ARG;
  if (t.last_counts[(size_t)stream * 2] < 0) return LINS_E_STATE;
  const int last = t.cur[stream] ^ 1;  // the slot of the scan taken in last
  const long long b = ((long long)stream * 2 + last) * kSlotSize;
  v->src[0] = t.d_arena + b + kSlotLessSharp, v->n[0] = t.last_counts[(size_t)stream * 2];
  v->src[1] = t.d_arena + b + kSlotLessFlat, v->n[1] = t.last_counts[(size_t)stream * 2 + 1];
  v->src[2] = t.d_outl + (size_t)(stream * 2 + last) * LINS_OUTLIER_MAX, v->n[2] = t.outl_counts[(size_t)stream * 2 + last];
  return LINS_OK;
}

void fe_free(lins_ctx* ctx) {
  auto& f = ctx->fe;
  void* ptrs[] = {f.d_scans, f.d_cloud, f.d_out, f.d_range, f.d_col, f.d_ground, f.d_picks, f.d_counts};
  for (void* p : ptrs) (void)hipFree(p);
  void* sg[] = {f.d_raw, f.d_raws, f.d_cellidx, f.d_segrows, f.d_outliers, f.d_outl};
  for (void* p : sg) (void)hipFree(p);
  (void)hipHostFree(f.h_raw);
  (void)hipHostFree(f.h_cloud), (void)hipHostFree(f.h_range), (void)hipHostFree(f.h_col), (void)hipHostFree(f.h_ground);
  f = lins_ctx::Frontend{};
}

}  // namespace lins

extern "C" {

// device buffers of the front-end for n scans (inputs, scratch, and the default output buffer d_out)
static int fe_alloc(lins_ctx* ctx, int n) {
  auto& f = ctx->fe;
  if (f.cap >= n) return LINS_OK;
  fe_free(ctx);
  const size_t c = (size_t)n, N = LINS_CLOUD_MAX;
  HIP_TRY(ctx, hipMalloc(&f.d_scans, c * sizeof(FeScan)));
  HIP_TRY(ctx, hipMalloc((void**)&f.d_cloud, c * N * sizeof(float4)));
  HIP_TRY(ctx, hipMalloc((void**)&f.d_range, c * N * sizeof(float)));
  HIP_TRY(ctx, hipMalloc((void**)&f.d_col, c * N * sizeof(unsigned)));
  HIP_TRY(ctx, hipMalloc((void**)&f.d_ground, c * N));
  HIP_TRY(ctx, hipMalloc((void**)&f.d_picks, c * fe_pick_stride() * sizeof(int)));
  HIP_TRY(ctx, hipMalloc((void**)&f.d_out, c * (192 + 1920 + 384 + N) * sizeof(float4)));
  HIP_TRY(ctx, hipMalloc((void**)&f.d_counts, c * 4 * sizeof(int)));
  f.cap = n;
  return LINS_OK;
}

static int fe_launch(lins_ctx* ctx, int n, double scan_period, float4* out_base, std::vector<int>& counts, uint64_t bytes);

// Front-end stage shared by lins_extract_features_batch and lins_streams_step: validate, upload the
// segmented scans, launch frontend_kernel with the feature clouds going to out_base + offs[k][0..3]
// (sharp, less sharp, flat, less flat), bring the four counts per scan back (synchronises).
static int fe_run(lins_ctx* ctx, int n, const lins_segmented_scan* in, double scan_period, float4* out_base,
                  const long long (*offs)[4], std::vector<int>& counts) {
  const size_t N = LINS_CLOUD_MAX;
  // pass 1 (serial): argument checks, packed layout (each scan's arrays start on a multiple of 4 points)
  std::vector<FeScan> hs(n);
  size_t total = 0;
  uint64_t bytes = 0;
  for (int k = 0; k < n; ++k) {
    const lins_segmented_scan& s = in[k];
    if (s.n < 0 || s.n > (int)N || (s.n && (!s.cloud || !s.range || !s.col || !s.ground))) return LINS_E_ARG;
    for (int r = 0; r < LINS_LINE_NUM; ++r)  // a sector must fit the per-wave sort network (a VLP-16 ring: <= 300)
      if ((s.end_ring[r] - s.start_ring[r]) / 6 + 2 > 510) return LINS_E_UNSUPPORTED;
    hs[k].off = (long long)total, hs[k].n = s.n, hs[k].pad = 0;
    for (int r = 0; r < LINS_LINE_NUM; ++r) hs[k].start_ring[r] = s.start_ring[r], hs[k].end_ring[r] = s.end_ring[r];
    hs[k].start_ori = s.start_ori, hs[k].end_ori = s.end_ori, hs[k].ori_diff = s.ori_diff;
    hs[k].o_sharp = offs[k][0], hs[k].o_less_sharp = offs[k][1], hs[k].o_flat = offs[k][2], hs[k].o_less_flat = offs[k][3];
    total += align4(s.n);
    bytes += (uint64_t)s.n * 25;
  }
  int rc0 = fe_alloc(ctx, n);
  if (rc0) return rc0;
  auto& f = ctx->fe;
  if (f.h_cap < total) {
    (void)hipHostFree(f.h_cloud), (void)hipHostFree(f.h_range), (void)hipHostFree(f.h_col), (void)hipHostFree(f.h_ground);
    f.h_cloud = nullptr, f.h_range = nullptr, f.h_col = nullptr, f.h_ground = nullptr, f.h_cap = 0;
    HIP_TRY(ctx, hipHostMalloc((void**)&f.h_cloud, total * sizeof(float4)));
    HIP_TRY(ctx, hipHostMalloc((void**)&f.h_range, total * sizeof(float)));
    HIP_TRY(ctx, hipHostMalloc((void**)&f.h_col, total * sizeof(unsigned)));
    HIP_TRY(ctx, hipHostMalloc((void**)&f.h_ground, total));
    f.h_cap = total;
  }
  // pass 2 (host pool): input contract + packing into the pinned staging; every complete chunk of scans is sent
  // while the next ones are being packed
  const int rcv = pack_pipelined(
      n, 64,
      [&](int k) -> int {
        const lins_segmented_scan& s = in[k];
        const size_t o = (size_t)hs[k].off;
        for (int i = 0; i < s.n; ++i) {
          const lins_point& p = s.cloud[i];
          if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z) || !std::isfinite(p.intensity) ||
              !std::isfinite(s.range[i]) || s.col[i] >= (uint32_t)LINS_SCAN_NUM)
            return LINS_E_INPUT;
        }
        if (s.n) {
          std::memcpy(f.h_cloud + o, s.cloud, s.n * sizeof(float4));
          std::memcpy(f.h_range + o, s.range, s.n * sizeof(float));
          std::memcpy(f.h_col + o, s.col, s.n * sizeof(unsigned));
          std::memcpy(f.h_ground + o, s.ground, s.n);
        }
        return 0;
      },
      [&](int lo, int hi) -> int {
        const size_t a = (size_t)hs[lo].off, cnt = (hi < n ? (size_t)hs[hi].off : total) - a;
        if (!cnt) return 0;
        HIP_TRY(ctx, hipMemcpyAsync(f.d_cloud + a, f.h_cloud + a, cnt * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(f.d_range + a, f.h_range + a, cnt * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(f.d_col + a, f.h_col + a, cnt * sizeof(unsigned), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(f.d_ground + a, f.h_ground + a, cnt, hipMemcpyHostToDevice, ctx->stream));
        return 0;
      });
  if (rcv) {
    (void)hipStreamSynchronize(ctx->stream);  // (copies of earlier chunks may still read the staging)
    return rcv;
  }
  HIP_TRY(ctx, hipMemcpyAsync(f.d_scans, hs.data(), (size_t)n * sizeof(FeScan), hipMemcpyHostToDevice, ctx->stream));
  return fe_launch(ctx, n, scan_period, out_base, counts, bytes);
}

// the front-end kernel over the n scans described by f.d_scans (filled by the host path above or by the
// segmentation kernel); brings the four counts per scan back (synchronises)
static int fe_launch(lins_ctx* ctx, int n, double scan_period, float4* out_base, std::vector<int>& counts, uint64_t bytes) {
  auto& f = ctx->fe;
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  launch_frontend(ctx->stream, n, f.d_scans, f.d_cloud, f.d_range, f.d_col, f.d_ground, scan_period, f.d_picks, out_base,
                  f.d_counts);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  counts.resize((size_t)n * 4);
  HIP_TRY(ctx, hipMemcpyAsync(counts.data(), f.d_counts, counts.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipEventElapsedTime(&f.ms, ctx->ev0, ctx->ev2));
  for (int k = 0; k < n; ++k) {
    if (counts[(size_t)k * 4 + 3] < 0) return LINS_E_UNSUPPORTED;  // a ring beyond the voxel sort network
    bytes += 16ull * (counts[k * 4] + counts[k * 4 + 1] + counts[k * 4 + 2] + counts[k * 4 + 3]);
  }
  f.bytes = bytes;
  return LINS_OK;
}

// image_projection stage on the device: n raw clouds -> the front-end's device input buffers (f.d_cloud /
// d_range / d_col / d_ground at k * LINS_CLOUD_MAX) and the head of each FeScan (n, ring indices, orientations);
// offs = where the front-end will later put the four feature clouds of each scan; outl / o_slots: null, or the arena the
// outlier clouds go to and the slot of each scan in it (LINS_OUTLIER_MAX points per slot)
static int sg_run(lins_ctx* ctx, int n, const lins_point* const* raw, const int32_t* n_raw, const long long (*offs)[4],
                  float4* outl = nullptr, const int* o_slots = nullptr) {
  const size_t N = LINS_CLOUD_MAX;
  size_t total = 0;
  std::vector<SgRaw> hr(n);
  for (int k = 0; k < n; ++k) {
    if (!raw[k] || n_raw[k] < 2 || n_raw[k] > 65536) return LINS_E_ARG;
    hr[k] = SgRaw{(long long)total, n_raw[k], outl ? o_slots[k] : 0};
    total += align4(n_raw[k]);
  }
  int rc = fe_alloc(ctx, n);
  if (rc) return rc;
  auto& f = ctx->fe;
  if (f.sg_cap < n) {
    void* old[] = {f.d_raws, f.d_cellidx, f.d_segrows, f.d_outliers};
    for (void* p : old) (void)hipFree(p);
    f.d_raws = nullptr, f.d_cellidx = nullptr, f.d_segrows = nullptr, f.d_outliers = nullptr, f.sg_cap = 0;
    const size_t c = (size_t)n;
    HIP_TRY(ctx, hipMalloc(&f.d_raws, c * sizeof(SgRaw)));
    HIP_TRY(ctx, hipMalloc((void**)&f.d_cellidx, c * N * sizeof(unsigned)));
    HIP_TRY(ctx, hipMalloc((void**)&f.d_segrows, c * N * sizeof(int)));
    HIP_TRY(ctx, hipMalloc((void**)&f.d_outliers, c * sizeof(int)));
    f.sg_cap = n;
  }
  if (f.raw_cap < total) {
    (void)hipFree(f.d_raw);
    f.d_raw = nullptr, f.raw_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&f.d_raw, total * sizeof(float4)));
    f.raw_cap = total;
  }
  if (f.h_raw_cap < total) {
    (void)hipHostFree(f.h_raw);
    f.h_raw = nullptr, f.h_raw_cap = 0;
    HIP_TRY(ctx, hipHostMalloc((void**)&f.h_raw, total * sizeof(float4)));
    f.h_raw_cap = total;
  }
  const int rcv = pack_pipelined(
      n, 64,
      [&](int k) -> int {
        // A real driver's cloud carries its no-returns as NaN points.  The reference drops them before anything else
        // (removeNaNFromPointCloud, IP:176) — also from the first / last points findStartEndAngle reads — so they are
        // dropped here, while the cloud is packed: the kernel never sees one (its lins_atan2f answers 0 for NaN
        // arguments: an all-NaN point WOULD project, to row 7 / column 1350).  Infinities stay an input error.
        const lins_point* p = raw[k];
        bool all_finite = true;
        for (int i = 0; i < n_raw[k]; ++i) {
          if (std::isinf(p[i].x) || std::isinf(p[i].y) || std::isinf(p[i].z)) return LINS_E_INPUT;
          all_finite = all_finite && !(std::isnan(p[i].x) || std::isnan(p[i].y) || std::isnan(p[i].z));
        }
        if (all_finite) {
          std::memcpy(f.h_raw + hr[k].off, p, (size_t)n_raw[k] * sizeof(float4));
          return 0;
        }
        float4* dst = f.h_raw + hr[k].off;  // (the slot was sized for n_raw[k] points: the kept ones fit)
        int m = 0;
        for (int i = 0; i < n_raw[k]; ++i)
          if (!(std::isnan(p[i].x) || std::isnan(p[i].y) || std::isnan(p[i].z))) std::memcpy(dst + m++, p + i, sizeof(float4));
        if (m < 2) return LINS_E_INPUT;  // fewer than two finite points: no start / end orientation
        hr[k].n = m;                     // (uploaded after the packing; one writer per scan)
        return 0;
      },
      [&](int lo, int hi) -> int {  // a complete chunk of clouds travels while the next ones are packed
        const size_t a = (size_t)hr[lo].off, cnt = (hi < n ? (size_t)hr[hi].off : total) - a;
        HIP_TRY(ctx, hipMemcpyAsync(f.d_raw + a, f.h_raw + a, cnt * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
        return 0;
      });
  if (rcv) {
    (void)hipStreamSynchronize(ctx->stream);
    return rcv;
  }
  std::vector<FeScan> hs(n);
  for (int k = 0; k < n; ++k) {
    std::memset(&hs[k], 0, sizeof hs[k]);
    hs[k].off = (long long)((size_t)k * N);
    hs[k].o_sharp = offs[k][0], hs[k].o_less_sharp = offs[k][1], hs[k].o_flat = offs[k][2], hs[k].o_less_flat = offs[k][3];
  }
  HIP_TRY(ctx, hipMemcpyAsync(f.d_raws, hr.data(), (size_t)n * sizeof(SgRaw), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(f.d_scans, hs.data(), (size_t)n * sizeof(FeScan), hipMemcpyHostToDevice, ctx->stream));
  // segmentAlphaX / Y and segmentTheta as the host restatement forms them (parameters.h:88-92)
  const float ax = (float)(0.2f / 180.0 * M_PI), ay = (float)(2.0f / 180.0 * M_PI);
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  launch_segment(ctx->stream, n, f.d_raws, f.d_raw, std::sin(ax), std::cos(ax), std::sin(ay), std::cos(ay), 1.0472f,
                 f.d_cellidx, f.d_segrows, f.d_scans, f.d_cloud, f.d_range, f.d_col, f.d_ground, f.d_outliers, outl);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  return LINS_OK;
}

// lins_segment_batch (outlier == nullptr: the kernel runs without the emission) and lins_segment_batch_outliers
static int segment_batch_impl(lins_ctx* ctx, int n, const lins_point* const* raw, const int32_t* n_raw, lins_segmented_scan* out,
                              lins_point* const* outlier) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;
  for (int k = 0; k < n; ++k)
    if (!out[k].cloud || !out[k].range || !out[k].col || !out[k].ground || (outlier && !outlier[k])) return LINS_E_ARG;
  std::vector<long long> offs((size_t)n * 4, 0);
  auto& f = ctx->fe;
  std::vector<int> o_slots((size_t)n);
  if (outlier) {
    if (int rc0 = fe_alloc(ctx, n)) return rc0;  // (first: growing the front-end's buffers drops every buffer of `f`)
    if (f.outl_cap < n) {
      (void)hipFree(f.d_outl);
      f.d_outl = nullptr, f.outl_cap = 0;
      HIP_TRY(ctx, hipMalloc((void**)&f.d_outl, (size_t)n * LINS_OUTLIER_MAX * sizeof(float4)));
      f.outl_cap = n;
    }
    for (int k = 0; k < n; ++k) o_slots[k] = k;
  }
  int rc = sg_run(ctx, n, raw, n_raw, reinterpret_cast<const long long(*)[4]>(offs.data()), outlier ? f.d_outl : nullptr, o_slots.data());
  if (rc) return rc;
  std::vector<FeScan> hs(n);
  std::vector<int> outl(n);
  HIP_TRY(ctx, hipMemcpyAsync(hs.data(), f.d_scans, (size_t)n * sizeof(FeScan), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(outl.data(), f.d_outliers, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipEventElapsedTime(&f.sg_ms, ctx->ev0, ctx->ev2));
  const size_t N = LINS_CLOUD_MAX;
  for (int k = 0; k < n; ++k) {
    lins_segmented_scan& o = out[k];
    o.n = hs[k].n;
    for (int r = 0; r < LINS_LINE_NUM; ++r) o.start_ring[r] = hs[k].start_ring[r], o.end_ring[r] = hs[k].end_ring[r];
    o.start_ori = hs[k].start_ori, o.end_ori = hs[k].end_ori, o.ori_diff = hs[k].ori_diff;
    o.n_outlier = outl[k];
    const size_t b = (size_t)k * N;
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<lins_point*>(o.cloud), f.d_cloud + b, o.n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<float*>(o.range), f.d_range + b, o.n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<uint32_t*>(o.col), f.d_col + b, o.n * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<uint8_t*>(o.ground), f.d_ground + b, o.n, hipMemcpyDeviceToHost, ctx->stream));
    if (outlier && o.n_outlier)
      HIP_TRY(ctx, hipMemcpyAsync(outlier[k], f.d_outl + (size_t)k * LINS_OUTLIER_MAX, (size_t)o.n_outlier * sizeof(float4),
                                  hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LINS_OK;
}

int lins_segment_batch(lins_ctx* ctx, int n, const lins_point* const* raw, const int32_t* n_raw, lins_segmented_scan* out) {
  if (!ctx || n < 0 || (n && (!raw || !n_raw || !out))) return LINS_E_ARG;
  if (n == 0) return LINS_OK;
  return segment_batch_impl(ctx, n, raw, n_raw, out, nullptr);
}

int lins_segment_batch_outliers(lins_ctx* ctx, int n, const lins_point* const* raw, const int32_t* n_raw, lins_segmented_scan* out,
                                lins_point* const* outlier) {
  if (!ctx || n < 0 || (n && (!raw || !n_raw || !out || !outlier))) return LINS_E_ARG;
  if (n == 0) return LINS_OK;
  return segment_batch_impl(ctx, n, raw, n_raw, out, outlier);
}

int lins_last_segment_ms(lins_ctx* ctx, float* kernel_ms) {
  if (!ctx || !kernel_ms) return LINS_E_ARG;
  *kernel_ms = ctx->fe.sg_ms;
  return LINS_OK;
}

int lins_extract_features_batch(lins_ctx* ctx, int n, const lins_segmented_scan* in, double scan_period,
                                lins_features* out) {
  if (!ctx || n < 0 || (n && (!in || !out))) return LINS_E_ARG;
  if (n == 0) return LINS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;
  for (int k = 0; k < n; ++k)
    if (!out[k].corner_sharp || !out[k].corner_less_sharp || !out[k].surf_flat || !out[k].surf_less_flat)
      return LINS_E_ARG;
  const long long per = 192 + 1920 + 384 + LINS_CLOUD_MAX;
  std::vector<long long> offs((size_t)n * 4);
  for (int k = 0; k < n; ++k) {
    long long* o = &offs[(size_t)k * 4];
    o[0] = k * per, o[1] = o[0] + 192, o[2] = o[1] + 1920, o[3] = o[2] + 384;
  }
  std::vector<int> counts;
  int rc = fe_alloc(ctx, n);  // (first, so that the default output buffer exists)
  if (rc) return rc;
  rc = fe_run(ctx, n, in, scan_period, ctx->fe.d_out, reinterpret_cast<const long long(*)[4]>(offs.data()), counts);
  if (rc) return rc;
  auto& f = ctx->fe;
  for (int k = 0; k < n; ++k) {
    const int* c = &counts[(size_t)k * 4];
    const long long* o = &offs[(size_t)k * 4];
    lins_features& ft = out[k];
    ft.n_corner_sharp = c[0], ft.n_corner_less_sharp = c[1], ft.n_surf_flat = c[2], ft.n_surf_less_flat = c[3];
    ft.n_segmented = in[k].n, ft.n_outlier = in[k].n_outlier;
    HIP_TRY(ctx, hipMemcpyAsync(ft.corner_sharp, f.d_out + o[0], c[0] * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ft.corner_less_sharp, f.d_out + o[1], c[1] * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ft.surf_flat, f.d_out + o[2], c[2] * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ft.surf_less_flat, f.d_out + o[3], c[3] * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LINS_OK;
}

// ---- device-resident streams: front-end -> IESKF update -> re-projection without the clouds leaving HBM ----

int lins_streams_init(lins_ctx* ctx, int n_streams) {
  if (!ctx || n_streams < 1) return LINS_E_ARG;
  if (n_streams > ctx->max_batch) return LINS_E_CAPACITY;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;
  streams_free(ctx);
  auto& t = ctx->st;
  const size_t pts = (size_t)n_streams * 2 * kSlotSize;
  if (pts >= (1ull << 31)) return LINS_E_CAPACITY;  // ScanDesc offsets are ints
  HIP_TRY(ctx, hipMalloc((void**)&t.d_arena, pts * sizeof(float4)));
  HIP_TRY(ctx, hipMalloc((void**)&t.d_sorted, pts * sizeof(float4)));
  HIP_TRY(ctx, hipMalloc((void**)&t.d_gsorted, pts * sizeof(float4)));
  HIP_TRY(ctx, hipMalloc((void**)&t.d_gridtab, (size_t)n_streams * sizeof(GridTables)));
  HIP_TRY(ctx, hipMalloc((void**)&t.d_desc, (size_t)n_streams * sizeof(ScanDesc)));
  HIP_TRY(ctx, hipMalloc((void**)&t.d_desc_next, (size_t)n_streams * sizeof(ScanDesc)));
  t.index_ready = false;
  HIP_TRY(ctx, hipMalloc(&t.d_jobs, (size_t)n_streams * 2 * sizeof(StreamCloud)));
  HIP_TRY(ctx, hipMalloc((void**)&t.d_outl, (size_t)n_streams * 2 * LINS_OUTLIER_MAX * sizeof(float4)));
  t.outl_counts.assign((size_t)n_streams * 2, 0), t.outl_put.assign((size_t)n_streams, 0), t.outl_pending = false;
  t.n = n_streams, t.cur.assign((size_t)n_streams, 0);
  t.last_counts.assign((size_t)n_streams * 2, -1);
  return LINS_OK;
}

int lins_streams_step_imu(lins_ctx* ctx, const lins_segmented_scan* scans, const int32_t* n_imu, const double* const* imu,
                          double scan_period, lins_result* out, int32_t* feature_counts, double* global_state_out) {
  if (!scans) return LINS_E_ARG;
  const StepImu si{n_imu, imu, global_state_out};
  return streams_step_impl(ctx, scans, nullptr, nullptr, nullptr, nullptr, scan_period, out, feature_counts, &si);
}

int lins_streams_step_imu_raw(lins_ctx* ctx, const lins_point* const* raw, const int32_t* n_raw, const int32_t* n_imu,
                              const double* const* imu, double scan_period, lins_result* out, int32_t* feature_counts,
                              double* global_state_out) {
  if (!raw || !n_raw) return LINS_E_ARG;
  const StepImu si{n_imu, imu, global_state_out};
  return streams_step_impl(ctx, nullptr, raw, n_raw, nullptr, nullptr, scan_period, out, feature_counts, &si);
}

int lins_streams_step(lins_ctx* ctx, const lins_segmented_scan* scans, const double* prior_state, const double* prior_cov,
                      double scan_period, lins_result* out, int32_t* feature_counts) {
  if (!scans) return LINS_E_ARG;
  return streams_step_impl(ctx, scans, nullptr, nullptr, prior_state, prior_cov, scan_period, out, feature_counts);
}

int lins_streams_step_raw(lins_ctx* ctx, const lins_point* const* raw, const int32_t* n_raw, const double* prior_state,
                          const double* prior_cov, double scan_period, lins_result* out, int32_t* feature_counts) {
  if (!raw || !n_raw) return LINS_E_ARG;
  return streams_step_impl(ctx, nullptr, raw, n_raw, prior_state, prior_cov, scan_period, out, feature_counts);
}

}  // extern "C"

// imu != nullptr: the prior comes from the streams' device filter (lins_streams_step_imu*); mach != nullptr (with imu):
// the state machine's step (lins_streams_process*, lins_capi_boot.hip) — each stream by its status, arguments checked there
int lins::streams_step_impl(lins_ctx* ctx, const lins_segmented_scan* scans, const lins_point* const* raw, const int32_t* n_raw,
                            const double* prior_state, const double* prior_cov, double scan_period, lins_result* out,
                            int32_t* feature_counts, const StepImu* imu, const StepMachine* mach) {
  if (!ctx || !out || (!imu && (!prior_state || !prior_cov))) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed) return LINS_E_STATE;  // (after a failed step: lins_streams_init again)
  if (imu && !mach) {  // every stream runs from its device filter against its resident last scan, or nothing is run
    if (int rc = streams_filter_check(ctx, imu->n_imu, imu->rows)) return rc;
    for (int k = 0; k < t.n; ++k)
      if (t.last_counts[(size_t)k * 2] < 0 || (t.b.on && t.b.status[k] != LINS_STREAM_RUNNING)) return LINS_E_STATE;
  }
  // the status each stream enters the step with (machine mode; otherwise every stream is treated as running)
  const std::vector<int> st_in = mach ? t.b.status : std::vector<int>((size_t)t.n, LINS_STREAM_RUNNING);
  // A step either completes for every stream — slots flipped, resident clouds re-projected — or marks the streams
  // context failed: no half-advanced state survives an early return.
  struct Guard {
    bool& failed;
    bool done = false;
    ~Guard() {
      if (!done) failed = true;
    }
  } guard{t.failed};
  const CallTrace trace;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;
  const int n = t.n;
  const std::vector<int>& cur = t.cur;
  ctx->n_uploaded = 0, ctx->ran = false;  // the batch buffers are reused below
  // 1. feature front-end, straight into this scan's slots
  std::vector<long long> offs((size_t)n * 4);
  for (int k = 0; k < n; ++k) {
    long long* o = &offs[(size_t)k * 4];
    const long long b = slot_base(k, cur[k]);
    o[0] = b + kSlotSharp, o[1] = b + kSlotLessSharp, o[2] = b + kSlotFlat, o[3] = b + kSlotLessFlat;
  }
  std::vector<int> counts;
  // this scan's outlier cloud: slot cur of the stream, as its feature clouds (the count of a segmented step: what
  // lins_streams_put_outliers left, else none)
  std::vector<int> n_outl((size_t)n, 0);
  int rc;
  if (scans) {
    if (t.outl_pending) n_outl = t.outl_put;
    rc = fe_run(ctx, n, scans, scan_period, t.d_arena, reinterpret_cast<const long long(*)[4]>(offs.data()), counts);
  } else {  // raw clouds: the image_projection stage on the device feeds the front-end where its output lies
    std::vector<int> o_slots((size_t)n);
    for (int k = 0; k < n; ++k) o_slots[k] = k * 2 + cur[k];
    rc = sg_run(ctx, n, raw, n_raw, reinterpret_cast<const long long(*)[4]>(offs.data()), t.d_outl, o_slots.data());
    if (rc) {
      guard.done = rc != LINS_E_HIP;  // (a rejected input has advanced nothing: only this scan's own slots were touched)
      return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(n_outl.data(), ctx->fe.d_outliers, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipEventElapsedTime(&ctx->fe.sg_ms, ctx->ev0, ctx->ev2));
    rc = fe_launch(ctx, n, scan_period, t.d_arena, counts, 0);
  }
  if (rc) {
    guard.done = rc != LINS_E_HIP;
    return rc;
  }
  t.frontend_ms = ctx->fe.ms;
  trace.mark("front-end done (synced)");
  // 2. IESKF update of every stream against its resident last scan (a stream's first scan: an update
  //    with no rows, which leaves the given state — the bootstrap pose — untouched)
  //    On the filter path the prior is first propagated over the stream's IMU rows (behind the front-end, so that a
  //    rejected input has advanced nothing), and a scan with too few features is gated (SE:436-440): no update, the
  //    stream's resident clouds and slot stay the old scan's.
  //    The state machine (mach): processImu by status — predict, pre-integrate, drop —; the bootstrap's own gate
  //    (SE:332-333, 380-381: strict bounds); a stream that is not RUNNING gets no update (zero queries), its first or
  //    second scan is dealt with behind the update (boot_mode: 1 / 2).  gated[k]: the scan is not kept.
  std::vector<char> gated((size_t)n, 0), unsupported((size_t)n, 0);
  std::vector<int> boot_mode((size_t)n, 0);
  bool any_gated = false;
  if (imu) {
    if (mach) {
      std::vector<int32_t> n_run((size_t)n);
      for (int k = 0; k < n; ++k) n_run[k] = st_in[k] == LINS_STREAM_RUNNING ? imu->n_imu[k] : 0;
      if (int rcp = streams_filter_predict_queue(ctx, n_run.data(), imu->rows)) return rcp;
      if (int rcp = streams_boot_preintegrate_queue(ctx, imu->n_imu, imu->rows)) return rcp;
    } else if (int rcp = streams_filter_predict_queue(ctx, imu->n_imu, imu->rows))
      return rcp;
    for (int k = 0; k < n; ++k) {
      const int* c = &counts[(size_t)k * 4];
      if (st_in[k] == LINS_STREAM_RUNNING)
        gated[k] = c[1] <= 5 || c[3] <= 10;
      else {
        gated[k] = c[1] < 10 || c[3] < 100;
        if (!gated[k]) boot_mode[k] = st_in[k] == LINS_STREAM_INIT ? 1 : 2;
        if (boot_mode[k] == 2) {  // estimateTransform needs the device ICP: its caps, ICP_FREQ 1 (as the divergence fallback)
          const int n_all = t.last_counts[(size_t)k * 2] + t.last_counts[(size_t)k * 2 + 1];
          if (t.last_counts[(size_t)k * 2] < 0 || n_all > lds_mr_np_cap() || n_all > kGridNpMax || ctx->prm.icp_freq != 1)
            boot_mode[k] = 0, gated[k] = 1, unsupported[k] = 1;
        }
      }
      any_gated = any_gated || gated[k];
    }
  }
  const double* d_prior_state = imu ? t.f.d_state : ctx->d_state_in;
  const double* d_prior_cov = imu ? t.f.d_cov : ctx->d_cov_in;
  bool lds_ok = true, mr_ok = true, lds3_ok = true;
  for (int k = 0; k < n; ++k) {
    const int* c = &counts[(size_t)k * 4];  // sharp, less sharp, flat, less flat
    const bool has_last = t.last_counts[(size_t)k * 2] >= 0 && !gated[k] && st_in[k] == LINS_STREAM_RUNNING;
    ScanDesc& d = ctx->h_desc[k];
    const long long bq = slot_base(k, cur[k]), bt = slot_base(k, cur[k] ^ 1);
    d.off_surf_q = (int)(bq + kSlotFlat), d.n_surf_q = has_last ? c[2] : 0;
    d.off_corner_q = (int)(bq + kSlotSharp), d.n_corner_q = has_last ? c[0] : 0;
    d.off_surf_t = (int)(bt + kSlotLessFlat), d.n_surf_t = has_last ? t.last_counts[(size_t)k * 2 + 1] : 0;
    d.off_corner_t = (int)(bt + kSlotLessSharp), d.n_corner_t = has_last ? t.last_counts[(size_t)k * 2] : 0;
    d.surf_sorted = d.corner_sorted = 1;  // the front-end emits ring-major clouds with ring ids < 16
    d.slot_base = k * LINS_MAX_QUERY, d.pad = 0;
    const int n_all = d.n_surf_t + d.n_corner_t;
    if (n_all > lds_np_cap()) lds_ok = false;
    if (n_all > lds_mr_np_cap()) mr_ok = false;
    if (d.n_surf_q + d.n_corner_q > 336) lds3_ok = false;
  }
  ctx->lds_ok = lds_ok, ctx->mr_ok = mr_ok, ctx->lds3_ok = lds3_ok;
  HIP_TRY(ctx, hipMemcpyAsync(t.d_desc, ctx->h_desc, (size_t)n * sizeof(ScanDesc), hipMemcpyHostToDevice, ctx->stream));
  if (!imu) {
    std::memcpy(ctx->h_state, prior_state, (size_t)n * 19 * 8);
    std::memcpy(ctx->h_cov, prior_cov, (size_t)n * 324 * 8);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_state_in, ctx->h_state, (size_t)n * 19 * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cov_in, ctx->h_cov, (size_t)n * 324 * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  bool idx_ready = false;
  {
    const int search = effective_search(ctx, n);
    const bool want_lds = search >= SEARCH_LDS, want_mr = search == SEARCH_MR;
    const bool use_mr = want_mr && mr_ok, use_lds = want_lds && !want_mr && lds_ok;
    if (use_mr || use_lds) {
      idx_ready = true;
      // the search index of the last scan's clouds: left by the step before, which re-projected and indexed them in one
      // kernel (step 3 below) — built here only when that step could not (its first scan, another search mode)
      if (!t.index_ready) launch_grid_index(ctx->stream, n, t.d_desc, t.d_arena, t.d_gsorted, t.d_gridtab);
      if (use_mr) {
        // several-part updates as in lins_batch_run (the relay + work queue): more streams than workgroup slots
        RelayArgs ra;
        const bool relay = n > ctx->queue_grid && ctx->prm.icp_freq == 1 && ctx->d_relay_hdr && ctx->relay_at != 0 && relay_max_parts(ctx->prm.num_iter, ctx->relay_at, ctx->relay_cuts) > 1;
        // launch order as in the batch calls: longest-expected-first by the prior's translation (launch_order above;
        // h_state holds this step's priors; the filter path's priors are on the device: natural order, same results)
        const bool ordered = ctx->use_order && n > ctx->queue_grid && !imu;
        if (ordered) {
          launch_order(ctx, n);
          HIP_TRY(ctx, hipMemcpyAsync(ctx->d_order, ctx->h_order, (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        }
        if (relay) {
          const int rcq = relay_prepare(ctx, n, ordered, ra);
          if (rcq) return rcq;
        }
        launch_lds_mr(ctx->stream, n, ctx->dprm, t.d_desc, relay ? ctx->d_order + ctx->max_batch : (ordered ? ctx->d_order : nullptr), t.d_arena, t.d_gsorted, t.d_gridtab, d_prior_state,
                      d_prior_cov, ctx->d_state_out, ctx->d_a6, ctx->d_cov_out, ctx->d_out, ctx->d_idx, nullptr, 0, nullptr, relay ? &ra : nullptr,
                      ctx->d_walk_cache, next_run_gen(ctx), ctx->d_relay_lane);
      } else
        launch_lds(ctx->stream, n, ctx->dprm, search == SEARCH_LDS3 ? 3 : 1, t.d_desc, t.d_arena, t.d_gsorted, t.d_gridtab, d_prior_state,
                   d_prior_cov, ctx->d_state_out, ctx->d_a6, ctx->d_cov_out, ctx->d_out, ctx->d_idx, nullptr, 0, nullptr, ctx->d_relay_lane);
    } else {
      DevParams dp = ctx->dprm;
      dp.search = want_lds ? (int)SEARCH_BINNED : search;
      launch_persistent(ctx->stream, n, dp, t.d_desc, t.d_arena, d_prior_state, d_prior_cov, ctx->d_state_out,
                        ctx->d_cov_out, ctx->d_a6, ctx->d_out, ctx->d_idx, nullptr, 0, t.d_sorted, nullptr);
    }
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_state, ctx->d_state_out, (size_t)n * 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_cov, ctx->d_cov_out, (size_t)n * 324 * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_out, (size_t)n * sizeof(OutRec), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (int rc = relay_check(ctx)) return rc;  // (the guard marks the streams context failed: no stale posterior is re-projected)
  HIP_TRY(ctx, hipEventElapsedTime(&t.update_ms, ctx->ev0, ctx->ev1));
  trace.mark("update done (synced)");
  for (int k = 0; k < n; ++k) {
    lins_result& r = out[k];
    std::memset(&r, 0, sizeof r);
    std::memcpy(r.state, ctx->h_state + (size_t)k * 19, sizeof r.state);
    std::memcpy(r.cov, ctx->h_cov + (size_t)k * 324, sizeof r.cov);
    const OutRec& o = ctx->h_out[k];
    const bool has_last = t.last_counts[(size_t)k * 2] >= 0 && !gated[k] && st_in[k] == LINS_STREAM_RUNNING;
    r.residual_norm = o.residual_norm, r.update_norm = o.update_norm;
    r.iters = has_last ? o.iters : 0, r.converged = has_last ? o.converged : 0, r.diverged = has_last ? o.diverged : 0;
    r.m_surf = o.m_surf, r.m_corner = o.m_corner;
    if (!has_last && !imu) {  // a stream's first scan: the given state and covariance, bit for bit (also as re-projection pose)
      std::memcpy(r.state, prior_state + (size_t)k * 19, sizeof r.state);
      std::memcpy(r.cov, prior_cov + (size_t)k * 324, sizeof r.cov);
      HIP_TRY(ctx, hipMemcpyAsync(ctx->d_state_out + (size_t)k * 19, ctx->d_state_in + (size_t)k * 19, 19 * 8,
                                  hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (st_in[k] != LINS_STREAM_RUNNING) {  // the state machine's other streams: filled in behind the bootstrap (2d)
      std::memset(&r, 0, sizeof r);
      r.reserved[0] = unsupported[k] ? LINS_E_UNSUPPORTED : (gated[k] ? LINS_STREAMS_GATED : 0);
      continue;
    }
    if (!has_last && imu) {  // a gated scan: the filter as predicted
      r.reserved[0] = LINS_STREAMS_GATED;
      HIP_TRY(ctx, hipMemcpyAsync(r.state, t.f.d_state + (size_t)k * 19, 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(r.cov, t.f.d_cov + (size_t)k * 324, 324 * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
  }
  if (any_gated) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  // 2b. diverged filters: the ICP fallback (SE:585-592) on the same resident clouds, pose into the state row
  for (int k = 0; k < n; ++k) {
    if (!out[k].diverged) continue;
    if (!mr_ok || ctx->prm.icp_freq != 1) {
      // this stream's clouds cannot take the device fallback: it keeps the un-updated filter (what performIESKF
      // holds before SE:585), flagged per stream — the other streams' step is not thrown away
      out[k].reserved[0] = LINS_E_UNSUPPORTED;
      continue;
    }
    if (!idx_ready) {  // (the update ran on the any-size kernel: no index yet)
      launch_grid_index(ctx->stream, n, t.d_desc, t.d_arena, t.d_gsorted, t.d_gridtab);
      idx_ready = true;
    }
    launch_lds_mr_icp(ctx->stream, 1, ctx->dprm, t.d_desc + k, t.d_arena, t.d_gsorted, t.d_gridtab + k, d_prior_state + (size_t)k * 19,
                      ctx->d_state_out + (size_t)k * 19, ctx->d_out + k, ctx->d_idx);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out[k].state, ctx->d_state_out + (size_t)k * 19, 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (imu) HIP_TRY(ctx, hipMemcpyAsync(out[k].cov, d_prior_cov + (size_t)k * 324, 324 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (!imu) std::memcpy(out[k].cov, prior_cov + (size_t)k * 324, 324 * 8);  // Pk_ un-updated
  }
  // 2c. the filter path: filter_->update, integrateTransformation, reset(1), correctRollPitch on the device
  //     (filter_finish_kernel reads the posterior rows and leaves them: the re-projection below reads linState_ there)
  if (imu) {
    std::vector<int> mode((size_t)n);
    for (int k = 0; k < n; ++k)
      mode[k] = gated[k] || st_in[k] != LINS_STREAM_RUNNING || (out[k].diverged && out[k].reserved[0] == LINS_E_UNSUPPORTED) ? 0 : (out[k].diverged ? 2 : 1);
    if (int rcf = streams_filter_finish_queue(ctx, mode.data())) return rcf;
    // 2d. the state machine's first and second scans: processFirstScan / processSecondScan on the device — the ICP of all
    //     second scans in one launch over their compact descriptor list (queries: this scan's flat / sharp clouds, targets:
    //     the resident first scan's, as extracted), then the finish kernel, which leaves linState_ in the rows the
    //     re-projection reads (identity for a first scan: its clouds stay as extracted)
    if (mach) {
      std::vector<ScanDesc> icp;
      for (int k = 0; k < n; ++k) {
        if (boot_mode[k] != 2) continue;
        const int* c = &counts[(size_t)k * 4];
        const long long bq = slot_base(k, cur[k]), bt = slot_base(k, cur[k] ^ 1);
        ScanDesc d{};
        d.off_surf_q = (int)(bq + kSlotFlat), d.n_surf_q = c[2];
        d.off_corner_q = (int)(bq + kSlotSharp), d.n_corner_q = c[0];
        d.off_surf_t = (int)(bt + kSlotLessFlat), d.n_surf_t = t.last_counts[(size_t)k * 2 + 1];
        d.off_corner_t = (int)(bt + kSlotLessSharp), d.n_corner_t = t.last_counts[(size_t)k * 2];
        d.surf_sorted = d.corner_sorted = 1;
        d.slot_base = k * LINS_MAX_QUERY, d.pad = 0;
        icp.push_back(d);
      }
      if (int rcb = streams_boot_finish(ctx, boot_mode.data(), icp, *mach, out)) return rcb;
    }
    if (imu->global_state_out)
      HIP_TRY(ctx, hipMemcpyAsync(imu->global_state_out, t.f.d_gstate, (size_t)n * 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  // 3. updatePointCloud: this scan's less-sharp / less-flat clouds to the scan end with the final pose
  //    (device-resident state rows), in place — they are the next step's targets
  std::vector<StreamCloud> jobs((size_t)n * 2);
  int max_n = 1;
  for (int k = 0; k < n; ++k) {
    const int* c = &counts[(size_t)k * 4];
    const long long b = slot_base(k, cur[k]);
    if (feature_counts) std::memcpy(feature_counts + (size_t)k * 4, c, 4 * sizeof(int));
    if (gated[k]) {  // nothing of this scan becomes a target
      jobs[(size_t)k * 2] = StreamCloud{b + kSlotLessSharp, 0, k}, jobs[(size_t)k * 2 + 1] = StreamCloud{b + kSlotLessFlat, 0, k};
      continue;
    }
    jobs[(size_t)k * 2] = StreamCloud{b + kSlotLessSharp, c[1], k};
    jobs[(size_t)k * 2 + 1] = StreamCloud{b + kSlotLessFlat, c[3], k};
    max_n = std::max(max_n, std::max(c[1], c[3]));
    t.last_counts[(size_t)k * 2] = c[1], t.last_counts[(size_t)k * 2 + 1] = c[3];
    t.outl_counts[(size_t)k * 2 + cur[k]] = n_outl[k];
  }
  // ... and, when the next step's update will search through the LDS grid, their search index in the same pass
  // (grid_index_kernel<true>: one read of the new clouds for the re-projected arena copy, the grid-sorted copy and the
  // tables; SURVEY f-2 "re-projection + target binning build")
  // (a gated stream keeps its old targets and their index: the step then runs the two kernels, and the next step builds
  // the index of every stream's resident clouds anew — same bits either way, tests/test_gpu_edge_cases.py)
  bool fuse = ctx->streams_fuse && effective_search(ctx, n) >= SEARCH_LDS && !any_gated;
  for (int k = 0; k < n && fuse; ++k) {
    const int* c = &counts[(size_t)k * 4];
    if (c[1] + c[3] > kGridNpMax || c[1] + c[3] > (effective_search(ctx, n) == SEARCH_MR ? lds_mr_np_cap() : lds_np_cap())) fuse = false;
  }
  if (fuse) {
    for (int k = 0; k < n; ++k) {
      const int* c = &counts[(size_t)k * 4];
      ScanDesc& d = ctx->h_desc[k];  // (the update's descriptors have been consumed: its kernel has finished)
      const long long b = slot_base(k, cur[k]);
      d.off_surf_t = (int)(b + kSlotLessFlat), d.n_surf_t = c[3];
      d.off_corner_t = (int)(b + kSlotLessSharp), d.n_corner_t = c[1];
    }
    HIP_TRY(ctx, hipMemcpyAsync(t.d_desc_next, ctx->h_desc, (size_t)n * sizeof(ScanDesc), hipMemcpyHostToDevice, ctx->stream));
  } else {
    HIP_TRY(ctx, hipMemcpyAsync(t.d_jobs, jobs.data(), jobs.size() * sizeof(StreamCloud), hipMemcpyHostToDevice, ctx->stream));
  }
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  if (fuse)
    launch_reproject_and_index(ctx->stream, n, t.d_desc_next, t.d_arena, t.d_gsorted, t.d_gridtab, ctx->d_state_out, (double)(1.f / (float)scan_period));
  else
    launch_reproject_in_place(ctx->stream, 2 * n, max_n, t.d_jobs, ctx->d_state_out, t.d_arena, (double)(1.f / (float)scan_period));
  t.index_ready = fuse;
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipEventElapsedTime(&t.reproject_ms, ctx->ev0, ctx->ev2));
  trace.mark("re-projection done (synced)");
  for (int k = 0; k < n; ++k)
    if (!gated[k]) t.cur[k] ^= 1;
  t.outl_pending = false;
  if (mach) {  // status_ after processPCL (SE:294-307)
    for (int k = 0; k < n; ++k) {
      if (st_in[k] == LINS_STREAM_INIT && boot_mode[k] == 1) t.b.status[k] = LINS_STREAM_FIRST_SCAN;
      if (st_in[k] == LINS_STREAM_FIRST_SCAN && !unsupported[k]) {
        t.b.status[k] = boot_mode[k] == 2 ? LINS_STREAM_RUNNING : LINS_STREAM_INIT;
        if (boot_mode[k] != 2) t.f.set[k] = 0;  // (back to INIT: the stream has no filter until its next first scan)
      }
      if (mach->status_out) mach->status_out[k] = t.b.status[k];
    }
  }
  guard.done = true;
  return LINS_OK;
}

extern "C" {

int lins_streams_put_outliers(lins_ctx* ctx, const lins_point* const* outlier, const int32_t* n_outlier) {
  if (!ctx || !outlier || !n_outlier) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed) return LINS_E_STATE;
  for (int k = 0; k < t.n; ++k) {
    if (n_outlier[k] < 0 || n_outlier[k] > LINS_OUTLIER_MAX || (n_outlier[k] && !outlier[k])) return LINS_E_ARG;
    for (int i = 0; i < n_outlier[k]; ++i) {
      const lins_point& p = outlier[k][i];
      if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z) || !std::isfinite(p.intensity)) return LINS_E_INPUT;
    }
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;
  for (int k = 0; k < t.n; ++k)  // into the slot the next scan's clouds go to
    if (n_outlier[k])
      HIP_TRY(ctx, hipMemcpyAsync(t.d_outl + (size_t)(k * 2 + t.cur[k]) * LINS_OUTLIER_MAX, outlier[k], (size_t)n_outlier[k] * sizeof(float4),
                                  hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the caller's clouds may go once this returns)
  t.outl_put.assign(n_outlier, n_outlier + t.n), t.outl_pending = true;
  return LINS_OK;
}

int lins_streams_map_cloud(lins_ctx* ctx, int stream, int which, lins_point* out, int cap) {
  if (!ctx || which < 0 || which > 2) return LINS_E_ARG;
  StreamMapClouds v;
  if (int rc = streams_map_clouds(ctx, stream, &v)) return rc;
  const int cnt = v.n[which];
  if (cnt > cap) return LINS_E_CAPACITY;
  if (!cnt) return 0;
  if (!out) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemcpy(out, v.src[which], (size_t)cnt * sizeof(float4), hipMemcpyDeviceToHost));
  for (int i = 0; i < cnt; ++i) {  // the mapping node's axes (SE:1128-1131): (x, y, z) <- (y, z, x)
    const lins_point p = out[i];
    out[i] = lins_point{p.y, p.z, p.x, p.intensity};
  }
  return cnt;
}

int lins_streams_stats(lins_ctx* ctx, float* frontend_ms, float* update_ms, float* reproject_ms) {
  if (!ctx) return LINS_E_ARG;
  if (frontend_ms) *frontend_ms = ctx->st.frontend_ms;
  if (update_ms) *update_ms = ctx->st.update_ms;
  if (reproject_ms) *reproject_ms = ctx->st.reproject_ms;
  return LINS_OK;
}

/* test aid: one resident cloud of a stream back to the host (which: 0 less sharp, 1 less flat of the LAST scan) */
int lins_streams_peek(lins_ctx* ctx, int stream, int which, lins_point* out, int cap) {
  if (!ctx || !out || stream < 0 || stream >= ctx->st.n || which < 0 || which > 1) return LINS_E_ARG;
  auto& t = ctx->st;
  const int cnt = t.last_counts[(size_t)stream * 2 + which];
  if (cnt < 0) return LINS_E_STATE;
  if (cnt > cap) return LINS_E_CAPACITY;
  const long long b = slot_base(stream, t.cur[stream] ^ 1) + (which ? kSlotLessFlat : kSlotLessSharp);
  HIP_TRY(ctx, hipMemcpy(out, t.d_arena + b, (size_t)cnt * sizeof(float4), hipMemcpyDeviceToHost));
  return cnt;
}

int lins_last_frontend_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* bytes) {
  if (!ctx) return LINS_E_ARG;
  if (kernel_ms) *kernel_ms = ctx->fe.ms;
  if (bytes) *bytes = ctx->fe.bytes;
  return LINS_OK;
}

int lins_transform_to_end_batch(lins_ctx* ctx, int n_jobs, const lins_reproject_job* jobs) {
  if (!ctx || n_jobs < 0 || (n_jobs && !jobs)) return LINS_E_ARG;
  if (n_jobs == 0) return LINS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;
  std::vector<ReprojectJob> hj(n_jobs);
  size_t off = 0;
  int max_n = 0;
  bool any_yzx = false;
  for (int k = 0; k < n_jobs; ++k) {
    const lins_reproject_job& j = jobs[k];
    if (j.n < 0 || (j.n && (!j.in || !j.out_xyz))) return LINS_E_ARG;
    if (off + align4(j.n) > ctx->arena_cap) return LINS_E_CAPACITY;
    for (int i = 0; i < j.n; ++i)
      if (!std::isfinite(j.in[i].x) || !std::isfinite(j.in[i].y) || !std::isfinite(j.in[i].z) ||
          !std::isfinite(j.in[i].intensity))
        return LINS_E_INPUT;
    if (j.n) std::memcpy(ctx->h_arena + off, j.in, sizeof(lins_point) * j.n);
    hj[k].off = (long long)off, hj[k].n = j.n, hj[k].has_yzx = j.out_yzx != nullptr;
    std::memcpy(hj[k].t, j.t, sizeof j.t);
    std::memcpy(hj[k].q, j.q, sizeof j.q);
    hj[k].inv_period = (double)(1.f / ctx->prm.scan_period);
    any_yzx = any_yzx || j.out_yzx;
    max_n = j.n > max_n ? j.n : max_n;
    off += align4(j.n);
  }
  if (any_yzx && !ctx->d_aux) HIP_TRY(ctx, hipMalloc((void**)&ctx->d_aux, ctx->arena_cap * sizeof(float4)));
  (void)hipFree(ctx->d_jobs);
  ctx->d_jobs = nullptr;
  HIP_TRY(ctx, hipMalloc(&ctx->d_jobs, (size_t)n_jobs * sizeof(ReprojectJob)));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_jobs, hj.data(), (size_t)n_jobs * sizeof(ReprojectJob), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_arena, ctx->h_arena, off * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  launch_transform_to_end(ctx->stream, n_jobs, max_n, ctx->d_jobs, ctx->d_arena, ctx->d_binned, ctx->d_aux);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  ctx->n_uploaded = 0;  // the arenas no longer hold an IESKF batch
  ctx->ran = false;
  uint64_t bytes = 0;
  for (int k = 0; k < n_jobs; ++k) bytes += (uint64_t)jobs[k].n * (jobs[k].out_yzx ? 48 : 32);
  for (int pass = 0; pass < (any_yzx ? 2 : 1); ++pass) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_arena, pass == 0 ? ctx->d_binned : ctx->d_aux, off * sizeof(float4),
                                hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n_jobs; ++k) {
      lins_point* dst = pass == 0 ? jobs[k].out_xyz : jobs[k].out_yzx;
      if (dst && jobs[k].n) std::memcpy(dst, ctx->h_arena + hj[k].off, sizeof(lins_point) * jobs[k].n);
    }
  }
  HIP_TRY(ctx, hipEventElapsedTime(&ctx->reproject_ms, ctx->ev0, ctx->ev2));
  ctx->reproject_bytes = bytes;
  return LINS_OK;
}

int lins_last_reproject_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* bytes) {
  if (!ctx) return LINS_E_ARG;
  if (kernel_ms) *kernel_ms = ctx->reproject_ms;
  if (bytes) *bytes = ctx->reproject_bytes;
  return LINS_OK;
}

}  // extern "C"
