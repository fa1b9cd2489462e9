// lins_capi_frontend.hip — the stages either side of the update in the C ABI (include/lins_ieskf.h, lins_host.h):
// image_projection (lins_segment_batch), the feature front-end (lins_extract_features_batch) and updatePointCloud's
// re-projection (lins_transform_to_end_batch).  The device-resident streams (lins_capi_streams.hip) run the first two
// through fe_run / sg_run / fe_launch.
#include "lins_ctx.h"

using namespace lins;

namespace lins {
void fe_free(lins_ctx* ctx) { ctx->fe = lins_ctx::Frontend{}; }

// device buffers of the front-end for n scans (inputs, scratch, and the default output buffer d_out)
static int fe_alloc(lins_ctx* ctx, int n) {
  auto& f = ctx->fe;
  if (f.d_scans.cap() >= (size_t)n) return LINS_OK;
  fe_free(ctx);
  const size_t c = (size_t)n, N = LINS_CLOUD_MAX;
  BUF_TRY(ctx, grow_all(f.d_scans, c, f.d_cloud, c * N, f.d_range, c * N, f.d_col, c * N, f.d_ground, c * N, f.d_picks, c * fe_pick_stride(), f.d_out,
                        c * kFeStride, f.d_counts, c * 4));
  return LINS_OK;
}

// Front-end stage shared by lins_extract_features_batch and the streams step: validate, upload the
// segmented scans, launch frontend_kernel with the feature clouds going to out_base + offs[k][0..3]
// (sharp, less sharp, flat, less flat), bring the four counts per scan back (synchronises).
int fe_run(lins_ctx* ctx, int n, const lins_segmented_scan* in, double scan_period, float4* out_base, const long long (*offs)[4],
           std::vector<int>& counts) {
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
  BUF_TRY(ctx, grow_all(f.h_cloud, total, f.h_range, total, f.h_col, total, f.h_ground, total));
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
int fe_launch(lins_ctx* ctx, int n, double scan_period, float4* out_base, std::vector<int>& counts, uint64_t bytes) {
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
int sg_run(lins_ctx* ctx, int n, const lins_point* const* raw, const int32_t* n_raw, const long long (*offs)[4], float4* outl,
           const int* o_slots) {
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
  const size_t c = (size_t)n;
  BUF_TRY(ctx, grow_all(f.d_raws, c, f.d_cellidx, c * N, f.d_segrows, c * N, f.d_outliers, c));
  BUF_TRY(ctx, f.d_raw.grow(total));
  BUF_TRY(ctx, f.h_raw.grow(total));
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

}  // namespace lins

extern "C" {

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
    BUF_TRY(ctx, f.d_outl.grow((size_t)n * LINS_OUTLIER_MAX));
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
  std::vector<long long> offs((size_t)n * 4);
  for (int k = 0; k < n; ++k) {
    long long* o = &offs[(size_t)k * 4];
    o[0] = k * kFeStride, o[1] = o[0] + kFeSharp, o[2] = o[1] + kFeLessSharp, o[3] = o[2] + kFeFlat;
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
  if (any_yzx) BUF_TRY(ctx, ctx->d_aux.grow(ctx->arena_cap));
  ctx->d_jobs.reset();  // (a block of exactly this call's extent)
  BUF_TRY(ctx, ctx->d_jobs.grow((size_t)n_jobs));
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
