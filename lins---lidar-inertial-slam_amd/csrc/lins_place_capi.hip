// lins_place_capi.hip — C ABI of place recognition (include/lins_place.h): host orchestration around place_kernels.hip.
// The descriptor store is the archive's (place.h PlaceStore, kept in lins_archive_capi.hip beside the key-pose mirror);
// a call packs ONE table — the stale frames of every slot it names | its entries | their (entry, first candidate) chunks —
// uploads it, queues the build launch and the two search launches, downloads the entries' best keys (and, for the test
// aid, one key per candidate) and synchronises once.  The marks "described below id" move only after that
// synchronisation: a call that failed on the way leaves them, and the frames are described again.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/lins_place.h"
#include "host/place_math.h"
#include "lins_ctx_priv.h"
#include "lins_launch.h"
#include "place.h"

using namespace lins;
using namespace lins_place;

namespace {

size_t align64(size_t x) { return (x + 63) & ~(size_t)63; }

// the store, switched on: LINS_E_STATE before lins_archive_init or lins_place_init
int store_of(lins_ctx* ctx, ArchivePlace* A) {
  if (int rc = archive_place(ctx, A)) return rc;
  return A->store->on ? LINS_OK : LINS_E_STATE;
}

// LINS_E_ARG / LINS_E_INPUT of one query, LINS_OK
int query_check(const ArchivePlace& A, const lins_place_query& q) {
  if (q.query_slot < 0 || q.query_slot >= A.n_slots || q.target_slot < 0 || q.target_slot >= A.n_slots) return LINS_E_ARG;
  if (q.query_id < 0 || q.query_id >= (int)(*A.frames)[q.query_slot].size()) return LINS_E_ARG;
  if (!std::isfinite(q.now) || std::isnan(q.min_gap_s)) return LINS_E_INPUT;
  return LINS_OK;
}

// One call: describes the stale frames of `slots` and of every slot the n queries name, then searches.  keys_row: null, or
// (n == 1) room for one key per frame of the target slot.  topk > 0: the search writes every entry's row on the device and
// the select launch behind it takes the topk best candidates more than min_sep ids apart — results holds n * topk records,
// rank-major per entry, counts (n) the ranks filled; the row stays on the device.  Arguments checked by the caller.
int run(lins_ctx* ctx, const ArchivePlace& A, int n_slots_named, const int32_t* slots, int n, const lins_place_query* qs, lins_place_result* results,
        unsigned long long* keys_row, int topk = 0, int min_sep = 0, int32_t* counts = nullptr) {
  PlaceStore* m = A.store;
  m->build_ms = m->search_ms = m->select_ms = 0.f, m->pairs = 0, m->built = 0;
  const bool with_row = keys_row || topk > 0;
  const std::vector<std::vector<ArFrame>>& frames = *A.frames;
  std::vector<int> mark = m->described;  // as they will stand after this call
  std::vector<PlStale> stale;
  auto describe = [&](int s) {
    const std::vector<ArFrame>& fr = frames[s];
    for (int i = mark[s]; i < (int)fr.size(); ++i) {
      PlStale z{};
      z.src = fr[i].off, z.dst = (long long)s * A.max_frames + i, z.time = fr[i].time;
      std::memcpy(z.n, fr[i].n, sizeof z.n);
      stale.push_back(z);
    }
    mark[s] = (int)fr.size();  // (a slot named again in this call adds nothing)
  };
  for (int k = 0; k < n_slots_named; ++k) describe(slots[k]);
  for (int k = 0; k < n; ++k) describe(qs[k].query_slot), describe(qs[k].target_slot);
  if (stale.size() > (size_t)INT_MAX) return LINS_E_CAPACITY;
  const int chunk = m->chunk;
  std::vector<PlEntry> entries((size_t)n);
  std::vector<int2> chunks;
  uint64_t pairs = 0;
  long long row_total = 0;
  for (int k = 0; k < n; ++k) {
    const lins_place_query& q = qs[k];
    PlEntry& e = entries[k];
    std::memset(&e, 0, sizeof e);
    e.q_rec = (long long)q.query_slot * A.max_frames + q.query_id;
    e.base = (long long)q.target_slot * A.max_frames;
    e.now = q.now, e.gap = q.min_gap_s;
    e.nf = (int)frames[q.target_slot].size();
    e.skip = q.target_slot == q.query_slot ? q.query_id : -1;
    e.row = row_total;
    if (with_row) row_total += e.nf;
    e.chunk0 = (int)chunks.size();
    for (long long c = 0; c < e.nf; c += chunk) {
      if (chunks.size() >= (size_t)INT_MAX) return LINS_E_CAPACITY;
      chunks.push_back(make_int2(k, (int)c));
    }
    e.n_chunks = (int)chunks.size() - e.chunk0;
    pairs += (uint64_t)e.nf;
  }
  if (stale.empty() && n == 0) return LINS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  // up: stale | entries | chunks.  down: the entries' keys | their top-K keys | the row's keys (downloaded for the test aid
  // only), and behind them (never downloaded) the chunks' bests
  const size_t o_entries = align64(stale.size() * sizeof(PlStale)), o_chunks = align64(o_entries + (size_t)n * sizeof(PlEntry)),
               up_bytes = align64(o_chunks + chunks.size() * sizeof(int2));
  const size_t o_top = align64((size_t)n * 8), o_row = align64(o_top + (size_t)n * topk * 8), o_best = align64(o_row + (size_t)row_total * 8),
               down_bytes = keys_row ? o_best : o_row, down_cap = align64(o_best + chunks.size() * 8);
  BUF_TRY(ctx, m->h_up.grow(up_bytes));
  BUF_TRY(ctx, m->d_up.grow(up_bytes));
  BUF_TRY(ctx, m->h_down.grow(down_bytes));
  BUF_TRY(ctx, m->d_down.grow(down_cap));
  for (int i = 0; i < 4; ++i) BUF_TRY(ctx, m->ev[i].create());
  if (!stale.empty()) std::memcpy(m->h_up, stale.data(), stale.size() * sizeof(PlStale));
  if (n) std::memcpy(m->h_up + o_entries, entries.data(), (size_t)n * sizeof(PlEntry));
  if (!chunks.empty()) std::memcpy(m->h_up + o_chunks, chunks.data(), chunks.size() * sizeof(int2));
  hipStream_t st = ctx_stream(ctx);
  const PlParams prm{m->prm.r_max, m->prm.lift, inv_r_of(m->prm.r_max), m->prm.up_axis, m->prm.clouds};
  HIP_TRY(ctx, hipMemcpyAsync(m->d_up, m->h_up, up_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipEventRecord(m->ev[0], st));
  launch_place_build(st, (int)stale.size(), (const PlStale*)m->d_up.get(), A.d_arena, prm, m->d_D, m->d_rec);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(m->ev[1], st));
  launch_place_search(st, n, (int)chunks.size(), (const PlEntry*)(m->d_up + o_entries), (const int2*)(m->d_up + o_chunks), chunk, m->d_rec,
                      (unsigned long long*)(m->d_down + o_best), with_row ? (unsigned long long*)(m->d_down + o_row) : nullptr,
                      (unsigned long long*)m->d_down.get());
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(m->ev[2], st));
  if (topk > 0) {
    launch_place_select(st, n, (const PlEntry*)(m->d_up + o_entries), (const unsigned long long*)(m->d_down + o_row), topk, min_sep,
                        (unsigned long long*)(m->d_down + o_top));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(m->ev[3], st));
  }
  if (n) HIP_TRY(ctx, hipMemcpyAsync(m->h_down, m->d_down, down_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipEventElapsedTime(&m->build_ms, m->ev[0], m->ev[1]));
  HIP_TRY(ctx, hipEventElapsedTime(&m->search_ms, m->ev[1], m->ev[2]));
  if (topk > 0) HIP_TRY(ctx, hipEventElapsedTime(&m->select_ms, m->ev[2], m->ev[3]));
  m->described = mark;
  m->built = (int)stale.size(), m->pairs = pairs;
  const unsigned long long* K = (const unsigned long long*)m->h_down.get();
  const unsigned long long* top = (const unsigned long long*)(m->h_down + o_top);
  const int per = topk > 0 ? topk : 1;
  for (int k = 0; k < n && results; ++k) {
    int admissible = 0;
    const std::vector<ArFrame>& fr = frames[qs[k].target_slot];
    for (int c = 0; c < (int)fr.size(); ++c)
      if (c != entries[k].skip && time_admits(fr[c].time, qs[k].now, qs[k].min_gap_s)) admissible += 1;
    int filled = 0;
    for (int j = 0; j < per; ++j) {
      lins_place_result& r = results[(size_t)k * per + j];
      const unsigned long long key = topk > 0 ? top[(size_t)k * per + j] : K[k];
      std::memset(&r, 0, sizeof r);
      r.id = -1, r.shift = 0, r.distance = 1.f, r.candidates = admissible;
      if (key != kNoKey) unpack_key(key, &r.distance, &r.id, &r.shift), filled += 1;
    }
    if (counts) counts[k] = filled;
  }
  if (keys_row && row_total) std::memcpy(keys_row, m->h_down + o_row, (size_t)row_total * 8);
  return LINS_OK;
}

}  // namespace

extern "C" {

void lins_place_default_params(lins_place_params* p) {
  if (p) default_params(p);
}

int lins_place_init(lins_ctx* ctx, const lins_place_params* params) {
  if (!ctx || !params_ok(params)) return LINS_E_ARG;
  ArchivePlace A;
  if (int rc = archive_place(ctx, &A)) return rc;
  if (A.max_frames > kMaxId) return LINS_E_CAPACITY;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  HIP_TRY(ctx, hipStreamSynchronize(ctx_stream(ctx)));
  PlaceStore* m = A.store;
  m->on = false;
  const size_t recs = (size_t)A.n_slots * A.max_frames;
  BUF_TRY(ctx, m->d_D.grow(recs * kCells));
  BUF_TRY(ctx, m->d_rec.grow(recs * kPlRecWords));
  m->prm = *params;
  m->described.assign(A.n_slots, 0);
  m->team.drop();  // (the ring keys are derived from the descriptors: the first team call sizes them again)
  m->build_ms = m->search_ms = m->select_ms = 0.f, m->pairs = 0, m->built = 0;
  m->on = true;
  return LINS_OK;
}

int lins_place_sync(lins_ctx* ctx, int n, const int32_t* slots) {
  if (!ctx || n < 0 || (n && !slots)) return LINS_E_ARG;
  ArchivePlace A;
  if (int rc = store_of(ctx, &A)) return rc;
  for (int k = 0; k < n; ++k)
    if (slots[k] < 0 || slots[k] >= A.n_slots) return LINS_E_ARG;
  return run(ctx, A, n, slots, 0, nullptr, nullptr, nullptr);
}

int lins_place_search_batch(lins_ctx* ctx, int n, const lins_place_query* queries, lins_place_result* results) {
  if (!ctx || n < 0 || (n && (!queries || !results))) return LINS_E_ARG;
  ArchivePlace A;
  if (int rc = store_of(ctx, &A)) return rc;
  for (int k = 0; k < n; ++k)
    if (int rc = query_check(A, queries[k])) return rc;
  return run(ctx, A, 0, nullptr, n, queries, results, nullptr);
}

int lins_place_topk_batch(lins_ctx* ctx, int n, const lins_place_query* queries, int k, int min_sep, lins_place_result* results, int32_t* counts) {
  if (!ctx || n < 0 || (n && (!queries || !results || !counts))) return LINS_E_ARG;
  ArchivePlace A;
  if (int rc = store_of(ctx, &A)) return rc;
  if (k < 1 || k > LINS_PLACE_MAX_K || min_sep < 0) return LINS_E_ARG;
  for (int i = 0; i < n; ++i)
    if (int rc = query_check(A, queries[i])) return rc;
  return run(ctx, A, 0, nullptr, n, queries, results, nullptr, k, min_sep, counts);
}

int lins_place_descriptor(lins_ctx* ctx, int slot, int id, float* out) {
  if (!ctx || !out) return LINS_E_ARG;
  ArchivePlace A;
  if (int rc = store_of(ctx, &A)) return rc;
  if (slot < 0 || slot >= A.n_slots || id < 0 || id >= (int)(*A.frames)[slot].size()) return LINS_E_ARG;
  const int32_t s = slot;
  if (int rc = run(ctx, A, 1, &s, 0, nullptr, nullptr, nullptr)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  hipStream_t st = ctx_stream(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(out, A.store->d_D + ((size_t)slot * A.max_frames + id) * kCells, kCells * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return LINS_OK;
}

int lins_place_distances(lins_ctx* ctx, const lins_place_query* query, float* d, int32_t* shift, int cap) {
  if (!ctx || !query || cap < 0) return LINS_E_ARG;
  ArchivePlace A;
  if (int rc = store_of(ctx, &A)) return rc;
  if (int rc = query_check(A, *query)) return rc;
  const int nf = (int)(*A.frames)[query->target_slot].size();
  if (nf > cap) return LINS_E_CAPACITY;
  if (nf && (!d || !shift)) return LINS_E_ARG;
  std::vector<unsigned long long> keys((size_t)nf + 1);
  lins_place_result r;
  if (int rc = run(ctx, A, 0, nullptr, 1, query, &r, keys.data())) return rc;
  for (int c = 0; c < nf; ++c) {
    int id;
    d[c] = -1.f, shift[c] = -1;
    if (keys[c] != kNoKey) unpack_key(keys[c], &d[c], &id, &shift[c]);
  }
  return nf;
}

int lins_place_set_chunk(lins_ctx* ctx, int chunk) {
  if (!ctx || chunk < 0) return LINS_E_ARG;
  ArchivePlace A;
  if (int rc = archive_place(ctx, &A)) return rc;
  A.store->chunk = chunk ? chunk : kPlChunk;
  return LINS_OK;
}

int lins_last_place_select_ms(lins_ctx* ctx, float* select_ms) {
  if (!ctx) return LINS_E_ARG;
  ArchivePlace A;
  if (int rc = archive_place(ctx, &A)) return rc;
  if (select_ms) *select_ms = A.store->select_ms;
  return LINS_OK;
}

int lins_last_place_stats(lins_ctx* ctx, float* build_ms, float* search_ms, uint64_t* pairs, int32_t* frames_built) {
  if (!ctx) return LINS_E_ARG;
  ArchivePlace A;
  if (int rc = archive_place(ctx, &A)) return rc;
  if (build_ms) *build_ms = A.store->build_ms;
  if (search_ms) *search_ms = A.store->search_ms;
  if (pairs) *pairs = A.store->pairs;
  if (frames_built) *frames_built = A.store->built;
  return LINS_OK;
}

}  // extern "C"
