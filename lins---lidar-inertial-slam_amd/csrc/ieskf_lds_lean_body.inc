#ifndef LINS_LEAN_PREFETCH
#define LINS_LEAN_PREFETCH 1
#endif
// ieskf_lds_lean_body.inc — one wave-round of the correspondence phase of the batch kernel in its register-lean form
// (ieskf_lds_lean.h says what is different and why).  Textually included by ieskf_lds_update() of ieskf_lds_impl.h in
// place of its one-lane-per-query block; in scope: ka, prm, sd, L, cs, cc, arena, idx_store, scan, iter, pad, prof,
// do_search, searched, total, lane, wave, tid, kind_s, slot, active, row, ms, mc, PROF2_ADD.
// Reference: findCorrespondingSurfFeatures SE:829-953, findCorrespondingCornerFeatures SE:955-1063, H rows SE:507-539.
{
  const bool is_surf = kind_s;  // (wave-uniform)
  const int qi = is_surf ? slot : slot - sd.n_surf_q;
  const LCloud& c = is_surf ? cs : cc;
  const float thr = prm.nearest_f;
  // the carry records hold kRelayLanes queries per scan; a scan with more keeps nothing between iterations (as the
  // several-round layouts of rounds 1-5 did)
  const bool warm_iter = searched && total <= kRelayLanes;  // certificates / warm candidates exist (uniform)
  const float margin = warm_iter ? prm.margin_warm : prm.margin_cold;
  const bool verify = KNOBS && (pad & 8) != 0;  // test aid: search anyway and count disagreements
  // (lanes a search may take: the batch shape spends few on the cold iteration, where every query searches; a shape with
  // one scan per CU — the single-scan latency path — has lanes to spare)
  const int coop_cap = warm_iter ? kCoopMaxLanes : (BLOCK >= 1024 ? kCoopMaxLanes : LINS_COOP_COLD);
  const unsigned long long kNone = ~0ull;
  const auto crs = carry_rsrc(ka.relay_lane + (size_t)scan * kRelayLaneInts);
  const bool carry = total <= kRelayLanes;  // (uniform) this scan's queries have records
  const int coff = (carry && active ? slot : 0) * 16;
  int qidx = (is_surf ? sd.off_surf_q : sd.off_corner_q) + qi;
  float sel0 = 0.f, sel1f = 0.f, sel2 = 0.f;  // the de-skewed query
  int rq = 0;                                 // its ring
  v4u n0 = v4u{0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};
  v2u n1 = v2u{0u, 0u};
#if LINS_LEAN_PREFETCH
  v4u pw0 = v4u{0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};
  v3u pw1 = v3u{0u, 0u, 0u};
#endif
  long long s0 = prof ? clock64() : 0, s1 = s0, s2 = s0;
  if (active) {
    float4 q;
    if (KNOBS && (pad & 0x400000))  // (counting aid: no query load)
      q = make_float4(1.f + lane, 2.f, 0.5f, 3.25f);
    else
      q = arena[qidx];
    if (warm_iter && do_search) {  // the nearest-neighbour part of the record, in flight with the query point
      n0 = __builtin_amdgcn_raw_buffer_load_b128(crs, coff, 0, kCarrySc1);
      n1 = __builtin_amdgcn_raw_buffer_load_b64(crs, 1 * kRelayLanes * 16 + coff, 0, kCarrySc1);
#if LINS_LEAN_PREFETCH
      // ... and the walk part with it: seven registers across the nearest-neighbour phase, where the 128-register budget of
      // two scans per CU has room — a late iteration, in which nobody searches, no longer waits for a second trip to L2
      pw0 = __builtin_amdgcn_raw_buffer_load_b128(crs, 2 * kRelayLanes * 16 + coff, 0, kCarrySc1);
      pw1 = __builtin_amdgcn_raw_buffer_load_b96(crs, 3 * kRelayLanes * 16 + coff, 0, kCarrySc1);
#endif
    }
    rq = ring_of(q.w);
    const V3 phi = L.ic.phi;
    const V3 t{L.ic.lin[0], L.ic.lin[1], L.ic.lin[2]};
    if (KNOBS && (pad & 0x100000))  // (counting aid: no de-skew)
      sel0 = q.x, sel1f = q.y, sel2 = q.z;
    else
      transform_to_start(prm, phi, t, q, sel0, sel1f, sel2, g_lds.trig);
  }
  if (prof) {
    s1 = clock64();
#ifndef LINS_PROF_WAVES
    if (tid == 0) L.prof_acc[6] += s1 - s0;
#endif
    PROF2_ADD(0, s1 - s0);
  }
  auto drift_from = [&](float cx, float cy, float cz) {
    const float ex = sel0 - cx, ey = sel1f - cy, ez = sel2 - cz;
    return bound_sqrtf(ex * ex + ey * ey + ez * ez);
  };
  int p1 = -1, p2 = -1, p3 = -1;  // grid positions of the three selected target points
  if (do_search) {
    // ---- nearest neighbour: certificate (owner) ----------------------------------------------------------------------------
    // The record holds the last search's winner A and runner-up B and a lower bound lb for the distance of every other
    // candidate.  While everybody else is certified to stay farther than the closer of A and B the selection is re-decided
    // between those two from their distances alone (same strict (distance, index) order as the search); otherwise the search
    // runs again, warm-started from A.
    int ring1 = -1;    // ring of p1
    int sel_old = -1;  // last iteration's nearest neighbour
    bool need_nn = false, nn_changed = false;
    int warm_a = -1, warm_r = -1;  // the search's warm start (candidate A and its ring)
    bool said = false;
    int pred = -1;
    bool reseed1 = false;  // the query moved far since its last search: the warm bound is loose, seed as a cold search does
    int j1 = -1;           // original index of p1: from the record a certificate holds, or from the search's own key
    {
      int a1 = lo16(n0.x), b1c = hi16(n0.x);
      int ra1 = (int)(signed char)((n0.y >> 16) & 0xFFu), rb1 = (int)n0.y >> 24;
      sel_old = lo16(n0.y);
      bool flip = false;
      if (active && KNOBS && (pad & 0x80000) && warm_iter) {  // (counting aid: every certificate holds, unchecked)
        pred = a1, said = true;
        if (a1 >= 0) j1 = pt_idx(L, c, a1);
      } else if (active) {
        // the records of A and B in one trip (pt_rec: fetched on clamped positions, kept under the guards of the distances)
        float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra;
        if (c.n > 0) ra = pt_rec(L, c, a1), rb = pt_rec(L, c, b1c);  // (wave-uniform)
        const float da = a1 >= 0 ? rec_sqdist(ra, sel0, sel1f, sel2) : INFINITY, db = b1c >= 0 ? rec_sqdist(rb, sel0, sel1f, sel2) : INFINITY;
        const float drift = drift_from(__uint_as_float(n0.w), __uint_as_float(n1.x), __uint_as_float(n1.y));
        reseed1 = drift > prm.reseed_drift;
        bool ok = warm_iter && !(KNOBS && (pad & 16)) && certified(fminf(fminf(da, db), thr), __uint_as_float(n0.z), drift);
        const unsigned long long ka_ = da < thr ? pack_key(da, rec_idx(ra)) : kNone;
        const unsigned long long kb_ = db < thr ? pack_key(db, rec_idx(rb)) : kNone;
        flip = kb_ < ka_;
        pred = (flip ? kb_ : ka_) == kNone ? -1 : (flip ? b1c : a1);
        j1 = rec_idx(flip ? rb : ra);  // original index of the prediction (read only where pred >= 0)
        said = ok;
        if (verify) ok = false;
        need_nn = !ok;
      }
      warm_a = a1, warm_r = ra1;
      // a certified lane is finished here: prediction taken, record written when it changed
      if (active && !need_nn) {
        p1 = pred;
        if (flip) {  // the runner-up took over: the two tracked candidates change places
          const int tp = a1, tr = ra1;
          a1 = b1c, ra1 = rb1, b1c = tp, rb1 = tr;
        }
        ring1 = ra1;
        nn_changed = p1 != sel_old;
        if (carry && (flip || nn_changed))
          __builtin_amdgcn_raw_buffer_store_b128(v4u{pack16(a1, b1c), ((unsigned)p1 & 0xFFFFu) | (((unsigned)ra1 & 0xFFu) << 16) | ((unsigned)rb1 << 24), n0.z, n0.w},
                                                 crs, coff, 0, kCarrySc1);
      }
    }
    {
      const int n_cert = __popcll(__ballot(active && !need_nn));
      if (lane == 0 && n_cert) atomicAdd(&L.dbg[1], n_cert);
    }
    // ---- nearest neighbour: the searches of this wave, coop_lanes() lanes each ----------------------------------------------
    // (two passes: the wave's searches, then — with up to kHardLanes lanes each — those of them that turned out hard and were
    // deferred, nn_lean)
    bool todo_nn = need_nn;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
      const CoopMap cm = coop_map(todo_nn, lane);
#ifdef LINS_PROF2
      if (prof && lane == 0 && iter >= LINS_PROF2 && cm.n && pass == 0) g_lds.prof3[wave * 4 + 0] += 1, g_lds.prof3[wave * 4 + 2] += cm.n;
#endif
      if (!cm.n) break;  // (wave-uniform)
      {
        const NnRes r = coop_nn_lean(L, c, cm, pass ? kHardLanes : coop_cap, todo_nn, lane, sel0, sel1f, sel2, (rq & 0xFF) | (reseed1 ? 0x100 : 0), warm_a, warm_r,
                                     thr, margin, KNOBS && (pad & 2) != 0, pass == 0);
        const bool done = todo_nn && r.low2 != 0xFFFFFFFFu;
        todo_nn = todo_nn && !done;
        if (done) {
          p1 = r.low ? nn_pos(r.low) : -1;  // (a winner beat the threshold sentinel, so its distance is < thr, SE:851)
          ring1 = r.low ? nn_ring(r.low) : -1;
          j1 = (int)(r.low >> 18) - 1;  // (nn_low: index + 1 above the position and the ring)
          const int b = r.low2 ? nn_pos(r.low2) : -1, rb = r.low2 ? nn_ring(r.low2) : -1;
          if (KNOBS && said && p1 != pred) atomicAdd(&L.dbg[0], 1);
          nn_changed = p1 != sel_old;
          if (carry) {
            __builtin_amdgcn_raw_buffer_store_b128(v4u{pack16(p1, b), ((unsigned)p1 & 0xFFFFu) | (((unsigned)ring1 & 0xFFu) << 16) | ((unsigned)rb << 24),
                                                       __float_as_uint(r.lb), __float_as_uint(sel0)},
                                                   crs, coff, 0, kCarrySc1);
            __builtin_amdgcn_raw_buffer_store_b64(v2u{__float_as_uint(sel1f), __float_as_uint(sel2)}, crs, 1 * kRelayLanes * 16 + coff, 0, kCarrySc1);
          }
        }
      }
    }
    if (prof) {
      s2 = clock64();
#ifndef LINS_PROF_WAVES
      if (tid == 0) L.prof_acc[7] += s2 - s1;
#endif
      PROF2_ADD(1, s2 - s1);
    }
    // ---- second / third point: the walk part of the record, the walk cache, the certificate (owner) ---------------------------
    bool need_walk = false;
    int warm2 = -1, warm3 = -1;
    bool set_ok = !nn_changed;  // the recorded second / third points belong to this nearest neighbour
    bool said23 = false;
    int pred2 = -1, pred3 = -1;
    bool reseed2 = false;
    {
#if LINS_LEAN_PREFETCH
      v4u w0 = pw0;
      v3u w1 = pw1;
#else
      v4u w0 = v4u{0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};
      v3u w1 = v3u{0u, 0u, 0u};
      if (active && warm_iter) {
        w0 = __builtin_amdgcn_raw_buffer_load_b128(crs, 2 * kRelayLanes * 16 + coff, 0, kCarrySc1);
        w1 = __builtin_amdgcn_raw_buffer_load_b96(crs, 3 * kRelayLanes * 16 + coff, 0, kCarrySc1);
      }
#endif
      bool dirty = false;  // the walk part changed without a walk (walk cache): both planes are written back
      // Walk cache (ieskf_lds_impl.h has the why): the second / third points and their certificate are kept PER NEAREST
      // NEIGHBOUR — on a change the outgoing neighbour's set goes to the query's entry in global memory and, if the entry
      // holds the set of the incoming one, that set comes back and is judged like any other.
      if (LINS_WALK_CACHE && warm_iter && nn_changed && active && ka.walk_cache && !(KNOBS && (pad & 0x800000))) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(ka.walk_cache + (size_t)sd.slot_base * 8, 0, total * 32, 0x00020000);
        const unsigned gen16 = (unsigned)ka.run_gen << 16;
        const v4u e0 = __builtin_amdgcn_raw_buffer_load_b128(rs, slot * 32, 0, 16);
        const v4u e1 = __builtin_amdgcn_raw_buffer_load_b128(rs, slot * 32 + 16, 0, 16);
        if (sel_old >= 0) {  // (the recorded set is sel_old's: a walk or a judged set stood behind every selected neighbour)
          __builtin_amdgcn_raw_buffer_store_b128(v4u{gen16 | (unsigned)sel_old, w0.x, w0.y, w0.z}, rs, slot * 32, 0, 16);
          __builtin_amdgcn_raw_buffer_store_b128(v4u{w0.w, w1.x, w1.y, w1.z}, rs, slot * 32 + 16, 0, 16);
        }
        // (both words of the entry have arrived when this block ends: left in flight on a miss, the second one's registers
        // stand between the records the certificate fetches below and put a wait into the middle of their trip)
        asm volatile("" ::"v"(e1.w));
        if (p1 >= 0 && e0.x == (gen16 | (unsigned)p1)) {
          w0 = v4u{e0.y, e0.z, e0.w, e1.x};
          w1 = v3u{e1.y, e1.z, e1.w};
          set_ok = true, dirty = true;
        }
      }
      int a2 = lo16(w0.x), b2c = hi16(w0.x), a3 = lo16(w0.y), b3c = hi16(w0.y);
      bool flip2 = false, flip3 = false;
      // the records of the four tracked candidates in one trip, by every lane of a warm iteration — also by the lanes that
      // will walk, and by those whose planes 2-3 are not their own (own_set below): pt_rec clamps what it is given, and
      // judge() below keeps a record only where it read one before.  (Line queries have no third point and fetch a3 / b3c,
      // -1 clamped, all the same: with them under `if (is_surf)` the other path's zeroes land between the loads, with a wait.)
      float4 r2a = make_float4(0.f, 0.f, 0.f, 0.f), r2b = r2a, r3a = r2a, r3b = r2a;
      if (warm_iter && c.n > 0) {  // (wave-uniform)
        r2a = pt_rec(L, c, a2), r2b = pt_rec(L, c, b2c), r3a = pt_rec(L, c, a3), r3b = pt_rec(L, c, b3c);
      }
      if (active && p1 >= 0) {  // (p1 >= 0 => p1 is candidate A, on ring ring1, and j1 its original index)
        need_walk = !set_ok || !warm_iter;
        if (!need_walk && KNOBS && (pad & 0x80000)) {
          pred2 = a2, pred3 = a3, said23 = true;
        } else if (!need_walk) {
          const WalkCtx w = make_walk_ctx(c, is_surf ? sd.n_surf_q : sd.n_corner_q, j1, ring1);
          const float dB = drift_from(__uint_as_float(w1.x), __uint_as_float(w1.y), __uint_as_float(w1.z));
          auto judge = [&](int pa, int pb, const float4& ra, const float4& rb, float lb, int& pd, bool& fl) {
            const float da = pa >= 0 ? rec_sqdist(ra, sel0, sel1f, sel2) : INFINITY, db = pb >= 0 ? rec_sqdist(rb, sel0, sel1f, sel2) : INFINITY;
            int rka = 0, rkb = 0;
            if (pa >= 0) walk_rank(w, rec_idx(ra), rka);
            if (pb >= 0) walk_rank(w, rec_idx(rb), rkb);
            const unsigned long long ka_ = da < thr ? pack_key(da, rka) : kNone;
            const unsigned long long kb_ = db < thr ? pack_key(db, rkb) : kNone;
            fl = kb_ < ka_;
            pd = (fl ? kb_ : ka_) == kNone ? -1 : (fl ? pb : pa);
            return certified(fminf(fminf(da, db), thr), lb, dB);
          };
          bool ok23 = judge(a2, b2c, r2a, r2b, __uint_as_float(w0.z), pred2, flip2);
          if (is_surf) ok23 = judge(a3, b3c, r3a, r3b, __uint_as_float(w0.w), pred3, flip3) && ok23;
          said23 = ok23;
          need_walk = !ok23 || verify;
        }
      }
      // (a query without a nearest neighbour last iteration has no walk part of its own: planes 2-3 then hold whatever an
      // earlier iteration, update or scan left in the slot — positions that may name the other cloud — never warm candidates)
      const bool own_set = sel_old >= 0 || dirty;
      warm2 = own_set ? a2 : -1, warm3 = own_set ? a3 : -1;
      if (need_walk && warm_iter) reseed2 = drift_from(__uint_as_float(w1.x), __uint_as_float(w1.y), __uint_as_float(w1.z)) > prm.reseed_drift;
      if (active && p1 >= 0 && !need_walk) {  // finished: predictions taken, record written when it changed
        p2 = pred2, p3 = pred3;
        if (flip2) {
          const int tp = a2;
          a2 = b2c, b2c = tp;
        }
        if (flip3) {
          const int tp = a3;
          a3 = b3c, b3c = tp;
        }
        if (carry && (flip2 || flip3 || dirty))
          __builtin_amdgcn_raw_buffer_store_b128(v4u{pack16(a2, b2c), pack16(a3, b3c), w0.z, w0.w}, crs, 2 * kRelayLanes * 16 + coff, 0, kCarrySc1);
        if (carry && dirty) __builtin_amdgcn_raw_buffer_store_b96(w1, crs, 3 * kRelayLanes * 16 + coff, 0, kCarrySc1);
      }
    }
    {
      const int n_cert = __popcll(__ballot(active && p1 >= 0 && !need_walk));
      if (lane == 0 && n_cert) atomicAdd(&L.dbg[2], n_cert);
    }
    // ---- second / third point: the walks of this wave -------------------------------------------------------------------------
    {
      const CoopMap cm = coop_map(need_walk, lane);
#ifdef LINS_PROF2
      if (prof && lane == 0 && iter >= LINS_PROF2 && cm.n) g_lds.prof3[wave * 4 + 1] += 1, g_lds.prof3[wave * 4 + 3] += cm.n;
#endif
      if (cm.n) {
        const int nq = is_surf ? sd.n_surf_q : sd.n_corner_q;
        const WalkRes r = coop_walk_lean(L, c, is_surf, nq, cm, coop_cap, need_walk, lane, sel0, sel1f, sel2, j1, ring1, warm2, warm3, (set_ok ? 0 : 1) | (reseed2 ? 2 : 0), thr, margin,
                                         KNOBS && (pad & 1) != 0);
        if (need_walk) {
          p2 = lo16(r.p2), p3 = lo16(r.p3);
          if (KNOBS && said23 && (p2 != pred2 || (is_surf && p3 != pred3))) atomicAdd(&L.dbg[0], 1);
          if (carry) {
            __builtin_amdgcn_raw_buffer_store_b128(v4u{r.p2, r.p3, __float_as_uint(r.lb2), __float_as_uint(r.lb3)}, crs, 2 * kRelayLanes * 16 + coff, 0, kCarrySc1);
            __builtin_amdgcn_raw_buffer_store_b96(v3u{__float_as_uint(sel0), __float_as_uint(sel1f), __float_as_uint(sel2)}, crs, 3 * kRelayLanes * 16 + coff, 0,
                                                  kCarrySc1);
          }
        }
      }
    }
#ifndef LINS_PROF_WAVES
    if (prof && tid == 0) L.prof_acc[8] += clock64() - s2;
#endif
    if (active && prm.icp_freq > 1) idx_store[sd.slot_base + slot] = make_int4(p1, p2, p3, 0);
  } else if (active) {
    const int4 s = idx_store[sd.slot_base + slot];
    p1 = s.x, p2 = s.y, p3 = s.z;
  }
  long long s3 = prof ? clock64() : 0;
  if (prof && do_search) PROF2_ADD(2, s3 - s2);
  // (the iteration constants the rows need — R^T, G^T — are read from LDS HERE, not hoisted above the searches)
  asm volatile("" ::: "memory");
  if (active && !(KNOBS && (pad & 0x20000))) {  // (counting aid: LINS_DEBUG_SKIP bit 0x20000 drops the rows)
#if LINS_LEAN_PREFETCH
    // the raw query point again (SE:948, 1058: the keypoint of a row is the raw point) — read a second time instead of held
    // in four registers across the searches, and read HERE, ahead of the row's geometry, which hides the trip to L2; the
    // index is laundered so that the two reads are not merged
    asm volatile("" : "+v"(qidx));
    float4 q2 = arena[qidx];
#endif
    auto pt4 = [&](int pos) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      pt_xyz(L, c, pos, v.x, v.y, v.z);
      return v;
    };
    QueryOut o;
    o.accepted = 0;
    o.c[0] = o.c[1] = o.c[2] = o.c[3] = 0.f;
    if (is_surf) {
      if (p1 >= 0 && p2 >= 0 && p3 >= 0) surf_row(prm, iter, sel0, sel1f, sel2, pt4(p1), pt4(p2), pt4(p3), o);
    } else if (p1 >= 0 && p2 >= 0) {
      corner_row(prm, iter, sel0, sel1f, sel2, pt4(p1), pt4(p2), o);
    }
    if (o.accepted) {
      // the raw query point again (SE:948, 1058: the keypoint of a row is the raw point) — read a second time instead of
      // held in four registers across the searches; the index is laundered so that the two reads are not merged
#if !LINS_LEAN_PREFETCH
      asm volatile("" : "+v"(qidx));
      float4 q2 = arena[qidx];
#endif
      if (KNOBS && (pad & 0x400000)) q2 = make_float4(1.f + lane, 2.f, 0.5f, 3.25f);
      const V3 cv{(double)o.c[0], (double)o.c[1], (double)o.c[2]};
      const V3 u = cross(V3{(double)q2.x, (double)q2.y, (double)q2.z}, mvec(L.ic.Rt, cv));
      const V3 a = mvec(L.ic.Gt, u);
      row[0] = cv.x, row[1] = cv.y, row[2] = cv.z, row[3] = a.x, row[4] = a.y, row[5] = a.z;
      row[6] = prm.lidar_scale * (double)o.c[3];
      if (is_surf)
        ++ms;
      else
        ++mc;
    }
  }
#ifndef LINS_PROF_WAVES
  if (prof && tid == 0) L.prof_acc[9] += clock64() - s3;
#endif
  if (prof) PROF2_ADD(3, clock64() - s3);
}
