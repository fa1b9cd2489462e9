"""Segmented scans built by hand for the feature stage (StateEstimator SE:619-827; frontend_kernels.hip and
host/frontend.cpp under the package's csrc/, oracle/frontend_oracle.cpp): each case decides the one rule it names, and says so in a dict of
claims that tests/test_fe_inputs.py checks with `model` below — a plain float64 statement of the stage that sees the
arrays alone.

Domain: what image projection can emit.  Ring-major, columns strictly increasing inside a ring, n <= 28 800, and the ring
indices exactly as IP:292-321 leaves them: a ring that begins when `count` points have been emitted and ends with `last`
gets start_ring = count - 1 + 5 and end_ring = last - 5 (an empty ring: count + 4 and count - 6).  For a ring of L points
whose first point is `first` that is start_ring = first + 4 — not first + 5 — so a ring's sectors span its local positions
4 .. L - 7: four points in front of them, six behind.

Ranges are dyadic (multiples of 1/8 below 2^10): the 11-tap f32 stencil and its square are exact, every curvature is the
same number in f32 and in float64.  Two regimes keep the rules apart:
  dense    consecutive columns around a base range of 32 (or 8), bumps of 1/8 and 1/4: below the 0.3 of the occlusion test
           and the 0.02 r of the parallel-beam test unless a case wants those;
  isolated columns 11 apart (no occlusion test passes, no neighbour is ever suppressed) around a base range of 512 with
           spikes of k / 8, k < 80: up to 80 distinct curvatures.
Unless a case says otherwise no pick is decided between equal curvatures (the reference's std::sort leaves that order
open): `model` records every such decision and the tests assert there is none.

Coordinates are free inputs of the stage.  By default point (ring, col) lies at the azimuth of its column (orientation
-3 + (col + 1/2) * 2 pi / 1800 against start_ori = -3), at the radius its range says and at height ring / 2.
"""
import numpy as np

ROWS, COLS, CLOUD_MAX = 16, 1800, 28800
START = -3.0
COMPACT_MAX = 64  # LINS_FE_COMPACT_MAX: edge candidates of a sector up to which the kernel deals them one per lane


def sectors(L):
    """the six (sp, ep) of a ring of L points, relative to its first point (SE:731-735 with start = 4, end = L - 6)"""
    s, e = 4, L - 6
    return [((s * (6 - j) + e * j) // 6, (s * (5 - j) + e * (j + 1)) // 6 - 1) for j in range(6)]


def ring(L, col0=0, step=1, base=32.0, cols=None):
    col = np.asarray(cols, np.int64) if cols is not None else col0 + step * np.arange(L, dtype=np.int64)
    return dict(col=col, range=np.full(len(col), base), ground=np.zeros(len(col), bool))


def assemble(rings, orientation=(START, START + 2 * np.pi, 2 * np.pi), claims=None, **more):
    """rings: {ring number: dict(col, range, ground[, xyz])} -> the case dict (segmented inputs + claims)"""
    cloud, rg, col, gd = [], [], [], []
    sr, er, first = np.zeros(ROWS, np.int32), np.zeros(ROWS, np.int32), np.zeros(ROWS, np.int64)
    count = 0
    for r in range(ROWS):
        sr[r], first[r] = count - 1 + 5, count
        g = rings.get(r)
        if g is not None and len(g["col"]):
            L = len(g["col"])
            c = np.asarray(g["col"], np.int64)
            assert (np.diff(c) > 0).all() and c[0] >= 0 and c[-1] < COLS
            p = np.zeros((L, 4), np.float32)
            if "xyz" in g:
                p[:, :3] = g["xyz"]
            else:
                a = START + (c + 0.5) * (2 * np.pi / COLS)
                rad = np.asarray(g.get("radius", g["range"]), np.float64)
                p[:, 0], p[:, 1], p[:, 2] = rad * np.cos(a), -rad * np.sin(a), 0.5 * r
            p[:, 3] = r + c / 10000.0
            cloud.append(p), rg.append(np.asarray(g["range"], np.float32)), col.append(c.astype(np.uint32))
            gd.append(np.asarray(g["ground"], np.uint8))
            count += L
        er[r] = count - 1 - 5
    n = count
    assert 0 < n <= CLOUD_MAX
    out = dict(cloud=np.ascontiguousarray(np.concatenate(cloud)), range=np.concatenate(rg), col=np.concatenate(col),
               ground=np.concatenate(gd), n=n, start_ring=sr, end_ring=er, orientation=np.array(orientation, np.float32),
               n_outlier=0, first=first, claims=claims or {})
    out.update(more)
    return out


# ---- the model ---------------------------------------------------------------------------------------------------------

def model(c):
    """The feature stage on the arrays of a case, in float64 and plain Python: curvatures, occlusion marks, per sector the
    candidate sets and the picks under the project's total order (curvature, then index: edges take the largest, planes
    the smallest), which picks were decided between equal curvatures, labels, the kept points of every ring, their voxel
    indices and centroids, and where undistortPcl's halfPassed flips."""
    n = int(c["n"])
    rg = c["range"][:n].astype(np.float64)
    col = c["col"][:n].astype(np.int64)
    gd = c["ground"][:n].astype(bool)
    assert np.array_equal(rg * 8, np.round(rg * 8)) and rg.max() < 1024 and rg.min() > 0  # the dyadic domain
    S = np.concatenate([[0.0], np.cumsum(rg)])
    d = np.zeros(n)
    i = np.arange(5, n - 5)
    d[i] = S[i + 6] - S[i - 5] - 11 * rg[i]
    curv = d * d
    picked = np.zeros(n, bool)
    for i in range(5, n - 6):  # markOccludedPoints
        if abs(col[i + 1] - col[i]) < 10:
            if rg[i] - rg[i + 1] > 0.3:
                picked[i - 5:i + 1] = True
            elif rg[i + 1] - rg[i] > 0.3:
                picked[i + 1:i + 7] = True
        if abs(rg[i - 1] - rg[i]) > 0.02 * rg[i] and abs(rg[i + 1] - rg[i]) > 0.02 * rg[i]:
            picked[i] = True
    occluded = picked.copy()
    label = np.zeros(n, np.int64)
    ind_of = lambda k: k if 5 <= k < n - 5 else 0  # cloudSmoothness[k].ind: value-initialised outside the stencil's reach

    def mark(ind):
        lo = hi = ind
        for l in range(1, 6):
            a, b = ind + l, ind + l - 1
            if a >= n or abs(col[a] - col[b]) > 10:
                break
            picked[a], hi = True, a
        for l in range(-1, -6, -1):
            a, b = ind + l, ind + l + 1
            if a < 0 or abs(col[a] - col[b]) > 10:
                break
            picked[a], lo = True, a
        return lo, hi

    secs, kept = [], []
    sharp, less_sharp, flat = [], [], []
    for r in range(ROWS):
        keep_r = []
        for j in range(6):
            s, e = int(c["start_ring"][r]), int(c["end_ring"][r])
            sp, ep = (s * (6 - j) + e * j) // 6, (s * (5 - j) + e * (j + 1)) // 6 - 1
            if s < 0 or e < 0:  # (C truncates towards zero; only an empty ring in front of everything gets here)
                sp, ep = int((s * (6 - j) + e * j) / 6), int((s * (5 - j) + e * (j + 1)) / 6) - 1
            sec = dict(ring=r, j=j, sp=sp, ep=ep, live=sp < ep and sp >= 0 and ep < n, sharp=[], less_sharp=[], flat=[],
                       edge_ties=[], plane_ties=[], marks=[])
            secs.append(sec)
            if not sec["live"]:
                continue
            m = ep - sp
            elems = [ind_of(sp + k) for k in range(m)]
            lane_of = {}
            ecand0 = [x for x in elems if curv[x] > 0.5 and not gd[x] and not picked[x]]
            sec["ecand0"] = list(ecand0)
            order = sorted(elems, key=lambda x: (curv[x], x))

            def edge_ok(x):
                return not picked[x] and curv[x] > 0.5 and not gd[x]

            def plane_ok(x):
                return not picked[x] and curv[x] < 0.5 and gd[x]

            n_ls = 0
            for pos, x in enumerate([ind_of(ep)] + order[::-1]):
                if not edge_ok(x):
                    if pos == 0:
                        rest = [y for y in elems if edge_ok(y)]
                        sec["n_ec"], sec["path"] = len(rest), path_of(len(rest))
                        lane_of = lanes(rest, elems, sec["path"])
                    continue
                if pos > 0:
                    twins = sorted({y for y in elems if edge_ok(y) and curv[y] == curv[x]})
                    if len(twins) > 1:
                        assert x == twins[-1]  # the largest index
                        sec["edge_ties"].append(dict(pick=x, twins=twins, lanes=sorted({lane_of[y] for y in twins}),
                                                     blocks=sorted({elems.index(y) // 64 for y in twins})))
                n_ls += 1
                if n_ls > 20:
                    break
                if n_ls <= 2:
                    label[x] = 2
                    sec["sharp"].append(x)
                else:
                    label[x] = 1
                sec["less_sharp"].append(x)
                picked[x] = True
                sec["marks"].append(mark(x))
                if pos == 0:
                    rest = [y for y in elems if edge_ok(y)]
                    sec["n_ec"], sec["path"] = len(rest), path_of(len(rest))
                    lane_of = lanes(rest, elems, sec["path"])
            for pos, x in enumerate(order + [ind_of(ep)]):
                if not plane_ok(x):
                    continue
                if pos < m:
                    twins = sorted({y for y in elems if plane_ok(y) and curv[y] == curv[x]})
                    if len(twins) > 1:
                        assert x == twins[0]  # the smallest index
                        sec["plane_ties"].append(dict(pick=x, twins=twins, lanes=sorted({elems.index(y) % 64 for y in twins}),
                                                      blocks=sorted({elems.index(y) // 64 for y in twins})))
                label[x] = -1
                sec["flat"].append(x)
                if len(sec["flat"]) >= 4:
                    break
                picked[x] = True
                sec["marks"].append(mark(x))
            sec["kept"] = [k for k in range(sp, ep + 1) if label[k] <= 0]
            keep_r += sec["kept"]
            sharp += sec["sharp"]
            less_sharp += sec["less_sharp"]
            flat += sec["flat"]
        kept.append(np.array(keep_r, np.int64))
    out = dict(d=d, curv=curv, occluded=occluded, picked=picked, label=label, sectors=secs, kept=kept,
               sharp=np.array(sharp, np.int64), less_sharp=np.array(less_sharp, np.int64), flat=np.array(flat, np.int64))
    out["voxels"] = [voxel_model(c["cloud"][k]) if len(k) else None for k in kept]
    out.update(undistort_model(c))
    return out


def path_of(n_ec):
    return "none" if n_ec == 0 else ("lane" if n_ec <= COMPACT_MAX else "mask")


def lanes(cands, elems, path):
    """the lane that holds each edge candidate: its rank among the candidates (one per lane), or its element's lane"""
    if path == "lane":
        order = sorted(cands, key=elems.index)
        return {x: k for k, x in enumerate(order)}
    return {x: elems.index(x) % 64 for x in cands}


def voxel_model(pts):
    """pcl::VoxelGrid, leaf 0.2, on the kept points of one ring in their order: the f32 product x * 5 decides the voxel
    (1 / 0.2f rounds to 5.0f), the centroid is the f32 sum in index order over the count.  -> index per point, box, the
    multiplicities in voxel order, the xyz centroids"""
    p = np.ascontiguousarray(pts[:, :3], np.float32)
    ijk = np.floor(p * np.float32(5.0)).astype(np.int64)
    mn, mx = ijk.min(0), ijk.max(0)
    dim = mx - mn + 1
    idx = (ijk[:, 0] - mn[0]) + (ijk[:, 1] - mn[1]) * dim[0] + (ijk[:, 2] - mn[2]) * dim[0] * dim[1]
    order = np.argsort(idx, kind="stable")
    uniq, start, counts = np.unique(idx[order], return_index=True, return_counts=True)
    cent = np.zeros((len(uniq), 3), np.float32)
    for v, (a, k) in enumerate(zip(start, counts)):
        s = np.zeros(3, np.float32)
        for q in order[a:a + k]:
            s = s + p[q]
        cent[v] = s / np.float32(k)
    packs = bool((ijk[:, :2] >= -1024).all() and (ijk[:, :2] < 1024).all() and (ijk[:, 2] >= -512).all() and (ijk[:, 2] < 511).all())
    exact = np.floor(p.astype(np.float64) * 5.0).astype(np.int64)  # without the f32 rounding of the product
    volume = int(dim[0]) * int(dim[1]) * int(dim[2])
    return dict(ijk=ijk, index=idx, dim=dim, min=mn, max=mx, counts=counts, centroids=cent, order=order, volume=volume,
                narrow=volume < 2 ** 21 - 1, packs=packs, rounding_decides=int((exact != ijk).any(1).sum()))


def undistort_model(c):
    """undistortPcl (SE:619-654) with numpy's float64 arctangent: flip = the first point whose corrected orientation passes
    start + pi (n: none), per point which of the five outcomes its correction took and its relative time"""
    n = int(c["n"])
    p = c["cloud"][:n].astype(np.float64)
    s, e, diff = [float(v) for v in c["orientation"]]
    raw = -np.arctan2(p[:, 1], p[:, 0])
    first = np.where(raw < s - np.pi / 2, raw + 2 * np.pi, np.where(raw > s + 1.5 * np.pi, raw - 2 * np.pi, raw))
    passed = np.nonzero(first - s > np.pi)[0]
    flip = int(passed[0]) if len(passed) else n
    second = raw + 2 * np.pi
    second = np.where(second < e - 1.5 * np.pi, second + 2 * np.pi, np.where(second > e + np.pi / 2, second - 2 * np.pi, second))
    half1 = np.arange(n) <= flip  # the flip point itself is still treated as first half
    ori = np.where(half1, first, second)
    branch = np.where(half1, np.where(raw < s - np.pi / 2, 1, np.where(raw > s + 1.5 * np.pi, 2, 0)),
                      np.where(raw + 2 * np.pi < e - 1.5 * np.pi, 4, np.where(raw + 2 * np.pi > e + np.pi / 2, 5, 3)))
    # how far any test that was taken lies from its threshold (whose arctangent is used must not matter)
    m1 = np.minimum.reduce([np.abs(raw - (s - np.pi / 2)), np.abs(raw - (s + 1.5 * np.pi)), np.abs(first - s - np.pi)])
    m2 = np.minimum(np.abs(raw + 2 * np.pi - (e - 1.5 * np.pi)), np.abs(raw + 2 * np.pi - (e + np.pi / 2)))
    margin = np.where(half1, m1, m2)
    tag = np.floor(p[:, 3]) + 0.1 * (ori - s) / diff
    return dict(flip=flip, branch=branch, tag=tag, ori_margin=float(margin.min()), first=first, second=second)


# ---- the cases ---------------------------------------------------------------------------------------------------------

def bump(g, at, h):
    for p in np.atleast_1d(at):
        g["range"][p] += h


def neighbour_gaps():
    """SE:764-779: a pick marks its neighbours one by one until two consecutive ones lie MORE than 10 columns apart.  Four
    sectors of one dense ring, each with a pick P (+1/4), a weaker candidate A next to it, a column gap of 10 or 11 two
    points away from P on one side, and a candidate B beyond the gap, four points from P.  A gap of 10: the marking goes
    on, P alone is picked.  A gap of 11: it stops, B is the sector's second pick.  A is never picked."""
    L, first = 310, 0
    g = ring(L)
    step = np.ones(L - 1, np.int64)
    edge, never = {}, []
    for j, (side, gap) in enumerate([(+1, 10), (+1, 11), (-1, 10), (-1, 11)]):
        q = sectors(L)[j][0] + 25
        bump(g, q, 0.25), bump(g, [q + side, q + 4 * side, q - 3 * side], 0.125)
        step[q + 2 if side > 0 else q - 3] = gap  # between q + 2 | q + 3, or q - 3 | q - 2
        edge[(2, j)] = [first + q] if gap == 10 else [first + q, first + q + 4 * side]
        never += [first + q + side] + ([first + q + 4 * side] if gap == 10 else [])
    g["col"] = np.concatenate([[0], np.cumsum(step)])
    return assemble({2: g}, claims=dict(edge_picks=edge, not_picked=never))


def ring_border_occlusion():
    """markOccludedPoints runs over the flat index: the pair (last point of ring r, first point of the next ring) is tested
    like any other.  Three pairs of rings of 40 points, the later ring's start_ring point (first + 4, its sector 0's sp)
    the only edge candidate: (1, 2) range steps UP by 0.5 five columns apart — first .. first + 5 of ring 2 are marked, not
    picked; (4, 5) steps DOWN — the mark falls on ring 4's last six points, outside every sector, picked; (7, 8) up again
    but exactly 10 columns apart — no mark, picked."""
    rings, L = {}, 40
    for r, col0, base in ((1, 0, 32.0), (2, 44, 32.5), (4, 200, 32.5), (5, 244, 32.0), (7, 400, 32.0), (8, 449, 32.5)):
        rings[r] = ring(L, col0, base=base)
    for r in (2, 5, 8):
        bump(rings[r], 4, 0.25)
    f = {2: 40, 5: 120, 8: 200}
    return assemble(rings, claims=dict(edge_picks={(2, 0): [], (5, 0): [f[5] + 4], (8, 0): [f[8] + 4]},
                                       occluded=list(range(40, 46)) + list(range(114, 120)), not_picked=[f[2] + 4]))


def occlusion_sides():
    """SE:680-713 inside one dense ring around a range of 8; i is the lower index of the pair the step lies between.
      (5 | 6)     +0.5: i = 5 is the first pair tested: 6 .. 11 marked, 5 picked
      i = 30      -0.5: i - 5 .. i marked, i + 1 picked
      i = 60      +0.25: nothing marked
      i = 110/135 +0.5 / -0.5 with 9 columns between the two: marked as above
      i = 160/205 +0.5 / -0.5 with 10 columns: nothing marked, the far side (made the stronger by 1/8) is picked
      i = 225     a lone +1/4: both neighbours differ by more than 0.02 r: marked, not picked
      i = 255     +1/4 on i and i + 1: one neighbour each: not marked, i + 1 picked
      (n-7 | n-6) -0.5: i = n - 7 is the last pair tested: n - 12 .. n - 7 marked, nothing picked."""
    L = 300
    g = ring(L, base=8.0)
    r = g["range"]
    step = np.ones(L - 1, np.int64)
    r[6:] += 0.5; r[0] -= 0.125
    r[31:] -= 0.5
    r[61:] += 0.25; r[55] += 0.125
    r[111:] += 0.5; step[110] = 9
    r[136:] -= 0.5; step[135] = 9; r[141] += 0.125
    r[161:] += 0.5; step[160] = 10; r[166] -= 0.125
    r[206:] -= 0.5; step[205] = 10; r[200] -= 0.125
    r[225] += 0.25
    r[255:257] += 0.25; r[250] += 0.125
    r[L - 6:] -= 0.5
    g["col"] = np.concatenate([[0], np.cumsum(step)])
    occ = list(range(6, 12)) + list(range(25, 31)) + list(range(111, 117)) + list(range(130, 136)) + [225] + list(range(L - 12, L - 6))
    return assemble({0: g}, claims=dict(occluded_exactly=occ, picked=[5, 31, 60, 110, 136, 161, 205, 256],
                                        not_picked=[6, 30, 61, 111, 135, 160, 206, 225, 255, L - 7]))


def occlusion_bounds():
    """The other side of occlusion_sides' index bounds: steps between (4 | 5) and (n - 6 | n - 5).  i = 4 and i = n - 6 are
    not tested: nothing is marked; 5 and n - 7 (the last sector's ep) are picked."""
    L = 60
    g = ring(L, base=8.0)
    g["range"][5:] += 0.5
    g["range"][L - 5:] -= 0.5
    return assemble({0: g}, claims=dict(occluded_exactly=[], picked=[5, L - 7]))


def zigzag(g, lo, hi, a0=1.0):
    """ranges lo .. hi - 1 alternate around the base with an amplitude that grows by 1/8 per point: |diffRange| = 12 x
    amplitude inside the run — all different"""
    k = np.arange(hi - lo)
    g["range"][lo:hi] += np.where(k % 2 == 0, 1.0, -1.0) * (a0 + k / 8.0)


def plane_ladder(g, sp, ground):
    """three bumps of 1/8, 3/8, 2/8 six points apart: the points between them have |diffRange| 1/8, 4/8, 5/8, 2/8 -> the
    four positions (in this order of position) that `ground` selects become plane candidates"""
    bump(g, sp + 3, 0.125), bump(g, sp + 9, 0.375), bump(g, sp + 15, 0.25)
    pos = [sp + 1, sp + 6, sp + 12, sp + 18]
    for p, on in zip(pos, ground):
        g["ground"][p] = on
    return pos


def ep_keeps_its_place():
    """SE:739-740 sorts [sp, ep): position ep is not part of the order — it is visited first by the edge loop and last by
    the plane loop whatever its curvature.  One isolated ring (columns 11 apart, range 512).
    Sector 1: 20 candidates with curvatures of 100 and more, ep with 11.390625 (what the zigzag's last member leaves in
    its stencil; a curvature just above 0.5 would need a lone 3/4 next to ep, whose other neighbours would then tie at
    0.5625) — lower than all of them and still the first sharp pick.
    Sector 3: ep is ground with curvature 0, three plane candidates before it: ep is the 4th flat pick.
    Sector 5: the same with four before it: ep is not picked."""
    L = 160
    g = ring(L, step=11, base=512.0)
    sec = sectors(L)
    sp, ep = sec[1]
    zigzag(g, sp, sp + 20)
    sp3, ep3 = sec[3]
    p3 = plane_ladder(g, sp3, [1, 1, 1, 0])
    g["ground"][ep3] = 1
    sp5, ep5 = sec[5]
    p5 = plane_ladder(g, sp5, [1, 1, 1, 1])
    g["ground"][ep5] = 1
    return assemble({3: g}, claims=dict(first_edge={(3, 1): ep}, curvature={ep: 11.390625}, n_less_sharp={(3, 1): 20},
                                        flat_picks={(3, 3): [p3[0], p3[1], p3[2], ep3], (3, 5): [p5[0], p5[3], p5[1], p5[2]]},
                                        not_picked=[ep5]))


def pick_limits():
    """SE:743-813 without suppression (isolated ring): sector 1 has 26 edge candidates, all different — exactly 2 sharp and
    18 more less-sharp picks, the six weakest left; sector 4 has six plane candidates — exactly 4 flat picks."""
    L = 163
    g = ring(L, step=11, base=512.0)
    sec = sectors(L)
    sp, ep = sec[1]
    assert ep - sp == 25
    zigzag(g, sp, ep + 1)
    sp4, ep4 = sec[4]
    assert ep4 - sp4 == 24
    g["ground"][sp4] = 1
    p = plane_ladder(g, sp4 + 3, [1, 1, 1, 1])
    g["ground"][ep4] = 1
    return assemble({6: g}, claims=dict(n_sharp={(6, 1): 2}, n_less_sharp={(6, 1): 20}, n_edge_candidates={(6, 1): 25},
                                        flat_picks={(6, 4): [sp4, p[0], p[3], p[1]]}, not_picked=[p[2], ep4]))



def handover():
    """SE:782-813: the 4th flat pick is labelled but neither marked picked nor marks its neighbours; the first three do,
    and so does every edge pick — across the sector's end.  One dense ring; every bump that only shapes a curvature sits
    on a ground point (never an edge candidate, and with a curvature of 1.56 no plane candidate).
    Sector 0: planes of curvature 0, 1/64, 1/16 and, at ep - 1, 9/64: the 4th.  The candidate E at ep + 2 (sector 1) stays
    eligible and is picked.  Sector 2: the same without the third plane: ep - 1 is the 3rd pick, marks ep - 6 .. ep + 4,
    E in sector 3 is suppressed.  Sector 4: an edge pick at ep - 1 suppresses the weaker candidate at ep + 2 of sector 5."""
    L = 310
    g = ring(L)
    sec = sectors(L)
    flat, edge = {}, {}
    for j, third in ((0, True), (2, False)):
        sp, ep = sec[j]
        G = [sp + 5, sp + 15, sp + 25, ep - 1]
        bump(g, sp + 17, 0.125), bump(g, sp + 27, 0.25), bump(g, ep + 2, 0.25), bump(g, ep + 3, 0.125)
        g["ground"][[sp + 17, sp + 27, ep + 3]] = 1
        g["ground"][[G[0], G[1], G[3]]] = 1
        g["ground"][G[2]] = third
        flat[(4, j)] = G if third else [G[0], G[1], G[3]]
        edge[(4, j + 1)] = [ep + 2] if third else []
    sp, ep = sec[4]
    bump(g, ep - 1, 0.25), bump(g, ep + 2, 0.125)
    edge[(4, 4)], edge[(4, 5)] = [ep - 1], []
    return assemble({4: g}, claims=dict(flat_picks=flat, edge_picks=edge, not_picked=[sec[2][1] + 2, ep + 2]))


def ties():
    """Equal curvatures: the project's total order takes the LARGEST index among equal edge keys and the SMALLEST among equal
    plane keys.  Ring 0: +1/4 every 12th point — 24 or 25 candidates a sector, all with |diffRange| 2.5: the one-per-lane
    path.  Ring 1: +1/4 every 4th point — three of four points are candidates (|diffRange| 2 on the bumps, 3/4 either side
    of them), more than 200 a sector in five 64-element blocks: the mask path.  Ring 2: ground at a constant range — every
    plane key is 0, three blocks a sector.  Every pick of this case is decided among equal keys in different lanes.
    Dropped, because the reference's std::sort leaves equal curvatures in an unspecified order: the comparison of WHICH
    points the reference picks, and of the less-flat cloud that depends on it; kept against the reference: the number
    of picks per cloud and the curvature of the pick at every position.  The independent checker orders by index too and is
    compared in full."""
    a, b, c = ring(1800), ring(1800), ring(800)
    a["range"][6::12] += 0.25
    b["range"][6::4] += 0.25
    c["ground"][:] = 1
    return assemble({0: a, 1: b, 2: c}, claims=dict(tie_picks=dict(lane=5, mask=5, plane=5)))


COUNT_RINGS = {0: 23, 1: 394, 2: 401, 3: 785, 4: 1169, 5: 1553, 6: 1800}  # ring -> points
COUNT_M = {(0, 0): 1, (1, 0): 63, (2, 0): 64, (2, 5): 65, (3, 0): 128, (3, 5): 129, (4, 0): 192, (4, 5): 193, (5, 0): 256,
           (5, 5): 257, (6, 0): 297, (6, 2): 298}  # (ring, sector) -> m = ep - sp; 298 is the most 1800 columns allow


def candidate_counts():
    """LINS_FE_COMPACT_MAX = 64: a sector's edge candidates are dealt one per lane up to 64, above that they stay in per-lane
    bit masks over the sector's 64-element blocks.  Ring lengths chosen for SE:731-735 give sectors of m = 1, 63, 64, 65,
    128, 129, 192, 193, 256, 257, 297 and 298 elements; every sector carries one +1/4 in its middle, except in ring 3
    (m = 128): sector 0 has no candidate, sector 2 one, sector 1 exactly 64 and sector 3 exactly 65 — runs of
    alternating +1/8 (and, for the even count, a lone +1/4) whose interior points all have |diffRange| 3/4, so equal keys decide picks there — and which twin is
    picked decides what it suppresses: against the reference ring 3 is left out of the comparison, the other rings are
    compared in full; the independent checker orders by index and is compared in full."""
    rings = {}
    for r, L in COUNT_RINGS.items():
        g = ring(L, col0=0)
        for j, (sp, ep) in enumerate(sectors(L)):
            if sp < ep and not (r == 3 and j in (0, 1, 3)):
                bump(g, (sp + ep) // 2, 0.25)
        rings[r] = g
    g, sec = rings[3], sectors(COUNT_RINGS[3])
    for j, want in ((1, 64), (3, 65)):
        sp, ep = sec[j]
        odd = want - 1 + want % 2  # (a run leaves an odd number; an even count takes a lone +1/4 far from the run as well)
        for k in range(odd, odd + 12):  # the run length that leaves exactly `odd` points with curvature > 0.5
            rg = g["range"].copy()
            rg[sp + 10:sp + 10 + k:2] += 0.125
            if odd < want:
                rg[sp + 110] += 0.25
            d = np.array([rg[i - 5:i + 6].sum() - 11 * rg[i] for i in range(sp, ep)])
            if (d * d > 0.5).sum() == want:
                g["range"] = rg
                break
        else:
            raise AssertionError("no run length gives %d candidates" % want)
    return assemble(rings, claims=dict(m=COUNT_M, n_ec0={(3, 0): 0, (3, 2): 1, (3, 1): 64, (3, 3): 65},
                                       path={(3, 0): "none", (3, 2): "lane", (3, 1): "lane", (3, 3): "mask"}))


def labels_into_less_flat():
    """SE:815-820: a ring's less-flat cloud holds every point of its sector spans whose label is <= 0.  One dense ring of
    310 points: three edge picks in sector 0 (two sharp, one less sharp), two flat picks in sector 2, an up and a down
    step of 0.5 in sector 4 (twelve points occlusion-marked only, two more edge picks).  Kept: 300 - 5 = 295 — the flat
    picks, the marked points and the ground bumps among them; the edge picks, the ring's first 4 and last 6 points not."""
    L = 310
    g = ring(L)
    sec = sectors(L)
    sp = sec[0][0]
    e = [sp + 10, sp + 25, sp + 40]
    bump(g, e, 0.25), bump(g, [e[1] + 3, e[2] + 3, e[2] - 3], 0.125)
    g["ground"][[e[1] + 3, e[2] + 3, e[2] - 3]] = 1
    sp = sec[2][0]
    f = [sp + 10, sp + 30]
    bump(g, sp + 32, 0.125)
    g["ground"][[f[0], f[1], sp + 32]] = 1
    sp = sec[4][0]
    i = sp + 15
    g["range"][i + 1:i + 21] += 0.5
    g["range"][i - 5] -= 0.125
    occ = list(range(i + 1, i + 7)) + list(range(i + 15, i + 21))
    edges = e + [i, i + 21]
    return assemble({5: g}, claims=dict(kept={5: 295}, occluded_exactly=occ, kept_includes=f + occ, picked=edges + f,
                                        kept_excludes=edges + [0, 1, 2, 3] + list(range(L - 6, L))))


RING_LENGTHS = {0: 0, 1: 1, 2: 11, 3: 12, 4: 13, 5: 17, 6: 18, 7: 23, 8: 24, 9: 30}
LIVE_SECTORS = {0: 0, 1: 0, 2: 0, 3: 0, 4: 0, 5: 1, 6: 2, 7: 6, 8: 6, 9: 6}  # floor((L - 10)(j + 1) / 6) - floor((L - 10) j / 6) >= 2


def ring_lengths():
    """SE:731-735 on short rings: a sector is worked on when sp < ep.  With end - start = L - 10, rings of up to 16 points
    have no live sector, 17 has one (the last), 18 two, 23 and more all six.  Every point of a live sector is kept for the
    less-flat cloud (constant ranges: no picks); each ring carries one +1/4 in its last sector where it has one."""
    rings = {}
    for r, L in RING_LENGTHS.items():
        if L:
            rings[r] = ring(L, col0=100 * r, base=32.0)
            if LIVE_SECTORS[r]:
                bump(rings[r], L - 8, 0.25)
    kept = {r: (sum(ep - sp + 1 for sp, ep in sectors(L) if sp < ep) - (1 if LIVE_SECTORS[r] else 0)) if L else 0
            for r, L in RING_LENGTHS.items()}
    return assemble(rings, claims=dict(live=LIVE_SECTORS, kept=kept))


def kept_ring(kept, col0=0, radius=None):
    """a ring of constant range: no picks, its kept points are its local positions 4 .. L - 7: L = kept + 10"""
    g = ring(kept + 10, col0)
    if radius is not None:
        g["radius"] = np.full(kept + 10, radius)
    return g


def voxel_ring(ijk, col0=0, frac=None):
    """a ring of constant range whose points lie in the voxels ijk (len = L: the first 4 and last 6 are outside the
    sectors), at the fractions `frac` of the 0.2 m cell (default: 0.3 .. 0.7 by position)"""
    ijk = np.asarray(ijk, np.float64)
    g = ring(len(ijk), col0)
    if frac is None:
        frac = 0.3 + 0.4 * (np.arange(len(ijk)) % 17)[:, None] / 17.0 + np.array([0.0, 0.01, 0.02])
    g["xyz"] = (ijk + frac) * 0.2
    return g


def box_ring(lo, hi, count, seed, corners=True, col0=0):
    """count + 10 points in distinct voxels of the box lo .. hi (inclusive), its two extreme corners among the kept ones"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(lo), np.array(hi)
    cells = set()
    while len(cells) < count + 10:
        cells.add(tuple(int(v) for v in rng.integers(lo, hi + 1)))
    cells = [list(v) for v in sorted(cells, key=lambda v: rng.random())]
    if corners:
        cells[5], cells[count // 2] = list(hi), list(lo)  # (the far corner first: the sort has to move it)
    return voxel_ring(cells, col0)


def voxel_sort_sizes():
    """The VoxelGrid stage of a ring (coordinates are free inputs; ranges constant: every sector point is kept).
    Rings 1-4: exactly 512, 513, 1024 and 1025 kept points — the 512-, 1024- and 2048-key sorts.
    Ring 5: a box of 127 x 129 x 128 = 2 097 024 voxels, below 2^21 - 1: 32-bit keys.  Ring 6: 129 x 128 x 128 =
    2 113 536, above: 64-bit keys; its far corner has voxel index 2 113 535 >= 2^21, which 32-bit keys would wrap.
    Ring 7: a small box around x = 210 m (ix ~ 1050: does not pack, narrow).  Ring 8: one point at ix = 1024 (just not
    packable), ring 11: at ix = -1024 (packs), ring 12: at -1025 (does not); ring 9: iz = 510 (packs), ring 10: 511 (does
    not).  Ring 13: coordinates exactly k * 0.2f, the float just below, and their negatives: for some the f32 product
    x * 5 lands on the other side of the border than the exact product would."""
    kept = {1: 512, 2: 513, 3: 1024, 4: 1025}
    rings = {r: kept_ring(k) for r, k in kept.items()}
    rings[5] = box_ring((-60, -64, -10), (66, 64, 117), 40, 5)
    rings[6] = box_ring((-60, -64, -11), (68, 63, 116), 40, 6)
    rings[7] = box_ring((1046, -4, -4), (1053, 3, 3), 40, 7)
    for r, corner in ((8, (1024, 0, 0)), (11, (-1024, 0, 0)), (12, (-1025, 0, 0)), (9, (0, 0, 510)), (10, (0, 0, 511))):
        g = box_ring((-3, -3, -3), (3, 3, 3), 30, r, corners=False)
        g["xyz"][:, 1] += 0.001 * r  # (no two points of the scan share their coordinates)
        g["xyz"][7] = (np.array(corner) + 0.5) * 0.2
        rings[r] = g
    k = np.arange(1, 26, dtype=np.float32)
    on = k * np.float32(0.2)
    xs = np.concatenate([on, np.nextafter(on, np.float32(0)), -on, -np.nextafter(on, np.float32(0))]).astype(np.float64)
    g = ring(len(xs) + 10, 0)
    x = np.concatenate([[0.31, 0.33, 0.35, 0.37], xs, [0.41, 0.43, 0.45, 0.47, 0.49, 0.51]])
    g["xyz"] = np.stack([x, 0.013 + 0.0007 * np.arange(len(x)), np.full(len(x), 0.05)], 1)
    rings[13] = g
    kept.update({5: 40, 6: 40, 7: 40, 8: 30, 9: 30, 10: 30, 11: 30, 12: 30, 13: 100})
    vox = {5: (True, True), 6: (False, True), 7: (True, False), 8: (True, False), 9: (True, True), 10: (True, False),
           11: (True, True), 12: (True, False), 13: (True, True)}  # ring -> (narrow, packs)
    return assemble(rings, claims=dict(kept=kept, voxel_keys=vox, volume={5: 127 * 129 * 128, 6: 129 * 128 * 128},
                                       one_point_per_voxel=[5, 6, 7], rounding_decides=13))


# multiplicities in voxel order; ring r's sorted list fills chunks 3 r .. 3 r + 2, a wave takes chunks (2 k, 2 k + 1)
CARRY_MULT = {
    0: [60, 4, 10, 50, 10, 58],   # 192: a run ends on lane 63 (60..63); one crosses 128, a pair's end (alone); the last reaches lane 63
    1: [60, 80, 10],              # 150: 60..139 starts in a pair's last chunk: finished alone across 64 and 128
    2: [50, 100, 42],             # 192: 50..149 crosses 64 inside a pair (carried) and 128 at its end (then finished alone)
    3: [100, 20, 20, 52],         # 192: 120..139 crosses 128, inside a pair here: carried
    4: [60, 10, 80],              # 150: 60..69 crosses 64 inside a pair: carried, and ends there
}
CARRY_PLACED = dict(ends_on_lane_63=(0, 60, 64), alone=(0, 124, 134), last_reaches_lane_63=(0, 134, 192), alone_twice=(1, 60, 140),
                    both=(2, 50, 150), carried=(4, 60, 70), carried_odd_ring=(3, 120, 140))
CARRY_KEPT = [192, 150, 192, 192, 150, 192, 130, 160, 192, 129, 170, 192, 180, 192, 140, 192]


def centroid_carry(thin=False):
    """The centroid pass takes the rings' sorted lists in chunks of 64 positions, a wave two consecutive chunks at a time
    when the scan has more than 32 of them; it then carries a voxel's partial sums over the border inside a pair, and the
    run at a pair's end is finished by one lane alone.  16 rings of 129 .. 192 kept points are 48 chunks.  The coordinates
    prescribe how many points each voxel holds, in voxel order (CARRY_MULT, CARRY_PLACED: where each run of interest
    lies); the other rings hold seven to a voxel.  A ring's points run through its voxels backwards, so the sort moves all.
    thin: every ring keeps 60 points — 16 chunks, one per wave step, nothing carried."""
    rings, kept = {}, {}
    for r, K in enumerate(CARRY_KEPT):
        K = 60 if thin else K
        mult = CARRY_MULT.get(r) if not thin else None
        if mult is None:
            mult = [7] * (K // 7) + ([K % 7] if K % 7 else [])
        assert sum(mult) == K
        vox = np.repeat(np.arange(len(mult)), mult)[::-1]  # kept point t -> voxel, descending
        vox = np.concatenate([np.full(4, len(mult) + 2), vox, np.full(6, len(mult) + 3)])
        frac = np.stack([0.1 + 0.8 * ((np.arange(len(vox)) * 37) % 101) / 101.0, np.full(len(vox), 0.5), np.full(len(vox), 0.5)], 1)
        rings[r] = voxel_ring(np.stack([vox + 10, np.full(len(vox), r), np.full(len(vox), r)], 1), col0=37 * r, frac=frac)
        kept[r] = K
    return assemble(rings, claims=dict(kept=kept, chunks=16 if thin else 48, mult={} if thin else CARRY_MULT,
                                       placed={} if thin else CARRY_PLACED))


def half_turns(start, shift=0, turn=2 * np.pi):
    """undistortPcl's branches: the orientation triple is an input.  Four rings of 300 points every sixth column at a
    radius of 100 (every kept point its own voxel, so every tag is seen), ranges constant.  start: start_ori; the cloud
    begins `shift` columns after the azimuth start_ori.  turn: end_ori - start_ori.  With a full turn the flip point would
    get the same orientation from either half's correction; with 2.7 pi it gets 2 pi more from the second half's, and it is
    a kept point of ring 0 in a voxel of its own: treating it as second half changes one tag of the less-flat cloud."""
    rings = {}
    for r in range(4):
        g = ring(300, col0=r, step=6)
        a = start + (g["col"] + shift + 0.5) * (2 * np.pi / COLS)
        g["xyz"] = np.stack([100 * np.cos(a), -100 * np.sin(a), np.full(300, 0.7 * r)], 1)
        rings[r] = g
    return assemble(rings, orientation=(start, start + turn, turn), claims=dict(kept={r: 290 for r in range(4)}, flip_seen=turn != 2 * np.pi))


CASES = {
    "neighbour_gaps": neighbour_gaps,
    "ring_border_occlusion": ring_border_occlusion,
    "occlusion_sides": occlusion_sides,
    "occlusion_bounds": occlusion_bounds,
    "ep_keeps_its_place": ep_keeps_its_place,
    "pick_limits": pick_limits,
    "handover": handover,
    "ties": ties,
    "candidate_counts": candidate_counts,
    "ring_lengths": ring_lengths,
    "labels_into_less_flat": labels_into_less_flat,
    "voxel_sort_sizes": voxel_sort_sizes,
    "centroid_carry": centroid_carry,
    "centroid_carry_thin": lambda: centroid_carry(thin=True),
    "half_turns_minus_pi": lambda: half_turns(-3.1, shift=-20),
    "half_turns_zero": lambda: half_turns(0.05),
    "half_turns_pi": lambda: half_turns(3.1),
    "half_turns_long_turn": lambda: half_turns(-1.0, turn=2.7 * np.pi),
    "half_turns_flip_at_0": lambda: half_turns(-1.0, shift=950),
}
TIE_CASES = ("ties", "candidate_counts")
TIE_RINGS = {"ties": (0, 1, 2), "candidate_counts": (3,)}  # the rings in which they do  # cases in which equal curvatures decide picks: compared with the checker and the reference up to that order

_BUILT = {}


def case(name):
    """the case `name`, built once per process (treat it as read-only)"""
    if name not in _BUILT:
        c = CASES[name]()
        for k in ("cloud", "range", "col", "ground"):
            c[k].setflags(write=False)
        _BUILT[name] = c
    return _BUILT[name]
