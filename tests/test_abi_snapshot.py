"""Stream snapshots (include/lins_snapshot.h): the prototypes compile as C99, the ctypes mirrors of the header, the
records and the plan's records have the C structs' sizes and offsets, both libraries export their calls, and the calls
that need no device keep the conventions (a NULL context is LINS_E_ARG; the host-only header check refuses garbage).
The n = 0 convention needs a context: tests/test_gpu_archive_snapshot.py."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_CALLS = ("lins_streams_snapshot_size", "lins_streams_snapshot", "lins_streams_restore", "lins_streams_migrate", "lins_snapshot_info_get",
             "lins_last_snapshot_stats")
HOST_CALLS = ("lins_host_snapshot_layout", "lins_host_snapshot_seal", "lins_host_snapshot_check", "lins_host_snapshot_info",
              "lins_host_snapshot_plan", "lins_host_snapshot_segments_ok")
E_ARG, E_INPUT = -1, -4


def test_prototypes_and_layouts_match_the_c_header(defs):
    protos = r"""
#include "lins_snapshot.h"
int (*a)(lins_ctx*, int, const int32_t*, uint64_t*) = lins_streams_snapshot_size;
int (*b)(lins_ctx*, int, const int32_t*, void* const*, const uint64_t*, uint64_t*) = lins_streams_snapshot;
int (*c)(lins_ctx*, int, const int32_t*, const void* const*, const uint64_t*) = lins_streams_restore;
int (*d)(lins_ctx*, int, lins_ctx*, int) = lins_streams_migrate;
int (*e)(const void*, uint64_t, lins_snapshot_info*) = lins_snapshot_info_get;
int (*f)(lins_ctx*, float*, float*, uint64_t*, int32_t*) = lins_last_snapshot_stats;
int (*g)(uint32_t, const lins_snapshot_counts*, lins_snapshot_dirent*, uint64_t*) = lins_host_snapshot_layout;
int (*h)(void*, uint64_t, uint32_t, const lins_snapshot_counts*, const lins_snapshot_facts*) = lins_host_snapshot_seal;
int (*i)(const void*, uint64_t, const lins_snapshot_facts*, const lins_snapshot_limits*, lins_snapshot_info*) = lins_host_snapshot_check;
int (*j)(const void*, uint64_t, lins_snapshot_info*) = lins_host_snapshot_info;
long long (*k)(uint32_t, const lins_snapshot_counts*, const lins_snapshot_place*, uint64_t, lins_snapshot_segment*, long long) = lins_host_snapshot_plan;
int (*l)(long long, const lins_snapshot_segment*, const int64_t*, uint64_t) = lins_host_snapshot_segments_ok;
/* the header brings the lifecycle's calls with it */
int (*m)(lins_ctx*, int, const int32_t*) = lins_streams_retire;
"""
    layout = r"""
#include <stddef.h>
#include <stdio.h>
#include "lins_snapshot.h"
#define S(t) printf("%zu ", sizeof(t))
#define O(t, f) printf("%zu ", offsetof(t, f))
int main(void) {
  S(lins_snapshot_counts); O(lins_snapshot_counts, ring_points); O(lins_snapshot_counts, graph_frames); O(lins_snapshot_counts, surround);
  S(lins_snapshot_facts); O(lins_snapshot_facts, boot); O(lins_snapshot_facts, machine); O(lins_snapshot_facts, map_interval);
  O(lins_snapshot_facts, surround_pose_leaf);
  S(lins_snapshot_info); O(lins_snapshot_info, total_bytes); O(lins_snapshot_info, modules); O(lins_snapshot_info, counts);
  O(lins_snapshot_info, facts); O(lins_snapshot_info, header_checksum);
  S(lins_snapshot_dirent); O(lins_snapshot_dirent, offset); O(lins_snapshot_dirent, bytes);
  S(lins_snapshot_stream_rec); O(lins_snapshot_stream_rec, filter_prm); O(lins_snapshot_stream_rec, imu_last);
  O(lins_snapshot_stream_rec, map_last_time); O(lins_snapshot_stream_rec, stepped); O(lins_snapshot_stream_rec, reserved);
  S(lins_snapshot_frame); O(lins_snapshot_frame, pose); O(lins_snapshot_frame, t); O(lins_snapshot_frame, time);
  S(lins_snapshot_loop); O(lins_snapshot_loop, var); O(lins_snapshot_loop, latest);
  S(lins_snapshot_limits); O(lins_snapshot_limits, surround_max); O(lins_snapshot_limits, archive_points);
  S(lins_snapshot_place); O(lins_snapshot_place, scan_off); O(lins_snapshot_place, ring_off); O(lins_snapshot_place, ar_n);
  S(lins_snapshot_segment); O(lins_snapshot_segment, buf_off); O(lins_snapshot_segment, units);
  printf("%d %d %d %d %d %llu\n", LINS_SNAP_SECTIONS, LINS_SNAP_FIRST_DEVICE_SEC, LINS_SNAP_FIRST_UNIT8_SEC, LINS_SNAP_BUFFERS,
         LINS_SNAP_FIRST_UNIT8_BUF, (unsigned long long)LINS_SNAPSHOT_MAGIC);
  return 0;
}
"""
    gcc = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    with tempfile.TemporaryDirectory() as d:
        p, c, exe = os.path.join(d, "p.c"), os.path.join(d, "c.c"), os.path.join(d, "c")
        open(p, "w").write(protos)
        open(c, "w").write(layout)
        subprocess.check_call(gcc + ["-c", p, "-o", os.path.join(d, "p.o")])  # (a changed signature is a compile error)
        subprocess.check_call(gcc + [c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    sz = C.sizeof
    K, F, I, D, R = defs.SnapshotCountsC, defs.SnapshotFactsC, defs.SnapshotInfoC, defs.SnapshotDirentC, defs.SnapshotStreamRecC
    Fr, L, Li, P, G = defs.SnapshotFrameC, defs.SnapshotLoopC, defs.SnapshotLimitsC, defs.SnapshotPlaceC, defs.SnapshotSegmentC
    want = [sz(K), K.ring_points.offset, K.graph_frames.offset, K.surround.offset,
            sz(F), F.boot.offset, F.machine.offset, F.map_interval.offset, F.surround_pose_leaf.offset,
            sz(I), I.total_bytes.offset, I.modules.offset, I.counts.offset, I.facts.offset, I.header_checksum.offset,
            sz(D), D.offset.offset, D.bytes.offset,
            sz(R), R.filter_prm.offset, R.imu_last.offset, R.map_last_time.offset, R.stepped.offset, R.reserved.offset,
            sz(Fr), Fr.pose.offset, Fr.t.offset, Fr.time.offset,
            sz(L), L.var.offset, L.latest.offset,
            sz(Li), Li.surround_max.offset, Li.archive_points.offset,
            sz(P), P.scan_off.offset, P.ring_off.offset, P.ar_n.offset,
            sz(G), G.buf_off.offset, G.units.offset,
            defs.SNAP_SECTIONS, defs.SNAP_FIRST_DEVICE_SEC, defs.SNAP_FIRST_UNIT8_SEC, defs.SNAP_BUFFERS, defs.SNAP_FIRST_UNIT8_BUF,
            defs.SNAPSHOT_MAGIC]
    assert got == want
    # the blob's own records have no padding the compiler chose: sizes are the sums of their fields
    assert (sz(K), sz(F), sz(I), sz(D), sz(R), sz(Fr), sz(L), sz(G)) == (56, 280, 384, 24, 272, 88, 112, 32)
    assert len(defs.SNAP_SEC_NAMES) == defs.SNAP_SECTIONS


def test_both_libraries_export_the_calls(host, ieskf):
    assert sorted(ieskf.SNAPSHOT_EXPORTS) == sorted(NEW_CALLS)
    assert not set(NEW_CALLS) & set(ieskf.EXPORTS) and not set(NEW_CALLS) & set(ieskf.LIFECYCLE_EXPORTS)
    for name in HOST_CALLS:
        assert hasattr(host.lib(), name), name
    for name in NEW_CALLS:
        assert hasattr(ieskf.lib(), name), name


def test_conventions_without_a_device(host, ieskf, defs):
    L = ieskf.lib()
    one = (C.c_int32 * 1)(0)
    size = (C.c_uint64 * 1)(0)
    L.lins_streams_snapshot_size.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.lins_streams_snapshot.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lins_streams_restore.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lins_streams_migrate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.lins_last_snapshot_stats.argtypes = [C.c_void_p] + [C.c_void_p] * 4
    L.lins_snapshot_info_get.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    for n in (0, 1):  # a NULL context is refused before n is looked at
        assert L.lins_streams_snapshot_size(None, n, one, size) == E_ARG
        assert L.lins_streams_snapshot(None, n, one, None, None, None) == E_ARG
        assert L.lins_streams_restore(None, n, one, None, None) == E_ARG
    assert L.lins_streams_migrate(None, 0, None, 0) == E_ARG
    assert L.lins_last_snapshot_stats(None, None, None, None, None) == E_ARG
    info = defs.SnapshotInfoC()
    junk = (C.c_uint8 * 1024)(*([7] * 1024))
    for lib_, name in ((L, "lins_snapshot_info_get"), (host.lib(), "lins_host_snapshot_info")):
        fn = getattr(lib_, name)
        fn.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        fn.restype = C.c_int
        assert fn(None, 0, C.byref(info)) == E_ARG
        assert fn(junk, 1024, None) == E_ARG
        assert fn(junk, 1024, C.byref(info)) == E_INPUT
        assert fn(junk, 0, C.byref(info)) == E_INPUT and fn(junk, 383, C.byref(info)) == E_INPUT


def test_a_blob_sealed_by_the_host_library_is_read_by_both(host, ieskf, defs):
    """a fresh stream's blob (all counts 0, every module): layout, seal, info through liblins_host.so, then the header check of
    liblins_ieskf.so on the same bytes"""
    H, L = host.lib(), ieskf.lib()
    counts, facts = defs.SnapshotCountsC(), defs.SnapshotFactsC()
    facts.params.num_iter, facts.ring_window = 8, 5
    total = C.c_uint64(0)
    directory = (defs.SnapshotDirentC * defs.SNAP_SECTIONS)()
    H.lins_host_snapshot_layout.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    assert H.lins_host_snapshot_layout(255, C.byref(counts), directory, C.byref(total)) == 0
    assert total.value % 16 == 0 and directory[0].offset == 384 + 24 * defs.SNAP_SECTIONS
    blob = (C.c_uint8 * total.value)()
    H.lins_host_snapshot_seal.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    assert H.lins_host_snapshot_seal(blob, total.value, 255, C.byref(counts), C.byref(facts)) == 0
    d = ieskf.snapshot_info(bytes(blob))
    assert d["total_bytes"] == total.value and d["modules"] == 255 and d["facts"]["num_iter"] == 8 and d["facts"]["ring_window"] == 5
    assert all(v == 0 for v in d["counts"].values())
    bad = bytearray(bytes(blob))
    bad[-1] ^= 1
    try:
        ieskf.snapshot_info(bytes(bad))
    except ieskf.LinsError as e:
        assert "error -4:" in str(e)
    else:
        raise AssertionError("a flipped byte was accepted")
