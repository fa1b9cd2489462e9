/*
 * lins_snapshot.h — snapshot and restore of streams: a robot's state leaves one context as a blob of plain host memory
 * and continues in another context, another slot, another process, bit for bit as if it had never moved (entry points
 * of liblins_ieskf.so: csrc/lins_snapshot_capi.hip, the modules' describe / check / apply functions in their own files
 * (csrc/snapshot.h), kernels snap_pack / snap_unpack of csrc/snapshot_kernels.hip; the blob's format and the copy plan
 * are one pure text for both libraries, csrc/host/snapshot_format.h, exported by liblins_host.so as lins_host_snapshot_*).
 *
 * A stream is a slot of every initialised module of its context: the resident scan and outlier cloud, the device
 * filter, the bootstrap's record, the odometry record, the map pose with its surround list, the local-map ring, the
 * key frames of the archive, the pose graph.  DESIGN.md section 5.3 "Stream snapshot" lists every field: in the blob,
 * or why not.
 *
 * The blob: a fixed header (lins_snapshot_info), a directory of LINS_SNAP_SECTIONS entries, the sections — host-only
 * sections first, then the sections that lie on the device, each 16-byte aligned.  Canonical: no pointers, no arena
 * offsets, no slot index, no uninitialised padding; the same stream state gives the same bytes wherever it lives.
 * The header records the context-wide facts a continuation's bits depend on; a destination that differs in one refuses.
 * Not in the blob: the team map's settings (lins_streams_map.h lins_streams_map_team and the groups of
 * lins_streams_map_team_groups).  They are context settings like lins_keyposes_set_mode — which slots share a map frame
 * is a fact about the destination's other slots, not about the stream — and the team selection keeps no list per
 * stream, so there is nothing of it to carry: the caller repeats mode and groups on the destination.  The format and
 * lins_snapshot_facts are unchanged.
 *
 * Conventions of lins_lifecycle.h: LINS_E_STATE before lins_streams_init; LINS_E_ARG for a stream out of range in any
 * initialised module or named twice; n = 0 is LINS_OK.  Everything that can refuse is asked first: a refused call
 * changes nothing anywhere.  Each call synchronises the context's stream before it touches state.
 *   LINS_E_STATE     the destination differs in a context-wide fact, lacks a module the blob carries, or its slot is
 *                    not what init / release leave
 *   LINS_E_CAPACITY  ring max_pts, archive max_frames or arena room, pose-graph sizes too small; caps[k] too small
 *   LINS_E_INPUT     wrong version, truncated or inconsistent blob, wrong checksum
 */
#ifndef LINS_SNAPSHOT_H_
#define LINS_SNAPSHOT_H_

#include "lins_lifecycle.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LINS_SNAPSHOT_MAGIC 0x3150414e534e494cull /* "LINSNAP1" */
#define LINS_SNAPSHOT_VERSION 1

/* modules a blob carries (lins_snapshot_info::modules) */
#define LINS_SNAP_STREAM 1u    /* resident scan, outlier cloud; always */
#define LINS_SNAP_FILTER 2u    /* the device filter's rows and globalState_ */
#define LINS_SNAP_BOOT 4u      /* machine mode: status, IMU row, pre-integration record */
#define LINS_SNAP_ODOM 8u      /* the odometry record */
#define LINS_SNAP_MAP_POSE 16u /* map pose, last_time, centre, transformLast, surround list */
#define LINS_SNAP_RING 32u     /* the local-map ring */
#define LINS_SNAP_ARCHIVE 64u  /* the key frames */
#define LINS_SNAP_GRAPH 128u   /* the pose graph */

/* sections, in blob order: the host-only ones, then the device-resident ones (16-byte units, then 8-byte units) */
enum {
  LINS_SNAP_SEC_STREAM_REC = 0, /* lins_snapshot_stream_rec */
  LINS_SNAP_SEC_SURROUND,       /* int32 ids */
  LINS_SNAP_SEC_RING_META,      /* lins_snapshot_frame per ring frame, oldest first */
  LINS_SNAP_SEC_AR_META,        /* lins_snapshot_frame per key frame, in id order */
  LINS_SNAP_SEC_PG_HOST,        /* Z[N][12] | T[N][12] doubles | held[N][6] floats | lins_snapshot_loop[L] */
  LINS_SNAP_SEC_SCAN_PTS,       /* less flat | less sharp */
  LINS_SNAP_SEC_OUTL_PTS,
  LINS_SNAP_SEC_RING_PTS,       /* per frame corner | surf | outlier, oldest first */
  LINS_SNAP_SEC_AR_PTS,         /* per frame corner | surf | outlier, in id order */
  LINS_SNAP_SEC_FILTER_ROWS,    /* state 19 | cov 324 | noise 144 | aux 16 | globalState_ 19 doubles */
  LINS_SNAP_SEC_BOOT_PRE,       /* 17 doubles */
  LINS_SNAP_SEC_ODOM,           /* lins_stream_odom */
  LINS_SNAP_SEC_MAP_POSE,       /* the 112-byte map pose record */
  LINS_SNAP_SEC_PG_D,           /* the solved increments: up_frames x 12 doubles */
  LINS_SNAP_SECTIONS
};
#define LINS_SNAP_FIRST_DEVICE_SEC LINS_SNAP_SEC_SCAN_PTS
#define LINS_SNAP_FIRST_UNIT8_SEC LINS_SNAP_SEC_FILTER_ROWS

typedef struct lins_snapshot_counts {
  int32_t has_scan;              /* 0: no resident scan (the two counts are 0) */
  int32_t less_sharp, less_flat; /* points of the resident scan */
  int32_t outliers;
  int32_t ring_frames, archive_frames;
  int64_t ring_points, archive_points;
  int32_t graph_frames, graph_loops;
  int32_t graph_up_frames; /* increments that live on the device (<= graph_frames) */
  int32_t surround;        /* ids of the surround list */
} lins_snapshot_counts;

/* what belongs to the context, not the stream, and the bits of a continuation depend on */
typedef struct lins_snapshot_facts {
  lins_params params;
  lins_boot_params boot; /* zeros without machine mode */
  int32_t machine, loop, surround;
  int32_t ring_window; /* 0: no local map */
  double map_interval; /* 0 without lins_streams_map_init */
  float surround_radius, surround_pose_leaf;
} lins_snapshot_facts;

/* the blob's header, and what lins_snapshot_info hands back */
typedef struct lins_snapshot_info {
  uint64_t magic;
  uint32_t version, header_bytes;
  uint64_t total_bytes;
  uint64_t checksum; /* of everything behind the header and the directory */
  uint32_t modules, n_sections;
  lins_snapshot_counts counts;
  lins_snapshot_facts facts;
  uint64_t header_checksum; /* of the header (this field as 0) and the directory */
} lins_snapshot_info;

typedef struct lins_snapshot_dirent {
  uint32_t id, unit; /* unit: 16 or 8 (device-resident), 1 (host only) */
  uint64_t offset, bytes; /* offset: from the blob's start, a multiple of 16; bytes: without the padding */
} lins_snapshot_dirent;

/* host-only records */
typedef struct lins_snapshot_stream_rec {
  int32_t outl_put, filter_set, status, imu_seen;
  lins_filter_params filter_prm;
  double imu_last[6];
  double map_last_time;
  float centre[3];
  int32_t stepped;
  float last6[6];
  int64_t reserved;
} lins_snapshot_stream_rec;

typedef struct lins_snapshot_frame {
  int32_t n[3], reserved; /* corner, surf, outlier */
  float pose[6];          /* x y z roll pitch yaw */
  float t[9];             /* the pose's trigonometry as the module holds it */
  float reserved2;
  double time; /* key frames of the archive; 0 on the ring */
} lins_snapshot_frame;

typedef struct lins_snapshot_loop {
  double Z[12], var;
  int32_t latest, closest;
} lins_snapshot_loop;

/* what a destination offers (lins_host_snapshot_check) */
typedef struct lins_snapshot_limits {
  uint32_t modules; /* the modules the destination has initialised */
  int32_t less_sharp_max, less_flat_max, outlier_max;
  int32_t ring_window, ring_max_pts;
  int32_t archive_frames; /* frames the slot still takes */
  int32_t graph_frames, graph_loops;
  int32_t surround_max;
  int64_t archive_points; /* points the arena still takes */
} lins_snapshot_limits;

/* where the device-resident pieces lie on the module side, in units of the piece's buffer */
typedef struct lins_snapshot_place {
  int64_t row; /* of the per-stream row buffers */
  int64_t scan_off[2]; /* less flat, less sharp: points into the streams' arena */
  int64_t outl_off;
  int64_t graph_off;         /* doubles into the increments' buffer */
  const int64_t* ring_off;   /* [ring_frames] points into the rings' buffer */
  const int64_t* ar_off;     /* [archive_frames] points into the archive's arena */
  const int32_t* ring_n;     /* points per ring frame */
  const int32_t* ar_n;       /* points per key frame */
} lins_snapshot_place;

/* module-side buffers of a plan */
enum {
  LINS_SNAP_BUF_SCAN = 0, /* float4 */
  LINS_SNAP_BUF_OUTL,
  LINS_SNAP_BUF_RING,
  LINS_SNAP_BUF_ARENA,
  LINS_SNAP_BUF_F_STATE, /* doubles */
  LINS_SNAP_BUF_F_COV,
  LINS_SNAP_BUF_F_NOISE,
  LINS_SNAP_BUF_F_AUX,
  LINS_SNAP_BUF_F_GSTATE,
  LINS_SNAP_BUF_B_PRE,
  LINS_SNAP_BUF_ODOM,
  LINS_SNAP_BUF_MAP_POSE,
  LINS_SNAP_BUF_PG_D,
  LINS_SNAP_BUFFERS
};
#define LINS_SNAP_FIRST_UNIT8_BUF LINS_SNAP_BUF_F_STATE

/* one copy segment: units of `unit` bytes between buffer `buffer` at buf_off and the staging buffer at stg_off (both in
 * units).  Invariants of a plan (lins_host_snapshot_segments_ok): segments are pairwise disjoint on the module side,
 * lie within the limits given, and — with the host-only sections — cover the blob exactly once.                     */
typedef struct lins_snapshot_segment {
  int32_t buffer, unit;
  int64_t buf_off, stg_off, units;
} lins_snapshot_segment;

int lins_streams_snapshot_size(lins_ctx* ctx, int n, const int32_t* streams, uint64_t* bytes /* [n] */);
/* blobs[k]: caps[k] bytes of host memory, 16-byte aligned; bytes[k] (may be NULL): what blob k takes.  A cap too small:
 * LINS_E_CAPACITY with every bytes[k] set and no blob written.  Read-only on the context.                           */
int lins_streams_snapshot(lins_ctx* ctx, int n, const int32_t* streams, void* const* blobs, const uint64_t* caps, uint64_t* bytes);
/* streams[k] must be what init / release leave in every module the blob carries */
int lins_streams_restore(lins_ctx* ctx, int n, const int32_t* streams, const void* const* blobs, const uint64_t* bytes);
/* snapshot of src_stream, restore into dst_stream, then lins_streams_retire of src_stream: dst is asked first, a refusal
 * leaves both contexts as they were                                                                                  */
int lins_streams_migrate(lins_ctx* src, int src_stream, lins_ctx* dst, int dst_stream);
/* host only: the blob's header after the full check of lins_host_snapshot_check without a destination */
int lins_snapshot_info_get(const void* blob, uint64_t bytes, lins_snapshot_info* out);
/* HIP-event time of the last pack / unpack launch, bytes staged, copy segments */
int lins_last_snapshot_stats(lins_ctx* ctx, float* pack_ms, float* unpack_ms, uint64_t* bytes, int32_t* segments);

/* ---- the format and the plan (liblins_host.so; the same inline text the device library runs) -------------------- */
/* counts + modules -> the directory (LINS_SNAP_SECTIONS entries) and the blob's size; LINS_E_ARG for counts no blob has */
int lins_host_snapshot_layout(uint32_t modules, const lins_snapshot_counts* counts, lins_snapshot_dirent* dir, uint64_t* total_bytes);
/* writes header and directory in front of the sections already in place, zeroes every section's padding, sums */
int lins_host_snapshot_seal(void* blob, uint64_t cap, uint32_t modules, const lins_snapshot_counts* counts, const lins_snapshot_facts* facts);
/* the whole check, in this order: LINS_E_INPUT (size, magic, version, header sum, directory against the counts, payload
 * sum, the frame and loop records against the counts), LINS_E_STATE (facts, when given, differ; a module limits lacks),
 * LINS_E_CAPACITY (a limit, when given, too small).  *out (may be NULL): the header.  Reads nothing beyond `bytes`.   */
int lins_host_snapshot_check(const void* blob, uint64_t bytes, const lins_snapshot_facts* facts, const lins_snapshot_limits* limits,
                             lins_snapshot_info* out);
int lins_host_snapshot_info(const void* blob, uint64_t bytes, lins_snapshot_info* out);
/* the copy segments of one stream: staging offsets count from stg_base (bytes, a multiple of 16) and follow the blob's
 * device-resident sections byte for byte.  Returns the number of segments (the first cap are written); LINS_E_ARG for
 * counts no blob has or a missing array.                                                                             */
long long lins_host_snapshot_plan(uint32_t modules, const lins_snapshot_counts* counts, const lins_snapshot_place* place, uint64_t stg_base,
                                  lins_snapshot_segment* segs, long long cap);
/* the invariants of a whole call's segments against the buffers' sizes (units; 0: no such buffer): LINS_OK or LINS_E_ARG */
int lins_host_snapshot_segments_ok(long long n, const lins_snapshot_segment* segs, const int64_t* buf_units /* [LINS_SNAP_BUFFERS] */,
                                   uint64_t stg_bytes);

#ifdef __cplusplus
}
#endif
#endif
