/*
 * lins_streams_map.h — the outlier cloud on the device and the hand-over of a stream's clouds to the mapping node
 * (entry points of liblins_ieskf.so; the host restatement lins_frontend_segment_outliers and LINS_OUTLIER_MAX are in
 * lins_host.h, lins_local_map_build_streams in lins_map.h).
 */
#ifndef LINS_STREAMS_MAP_H_
#define LINS_STREAMS_MAP_H_

#include "lins_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lins_segment_batch plus that cloud: outlier[k] is caller-allocated with LINS_OUTLIER_MAX entries and receives
 * out[k].n_outlier points, identical to lins_frontend_segment_outliers().  (lins_segment_batch runs the same kernel
 * without the emission.)                                                                                            */
int lins_segment_batch_outliers(lins_ctx* ctx, int n, const lins_point* const* raw, const int32_t* n_raw,
                                lins_segmented_scan* out, lins_point* const* outlier);

/* What the mapping node reads of a stream.  The raw-cloud steps (lins_streams_step_raw, lins_streams_step_imu_raw) keep
 * the outlier cloud (lins_frontend_segment_outliers) of the scan just taken in resident beside the feature clouds.  The
 * segmented-input steps have no outlier cloud in their input: lins_streams_put_outliers uploads one per stream
 * (n_outlier[k] <= LINS_OUTLIER_MAX points; outlier[k] may be null where n_outlier[k] is 0) for the NEXT step, which
 * consumes it; a segmented step without it leaves the stream's outlier cloud EMPTY.  A raw step ignores (and drops) a
 * pending upload.  A scan the feature gate stops (LINS_STREAMS_GATED) leaves all three clouds the last accepted scan's.
 * Clouds: finite, else LINS_E_INPUT.                                                                                  */
int lins_streams_put_outliers(lins_ctx* ctx, const lins_point* const* outlier, const int32_t* n_outlier);
/* The clouds StateEstimator::publishTopics would publish after the last step (SE:1125-1147), in the mapping node's axes
 * (x, y, z) <- (y, z, x), intensity kept: which = 0 the re-projected less-sharp cloud (laser_cloud_corner_last), 1 the
 * re-projected less-flat cloud (laser_cloud_surf_last), 2 the outlier cloud, NOT re-projected (outlier_cloud_last).
 * Returns the count; LINS_E_STATE before the stream's first step or on a failed streams context, LINS_E_CAPACITY when
 * cap is too small.  lins_local_map_build_streams (lins_map.h) reads the same clouds where they lie.                  */
int lins_streams_map_cloud(lins_ctx* ctx, int stream, int which, lins_point* out, int cap);

#ifdef __cplusplus
}
#endif
#endif
