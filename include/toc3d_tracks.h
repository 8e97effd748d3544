/*
 * libtoc3d_gfx950 -- greedy centre-distance tracking of the submission records, on the device.  The reference tracks after the run, on the host:
 * nusc_tracking/pub_tracker.py:26-186 (PubTracker.step_centertrack), nusc_tracking/track_utils.py:3-12 (greedy_assignment), driven per frame by
 * nusc_tracking/pub_test.py:77-153 -- an N x M float64 distance matrix, a deep copy of it, a Python loop with one argmin per detection, and the tracks as a list of
 * dicts mutated in place.  Here one launch does a step for every camera stream, from the tensors toc3d_boxes_to_global (include/toc3d_results.h) leaves on the
 * device, with each stream's tracks in device memory from frame to frame.  Compiled into the same library as include/toc3d.h, whose conventions, error codes and
 * toc3d_stream_t it shares; consumed by toc3d_amd.PubTracker (toc3d_amd/tracking.py), which names the classes and writes the JSON.
 *
 * Kept beside toc3d.h, with a version of its own, as the other side headers are: TOC3D_ABI_MINOR stays where the tests of the 11.1 surface pin it.
 * toc3d_amd/lib.py keeps the signatures in a table of its own (_TRACKS_SIGS) and binds them at first use.
 *
 * THE STATE of one stream, TOC3D_TRACKS_STATE_BYTES(capacity) = 32 + 48 * capacity bytes on an 8-byte boundary, streams back to back:
 *   byte 0   int32 count            tracks held (rows [0, count) below are live, every row at or beyond count is zeros)
 *   byte 4   int32 id_count         the last tracking id handed out (pub_tracker.py:38, :164)
 *   byte 8   f64   last_timestamp   pub_test.py:105-108
 *   byte 16  16 bytes of zeros
 *   byte 32  f64 ct [capacity][2];  then f64 tracking [capacity][2];  then int32 label [capacity], tracking_id [capacity], age [capacity], active [capacity]
 * A step READS state_in and WRITES state_out (every byte of it, none twice): the two must not overlap, and the host swaps them after the step.  The state after a
 * step is a function of the state before it and the inputs alone.
 *
 * THE STEP, per stream b, restated from pub_tracker.py:41-186:
 *   0. first[b] != 0: the state read is taken as empty (no tracks, id_count 0, last_timestamp = timestamp[b]): tracker.reset() of pub_test.py:101-105.
 *      time_lag = timestamp[b] - last_timestamp in float64; last_timestamp = timestamp[b] (pub_test.py:107-108).
 *   1. filter (:62-72): the rows i < kept[b] with 0 <= name < num_classes, 0 <= track_label[name] < num_track_labels and !((double)score < score_thr), in input
 *      order.  ct = translation[:2];  tracking = (velocity[:2] * -1) * time_lag, in float64, each product rounded once.
 *   2. positions (:103-116): p = (float)(ct + (double)(float)tracking) of a detection;  q = (float)ct of a track.
 *   3. distance (:119-124), in float32 with every operation rounded once (no fused multiply-add): dx = q.x - p.x, dy = q.y - p.y, d = sqrt(dx * dx + dy * dy).
 *      A pair is valid when the labels are equal and !(d > max_diff[label]): a distance equal to the gate is valid.
 *   4. greedy assignment (track_utils.py:7-11): detection i, in order, takes the valid track not yet taken with the smallest d, the lowest track index on a tie.
 *   5. the new state, in this order: the matches in detection order (tracking_id and active + 1 from the track, age 1, ct and tracking from the detection, :155-160);
 *      the unmatched detections in detection order (tracking_id = ++id_count, age 1, active 1, :162-168); the unmatched tracks with age < max_age in track order
 *      (age + 1, active 0, ct = ct + tracking * -1 in float64, :172-183).  Every other track is dropped.
 *   6. THE EMPTY-FRAME QUIRK, reproduced: when no detection survives the filter (:42-59, :81-98) the reference returns early and does NOT replace self.tracks.
 *      Every track stays, in place and in order; those with age < max_age get age + 1, active 0 and the ct move; those with age >= max_age are left untouched --
 *      they are not dropped, and can match on the next frame.  num_out = 0.
 * OUTPUTS, per input row: track_id and active (both 0 for a row filtered out or at or beyond kept[b]); order: the input rows in the order the reference returns
 * them -- matches in detection order, then unmatched detections in detection order (:154-168) -- and -1 from num_out[b] on; num_out = the detections that survive.
 * DIFFERENCES to the reference: (a) a distance that is NaN is invalid here (numpy's argmin would take the first NaN); records made by toc3d_boxes_to_global are
 * finite, so this needs a timestamp that is not; (b) a name outside [0, num_classes) or a label outside [0, num_track_labels) is filtered out, where the reference
 * would raise; (c) the unmatched tracks the reference returns in its list with active 0 are state here, not output rows.
 *
 * One workgroup of 512 threads per stream.  The detections are filtered and compacted stably with wave ballots and an LDS prefix; matching never crosses labels,
 * so wavefront w walks the detections of labels w, w + 8, ... in order, its lanes striding over that label's tracks (compacted per label in LDS as float32
 * positions) with a (distance, index) minimum across the wavefront made of DPP moves and permlane swaps: the sequential depth is the largest class, not N.  The
 * three groups of the new state are placed by ballots and prefix sums again.  No atomics: nothing depends on scheduling.  Plain vector stores, no inline assembly.
 */
#ifndef TOC3D_TRACKS_H_
#define TOC3D_TRACKS_H_

#include "toc3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TOC3D_TRACKS_ABI 1

#define TOC3D_TRACKS_MAX_TRACKS 8192     /* capacity: a step holds at most K * (max_age + 1) tracks */
#define TOC3D_TRACKS_MAX_BOXES 2048      /* K: TOC3D_RESULTS_MAX_BOXES */
#define TOC3D_TRACKS_MAX_CLASSES 64      /* num_classes and num_track_labels */
#define TOC3D_TRACKS_REC 12              /* doubles a record: TOC3D_RESULTS_REC; translation at 0, velocity at 10 */
#define TOC3D_TRACKS_HEADER_BYTES 32
#define TOC3D_TRACKS_ROW_BYTES 48
#define TOC3D_TRACKS_STATE_BYTES(capacity) (TOC3D_TRACKS_HEADER_BYTES + TOC3D_TRACKS_ROW_BYTES * (int64_t)(capacity))

int toc3d_tracks_abi(void);

/* *bytes (host memory) = TOC3D_TRACKS_STATE_BYTES(capacity).  TOC3D_ERR_ARG: capacity outside [0, 8192], bytes null. */
int toc3d_tracks_state_bytes(int64_t capacity, int64_t* bytes);

/* One launch for all B streams (none when B == 0: nothing is then written).  Every buffer is device memory.
 *   rec          f64 [B, K, 12];  score  f32 [B, K];  name  int32 [B, K];  kept  int64 [B]: as toc3d_boxes_to_global writes them; rows at or beyond kept[b] are not
 *                read (a count below 0 is taken as 0, one above K as K)
 *   track_label  int32 [num_classes]: detection class -> tracking label, the index in NUSCENES_TRACKING_NAMES (pub_tracker.py:9-12); -1 = not tracked
 *   max_diff     f32 [num_track_labels]: 2.5 for every label in the reference (:15-23)
 *   score_thr    a detection is dropped when (double)score < score_thr (:66)
 *   timestamp    f64 [B], seconds;  first  int32 [B]
 *   state_in, state_out  B states of TOC3D_TRACKS_STATE_BYTES(capacity) bytes each; a count read from state_in is clamped to [0, capacity]
 *   track_id, active, order  int32 [B, K];  num_out  int64 [B]
 * Every byte of state_out and of the four outputs is written by this launch, none twice; no memset is ordered against it.
 * TOC3D_ERR_ARG, before any launch: B or K negative, K > 2048, B > 65535; max_age negative; capacity > 8192 or capacity < K * (max_age + 1); a null buffer with
 * B > 0 (rec, score and name may be null when K == 0); num_classes or num_track_labels outside [1, 64]; score_thr not finite; rec, timestamp, state_in or state_out
 * off an 8-byte boundary; state_in and state_out overlapping; a pointer that is not device memory (checked last, with hipPointerGetAttributes). */
int toc3d_tracks_step(const double* rec, const float* score, const int32_t* name, const int64_t* kept, int64_t B, int64_t K, const int32_t* track_label,
                      int64_t num_classes, const float* max_diff, int64_t num_track_labels, double score_thr, int64_t max_age, const double* timestamp,
                      const int32_t* first, const void* state_in, void* state_out, int64_t capacity, int32_t* track_id, int32_t* active, int32_t* order,
                      int64_t* num_out, toc3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TOC3D_TRACKS_H_ */
