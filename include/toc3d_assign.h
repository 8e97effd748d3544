/*
 * libtoc3d_gfx950 -- the tracking step with the reference's hungarian=True: nusc_tracking/pub_tracker.py:27 (`hungarian=False, max_age=0`), :127-129 and :143-150,
 * exposed by nusc_tracking/pub_test.py:28,81 as --hungarian.  There the N x M float64 matrix goes to scipy.optimize.linear_sum_assignment; here one launch does the
 * step for every camera stream with that solver REPLAYED, operation for operation, by one workgroup a stream: the matrix is never materialised and the solver's
 * state stays in LDS.  The companion of include/toc3d_tracks.h (the greedy step), whose state layout, inputs, outputs, constants and conventions it shares; consumed
 * by toc3d_amd.HungarianPubTracker (toc3d_amd/tracking.py), which toc3d_amd.build_tracker(hungarian=True) returns.
 *
 * Kept beside toc3d.h, with a version of its own, as the other side headers are; toc3d_amd/lib.py keeps the signatures in a table of its own (_ASSIGN_SIGS).
 *
 * WHY A REPLAY.  Under hungarian=True the reference's result is defined by the float64 arithmetic of scipy's solver on the matrix :119-129 builds: an invalid pair
 * costs exactly 1e18, a valid one its float32 distance, 2.5 at most.  Float64 values near 1e18 are 128 apart, so once a dual variable reaches that size the small
 * costs are absorbed, and the solver returns valid matches an exact optimum would not (on 607 of 3000 seeded tracker-shaped matrices, against the same solver with
 * 1e4 for an invalid pair).  Which detections end on which tracks is then the solver's arithmetic and tie-breaking, and both are reproduced.
 *
 * THE STEP, per stream b.  Points 0-3 and 6 are those of include/toc3d_tracks.h, unchanged (the state read or reset, the filter, the float32 positions, the
 * once-rounded float32 distance and its validity, the empty-frame quirk).  Points 4 and 5 become:
 *   4h. cost[i][j] = valid(i, j) ? (double)d : 1e18 (:126-128: d + invalid * 1e18, clamped at 1e18).  With N > 0 and M > 0 the N x M problem is solved as scipy
 *       solves it (THE SOLVER below): every one of min(N, M) rows is matched, many of them to a 1e18 entry.  matched_indices is sorted by detection.
 *   5h. the new state, in this order: (1) the matches with cost <= 1e16 in detection order (:145-149; id and active + 1 from the track); (2) the detections in no
 *       match, in detection order; (3) the detections in a match with cost > 1e16, in detection order (:147 appends them behind the others); groups 2 and 3 together
 *       take tracking_id = ++id_count in that sequence (:162-168); (4) the tracks IN NO MATCH AT ALL with age < max_age, in track order (:140, :172-183).
 *   QUIRK A, reproduced: a track in an invalid match is in matched_indices[:, 1], so :140 does not list it and nothing adds it again: it is dropped at once,
 *       whatever its age.  With N >= M that is every track without a valid match.
 *   QUIRK B, reproduced: with N > M the detections the solver parks on tracks at 1e18 get their new ids after the unmatched ones.
 * OUTPUTS: track_id, active, order and num_out as toc3d_tracks_step writes them (order: groups 1, 2, 3), and rounds[b]: the scan rounds the solver made for the
 * stream (0 when N == 0 or M == 0) -- a witness that the same path was walked, and the unit the kernel's time is read in.
 * DIFFERENCES to the reference: those of include/toc3d_tracks.h, (a) read for this path: a distance that is NaN is an invalid pair (cost 1e18), where the reference
 * would raise inside scipy ("matrix contains invalid numeric entries").
 *
 * THE SOLVER (scipy/optimize/rectangular_lsap: the shortest augmenting path of Crouse's rectangular algorithm), restated.  nr x nc is the matrix: if N > M it is
 * transposed (rows are tracks, columns detections; the result is mapped back and sorted by detection), otherwise rows are detections.
 *   u[nr] = v[nc] = 0.0; col4row[nr] = row4col[nc] = -1.  For cur = 0 .. nr - 1:
 *     minVal = 0.0, i = cur; remaining = [nc - 1, nc - 2, ..., 0], nrem = nc; SR, SC cleared; spc[nc] = +inf.  Repeat until a sink is found:
 *       SR[i] = true.  For it = 0 .. nrem - 1 in list order, j = remaining[it]:  r = ((minVal + cost[i][j]) - u[i]) - v[j] in float64, each operation rounded once, in
 *       that order; if r < spc[j]: path[j] = i, spc[j] = r.  The pick is the position with the smallest spc[j]; among equal smallest values the LAST position in list
 *       order whose column is unassigned (row4col[j] == -1), and if none is unassigned the FIRST position.
 *       minVal = spc of the pick, j = remaining[pick].  If row4col[j] == -1 then sink = j, else i = row4col[j].  SC[j] = true; remaining[pick] = remaining[--nrem]
 *       (the list order changes by this move, and the tie rule reads it).
 *     duals: u[cur] += minVal; for every i != cur with SR[i]: u[i] += minVal - spc[col4row[i]]; for every j with SC[j]: v[j] -= minVal - spc[j].
 *     augment: j = sink; repeat i = path[j]; row4col[j] = i; swap(col4row[i], j) until i == cur.
 *   Every cost is finite, so minVal is never infinite and a row's search takes at most cur + 1 rounds: every loop of the kernel has that bound.
 *
 * One workgroup of 256 threads (four wavefronts, one per SIMD) per stream.  spc, v, path, row4col and remaining are kept per column in LDS, u and col4row per row;
 * a cost is computed where it is read, from the float32 positions, labels and gates compacted in LDS.  A round is: each thread walks its list positions; the pick is
 * a lexicographic minimum over (the order-preserving image of spc -- sign-aware: spc can come out slightly negative --, unassigned first, position descending if
 * unassigned and ascending if not), inside a wavefront by DPP moves and permlane swaps and across the four through LDS behind ONE barrier; every thread then does
 * the round's bookkeeping in registers and the thread that owns the picked position moves the list's last entry into it.  SR and SC are not stored: the columns of
 * SC are the list's tail, the rows of SR their row4col.  Nothing depends on scheduling; plain vector stores, no inline assembly.
 */
#ifndef TOC3D_ASSIGN_H_
#define TOC3D_ASSIGN_H_

#include "toc3d_tracks.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TOC3D_ASSIGN_ABI 1

#define TOC3D_ASSIGN_MAX_BOXES 512       /* K: holds the shipped max_num 300; bounds the rounds of a stream at 512 * 513 / 2 */
#define TOC3D_ASSIGN_MAX_TRACKS 2048     /* capacity: 300 boxes at max_age 3 need 1200; bounds the per-column state at 64 KiB of LDS */

int toc3d_assign_abi(void);

/* toc3d_tracks_step (include/toc3d_tracks.h) with points 4h and 5h: the same arguments, the same state layout, the same outputs, and
 *   rounds  int32 [B]
 * Every byte of state_out and of the five outputs is written by this launch, none twice; no memset is ordered against it.
 * TOC3D_ERR_ARG, before any launch: K > 512 or capacity > 2048 (larger problems are not solved here); every other refusal of toc3d_tracks_step, rounds null with
 * B > 0 or not device memory among them. */
int toc3d_tracks_step_hungarian(const double* rec, const float* score, const int32_t* name, const int64_t* kept, int64_t B, int64_t K, const int32_t* track_label,
                                int64_t num_classes, const float* max_diff, int64_t num_track_labels, double score_thr, int64_t max_age, const double* timestamp,
                                const int32_t* first, const void* state_in, void* state_out, int64_t capacity, int32_t* track_id, int32_t* active, int32_t* order,
                                int64_t* num_out, int32_t* rounds, toc3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TOC3D_ASSIGN_H_ */
