/*
 * libtoc3d_gfx950 -- decoded boxes to nuScenes submission records in the global frame, on the device.  What the reference's --eval and its submission files read
 * is made on the host by the vendored mmdet3d: mmdet3d/datasets/nuscenes_dataset.py:301-368 (_format_bbox), :576-619 (output_to_nusc_box) and :622-657
 * (lidar_nusc_box_to_global), with the class ranges clamped by projects/mmdet3d_plugin/datasets/nuscenes_dataset.py:56-58 (max_depth): a Python loop that builds
 * one pyquaternion object and one NuScenesBox per detection.  Here one launch does it for every sample of a step, from the fixed-capacity tensors
 * NMSFreeCoder.decode_fixed leaves on the device.  Compiled into the same library as include/toc3d.h, whose conventions, error codes and toc3d_stream_t it shares;
 * consumed by toc3d_amd.NuScenesResults (toc3d_amd/nusc_results.py), which names the classes and attributes and writes the JSON.
 *
 * Kept beside toc3d.h, with a version of its own, as the other side headers are: TOC3D_ABI_MINOR stays where the tests of the 11.1 surface pin it.
 * toc3d_amd/lib.py keeps the signature in a table of its own (_RESULTS_SIGS) and binds it at first use: a library built before this header existed lacks the
 * symbols and is told to rebuild.
 *
 * PER BOX, in float64 except where noted, each operation rounded once in the order written (the kernel is compiled without contraction into fused multiply-adds):
 *   1. gravity centre: zg = z_bottom + dz * 0.5f, formed in float32 and then promoted (core/bbox/structures/lidar_box3d.py:41-47 forms it in torch float32);
 *      x, y, dx, dy, dz, yaw, vx, vy are promoted from float32.
 *   2. size (w, l, h) = (dy, dx, dz): columns [4, 3, 5] (:598).
 *   3. orientation q0 = (cos(yaw / 2), 0, 0, sin(yaw / 2)), the yaw promoted to float64 BEFORE it is halved: what pyquaternion.Quaternion(axis=[0, 0, 1],
 *      radians=np.float32) computes under NumPy 1.x promotion (float32 scalar / Python float -> float64), which mmdet3d 1.0.0rc6 runs on.  (NumPy 2 keeps such a
 *      quotient in float32; the records here do not follow that.)
 *   4. to ego, with the pose (q1, t1), q = (w, x, y, z) a unit quaternion:
 *        R = [1 - 2 (yy + zz), 2 (xy - wz), 2 (xz + wy);  2 (xy + wz), 1 - 2 (xx + zz), 2 (yz - wx);  2 (xz - wy), 2 (yz + wx), 1 - 2 (xx + yy)]
 *      (the identity quaternion gives exactly I);  c = R c + t, each row ((R0 c0 + R1 c1) + R2 c2) + t;  q = q1 (x) q0, the Hamilton product with the pose on the
 *      left, as Box.rotate does;  v = R (vx, vy, 0).
 *   5. range filter: radius = sqrt(cx cx + cy cy) in the ego frame; the box is dropped when radius > class_range[label] (:648-652).
 *   6. to global: step 4 with (q2, t2).
 *   7. attribute: sqrt(vx vx + vy vy) > speed_thr on the GLOBAL velocity chooses attr_moving[label], otherwise attr_still[label] (:327-346).
 * DIFFERENCES to the reference: (a) the float64 rounding order above (pyquaternion normalises the pose again and forms R as a product of two 4 x 4 matrices);
 * (b) DROPPED, where the reference would raise or write NaN into the JSON: a box whose label is outside [0, num_classes), or with a value that is not finite among
 * its used columns (seven, nine with the velocity), in its float32 gravity centre or in its score; (c) the NumPy 1.x promotion of the yaw stated in step 3.
 */
#ifndef TOC3D_RESULTS_H_
#define TOC3D_RESULTS_H_

#include "toc3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TOC3D_RESULTS_ABI 1

#define TOC3D_RESULTS_MAX_BOXES 2048     /* K: the decoder's own cap (DECODE_MAX_NUM) */
#define TOC3D_RESULTS_MAX_CLASSES 64
#define TOC3D_RESULTS_REC 12             /* doubles a record: translation 3, size 3, rotation 4 (w, x, y, z), velocity 2 */

int toc3d_results_abi(void);

/* One launch for all B samples (none when B == 0 or K == 0: nothing is then written, kept included).  Every buffer is device memory.
 *   boxes         f32 [B, K, >= 7]: rows box_stride elements apart, samples sample_stride elements apart; columns (x, y, z_bottom, dx, dy, dz, yaw[, vx, vy]) as
 *                 decode_fixed(..., sub_half_height=True) leaves them
 *   scores        f32 [B, K];  labels  int64 [B, K], both contiguous
 *   counts        int64 [B]: rows at or beyond counts[b] are not read (a count below 0 is taken as 0, one above K as K)
 *   with_velocity 0: the velocity is (0, 0, 0) and columns 7, 8 are not read;  1: box_stride >= 9
 *   poses         f64 [B, 2, 7]: per sample lidar -> ego, then ego -> global, each (w, x, y, z, tx, ty, tz); the host normalises the quaternions
 *   class_range   f64 [num_classes];  attr_moving, attr_still  int32 [num_classes], -1 = the empty attribute
 *   speed_thr     0.2 in the reference
 *   rec           f64 [B, K, 12];  score  f32 [B, K];  name  int32 [B, K] (the label);  attr  int32 [B, K];  src  int32 [B, K] (the input row);  kept  int64 [B]
 * Kept boxes are compacted stably (input order, descending score, is preserved); every row at or beyond kept[b] is written as zeros with name, attr and src -1.
 * Every output byte is written by this launch, none twice; no memset is ordered against it.
 * One workgroup of 256 threads per sample walks its K rows in chunks of 256, a thread per box; each wavefront leaves a 64-bit ballot of its keep flags, the
 * per-wave counts are prefix-summed through LDS onto a base carried across the chunks, and the tail is zeroed from the final base.  No atomics: the result does
 * not depend on scheduling.  Plain vector stores, no inline assembly.
 * TOC3D_ERR_ARG, before any launch: B or K negative, K > 2048, B > 65535; a null buffer with B * K > 0; box_stride < 7 (9 with the velocity: a stride smaller than
 * a row); sample_stride < K * box_stride; num_classes outside [1, 64]; speed_thr not finite; boxes off a 4-byte boundary; rec or poses off an 8-byte boundary;
 * a pointer that is not device memory (checked last, with hipPointerGetAttributes). */
int toc3d_boxes_to_global(const float* boxes, int64_t box_stride, int64_t sample_stride, const float* scores, const int64_t* labels, const int64_t* counts,
                          int64_t B, int64_t K, int with_velocity, const double* poses, const double* class_range, const int32_t* attr_moving,
                          const int32_t* attr_still, int64_t num_classes, double speed_thr, double* rec, float* score, int32_t* name, int32_t* attr, int32_t* src,
                          int64_t* kept, toc3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TOC3D_RESULTS_H_ */
