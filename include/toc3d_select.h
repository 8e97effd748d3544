/*
 * libtoc3d_gfx950 -- the entry point of FocalHead's selection-only path: what the detector needs of its 2-D auxiliary head at eval (compiled into the same
 * library as include/toc3d.h, whose conventions, dtype codes, error codes and toc3d_stream_t it shares).
 *
 * Kept beside toc3d.h, with a version of its own, as include/toc3d_streams.h, include/toc3d_focal.h and include/toc3d_sampled.h are: TOC3D_ABI_MINOR stays
 * where the tests of the 11.1 surface pin it, and include/toc3d_focal.h stays the two functions its tests pin.  toc3d_amd/lib.py keeps the signature in a table
 * of its own (_SELECT_SIGS) and binds it at first use: a library built before this header existed lacks the symbol and is told to rebuild.
 *
 * Petr3D.simple_test_pts takes outs_roi['topk_indexes'] from FocalHead and nothing else (detectors/petr3d.py:524-525), and topk_indexes ranks
 * sample_weight = sigmoid(max_c cls) * sigmoid(centerness), which the class tower alone decides (dense_heads/focal_head.py:159-160, 178-180).  The
 * selection-only frame (toc3d_amd.FocalHead.select_rows) is four launches: toc3d_conv3x3_nhwc of shared_cls.0 alone into f32 rows x [V*T, E],
 * toc3d_focal_gn_stats with branches = 1, the entry point below, toc3d_rank_desc.
 */
#ifndef TOC3D_SELECT_H_
#define TOC3D_SELECT_H_

#include "toc3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TOC3D_SELECT_ABI 1

int toc3d_select_abi(void);

/* The class half of toc3d_focal_heads (include/toc3d_focal.h) and nothing else: one pass over the rows of x [V*T, ldx] in `dtype` (TOC3D_DTYPE_F32: the conv's
 * f32 rows; nothing else is served), the class tower in columns [0, E) -- NOTHING from column E on is read, so x may be the class-only conv's [V*T, E] rows or
 * the two-tower buffer with ldx = 2*E.  The GroupNorm affine + ReLU on load from stats f32 [V, 32, 2] = (mean, rstd) per (view, group) (toc3d_focal_gn_stats
 * with branches = 1) and gamma, beta f32 [E]; the num_classes + 1 dot products with w_cls f32 [num_classes + 1, E] (centerness is the last row) plus b_cls
 * [num_classes + 1], as f32 FMA chains from LDS-resident weights; the running maximum over the classes and the two sigmoids:
 * sample_weight f32 [V*T] = sigmoid(max_c cls) * sigmoid(centerness) (focal_head.py:178-180), row m = (view, pixel) -- with views ordered (b, n) the [B, N*h*w]
 * layout toc3d_rank_desc takes.
 * Every element holds the bits toc3d_focal_heads writes to its sample_weight for the same row from the same class-tower columns, statistics and weights: the
 * two kernels share one spelling of the per-row operation sequence (csrc/focal_row.h).
 * TOC3D_ERR_ARG, before any launch: a null buffer, a dtype other than F32, V, T, E or num_classes <= 0, E % 32 != 0 or E > 1024, num_classes > 64,
 * (num_classes + 1) * E floats beyond 64 KB of LDS, ldx < E or not a multiple of 4, misaligned x / gamma / beta / w_cls, too many rows. */
int toc3d_focal_sample_weight(int dtype, const void* x, int64_t ldx, const float* stats, const float* gamma, const float* beta, const float* w_cls,
                              const float* b_cls, int64_t V, int64_t T, int64_t E, int64_t num_classes, float* sample_weight, toc3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TOC3D_SELECT_H_ */
