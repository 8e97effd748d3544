/*
 * libtoc3d_gfx950 -- entry points of the 2-D auxiliary head, FocalHead (compiled into the same library as include/toc3d.h, whose conventions, dtype codes,
 * error codes and toc3d_stream_t they share).
 *
 * Kept beside toc3d.h, with a version of its own, as include/toc3d_streams.h is: TOC3D_ABI_MINOR stays where the tests of the 11.1 surface pin it, and at
 * ABI 11.2 this header folds into toc3d.h ("ABI").  toc3d_amd/lib.py keeps the signatures in a table of their own (_FOCAL_SIGS) and binds them at
 * first use: a library built before this header existed lacks the symbols and is told to rebuild.
 *
 * The frame of FocalHead.forward at eval (dense_heads/focal_head.py:140-193) is four launches.  The two 3x3 convs (shared_cls.0 | shared_reg.0, :123,:128,
 * weights stacked along Cout) are ONE toc3d_conv3x3_nhwc (include/toc3d.h) into f32 rows x [V*T, 2*E]: the class branch in columns [0, E), the box branch in
 * [E, 2*E).  The two entry points below are launches 2 and 3; launch 4 is toc3d_rank_desc on sample_weight.
 */
#ifndef TOC3D_FOCAL_H_
#define TOC3D_FOCAL_H_

#include "toc3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TOC3D_FOCAL_ABI 1

int toc3d_focal_abi(void);

/* The statistics of the two nn.GroupNorm(32, embed_dims) (dense_heads/focal_head.py:124,129 -- shared_reg.1 / shared_cls.1).  x [V*T, ldx] in `dtype`
 * (TOC3D_DTYPE_F32: the conv's f32 rows; nothing else is served), T = h*w pixels per view; columns [0, branches*E) hold `branches` towers of E channels, each
 * normalised in 32 groups of E/32 consecutive channels over the T pixels of one view.  stats f32 [V, branches*32, 2] = (mean, rstd = 1/sqrt(var + eps)) with
 * the biased variance, taken in two passes (the second on x - mean: no cancellation).  Fixed summation order, no atomics: two runs give the same bits.
 * TOC3D_ERR_ARG, before any launch: a null buffer, a dtype other than F32, V, T, E or branches <= 0, E % 32 != 0 or E > 1024, ldx < branches*E, too many views. */
int toc3d_focal_gn_stats(int dtype, const void* x, int64_t ldx, int64_t V, int64_t T, int64_t E, int64_t branches, float eps, float* stats,
                         toc3d_stream_t stream);

/* Everything of FocalHead.forward behind the statistics (dense_heads/focal_head.py:159-180), one pass over the rows of x [V*T, ldx] (as above, two towers):
 * the GroupNorm affine + ReLU on both halves (gamma, beta f32 [2*E]: the class tower's, then the box tower's), the 1x1 convs -- cls | centerness from the class
 * half (w_cls f32 [num_classes + 1, E], b_cls [num_classes + 1]: centerness is the last row), ltrb | center2d from the box half (w_reg f32 [6, E], b_reg [6]) --
 * as f32 FMA chains from LDS-resident weights, then ltrb.sigmoid() and apply_ltrb (models/utils/misc.py:26-43: clamp to [0, 1], xyxy -> cxcywh),
 * apply_center_offset (:45-56: sigmoid(inverse_sigmoid(location) + offset), mmdet's inverse_sigmoid with eps 1e-5) on location f32 [V*T, 2], and
 * sample_weight = sigmoid(max_c cls) * sigmoid(centerness) (focal_head.py:178-180).
 * Outputs, f32, row m = (view, pixel): cls_out [V*T, ld_cls] (num_classes valid columns, the others untouched), bbox_out [V*T, 4], centers_out [V*T, 2],
 * centerness_out [V*T], sample_weight [V*T] -- which, with views ordered (b, n), is the reference's [B, N*h*w] layout.
 * TOC3D_ERR_ARG, before any launch: a null buffer, a dtype other than F32, V, T, E or num_classes <= 0, E % 32 != 0 or E > 1024, num_classes > 57,
 * (num_classes + 7) * E floats beyond 64 KB of LDS, ldx < 2*E or not a multiple of 4, ld_cls < num_classes, misaligned x / gamma / beta / weights, too many rows. */
int toc3d_focal_heads(int dtype, const void* x, int64_t ldx, const float* stats, const float* gamma, const float* beta, const float* w_cls,
                      const float* b_cls, const float* w_reg, const float* b_reg, const float* location, int64_t V, int64_t T, int64_t E,
                      int64_t num_classes, float* cls_out, int64_t ld_cls, float* bbox_out, float* centers_out, float* centerness_out,
                      float* sample_weight, toc3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TOC3D_FOCAL_H_ */
