/*
 * libtoc3d_gfx950 -- entry points of the head's token side on SAMPLED tokens: the topk_indexes that toc3d_amd.FocalHead returns, consumed by
 * toc3d_amd.HeadTokenEmbedding (compiled into the same library as include/toc3d.h, whose conventions, dtype codes, error codes and toc3d_stream_t they share).
 *
 * Kept beside toc3d.h, with a version of its own, as include/toc3d_streams.h and include/toc3d_focal.h are: TOC3D_ABI_MINOR stays where the tests of the 11.1
 * surface pin it, and at ABI 11.2 this header folds into toc3d.h ("ABI").  toc3d_amd/lib.py keeps the signatures in a table of their own
 * (_SAMPLED_SIGS) and binds them at first use: a library built before this header existed lacks the symbols and is told to rebuild.
 *
 * The reference gathers before any arithmetic (dense_heads/streampetr_head.py:379-422 position_embeding, :627-639 forward; models/utils/misc.py:13-23
 * topk_gather), so its whole token side runs on the K listed rows of a sample instead of its LEN = N*h*w tokens.  An index list is int64 [B, K] on the device;
 * entry j of sample b names token index[b, j] of THAT sample, and output row b*K + j belongs to it.  Lists need not be sorted and may repeat a token.
 *
 * INDEX RANGE: both kernels clamp every index into [0, LEN - 1] before they use it.  Whatever the list holds, nothing outside the source buffers is read and
 * nothing outside rows [0, B*K) of the outputs is written; an index outside the range yields the row of token 0 or LEN - 1, not an error.
 */
#ifndef TOC3D_SAMPLED_H_
#define TOC3D_SAMPLED_H_

#include "toc3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TOC3D_SAMPLED_ABI 1

int toc3d_sampled_abi(void);

/* toc3d_head_frustum_inputs (include/toc3d.h) on the K tokens per sample that `index` [B, K] lists.  Output row b*K + j -- of pos_in [B*K, ld_pos] and
 * cone_act [B*K, ld_cone] in `dtype` (TOC3D_DTYPE_F32, _BF16 or _F32X3P) and of cone f32 [B*K, 8] -- is what the full entry point writes to row b*N*h*w + i for
 * token i = index[b, j]: view b*N + i / (h*w), pixel i % (h*w), and the intrinsics of camera i % N (the reference's repeat order, streampetr_head.py:385-386).
 * The f32 operation sequence is the full entry point's, so the bits are.  Every other argument as there; position_range is a host pointer.
 * TOC3D_ERR_ARG, before any launch: a null buffer, a bad dtype, a non-positive dimension or one beyond 31 bits, depth_num < 30, K <= 0 or K > N*h*w,
 * ld_pos < 3*depth_num, ld_cone < 8, planes rows that do not start on 128-byte boundaries, more rows than one launch's grid holds. */
int toc3d_head_frustum_inputs_sampled(int dtype, const float* img2lidar, const float* intrinsics, const float* coords_d, const float* position_range,
                                      const int64_t* index, int64_t B, int64_t N, int64_t h, int64_t w, int64_t K, int64_t D, int64_t stride, int64_t pad_h,
                                      int64_t pad_w, void* pos_in, int64_t ld_pos, void* cone_act, int64_t ld_cone, float* cone, toc3d_stream_t stream);

/* topk_gather (models/utils/misc.py:13-23) of act rows: dst row b*K + j = src row b*LEN + index[b, j], over the C valid columns, byte for byte, for src
 * [B*LEN, ld_src] and dst [B*K, ld_dst] in `dtype` (TOC3D_DTYPE_F32, _BF16 or _F32X3P; a planes row keeps element c's halves in its 128-byte group c / 32, and
 * exactly those bytes move).  Columns [C, ld_dst) of dst are not written.  One wavefront per row; 16-byte units where C, the leading dimensions and the buffers'
 * alignment allow (C % 4 == 0 for f32, % 8 for bf16 and planes), 2-byte units otherwise.
 * TOC3D_ERR_ARG, before any launch: a null buffer, a bad dtype, B, LEN or C <= 0 (or beyond 31 bits; C > 2^24), K <= 0 or K > LEN, ld_src < C or ld_dst < C,
 * planes rows that do not start on 128-byte boundaries, more rows than one launch's grid holds. */
int toc3d_gather_token_rows(int dtype, const void* src, int64_t ld_src, const int64_t* index, int64_t B, int64_t LEN, int64_t K, int64_t C, void* dst,
                            int64_t ld_dst, toc3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TOC3D_SAMPLED_H_ */
