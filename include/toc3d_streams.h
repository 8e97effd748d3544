/*
 * libtoc3d_gfx950 -- entry points for stepping several camera streams per forward (compiled into the same library as include/toc3d.h, whose
 * conventions, dtype codes, error codes and toc3d_stream_t they share).
 *
 * Kept beside toc3d.h, with a version of its own, so that TOC3D_ABI_MINOR stays where the tests of the 11.1 surface pin it; at ABI 11.2 this header
 * folds into toc3d.h ("ABI").  toc3d_amd/lib.py keeps the signatures in a table of their own (_STREAMS_SIGS) and binds them at first use:
 * a library built before this header existed lacks the symbols and is told to rebuild.
 */
#ifndef TOC3D_STREAMS_H_
#define TOC3D_STREAMS_H_

#include "toc3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TOC3D_STREAMS_ABI 1

int toc3d_streams_abi(void);

/* A step in which some frames of the batch start a scene while the others continue (backbones/toc3d_utils.py:110-129 is the scorer of a frame that
 * starts one, ScoreBasedTokenSelector.score; :255-273 the query-guided scorer of a frame that continues, which chooses between the two with ONE
 * prev_exists for the whole batch).  toc3d_score_head_frames is toc3d_score_head for the rows of the flagged frames only: row r belongs to frame
 * r / rows_per_frame; for frames with frame_new[frame] != 0 it writes pred, score and mask_out with exactly the bits toc3d_score_head writes for that
 * row; the rows of every other frame are neither read nor written -- they keep what toc3d_score_tokens put there.  frame_new f32 [M / rows_per_frame]
 * lives in DEVICE memory, so one recorded launch serves every pattern of new frames.  gumbel, dtypes (BF16, F32), alignment and the 32-bit count limits
 * as toc3d_score_head.  TOC3D_ERR_ARG, before any launch: a null buffer, rows_per_frame <= 0, M % rows_per_frame != 0, a bad dtype, ld or kdim. */
int toc3d_score_head_frames(int dtype, const void* f, int64_t ld, int64_t kdim, const float* w, const float* b, const float* gumbel,
                            const float* frame_new, int64_t rows_per_frame, int64_t M, float* pred, float* score, float* mask_out,
                            toc3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TOC3D_STREAMS_H_ */
