/*
 * libtoc3d_gfx950 -- token selection overlays: the images the reference's token_selection_vis (models/utils/token_select_vis.py:27-80, called by
 * Petr3D.simple_test at detectors/petr3d.py:562-579 when token_select_vis=True) makes on the host -- the denormalised camera image, and per selection stage the
 * same image with an alpha plane that shows which tokens the stage kept -- made on the device, as the uint8 arrays cv2.imwrite turns the reference's float32
 * arrays into.  Compiled into the same library as include/toc3d.h, whose conventions, error codes and toc3d_stream_t it shares; consumed by toc3d_amd.TokenVis
 * (toc3d_amd/token_vis.py), which encodes the files.
 *
 * Kept beside toc3d.h, with a version of its own, as include/toc3d_streams.h, toc3d_focal.h, toc3d_sampled.h, toc3d_select.h and toc3d_ingest.h are:
 * TOC3D_ABI_MINOR stays where the tests of the 11.1 surface pin it.  toc3d_amd/lib.py keeps the signatures in a table of its own (_VIS_SIGS) and binds them at
 * first use: a library built before this header existed lacks the symbols and is told to rebuild.
 *
 * THE ARITHMETIC is the reference's float32 numpy arithmetic followed by OpenCV's saturate_cast<uchar> (round half to even, as np.rint; then clipped to
 * [0, 255]; a NaN gives 0 here).  Every product and every sum below is rounded to float32 on its own: two roundings, no FMA contraction.
 *     alpha byte of a token:   rint(f32(255) * f32(f32(m * span) + lo))        lo = f32(min_alpha), span = f32(max_alpha - min_alpha), the difference formed in
 *                                                                               double as Python forms it; m: the mask value, or 0 / 1 membership in the keep list
 *     image byte, f32 source:  rint(f32(f32(x * std[c]) + mean[c]))             array channel c of pixel x: mmcv.imdenormalize(to_bgr=False), restated in numpy
 *     image byte, u8 source:   the source byte of channel (to_rgb ? 2 - c : c); outside the H0 x W0 source, up to the padded H x W: rint(mean[c]), which is what
 *                              the reference gets from a zero-padded normalised image
 * With the defaults (0.3, 1.0) a dropped token is 76, not 77: f32(255 * 0.3f) is exactly 76.5, which rounds half to even.  A kept token is 255.
 */
#ifndef TOC3D_VIS_H_
#define TOC3D_VIS_H_

#include "toc3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TOC3D_VIS_ABI 1

/* the most tokens of one view (T = (H / patch) * (W / patch)): toc3d_token_alpha keeps one byte per token of a view in LDS.  5000 at 1600 x 800. */
#define TOC3D_VIS_MAX_TOKENS 8192

int toc3d_vis_abi(void);

/* One selection stage's mask and keep list -> two alpha planes, one byte per token, in one launch of V workgroups.
 *   mask        f32 [V*T]: the backbone's (V, hp, wp, 1) token mask of the stage
 *   keep        int64 [V, K], rows keep_stride elements apart: the token indices the stage kept.  K may be 0 (keep may then be NULL)
 *   alpha_mask  u8 [V*T]: the byte of mask[i]
 *   alpha_keep  u8 [V*T]: the byte of 1 where the token is in its view's keep row, of 0 elsewhere.  NULL: not made (keep is not read)
 * Workgroup v keeps a T-byte membership table in LDS: clear, barrier, scatter, barrier, write out -- no atomics, no memset ordered against another launch.  An
 * index outside [0, T) is ignored (the reference asserts there is none; a negative one does not wrap here), so nothing is written out of range; a duplicate
 * is harmless.  min_alpha and max_alpha arrive as doubles so that span is formed as Python forms it.
 * TOC3D_ERR_ARG, before any launch: mask or alpha_mask NULL; keep NULL with alpha_keep given and K > 0; V or T <= 0, V beyond a launch's grid, K < 0;
 * T > TOC3D_VIS_MAX_TOKENS; keep_stride < K (a stride smaller than a row); a pointer that is not device memory (checked last, with
 * hipPointerGetAttributes). */
int toc3d_token_alpha(const float* mask, const int64_t* keep, int64_t keep_stride, int64_t K, int64_t V, int64_t T, double min_alpha, double max_alpha,
                      uint8_t* alpha_mask, uint8_t* alpha_keep, toc3d_stream_t stream);

/* The pixels of every plane, in one launch; each source pixel is read once.
 *   src         src_u8 == 0: f32 NCHW [V, 3, H, W], contiguous: the normalised images (H0 == H and W0 == W are required; src_stride and to_rgb are not read)
 *               src_u8 != 0: u8 HWC [V, H0, W0, 3] raw frames with rows src_stride bytes apart (view v starts at row v*H0), H0 <= H, W0 <= W
 *   alpha       u8 [A, V, (H/patch)*(W/patch)]: A planes of token alphas (toc3d_token_alpha's outputs)
 *   mean0..std2 the three means and standard deviations of img_norm_cfg, by value (std is not read for a u8 source)
 *   ori         u8 [V, H, W, 3]:     ori[v, y, x, c] = image byte c
 *   rgba        u8 [A, V, H, W, 4]:  rgba[a, v, y, x] = (image byte 0, 1, 2, alpha[a, v, (y/patch)*(W/patch) + x/patch])
 * Access widths are chosen on the host from pointers, strides and W; the bytes are the same in every form.  Wide form (W % 4 == 0, rgba 16-byte aligned, ori
 * 4-byte aligned): a thread owns four pixels of a row, stores 16 bytes per plane and three dwords of ori; it reads an f32 source as three 16-byte loads where
 * src is 16-byte aligned, a u8 source as three dwords where src and src_stride are multiples of 4 and its four pixels lie inside W0, in single elements
 * otherwise.  Narrow form: a thread owns one pixel; rgba is stored as one dword per plane where it is 4-byte aligned, in bytes otherwise; ori in bytes.  No
 * atomics, no inline assembly, plain vector stores.
 * TOC3D_ERR_ARG, before any launch: a null buffer; A, V, H0, W0, H, W or patch <= 0; H or W not a multiple of patch; H0 > H or W0 > W (an f32 source: H0 != H
 * or W0 != W); (H/patch)*(W/patch) > TOC3D_VIS_MAX_TOKENS; V, or H * W, beyond a launch's grid (V <= 65535, H * W < 2^31); a u8 source with
 * src_stride < 3*W0 (a stride smaller than a row); an f32 source off a 4-byte boundary; a pointer that is not device memory (checked last). */
int toc3d_token_vis_render(const void* src, int src_u8, int64_t src_stride, int64_t V, int64_t H0, int64_t W0, int64_t H, int64_t W, int64_t patch,
                           const uint8_t* alpha, int64_t A, float mean0, float mean1, float mean2, float std0, float std1, float std2, int to_rgb,
                           uint8_t* ori, uint8_t* rgba, toc3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TOC3D_VIS_H_ */
