/*
 * libtoc3d_gfx950 -- predicted 3-D boxes drawn on the camera views and on a top-down (BEV) panel, on the device.  What the reference shows through
 * tools/visualize.py -> tools/visual_nuscenes.py::render_sample, and the vendored mmdet3d through core/visualizer/image_vis.py:61-126
 * (draw_lidar_bbox3d_on_img -> plot_rect3d_on_img, cv2.line), from the tensors HeadOutputs.get_bboxes holds on the device and the frame's lidar2img, onto the
 * images the frame holds.  Compiled into the same library as include/toc3d.h, whose conventions, error codes and toc3d_stream_t it shares; consumed by
 * toc3d_amd.BoxVis (toc3d_amd/box_vis.py), which encodes the files.
 *
 * Kept beside toc3d.h, with a version of its own, as the other side headers are: TOC3D_ABI_MINOR stays where the tests of the 11.1 surface pin it, and
 * include/toc3d_vis.h keeps its two entry points.  toc3d_amd/lib.py keeps the signatures in a table of its own (_BOXES_SIGS) and binds them at first use: a
 * library built before this header existed lacks the symbols and is told to rebuild.
 *
 * GEOMETRY (float32 on the device; tests/box_vis_cases.py restates it in float64).
 *   A box row is (x, y, z_bottom, dx, dy, dz, yaw, ...).  Its eight corners are those of LiDARInstance3DBoxes.corners (core/bbox/structures/lidar_box3d.py:50-90):
 *   the unit offsets (0,0,0) (0,0,1) (0,1,1) (0,1,0) (1,0,0) (1,0,1) (1,1,1) (1,1,0), minus (0.5, 0.5, 0), times (dx, dy, dz); rotated by yaw about z as
 *   rotation_3d_in_axis does (structures/utils.py:79-106): x' = x cos - y sin, y' = x sin + y cos; plus (x, y, z_bottom).
 *   The twelve edges are image_vis.py:77's: (0,1) (0,3) (0,4) (1,2) (1,5) (3,2) (3,7) (4,5) (4,7) (2,6) (5,6) (6,7).
 *   Camera form: h = proj[v] . (corner, 1); depth h[2]; pixel (h[0] / h[2], h[1] / h[2]).  NEAR PLANE: an edge with both depths < near is dropped; with exactly
 *   one, that end becomes the point of depth `near` on the 3-D edge -- h is interpolated BEFORE the division (image_vis.py:119 clamps the depth to 1e-5 instead,
 *   which smears a box behind the camera across the image).
 *   BEV form: scale = S / (2 range_m) pixels per metre; col = S/2 - y scale, row = S/2 - x scale (ego forward is up, left is left).  Five segments: the footprint
 *   (0,3) (3,7) (7,4) (4,0) and a heading stroke from the box centre to the middle of edge (4,7).
 *   RECTANGLE: a segment (x0, y0, x1, y1) = (col, row, col, row) is clipped to [-guard, W-1+guard] x [-guard, H-1+guard] with Liang-Barsky and dropped when
 *   nothing of it is inside; the ends of a kept segment are then set into the rectangle (fmin / fmax: this absorbs the rounding of the clip's own
 *   interpolation and moves an end by at most that), so segf is bounded by it and segi = (int32) rintf(segf), round half to even, cannot overflow.
 *   NOT DRAWN (cidx = 255, the four coordinates written as 0): score < score_thr; label outside [0, num_colors); a non-finite value in the box's seven columns, in
 *   proj[v], or in the coordinates before or after the rectangle clip.  Nothing else is clamped or dropped.
 *
 * COVERAGE, in integers (so it does not depend on how the work is split).  Pixel (px, py) is covered by segment (x0, y0, x1, y1) at thickness t when, with
 *   d = (x1-x0, y1-y0), p = (px-x0, py-y0), dd = d.d, u = p.d:
 *     dd == 0 or u <= 0:   4 (p.p) <= t^2
 *     u >= dd:             4 (r.r) <= t^2, r = p - d
 *     otherwise:           4 c^2 <= t^2 dd, c = p.x d.y - p.y d.x
 *   (a stroke of width t with round caps).  With H, W <= 8192 and guard <= 16 every first-level product and sum stays below 2^31 and every second-level one below
 *   2^63, so the kernel forms the former in int32 and the latter in int64 and gets what int64 throughout gives.
 *   A covered pixel takes palette[cidx[s]] of the SMALLEST covering segment index s that is drawn: box 0, the highest score, ends on top.
 */
#ifndef TOC3D_BOXES_H_
#define TOC3D_BOXES_H_

#include "toc3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TOC3D_BOXES_ABI 1

#define TOC3D_BOXES_CAMERA_EDGES 12      /* E of toc3d_box_segments */
#define TOC3D_BOXES_BEV_EDGES 5          /* E of toc3d_box_segments_bev */
#define TOC3D_BOXES_MAX_SIDE 8192        /* H, W and the BEV side */
#define TOC3D_BOXES_MAX_GUARD 16
#define TOC3D_BOXES_MAX_THICKNESS 15
#define TOC3D_BOXES_TILE_W 64            /* the pixel tile of one workgroup of toc3d_segments_render */
#define TOC3D_BOXES_TILE_H 16

int toc3d_boxes_abi(void);

/* Boxes -> the segment tables of every camera view, one thread per (view, box), one launch (none when n == 0).
 *   boxes       f32 [n, >= 7], rows box_stride elements apart: (x, y, z_bottom, dx, dy, dz, yaw, ...) as HeadOutputs.get_bboxes returns them
 *   scores      f32 [n];  labels  int64 [n]
 *   proj        f32 [V, 4, 4], contiguous: the frame's lidar2img
 *   thickness   the stroke the tables will be rendered with: only checked against guard (a clipped end's cap must stay outside the image)
 *   segf        f32 [V, n, 12, 4]: (x0, y0, x1, y1);  segi  int32, same shape;  cidx  u8 [V, n, 12]: labels[b], or 255 = not drawn
 * TOC3D_ERR_ARG, before any launch: a null buffer (with n > 0); n < 0; V, H or W <= 0; H or W > 8192; thickness outside [1, 15]; guard outside
 * [(thickness + 1) / 2, 16]; box_stride < 7 (a stride smaller than a row); num_colors outside [1, 254]; V * n beyond a launch's grid (< 2^31 / 12); a pointer
 * that is not device memory (checked last, with hipPointerGetAttributes). */
int toc3d_box_segments(const float* boxes, int64_t box_stride, const float* scores, const int64_t* labels, int64_t n, float score_thr, int64_t num_colors,
                       const float* proj, int64_t V, float near, int64_t H, int64_t W, int64_t guard, int64_t thickness, float* segf, int32_t* segi, uint8_t* cidx,
                       toc3d_stream_t stream);

/* The same for the top-down panel of S x S pixels: V = 1, five segments a box, no matrix.  segf / segi [n, 5, 4], cidx [n, 5].
 * TOC3D_ERR_ARG as above, with S for H and W, and range_m that is not a positive finite number. */
int toc3d_box_segments_bev(const float* boxes, int64_t box_stride, const float* scores, const int64_t* labels, int64_t n, float score_thr, int64_t num_colors,
                           int64_t S, float range_m, int64_t guard, int64_t thickness, float* segf, int32_t* segi, uint8_t* cidx, toc3d_stream_t stream);

/* The pixels, in one launch: every destination pixel is written once, every source pixel read at most once.
 *   src         src_kind 0: f32 NCHW [V, 3, H, W], contiguous: the normalised images (src_stride is not read)
 *               src_kind 1: u8 HWC [V, H, W, 3] raw frames with rows src_stride bytes apart (view v starts at row v*H)
 *               src_kind 2: none (src is not read, NULL allowed): every base pixel is (bg_r, bg_g, bg_b)
 *   mean0..std2, to_rgb   img_norm_cfg by value.  The base byte triple is toc3d_token_vis_render's image byte (include/toc3d_vis.h: float32, two roundings, round
 *               half to even, clip, NaN -> 0; for u8 the source byte of channel to_rgb ? 2 - c : c), and out is always RED FIRST: where to_rgb is 0 the
 *               triple is reversed.  (std is not read for a u8 source; none of them for kind 2.)
 *   segi        int32 [V, nseg, 4];  cidx  u8 [V, nseg].  nseg may be 0 (both may then be NULL): the base only.  Not drawn: cidx[s] >= num_colors (255 among
 *               them), and a segment with an end outside [-guard, W-1+guard] x [-guard, H-1+guard] (toc3d_box_segments makes none; it keeps the integer
 *               products inside their widths whatever table is passed)
 *   palette     u8 [num_colors, 3], RGB
 *   out         u8 [V, H, W, 3], contiguous
 * A workgroup of 256 threads owns a tile of 64 x 16 pixels, a thread four consecutive pixels of a row.  The workgroup walks the view's segments in chunks of
 * 256 staged in LDS: a thread loads one segment, tests its bounding box, grown by (thickness + 1) / 2, against the tile, and each wavefront leaves a 64-bit
 * ballot of the hits; every thread then visits the hits and keeps the smallest covering index in a register.  No atomics, no winner plane, no memset ordered
 * against another launch.  Access widths are chosen on the host from pointers, strides and W; the bytes are the same in every form: out as three dwords where
 * W % 4 == 0 and out is 4-byte aligned, in bytes otherwise; an f32 source as 16-byte loads where W % 4 == 0 and src is 16-byte aligned, a u8 source as three
 * dwords where src and src_stride are multiples of 4 and the four pixels lie inside W; segi in dwords.  Plain vector stores, no inline assembly.
 * TOC3D_ERR_ARG, before any launch: out, palette or (kinds 0, 1) src NULL, segi or cidx NULL with nseg > 0; src_kind outside 0..2; nseg < 0 or >= 2^31 - 256;
 * V, H or W <= 0; H or W > 8192; V > 65535 (a launch's grid); thickness outside [1, 15]; guard outside [(thickness + 1) / 2, 16]; a u8 source with
 * src_stride < 3*W (a stride smaller than a row); an f32 source off a 4-byte boundary, segi off a 4-byte boundary; num_colors outside [1, 254]; a background
 * byte outside [0, 255]; a pointer that is not device memory (checked last). */
int toc3d_segments_render(const void* src, int src_kind, int64_t src_stride, int64_t V, int64_t H, int64_t W, float mean0, float mean1, float mean2,
                          float std0, float std1, float std2, int to_rgb, int bg_r, int bg_g, int bg_b, const int32_t* segi, const uint8_t* cidx, int64_t nseg,
                          const uint8_t* palette, int64_t num_colors, int64_t thickness, int64_t guard, uint8_t* out, toc3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TOC3D_BOXES_H_ */
