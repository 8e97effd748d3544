/*
 * libtoc3d_gfx950 -- camera ingest: the resize and crop of raw uint8 camera frames that the reference's test pipeline does on the host with Pillow
 * (ResizeCropFlipRotImage(training=False), datasets/pipelines/transform_3d.py:108-172, :247-298: Image.resize(resize_dims), Image.crop(crop)), with Pillow's
 * bytes.  Compiled into the same library as include/toc3d.h, whose conventions, error codes and toc3d_stream_t it shares; consumed by
 * toc3d_amd.ResizeCropFlipRotImage (toc3d_amd/preprocess.py), which builds the tables.
 *
 * Kept beside toc3d.h, with a version of its own, as include/toc3d_streams.h, toc3d_focal.h, toc3d_sampled.h and toc3d_select.h are: TOC3D_ABI_MINOR stays where
 * the tests of the 11.1 surface pin it.  toc3d_amd/lib.py keeps the signature in a table of its own (_INGEST_SIGS) and binds it at first use: a library built
 * before this header existed lacks the symbol and is told to rebuild.
 *
 * THE ARITHMETIC is Pillow's ImagingResample for 8-bit data (src/libImaging/Resample.c): two separable passes over integer coefficients (the double-precision
 * filter weights times 2^22, rounded half away from zero -- the host's table), each
 *     acc = 2^21 + sum over taps (pixel * k)      in 32-bit integers
 *     byte = clamp(acc >> 22, 0, 255)             arithmetic shift
 * per channel.  The horizontal pass runs first and is ROUNDED TO uint8; the vertical pass reads those bytes.  That rounding is part of Pillow's result.
 * Coefficients lie within signed 24 bits (a resampling table's are at most 2^22 up to rounding; the host asserts it) and are multiplied as such: of any other
 * value the low 24 bits count.
 *
 * TABLES, per axis, int32 on the device, already restricted to the cropped output range: coef [n_out, ksize] and bounds [n_out, 2] = (first source index, tap
 * count) for each output column (row).  Output column x is sum_k coef_h[x, k] * source column (bounds_h[x, 0] + k), k < bounds_h[x, 1].
 *
 * INDEX RANGE: every source index is clamped into the image, every tap count into [0, ksize] (along a row also to the taps that lie in the image: the rest
 * are dropped), every row of the intermediate into the rows the workgroup holds.  Whatever a table holds, nothing outside the V*H0 source rows (3*W0 bytes
 * of each) is read and nothing outside the 3*fW bytes of the V*fH destination rows is written; a table that is not a resampling table yields wrong bytes, not
 * an error.
 */
#ifndef TOC3D_INGEST_H_
#define TOC3D_INGEST_H_

#include "toc3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TOC3D_INGEST_ABI 1

/* the kernel's tile and its LDS budget (fixed here; a launch allocates what its max_span and ksizes need of it): a workgroup owns TILE_W x TILE_H output
 * pixels and keeps at most LDS_ROWS rows of the intermediate (TILE_W pixels of 3 bytes each) and MAX_KSIZE coefficients per output column and row in LDS */
#define TOC3D_INGEST_TILE_W 64
#define TOC3D_INGEST_TILE_H 32
#define TOC3D_INGEST_LDS_ROWS 168
#define TOC3D_INGEST_MAX_KSIZE 32

int toc3d_ingest_abi(void);

/* src uint8 HWC [V, H0, W0, 3] with rows src_stride bytes apart (view v starts at row v*H0) -> dst uint8 HWC [V, fH, fW, 3] with rows dst_stride bytes apart,
 * in one launch: workgroup (tx, ty, v) owns output columns [64 tx, 64 tx + 64) of rows [32 ty, 32 ty + 32) of view v.  It stages its slices of the four tables
 * in LDS (one barrier), writes the horizontal pass of the source rows its vertical taps span (first row: bounds_v[32 ty, 0]; one past the last: bounds_v + count of the
 * tile's last row) into LDS as bytes, synchronises, and finishes the tile with the vertical pass.  No atomics, no inline assembly, plain stores; bytes
 * [3*fW, dst_stride) of a destination row are not written.  max_span: the largest number of source rows a tile's vertical taps span (the host computes it from
 * bounds_v for TILE_H); a tile never holds more rows than that.  Access widths are chosen on the host from pointers and strides: the source is read as
 * aligned 4-byte units where src, src_stride and 3*W0 are multiples of 4 and ksize_h is 1, 5, 7, 9 or 11 (a thread reads the dwords that hold its taps' bytes),
 * one byte at a time otherwise; the destination is stored in 4-byte units where dst and dst_stride are multiples of 4, in bytes otherwise.  The same bytes in
 * every form.
 * TOC3D_ERR_ARG, before any launch: a null buffer; V, H0, W0, fH or fW <= 0 or beyond 31 bits (V and the tile counts beyond a launch's grid); a stride smaller
 * than a row (src_stride < 3*W0, dst_stride < 3*fW); ksize_h or ksize_v outside [1, TOC3D_INGEST_MAX_KSIZE]; max_span outside [1, TOC3D_INGEST_LDS_ROWS]; a
 * pointer that is not device memory (checked last, with hipPointerGetAttributes). */
int toc3d_resize_crop_u8(const uint8_t* src, int64_t src_stride, int64_t V, int64_t H0, int64_t W0, uint8_t* dst, int64_t dst_stride, int64_t fH, int64_t fW,
                         const int32_t* coef_h, const int32_t* bounds_h, int64_t ksize_h, const int32_t* coef_v, const int32_t* bounds_v, int64_t ksize_v,
                         int64_t max_span, toc3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TOC3D_INGEST_H_ */
