// The image byte that the two visualisations share: toc3d_token_vis_render (token_vis.hip: ori and the RGBA planes) and toc3d_segments_render (box_vis.hip:
// the base of every pixel no segment covers).  ONE spelling of the float32 sequence -- a product rounded, a sum rounded, round half to even, clip -- so that
// the base bytes of the box overlays are TokenVis's bytes.
#pragma once
#include "common.h"

// OpenCV's saturate_cast<uchar>(float): round half to even, clip.  (fmaxf returns its other operand for a NaN: 0.)
TOC3D_DEV uint32_t sat_u8(float v) { return (uint32_t)(int)fminf(fmaxf(rintf(v), 0.f), 255.f); }
// x * s, rounded, then + m, rounded.  The pragma is what keeps the two apart: hipcc contracts by default, and it fuses __fadd_rn(__fmul_rn(x, s), m) as well
// (seen in token_vis.hip's assembly: v_fma_f32).  The assembly of the kernels that use it holds v_mul_f32 and v_add_f32 and no v_fma_f32 / v_fmac_f32 on floats.
TOC3D_DEV float mul_then_add(float x, float s, float m) {
#pragma clang fp contract(off)
    const float p = x * s;
    return p + m;
}
TOC3D_DEV uint32_t denorm_byte(float x, float sd, float mu) { return sat_u8(mul_then_add(x, sd, mu)); }
