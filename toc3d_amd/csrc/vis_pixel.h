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

// Four 3-byte pixels as three dwords, the wide form of both kernels.  Byte `at` (0 .. 11) of a group read as d[0 .. 2] ...
TOC3D_DEV uint32_t group_byte(const uint32_t d[3], int at) { return (d[at >> 2] >> (8 * (at & 3))) & 255u; }
// ... and the bytes b[pixel][channel] of a group stored: 12 bytes at a multiple of 12 behind a dword boundary.
TOC3D_DEV void store_group(uint8_t* o, const uint32_t b[4][3]) {
    uint32_t* ow = reinterpret_cast<uint32_t*>(o);
    ow[0] = b[0][0] | b[0][1] << 8 | b[0][2] << 16 | b[1][0] << 24;
    ow[1] = b[1][1] | b[1][2] << 8 | b[2][0] << 16 | b[2][1] << 24;
    ow[2] = b[2][2] | b[3][0] << 8 | b[3][1] << 16 | b[3][2] << 24;
}
