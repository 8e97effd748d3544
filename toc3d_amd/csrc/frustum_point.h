// The per-(token, depth bin) body of the head's frustum kernels: toc3d_head_frustum_inputs (head_tokens.hip: every token of every view) and
// toc3d_head_frustum_inputs_sampled (head_tokens_sampled.hip: the tokens an index list names).  ONE spelling of the f32 operation sequence -- every product, sum
// and quotient is a __f*_rn intrinsic, so nothing contracts or reassociates -- which is why a sampled row holds the bits of the full kernel's row.
#pragma once
#include "act_rows.h"

struct FrustumArgs {
    const float* img2lidar;     // [B*N, 16] inverse of lidar2img
    const float* intrinsics;    // [B*N, 16]
    const float* coords_d;      // [D]
    float pr[6];                // position_range
    int B, N, h, w, D, stride, pad_h, pad_w;
};

// Depth bin d of the token at pixel `pix` of view `view` (= b*N + n), which is token `tok_in_b` (= n*hw + pix) of its sample; written to row `row` of the outputs.
// The 3-D point of the pixel centre at that depth through lidar2img^-1 (dense_heads/streampetr_head.py:391-413)
template <typename T>
TOC3D_DEV void frustum_point(const FrustumArgs& a, int view, int pix, int tok_in_b, int d, int64_t row, T* __restrict__ pin, int64_t ld_pin,
                             T* __restrict__ cone_act, int64_t ld_cone, float* __restrict__ cone) {
    const int y = pix / a.w, x = pix % a.w;
    // locations() (misc.py:70-77) then * pad (streampetr_head.py:392-393), as the reference rounds them
    const float cx = __fmul_rn(__fdiv_rn((float)(x * a.stride + a.stride / 2), (float)a.pad_w), (float)a.pad_w);
    const float cy = __fmul_rn(__fdiv_rn((float)(y * a.stride + a.stride / 2), (float)a.pad_h), (float)a.pad_h);
    const float dep = a.coords_d[d];
    const float sc = fmaxf(dep, 1e-5f);
    const float c0 = __fmul_rn(cx, sc), c1 = __fmul_rn(cy, sc);
    const float* M = a.img2lidar + (int64_t)view * 16;
    float p[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float s = __fmul_rn(M[i * 4], c0);
        s = __fadd_rn(s, __fmul_rn(M[i * 4 + 1], c1));
        s = __fadd_rn(s, __fmul_rn(M[i * 4 + 2], dep));
        s = __fadd_rn(s, M[i * 4 + 3]);
        p[i] = __fdiv_rn(__fsub_rn(s, a.pr[i]), __fsub_rn(a.pr[3 + i], a.pr[i]));
    }
    T* dst = pin + row * ld_pin + d * 3;
    put1(dst, inverse_sigmoid(p[0]));
    put1(dst + 1, inverse_sigmoid(p[1]));
    put1(dst + 2, inverse_sigmoid(p[2]));
    // cone (:419-420): [|fx|, |fy|] / 1e3 of camera (token index % N) -- the reference's repeat order (:385-386) --, then the points
    // of the last depth bin and of bin D - 30
    float* cr = cone + row * 8;
    T* ca = cone_act + row * ld_cone;
    if (d == a.D - 1 || d == a.D - 30) {
        const int o = d == a.D - 1 ? 2 : 5;
#pragma unroll
        for (int i = 0; i < 3; ++i) { cr[o + i] = p[i]; put1(ca + o + i, p[i]); }
    }
    if (d == 0) {
        const int b = view / a.N;
        const float* K = a.intrinsics + (int64_t)(b * a.N + tok_in_b % a.N) * 16;
        const float fx = __fdiv_rn(fabsf(K[0]), 1e3f), fy = __fdiv_rn(fabsf(K[5]), 1e3f);
        cr[0] = fx; cr[1] = fy;
        put1(ca, fx); put1(ca + 1, fy);
    }
}

// an act output [rows, ld] of an entry point that also takes TOC3D_DTYPE_F32X3P: planes rows are whole 128-byte groups on 128-byte boundaries (the refusal of
// toc3d_head_query_inputs); the other dtypes keep their checks
#define TOC3D_PLANES_ROWS(fn, what, act, ld)                                                                                                           \
    TOC3D_REQUIRE(dtype != TOC3D_F32X3P || planes_rows_ok(act, ld), fn ": " what ": rows of (hi, lo) planes start on 128-byte boundaries (buffer aligned, leading dimension a multiple of 32)")
