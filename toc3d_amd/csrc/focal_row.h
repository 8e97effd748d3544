// The per-row body that FocalHead's two row kernels share: toc3d_focal_heads (focal_head.hip: both towers, every output) and toc3d_focal_sample_weight
// (focal_select.hip: the class tower and sample_weight alone).  ONE spelling of the f32 operation sequence -- the GroupNorm affine is __f*_rn intrinsics, so it
// contracts the same way wherever it is inlined; the dot products are explicit fmaf chains in one lane order behind one wave_sum; the product of the two
// sigmoids is __fmul_rn -- which is why the selection kernel's sample_weight holds the bits of the full kernel's.
#pragma once
#include "act_rows.h"

constexpr int FH_ROWS = 32;                              // pixel rows per workgroup of both kernels (4 wavefronts x 8), all of one view

// one wavefront per row; a lane owns the 4 consecutive columns 4 lane + 256 i (i < 4: E <= 1024) of a tower
struct Row4 {
    f32x4 v[4];
};

TOC3D_DEV float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// the GroupNorm group of each of a lane's columns (the same in both towers, and for every row: the divisions are done once per workgroup)
TOC3D_DEV void focal_lane_groups(int lane, int E, int (&grp)[4][4]) {
    const int cpg = E / 32;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * lane + 256 * i + e;
            grp[i][e] = c < E ? c / cpg : 0;
        }
}

// relu(GroupNorm(x)) of one tower on load: xr, gamma and beta point at the tower's column 0, st at its 32 (mean, rstd) pairs (LDS).  Columns past E stay 0.
// ((x - mean) * rstd) * gamma + beta with the last two as ONE fused multiply-add: the sequence the compiler contracted the plain expression to.
TOC3D_DEV void focal_load_tower(Row4& h, const float* __restrict__ xr, const float* __restrict__ gamma, const float* __restrict__ beta, const float* st,
                                const int (&grp)[4][4], int lane, int E) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = 4 * lane + 256 * i;
        if (c < E) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + c);
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c), b = *reinterpret_cast<const f32x4*>(beta + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float* s = st + grp[i][e] * 2;
                h.v[i][e] = fmaxf(__fmaf_rn(__fmul_rn(__fsub_rn(xv[e], s[0]), s[1]), g[e], b[e]), 0.f);
            }
        } else {
            h.v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

// every lane returns the whole row's u . w (w: E floats in LDS): per lane an fmaf chain over its columns in rising order, then wave_sum
TOC3D_DEV float focal_dot(const Row4& u, const float* w, int lane, int E) {
    float p = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int col = 4 * lane + 256 * i;
        if (col < E) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(w + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) p = fmaf(u.v[i][e], wv[e], p);
        }
    }
    return wave_sum(p);
}

// the class half's logits from LDS-resident weights s_w [NC + 1][E] and biases s_b [NC + 1]: lane n keeps class n in `mine`, every lane the running maximum
// over the classes (cls_logits.topk(1), focal_head.py:178) in `best`; returns the centerness logit (the last row)
TOC3D_DEV float focal_class_logits(const Row4& h, const float* s_w, const float* s_b, int NC, int lane, int E, float& mine, float& best) {
    mine = 0.f;
    best = -INFINITY;
    for (int n = 0; n < NC; ++n) {
        const float p = focal_dot(h, s_w + n * E, lane, E) + s_b[n];
        if (lane == n) mine = p;
        best = fmaxf(best, p);
    }
    return focal_dot(h, s_w + NC * E, lane, E) + s_b[NC];
}

// sample_weight = sigmoid(max_c cls) * sigmoid(centerness) (focal_head.py:180) from the two sigmoids
TOC3D_DEV float focal_sample_weight(float sig_best, float sig_ctr) { return __fmul_rn(sig_best, sig_ctr); }
