// FocalHead, the 2-D auxiliary head, at eval (gfx950): what sits behind its two 3x3 convs.
//
// Reference: FocalHead.forward (dense_heads/focal_head.py:140-193) over _init_layers (:119-134), apply_ltrb and apply_center_offset (models/utils/misc.py:26-56).
//
// shared_cls.0 and shared_reg.0 read the same feature map: their weights are stacked along Cout and run as ONE implicit-GEMM conv (toc3d_conv3x3_nhwc), so the
// two towers live side by side in one f32 buffer x [V*T, 2E]: class tower in columns [0, E), box tower in [E, 2E).  This file holds the rest:
//   * gn_stats_kernel     mean and rstd of the two GroupNorm(32, E) for every (view, tower, group): a workgroup owns 8 consecutive groups of one view (8 E/32
//                         consecutive columns), its lanes run along the row, and the sums are taken in two passes (the second on x - mean) in a fixed order: per
//                         thread down the rows, then one wavefront per group over the threads' partial sums.  No atomics;
//   * focal_heads_kernel  one wavefront per pixel row: GroupNorm affine + ReLU on load, the num_classes + 1 (cls | centerness) and 4 + 2 (ltrb | center2d) output
//                         channels of the 1x1 convs as f32 FMA chains from LDS-resident weights (17 columns would pad an MFMA tile to 128), then the sigmoids, the
//                         box geometry and the sampling weight.
// exp / log are the libm forms (no fast-math intrinsics): sample_weight decides a ranking.
#include "focal_row.h"

#include "../../include/toc3d_focal.h"

namespace {

constexpr int GN_THREADS = 1024, GN_GROUPS = 8;          // groups per workgroup: 32 groups per tower, so a workgroup never straddles two towers

// the sum of a group's partial sums part[r * wc + g * cpg + c], r < R, c < cpg (at most 128 of them), by one wavefront: every lane returns it
TOC3D_DEV float group_sum(const float* part, int R, int wc, int g, int cpg, int lane) {
    float a = 0.f;
    for (int i = lane; i < R * cpg; i += 64) a += part[(i / cpg) * wc + g * cpg + (i % cpg)];
    return wave_sum(a);
}

__global__ __launch_bounds__(GN_THREADS) void gn_stats_kernel(const float* __restrict__ x, int64_t ldx, int T, int cpg, int blocks_per_view, float eps,
                                                              float* __restrict__ stats) {
    __shared__ float s_part[GN_THREADS];
    __shared__ float s_mean[GN_GROUPS];
    const int v = blockIdx.x / blocks_per_view, gb = blockIdx.x % blocks_per_view;
    const int wc = GN_GROUPS * cpg;                      // this workgroup's columns: [gb * wc, (gb + 1) * wc)
    const int R = GN_THREADS / wc;                       // rows in flight: thread t reads column t % wc of rows t / wc, t / wc + R, ...
    const int t = threadIdx.x, col = t % wc, rl = t / wc, wave = t >> 6, lane = t & 63;
    const bool active = rl < R;
    const float* base = x + (int64_t)v * T * ldx + (int64_t)gb * wc + col;
    const float n = (float)cpg * (float)T;
    float s = 0.f;
    if (active)
        for (int r = rl; r < T; r += R) s += base[(int64_t)r * ldx];
    s_part[t] = s;                                       // (active threads: t == rl * wc + col)
    __syncthreads();
    if (wave < GN_GROUPS) {
        const float m = group_sum(s_part, R, wc, wave, cpg, lane) / n;
        if (lane == 0) s_mean[wave] = m;
    }
    __syncthreads();
    const float mean = s_mean[col / cpg];
    float q = 0.f;
    if (active)
        for (int r = rl; r < T; r += R) { const float d = base[(int64_t)r * ldx] - mean; q += d * d; }
    s_part[t] = q;
    __syncthreads();
    if (wave < GN_GROUPS) {
        const float var = group_sum(s_part, R, wc, wave, cpg, lane) / n;
        if (lane == 0) {
            float* o = stats + ((int64_t)blockIdx.x * GN_GROUPS + wave) * 2;          // group index (v * blocks_per_view + gb) * 8 + wave
            o[0] = s_mean[wave];
            o[1] = 1.0f / sqrtf(var + eps);
        }
    }
}

TOC3D_DEV float clamp01(float x) { x = x < 0.f ? 0.f : x; return x > 1.f ? 1.f : x; }          // torch.where(x < 0, 0, x), torch.where(x > 1, 1, x): a NaN stays

struct FocalArgs {
    const float* x;                      // [V*T, ldx]: class tower in columns [0, E), box tower in [E, 2E), both BEFORE GroupNorm / ReLU
    int64_t ldx;
    const float* stats;                  // [V, 64, 2]
    const float *gamma, *beta;           // [2E]
    const float *w_cls, *b_cls, *w_reg, *b_reg, *loc;
    float* cls;
    int64_t ldc;
    float *box, *ctr2d, *ctrness, *weight;
    int T, E, NC, chunks;                // chunks = ceil(T / FH_ROWS) workgroups per view
};

__global__ __launch_bounds__(256) void focal_heads_kernel(const FocalArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_w[];                  // [NC + 1][E] class-half weights, [6][E] box-half weights, [128] stats, [NC + 7] biases
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int E = a.E, NC = a.NC, nc4 = (NC + 1) * E / 4, nr4 = 6 * E / 4;
    const int v = blockIdx.x / a.chunks, chunk = blockIdx.x % a.chunks;
    float* s_reg = s_w + (NC + 1) * E;
    float* s_st = s_reg + 6 * E;
    float* s_b = s_st + 128;
    for (int i = threadIdx.x; i < nc4; i += 256) reinterpret_cast<f32x4*>(s_w)[i] = reinterpret_cast<const f32x4*>(a.w_cls)[i];
    for (int i = threadIdx.x; i < nr4; i += 256) reinterpret_cast<f32x4*>(s_reg)[i] = reinterpret_cast<const f32x4*>(a.w_reg)[i];
    if (threadIdx.x < 128) s_st[threadIdx.x] = a.stats[(int64_t)v * 128 + threadIdx.x];
    if (threadIdx.x < NC + 1) s_b[threadIdx.x] = a.b_cls[threadIdx.x];
    if (threadIdx.x >= 64 && threadIdx.x < 70) s_b[NC + 1 + threadIdx.x - 64] = a.b_reg[threadIdx.x - 64];
    __syncthreads();
    int grp[4][4];
    focal_lane_groups(lane, E, grp);
    const int r_end = min(a.T, (chunk + 1) * FH_ROWS);
    for (int r = chunk * FH_ROWS + wave; r < r_end; r += 4) {
        const int64_t row = (int64_t)v * a.T + r;
        const float* xr = a.x + row * a.ldx;
        Row4 h[2];
        // relu(GroupNorm(x)) of both towers on load (focal_row.h)
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) focal_load_tower(h[hb], xr + hb * E, a.gamma + hb * E, a.beta + hb * E, s_st + hb * 64, grp, lane, E);
        auto dot = [&](const Row4& u, const float* w) { return focal_dot(u, w, lane, E); };
        // cls | centerness from the class half; lane n keeps class n, every lane the running maximum (cls_logits.topk(1), :178)
        float mine, best;
        const float ctr = focal_class_logits(h[0], s_w, s_b, NC, lane, E, mine, best);
        // ltrb | center2d from the box half
        float o[6];
#pragma unroll
        for (int n = 0; n < 6; ++n) o[n] = dot(h[1], s_reg + n * E) + s_b[NC + 1 + n];
        const f32x2 loc = *reinterpret_cast<const f32x2*>(a.loc + row * 2);
        // the eight sigmoids, one per lane: ltrb (:169), the centre (misc.py:51-54), the best class and the centerness (:180)
        float z = lane == 0 ? o[0] : lane == 1 ? o[1] : lane == 2 ? o[2] : lane == 3 ? o[3] : lane == 6 ? best : ctr;
        if (lane == 4 || lane == 5) z = inverse_sigmoid(lane == 4 ? loc[0] : loc[1]) + (lane == 4 ? o[4] : o[5]);
        const float sg = sigmoidf_(z);
        const float s0 = __shfl(sg, 0), s1 = __shfl(sg, 1), s2 = __shfl(sg, 2), s3 = __shfl(sg, 3);
        if (lane < NC) a.cls[row * a.ldc + lane] = mine;
        if (lane == 4 || lane == 5) a.ctr2d[row * 2 + lane - 4] = sg;
        const float wgt = focal_sample_weight(__shfl(sg, 6), __shfl(sg, 7));
        if (lane == 0) {
            // apply_ltrb (misc.py:26-43), then mmdet's bbox_xyxy_to_cxcywh: (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1
            const float x1 = clamp01(loc[0] - s0), y1 = clamp01(loc[1] - s1), x2 = clamp01(loc[0] + s2), y2 = clamp01(loc[1] + s3);
            *reinterpret_cast<f32x4*>(a.box + row * 4) = f32x4{(x1 + x2) * 0.5f, (y1 + y2) * 0.5f, x2 - x1, y2 - y1};
            a.ctrness[row] = ctr;
            a.weight[row] = wgt;
        }
    }
}

}  // namespace

extern "C" {

int toc3d_focal_abi(void) { return TOC3D_FOCAL_ABI; }

int toc3d_focal_gn_stats(int dtype, const void* x, int64_t ldx, int64_t V, int64_t T, int64_t E, int64_t branches, float eps, float* stats,
                         toc3d_stream_t stream) {
    TOC3D_REQUIRE(x && stats, "toc3d_focal_gn_stats: null buffer");
    TOC3D_REQUIRE(dtype == TOC3D_F32, "toc3d_focal_gn_stats: bad dtype (the conv's rows are TOC3D_DTYPE_F32)");
    TOC3D_REQUIRE(V > 0 && T > 0 && E > 0 && branches > 0, "toc3d_focal_gn_stats: V, T, E and branches must be positive");
    TOC3D_REQUIRE(E % 32 == 0 && E <= 1024, "toc3d_focal_gn_stats: embed_dims %% 32 != 0 or above 1024 (GroupNorm(32, .): 32 groups of whole channels)");
    TOC3D_REQUIRE(branches <= 64 && ldx >= branches * E, "toc3d_focal_gn_stats: ldx below branches * E (at most 64 branches)");
    TOC3D_REQUIRE(T < (1ll << 31) - GN_THREADS && V * branches * (32 / GN_GROUPS) < (1ll << 31), "toc3d_focal_gn_stats: too many pixels or views for one launch");
    const int blocks_per_view = (int)branches * (32 / GN_GROUPS);
    toc3d_launch(gn_stats_kernel, dim3((unsigned)(V * blocks_per_view)), dim3(GN_THREADS), 0, as_stream(stream), (const float*)x, ldx, (int)T, (int)(E / 32),
                 blocks_per_view, eps, stats);
    TOC3D_LAUNCH_CHECK("toc3d_focal_gn_stats");
    return TOC3D_OK;
}

int toc3d_focal_heads(int dtype, const void* x, int64_t ldx, const float* stats, const float* gamma, const float* beta, const float* w_cls,
                      const float* b_cls, const float* w_reg, const float* b_reg, const float* location, int64_t V, int64_t T, int64_t E,
                      int64_t num_classes, float* cls_out, int64_t ld_cls, float* bbox_out, float* centers_out, float* centerness_out,
                      float* sample_weight, toc3d_stream_t stream) {
    TOC3D_REQUIRE(x && stats && gamma && beta && w_cls && b_cls && w_reg && b_reg && location && cls_out && bbox_out && centers_out && centerness_out &&
                      sample_weight, "toc3d_focal_heads: null buffer");
    TOC3D_REQUIRE(dtype == TOC3D_F32, "toc3d_focal_heads: bad dtype (the conv's rows are TOC3D_DTYPE_F32)");
    TOC3D_REQUIRE(V > 0 && T > 0 && E > 0 && num_classes > 0, "toc3d_focal_heads: V, T, E and num_classes must be positive");
    TOC3D_REQUIRE(E % 32 == 0 && E <= 1024, "toc3d_focal_heads: embed_dims %% 32 != 0 or above 1024 (GroupNorm(32, .): 32 groups of whole channels)");
    const int64_t lds = ((num_classes + 7) * E + 128 + num_classes + 7) * 4;
    TOC3D_REQUIRE(num_classes <= 64 && lds <= 64 * 1024, "toc3d_focal_heads: num_classes above 64, or the weight blocks ((num_classes + 7) * E floats) beyond 64 KB of LDS");
    TOC3D_REQUIRE(ldx >= 2 * E && ldx % 4 == 0 && ld_cls >= num_classes, "toc3d_focal_heads: leading dimension too small (ldx >= 2 E and a multiple of 4, ld_cls >= num_classes)");
    TOC3D_REQUIRE(aligned(x, 16) && aligned(gamma, 16) && aligned(beta, 16) && aligned(w_cls, 16) && aligned(w_reg, 16) && aligned(bbox_out, 16) && aligned(location, 8),
                  "toc3d_focal_heads: x, gamma, beta, the weights and bbox_out must be 16-byte aligned, location 8-byte aligned");
    const int64_t chunks = (T + FH_ROWS - 1) / FH_ROWS;
    TOC3D_REQUIRE(T < (1ll << 31) - FH_ROWS && V * chunks < (1ll << 31), "toc3d_focal_heads: too many rows for one launch");
    FocalArgs a;
    a.x = (const float*)x; a.ldx = ldx; a.stats = stats; a.gamma = gamma; a.beta = beta; a.w_cls = w_cls; a.b_cls = b_cls; a.w_reg = w_reg; a.b_reg = b_reg;
    a.loc = location; a.cls = cls_out; a.ldc = ld_cls; a.box = bbox_out; a.ctr2d = centers_out; a.ctrness = centerness_out; a.weight = sample_weight;
    a.T = (int)T; a.E = (int)E; a.NC = (int)num_classes; a.chunks = (int)chunks;
    toc3d_launch(focal_heads_kernel, dim3((unsigned)(V * chunks)), dim3(256), (size_t)lds, as_stream(stream), a);
    TOC3D_LAUNCH_CHECK("toc3d_focal_heads");
    return TOC3D_OK;
}

}  // extern "C"
