// FocalHead's selection-only path at eval (gfx950): sample_weight from the class tower alone.
//
// Reference: Petr3D.simple_test_pts reads outs_roi['topk_indexes'] and nothing else (detectors/petr3d.py:524-525), and topk_indexes depends on the class tower
// only: sample_weight = sigmoid(max_c cls) * sigmoid(centerness) (dense_heads/focal_head.py:159-160, 178-180).  sample_weight_kernel is the class half of
// focal_heads_kernel (focal_head.hip) and nothing else: the same launch shape (one wavefront per pixel row, 32 rows of one view per workgroup, the class-half
// weights, the view's 32 (mean, rstd) pairs and the biases staged once in LDS), and the same per-row operation sequence, spelled once in focal_row.h -- so every
// weight holds the bits toc3d_focal_heads writes for the row.  No box tower: neither its columns of x, nor its statistics, weights or outputs are touched.
#include "focal_row.h"

#include "../../include/toc3d_select.h"

namespace {

struct SelectArgs {
    const float* x;                      // [V*T, ldx]: the class tower in columns [0, E), BEFORE GroupNorm / ReLU; nothing from column E on is read
    int64_t ldx;
    const float* stats;                  // [V, 32, 2]
    const float *gamma, *beta;           // [E]
    const float *w_cls, *b_cls;          // [NC + 1, E], [NC + 1]
    float* weight;                       // [V*T]
    int T, E, NC, chunks;                // chunks = ceil(T / FH_ROWS) workgroups per view
};

__global__ __launch_bounds__(256) void sample_weight_kernel(const SelectArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_w[];                  // [NC + 1][E] class-half weights, [64] stats, [NC + 1] biases
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int E = a.E, NC = a.NC, nc4 = (NC + 1) * E / 4;
    const int v = blockIdx.x / a.chunks, chunk = blockIdx.x % a.chunks;
    float* s_st = s_w + (NC + 1) * E;
    float* s_b = s_st + 64;
    for (int i = threadIdx.x; i < nc4; i += 256) reinterpret_cast<f32x4*>(s_w)[i] = reinterpret_cast<const f32x4*>(a.w_cls)[i];
    if (threadIdx.x < 64) s_st[threadIdx.x] = a.stats[(int64_t)v * 64 + threadIdx.x];
    if (threadIdx.x >= 64 && threadIdx.x < 64 + NC + 1) s_b[threadIdx.x - 64] = a.b_cls[threadIdx.x - 64];
    __syncthreads();
    int grp[4][4];
    focal_lane_groups(lane, E, grp);
    const int r_end = min(a.T, (chunk + 1) * FH_ROWS);
    for (int r = chunk * FH_ROWS + wave; r < r_end; r += 4) {
        const int64_t row = (int64_t)v * a.T + r;
        Row4 h;
        focal_load_tower(h, a.x + row * a.ldx, a.gamma, a.beta, s_st, grp, lane, E);
        float mine, best;
        const float ctr = focal_class_logits(h, s_w, s_b, NC, lane, E, mine, best);
        // the two sigmoids, one per lane (:180)
        const float sg = sigmoidf_(lane == 0 ? best : ctr);
        const float wgt = focal_sample_weight(__shfl(sg, 0), __shfl(sg, 1));
        if (lane == 0) a.weight[row] = wgt;
    }
}

}  // namespace

extern "C" {

int toc3d_select_abi(void) { return TOC3D_SELECT_ABI; }

int toc3d_focal_sample_weight(int dtype, const void* x, int64_t ldx, const float* stats, const float* gamma, const float* beta, const float* w_cls,
                              const float* b_cls, int64_t V, int64_t T, int64_t E, int64_t num_classes, float* sample_weight, toc3d_stream_t stream) {
    TOC3D_REQUIRE(x && stats && gamma && beta && w_cls && b_cls && sample_weight, "toc3d_focal_sample_weight: null buffer");
    TOC3D_REQUIRE(dtype == TOC3D_F32, "toc3d_focal_sample_weight: bad dtype (the conv's rows are TOC3D_DTYPE_F32)");
    TOC3D_REQUIRE(V > 0 && T > 0 && E > 0 && num_classes > 0, "toc3d_focal_sample_weight: V, T, E and num_classes must be positive");
    TOC3D_REQUIRE(E % 32 == 0 && E <= 1024, "toc3d_focal_sample_weight: embed_dims %% 32 != 0 or above 1024 (GroupNorm(32, .): 32 groups of whole channels)");
    TOC3D_REQUIRE(num_classes <= 64, "toc3d_focal_sample_weight: num_classes above 64 (lane n of a wavefront keeps class n)");
    const int64_t lds = ((num_classes + 1) * E + 64 + num_classes + 1) * 4;
    TOC3D_REQUIRE(lds <= 64 * 1024, "toc3d_focal_sample_weight: the weight block ((num_classes + 1) * E floats) beyond 64 KB of LDS");
    TOC3D_REQUIRE(ldx >= E && ldx % 4 == 0, "toc3d_focal_sample_weight: leading dimension too small (ldx >= E and a multiple of 4)");
    TOC3D_REQUIRE(aligned(x, 16) && aligned(gamma, 16) && aligned(beta, 16) && aligned(w_cls, 16),
                  "toc3d_focal_sample_weight: x, gamma, beta and w_cls must be 16-byte aligned");
    const int64_t chunks = (T + FH_ROWS - 1) / FH_ROWS;
    TOC3D_REQUIRE(T < (1ll << 31) - FH_ROWS && V * chunks < (1ll << 31), "toc3d_focal_sample_weight: too many rows for one launch");
    SelectArgs a;
    a.x = (const float*)x; a.ldx = ldx; a.stats = stats; a.gamma = gamma; a.beta = beta; a.w_cls = w_cls; a.b_cls = b_cls; a.weight = sample_weight;
    a.T = (int)T; a.E = (int)E; a.NC = (int)num_classes; a.chunks = (int)chunks;
    toc3d_launch(sample_weight_kernel, dim3((unsigned)(V * chunks)), dim3(256), (size_t)lds, as_stream(stream), a);
    TOC3D_LAUNCH_CHECK("toc3d_focal_sample_weight");
    return TOC3D_OK;
}

}  // extern "C"
