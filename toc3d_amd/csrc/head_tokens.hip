// Token side of StreamPETRHead.forward (second half): what consumes the neck's features behind the
// backbone.  Reference: dense_heads/streampetr_head.py position_embeding :378-422, forward :627-639; models/utils/misc.py
// locations :59-82, MLN :154-188, SELayer_Linear :139-151.  The linear layers run on toc3d_linear; this file holds the elementwise /
// geometry kernels around them.  All HBM-bound byte work on [tokens, 64..1024] rows.  Act rows are stored with put1 / put4 (act_rows.h).
#include "act_rows.h"
#include "frustum_point.h"

namespace {

// one thread per (token, depth bin): frustum_point (frustum_point.h) for every token of every view, row = the token's own index
template <typename T>
__global__ __launch_bounds__(256) void frustum_kernel(FrustumArgs a, T* __restrict__ pin, int64_t ld_pin, T* __restrict__ cone_act,
                                                      int64_t ld_cone, float* __restrict__ cone) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int hw = a.h * a.w;
    const int64_t total = (int64_t)a.B * a.N * hw * a.D;
    if (id >= total) return;
    const int d = (int)(id % a.D);
    const int64_t tokg = id / a.D;                                       // b * N*hw + n*hw + y*w + x
    const int pix = (int)(tokg % hw), view = (int)(tokg / hw);           // view = b*N + n
    frustum_point(a, view, pix, (int)(tokg - (int64_t)(view / a.N) * a.N * hw), d, tokg, pin, ld_pin, cone_act, ld_cone, cone);
}

template <typename T>
__global__ void relu_kernel(T* __restrict__ x, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const float v = from_act(x[i]); x[i] = to_act<T>(v > 0.f ? v : 0.f); }
}

// NCHW f32 [V, C, hw] -> rows [V*hw, ld] act
template <typename T>
__global__ __launch_bounds__(256) void nchw_rows_kernel(const float* __restrict__ x, T* __restrict__ out, int64_t ld, int C, int hw) {
    __shared__ float tile[32][33];
    const int v = blockIdx.z, c0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, t = t0 + tx;
        tile[r][tx] = (c < C && t < hw) ? x[((int64_t)v * C + c) * hw + t] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int t = t0 + r, c = c0 + tx;
        if (t < hw && c < C) put1(out + ((int64_t)v * hw + t) * ld + c, tile[tx][r]);
    }
}

// The neck's conv rows x f32 [V*T, ldx], read ONCE, written twice: rows [V*T, ld] act straight from the registers (what nchw_rows_kernel would make of the
// NCHW tensor: the same put1 per element, valid columns only), and NCHW f32 [V, C, T] through nhwc_to_nchw_kernel's padded 32 x 32 tile.  One workgroup per
// (view, 32 tokens, 32 channels).  VIN: x and rows take 4-column accesses (16-byte loads; host-checked alignment, C % 4 == 0) -- thread = (token tid / 8,
// column quad tid % 8); VOUT: nchw takes 16-byte stores along T (T % 4 == 0) -- thread = (channel tid / 8, token quad tid % 8).  LDS traffic is dword-wide
// either way; with the row stride of 33 the 32 lanes of a half-wave (the conflict group of ds_read_b32 / ds_write_b32) hit 32 different banks in all four
// patterns: write (r + 4 q + k) % 32 over r 0..3, q 0..7; read (4 j + k + c) % 32 over c 0..3, j 0..7; the scalar forms as in the two kernels this one replaces.
template <typename T, bool VIN, bool VOUT>
__global__ __launch_bounds__(256) void neck_rows_fanout_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ nchw, T* __restrict__ rows, int64_t ld,
                                                               int Tn, int C) {
    __shared__ float tile[32][33];
    const int v = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tid = threadIdx.x;
    if (VIN) {
        const int r = tid >> 3, q4 = (tid & 7) * 4;
        const int t = t0 + r, c = c0 + q4;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        if (t < Tn && c < C) {                                            // C % 4 == 0: a quad is valid as a whole
            const int64_t row = (int64_t)v * Tn + t;
            const f32x4 g = *reinterpret_cast<const f32x4*>(x + row * ldx + c);
            a[0] = g[0]; a[1] = g[1]; a[2] = g[2]; a[3] = g[3];
            put4(rows + row * ld + c, a);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) tile[r][q4 + k] = a[k];
    } else {
        const int tx = tid & 31, ty = tid >> 5;
        for (int i = ty; i < 32; i += 8) {
            const int t = t0 + i, c = c0 + tx;
            float a = 0.f;
            if (t < Tn && c < C) {
                const int64_t row = (int64_t)v * Tn + t;
                a = x[row * ldx + c];
                put1(rows + row * ld + c, a);
            }
            tile[i][tx] = a;
        }
    }
    __syncthreads();
    if (VOUT) {
        const int cl = tid >> 3, j4 = (tid & 7) * 4;
        const int c = c0 + cl, t = t0 + j4;
        if (c < C && t < Tn)                                              // T % 4 == 0: likewise
            *reinterpret_cast<f32x4*>(nchw + ((int64_t)v * C + c) * Tn + t) = f32x4{tile[j4][cl], tile[j4 + 1][cl], tile[j4 + 2][cl], tile[j4 + 3][cl]};
    } else {
        const int tx = tid & 31, ty = tid >> 5;
        for (int i = ty; i < 32; i += 8) {
            const int c = c0 + i, t = t0 + tx;
            if (t < Tn && c < C) nchw[((int64_t)v * C + c) * Tn + t] = tile[tx][i];
        }
    }
}

// MLN.forward (misc.py:181-188): out = gamma * LayerNorm(x; no affine, eps 1e-5) + beta; one wavefront per row, E <= 1024
template <typename T>
__global__ __launch_bounds__(256) void mln_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  int E, float* __restrict__ out, T* __restrict__ out_act, int64_t ld_act, int M) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    if (row >= M) return;
    float v[16];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { const int c = lane + 64 * i; v[i] = c < E ? x[(int64_t)row * E + c] : 0.f; s += v[i]; }
    const float mean = wave_sum(s) / (float)E;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { const int c = lane + 64 * i; const float dlt = c < E ? v[i] - mean : 0.f; q += dlt * dlt; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)E + 1e-5f);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + 64 * i;
        if (c < E) {
            const float o = gamma[(int64_t)row * E + c] * ((v[i] - mean) * rstd) + beta[(int64_t)row * E + c];
            out[(int64_t)row * E + c] = o;
            put1(out_act + (int64_t)row * ld_act + c, o);
        }
    }
}

// SELayer_Linear gate (misc.py:151): out = pos * sigmoid(se)
__global__ void se_gate_kernel(const float* __restrict__ pos, const float* __restrict__ se, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = pos[i] * (1.0f / (1.0f + expf(-se[i])));
}

}  // namespace

extern "C" {

int toc3d_head_frustum_inputs(int dtype, const float* img2lidar, const float* intrinsics, const float* coords_d, const float* position_range,
                              int64_t B, int64_t N, int64_t h, int64_t w, int64_t D, int64_t stride, int64_t pad_h, int64_t pad_w,
                              void* pos_in, int64_t ld_pos, void* cone_act, int64_t ld_cone, float* cone, toc3d_stream_t stream) {
    TOC3D_REQUIRE(img2lidar && intrinsics && coords_d && position_range && pos_in && cone_act && cone, "toc3d_head_frustum_inputs: null buffer");
    TOC3D_REQUIRE(B > 0 && N > 0 && h > 0 && w > 0 && D >= 30 && stride > 0 && pad_h > 0 && pad_w > 0 && ld_pos >= 3 * D && ld_cone >= 8,
                  "toc3d_head_frustum_inputs: bad dims (depth_num >= 30, ld_pos >= 3*depth_num, ld_cone >= 8)");
    TOC3D_PLANES_ROWS("toc3d_head_frustum_inputs", "pos_in", pos_in, ld_pos);
    TOC3D_PLANES_ROWS("toc3d_head_frustum_inputs", "cone_act", cone_act, ld_cone);
    FrustumArgs a;
    a.img2lidar = img2lidar; a.intrinsics = intrinsics; a.coords_d = coords_d;
    for (int i = 0; i < 6; ++i) a.pr[i] = position_range[i];              // host pointer
    a.B = (int)B; a.N = (int)N; a.h = (int)h; a.w = (int)w; a.D = (int)D; a.stride = (int)stride; a.pad_h = (int)pad_h; a.pad_w = (int)pad_w;
    const int64_t total = B * N * h * w * D;
    dim3 grid((unsigned)((total + 255) / 256));
    if (int rc = toc3d_dispatch_act<ACT_ANY>("toc3d_head_frustum_inputs", dtype, [&](auto tag) {
            using T = typename decltype(tag)::type;
            toc3d_launch(frustum_kernel<T>, grid, dim3(256), 0, as_stream(stream), a, (T*)pos_in, ld_pos, (T*)cone_act, ld_cone, cone);
        })) return rc;
    TOC3D_LAUNCH_CHECK("toc3d_head_frustum_inputs");
    return TOC3D_OK;
}

int toc3d_relu_inplace(int dtype, void* x, int64_t n, toc3d_stream_t stream) {
    TOC3D_REQUIRE(x && n >= 0, "toc3d_relu_inplace: bad arguments");
    TOC3D_REQUIRE(n <= ((1ll << 31) - 1) * 256, "toc3d_relu_inplace: too many elements for one launch");      // the grid below: at most 2^31 - 1 workgroups
    if (n == 0) return TOC3D_OK;
    dim3 grid((unsigned)((n + 255) / 256));
    if (int rc = toc3d_dispatch_act<ACT_BF16 | ACT_F32>("toc3d_relu_inplace", dtype, [&](auto tag) {
            using T = typename decltype(tag)::type;
            toc3d_launch(relu_kernel<T>, grid, dim3(256), 0, as_stream(stream), (T*)x, n);
        })) return rc;
    TOC3D_LAUNCH_CHECK("toc3d_relu_inplace");
    return TOC3D_OK;
}

int toc3d_nchw_to_rows(int dtype, const float* x, void* out, int64_t ldo, int64_t V, int64_t C, int64_t hw, toc3d_stream_t stream) {
    TOC3D_REQUIRE(x && out && V > 0 && C > 0 && hw > 0 && ldo >= C && V <= 65535, "toc3d_nchw_to_rows: bad arguments");
    TOC3D_PLANES_ROWS("toc3d_nchw_to_rows", "out", out, ldo);
    dim3 grid((unsigned)((hw + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)V);
    if (int rc = toc3d_dispatch_act<ACT_ANY>("toc3d_nchw_to_rows", dtype, [&](auto tag) {
            using T = typename decltype(tag)::type;
            toc3d_launch(nchw_rows_kernel<T>, grid, dim3(256), 0, as_stream(stream), x, (T*)out, ldo, (int)C, (int)hw);
        })) return rc;
    TOC3D_LAUNCH_CHECK("toc3d_nchw_to_rows");
    return TOC3D_OK;
}

int toc3d_neck_rows_fanout(int dtype, const float* x, int64_t ldx, float* nchw, void* rows, int64_t ld_rows, int64_t V, int64_t T, int64_t C,
                           toc3d_stream_t stream) {
    TOC3D_REQUIRE(x && nchw && rows, "toc3d_neck_rows_fanout: null buffer");
    TOC3D_REQUIRE(act_served(ACT_ANY, dtype), "toc3d_neck_rows_fanout: bad dtype");
    TOC3D_REQUIRE(V > 0 && T > 0 && C > 0, "toc3d_neck_rows_fanout: bad dims (V, T, C > 0)");
    TOC3D_REQUIRE(V <= 65535 && T <= 0x7fffffffll - 31 && C <= 65535ll * 32, "toc3d_neck_rows_fanout: bad dims (V <= 65535 views, T and C within one launch's grid)");
    TOC3D_REQUIRE(ldx >= C && ld_rows >= C, "toc3d_neck_rows_fanout: bad leading dimensions (ldx >= C, ld_rows >= C)");
    TOC3D_PLANES_ROWS("toc3d_neck_rows_fanout", "rows", rows, ld_rows);
    // 4-column accesses: 16-byte loads of x; stores of 16 (f32) / 8 (bf16, each plane) bytes to rows
    const uintptr_t row_align = dtype == TOC3D_BF16 ? 8 : 16;
    const bool vin = C % 4 == 0 && ldx % 4 == 0 && ld_rows % 4 == 0 && aligned(x, 16) && aligned(rows, row_align);
    const bool vout = T % 4 == 0 && aligned(nchw, 16);
    dim3 grid((unsigned)((T + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)V);
    if (int rc = toc3d_dispatch_act<ACT_ANY>("toc3d_neck_rows_fanout", dtype, [&](auto tag) {
            using E = typename decltype(tag)::type;          // (T is the token count here)
            auto launch = [&](auto kernel) { toc3d_launch(kernel, grid, dim3(256), 0, as_stream(stream), x, ldx, nchw, (E*)rows, ld_rows, (int)T, (int)C); };
            if (vin && vout) launch(neck_rows_fanout_kernel<E, true, true>);
            else if (vin) launch(neck_rows_fanout_kernel<E, true, false>);
            else if (vout) launch(neck_rows_fanout_kernel<E, false, true>);
            else launch(neck_rows_fanout_kernel<E, false, false>);
        })) return rc;
    TOC3D_LAUNCH_CHECK("toc3d_neck_rows_fanout");
    return TOC3D_OK;
}

int toc3d_mln_apply(int dtype, const float* x, const float* gamma, const float* beta, int64_t M, int64_t E, float* out, void* out_act, int64_t ld_act,
                    toc3d_stream_t stream) {
    TOC3D_REQUIRE(x && gamma && beta && out && out_act && M >= 0 && E > 0 && E <= 1024 && ld_act >= E, "toc3d_mln_apply: bad arguments (E <= 1024)");
    TOC3D_PLANES_ROWS("toc3d_mln_apply", "out_act", out_act, ld_act);
    if (M == 0) return TOC3D_OK;
    dim3 grid((unsigned)((M + 3) / 4));
    if (int rc = toc3d_dispatch_act<ACT_ANY>("toc3d_mln_apply", dtype, [&](auto tag) {
            using T = typename decltype(tag)::type;
            toc3d_launch(mln_kernel<T>, grid, dim3(256), 0, as_stream(stream), x, gamma, beta, (int)E, out, (T*)out_act, ld_act, (int)M);
        })) return rc;
    TOC3D_LAUNCH_CHECK("toc3d_mln_apply");
    return TOC3D_OK;
}

int toc3d_se_gate(const float* pos, const float* se, float* out, int64_t n, toc3d_stream_t stream) {
    TOC3D_REQUIRE(pos && se && out && n >= 0, "toc3d_se_gate: bad arguments");
    if (n == 0) return TOC3D_OK;
    toc3d_launch(se_gate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), pos, se, out, n);
    TOC3D_LAUNCH_CHECK("toc3d_se_gate");
    return TOC3D_OK;
}

}  // extern "C"
