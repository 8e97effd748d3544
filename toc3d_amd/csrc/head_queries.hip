// Query side of StreamPETRHead (gfx950): what turns the temporal memory bank into the decoder's inputs.
//
// Reference: StreamPETRHead.forward (dense_heads/streampetr_head.py:641-652) and StreamPETRHead.temporal_alignment (:424-453) over pos2posemb3d, pos2posemb1d,
// nerf_positional_encoding (models/utils/positional_encoding.py:14-81) and MLN (models/utils/misc.py:154-188).
//
// The Linear layers (query_embedding, time_embedding.0, the MLNs' reduce / gamma / beta) are GEMMs (toc3d_linear_fused).  This file holds what surrounds them:
//   * query_inputs_kernel    the three GEMM A operands of a memory entry in one launch -- pos2posemb3d of the pc_range-normalised reference point [384], the NeRF
//                            encoding of the ego-motion vector [180, padded to 192 with zeros], pos2posemb1d of the f64 timestamp [256] -- in the act dtype or as
//                            (hi, lo) planes, read through per-sample strides (the bank's views are strided for B > 1); the normalised reference points of the first
//                            `np` entries of every sample go straight into the tail of the concatenated reference_points;
//   * query_combine_kernel   both MLNs and the time embedding's LayerNorm, one wavefront per row: temp_pos = gamma_pe * LN0(qe) + beta_pe + LN(te; w, b),
//                            temp_memory = gamma_mem * LN0(memory_embedding) + beta_mem; rows < np of a sample are stored into the tails of query_pos / tgt, the others
//                            into temp_pos / temp_memory: the torch.cat of :446-451 is a store address.
// sinf / cosf / sin / cos are the range-reduced libm forms and every division is the correctly rounded one (this file is built without fast-math): the arguments
// reach 2 pi * 1.5e9 (epoch timestamps) and 32 * 1.5e9, and a 1-ulp change of an argument of that size is a different result.
#include "act_rows.h"

namespace {

constexpr int QE = 256;                                    // embed_dims: pos2posemb3d yields 3 * 128, pos2posemb1d 256, MLN(180) has f_dim 256
constexpr int POS_W = 384, NERF_W = 180, NERF_WP = 192, T1D_W = 256;
constexpr int QUADS_POS = POS_W / 4, QUADS_NERF = NERF_WP / 4, QUADS_T1D = T1D_W / 4, QUADS_ROW = QUADS_POS + QUADS_NERF + QUADS_T1D;      // 96 + 48 + 64 = 208

struct QueryInArgs {
    const float* ref;                    // [B][n][3], sample stride ref_stride (elements)
    int64_t ref_stride;
    const float* velo;                   // [B][n][2]
    int64_t velo_stride;
    const double* ts;                    // [B][n]
    int64_t ts_stride;
    const float* pose;                   // [B][n][4][4]
    int64_t pose_stride;
    const float *dimt3, *dimt1;          // the dim_t tables of pos2posemb3d [128] and pos2posemb1d [256], computed by the host with the reference's expression
    float lo0, lo1, lo2, span0, span1, span2;      // pc_range[0:3], pc_range[3:6] - pc_range[0:3] (f32 subtraction, as the reference's tensor expression)
    int64_t ld_pos, ld_nerf, ld_t1d;
    float* ref_out;                      // normalised reference points of rows < np of sample b -> ref_out + b * ref_out_stride + 3 r
    int64_t ref_out_stride;
    int n, np;
    int64_t rows;                        // B * n
};

template <typename T>
__global__ __launch_bounds__(256) void query_inputs_kernel(const QueryInArgs a, T* __restrict__ pos3d, T* __restrict__ nerf, T* __restrict__ t1d) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= a.rows * QUADS_ROW) return;
    const int64_t row = id / QUADS_ROW;
    const int q = (int)(id - row * QUADS_ROW);
    const int64_t b = row / a.n;
    const int r = (int)(row - b * a.n);
    float y[4];
    if (q < QUADS_POS) {
        // temp_reference_point = (memory_reference_point - pc_range[:3]) / (pc_range[3:6] - pc_range[0:3]) (:427); pos2posemb3d, concatenated (y, x, z)
        const float* p = a.ref + b * a.ref_stride + (int64_t)r * 3;
        const int c = 4 * q, blk = c >> 7, f = c & 127;
        const int coord = blk == 0 ? 1 : (blk == 1 ? 0 : 2);
        const float lo = coord == 0 ? a.lo0 : (coord == 1 ? a.lo1 : a.lo2), span = coord == 0 ? a.span0 : (coord == 1 ? a.span1 : a.span2);
        const float pn = __fdiv_rn(__fsub_rn(p[coord], lo), span);
        const float scaled = __fmul_rn(pn, 6.283185307179586f);              // pos * float(2 * math.pi)
        const f32x4 dt = *reinterpret_cast<const f32x4*>(a.dimt3 + f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float arg = __fdiv_rn(scaled, dt[e]);
            y[e] = (e & 1) ? cosf(arg) : sinf(arg);
        }
        put4<T>(pos3d + row * a.ld_pos + c, y);
        if (q == 0 && r < a.np) {
            float* o = a.ref_out + b * a.ref_out_stride + (int64_t)r * 3;
            o[0] = __fdiv_rn(__fsub_rn(p[0], a.lo0), a.span0);
            o[1] = __fdiv_rn(__fsub_rn(p[1], a.lo1), a.span1);
            o[2] = __fdiv_rn(__fsub_rn(p[2], a.lo2), a.span2);
        }
    } else if (q < QUADS_POS + QUADS_NERF) {
        if (!nerf) return;
        // memory_ego_motion = cat([velo, timestamp, egopose[..., :3, :].flatten(-2)]).float() (:437); frequency-major [sin(2^k e), cos(2^k e)], k = 0..5
        const int c = 4 * (q - QUADS_POS);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = c + e;
            float v = 0.f;
            if (i < NERF_W) {
                const int k = i / 30, rr = i - 30 * k, j = rr < 15 ? rr : rr - 15;
                float m;
                if (j < 2) m = a.velo[b * a.velo_stride + (int64_t)r * 2 + j];
                else if (j == 2) m = (float)a.ts[b * a.ts_stride + r];
                else m = a.pose[b * a.pose_stride + (int64_t)r * 16 + (j - 3)];
                const float arg = __fmul_rn(m, (float)(1 << k));
                v = rr < 15 ? sinf(arg) : cosf(arg);
            }
            y[e] = v;
        }
        put4<T>(nerf + row * a.ld_nerf + c, y);
    } else {
        // pos2posemb1d(memory_timestamp) in f64 (the timestamp's dtype; dim_t promotes), then .float() (:443)
        const int c = 4 * (q - QUADS_POS - QUADS_NERF);
        const double scaled = a.ts[b * a.ts_stride + r] * 6.283185307179586;
        const f32x4 dt = *reinterpret_cast<const f32x4*>(a.dimt1 + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double arg = scaled / (double)dt[e];
            y[e] = (float)((e & 1) ? cos(arg) : sin(arg));
        }
        put4<T>(t1d + row * a.ld_t1d + c, y);
    }
}

// LayerNorm without affine over the 256 columns of a row held 4 per lane: f32 statistics, biased variance, two passes.  A zero row gives exactly zero.
TOC3D_DEV f32x4 ln0_256(f32x4 v, float eps) {
    const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) / (float)QE;
    f32x4 d;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { d[e] = v[e] - mean; q += d[e] * d[e]; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)QE + eps);
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] *= rstd;
    return d;
}

struct QueryCombineArgs {
    const float* qe;                     // [rows, ld_qe]   query_embedding(pos2posemb3d(.))
    int64_t ld_qe;
    const float* gb_pe;                  // [rows, ld_gb_pe >= 512]  gamma | beta of ego_pose_pe, or NULL (with_ego_pos = False)
    int64_t ld_gb_pe;
    const float* te;                     // [rows, ld_te]   time_embedding.0(pos2posemb1d(.))
    int64_t ld_te;
    const float *ln_w, *ln_b;            // time_embedding.1
    float eps;
    const float* mem;                    // memory_embedding [B][n][256]: sample stride mem_stride, row stride ld_mem
    int64_t mem_stride, ld_mem;
    const float* gb_mem;                 // gamma | beta of ego_pose_memory, or NULL
    int64_t ld_gb_mem;
    float *qpos_tail, *tgt_tail;         // rows < np of sample b -> tail + b * tail_stride + r * ld_tail
    int64_t qpos_stride, tgt_stride, ld_tail;
    float *temp_pos, *temp_mem;          // rows >= np -> [(b * (n - np) + r - np) * ld_temp]
    int64_t ld_temp;
    int n, np, rows;
};

__global__ __launch_bounds__(256) void query_combine_kernel(const QueryCombineArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    if (row >= a.rows) return;
    const int b = row / a.n, r = row - b * a.n, c = 4 * lane;
    auto ld4 = [&](const float* p) { return *reinterpret_cast<const f32x4*>(p + c); };
    // temp_pos = ego_pose_pe(query_embedding(.), nerf) + time_embedding(pos2posemb1d(.))  (:428, :439, :443)
    f32x4 pos = ld4(a.qe + (int64_t)row * a.ld_qe);
    if (a.gb_pe) {
        const f32x4 nrm = ln0_256(pos, 1e-5f), g = ld4(a.gb_pe + (int64_t)row * a.ld_gb_pe), bt = ld4(a.gb_pe + (int64_t)row * a.ld_gb_pe + QE);
#pragma unroll
        for (int e = 0; e < 4; ++e) pos[e] = g[e] * nrm[e] + bt[e];
    }
    {
        const f32x4 nrm = ln0_256(ld4(a.te + (int64_t)row * a.ld_te), a.eps), w = ld4(a.ln_w), lb = ld4(a.ln_b);
#pragma unroll
        for (int e = 0; e < 4; ++e) pos[e] += nrm[e] * w[e] + lb[e];
    }
    // temp_memory = ego_pose_memory(memory_embedding, nerf)  (:429, :440)
    f32x4 m = ld4(a.mem + (int64_t)b * a.mem_stride + (int64_t)r * a.ld_mem);
    if (a.gb_mem) {
        const f32x4 nrm = ln0_256(m, 1e-5f), g = ld4(a.gb_mem + (int64_t)row * a.ld_gb_mem), bt = ld4(a.gb_mem + (int64_t)row * a.ld_gb_mem + QE);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = g[e] * nrm[e] + bt[e];
    }
    float *dp, *dm;
    if (r < a.np) {
        dp = a.qpos_tail + (int64_t)b * a.qpos_stride + (int64_t)r * a.ld_tail;
        dm = a.tgt_tail + (int64_t)b * a.tgt_stride + (int64_t)r * a.ld_tail;
    } else {
        const int64_t o = ((int64_t)b * (a.n - a.np) + (r - a.np)) * a.ld_temp;
        dp = a.temp_pos + o;
        dm = a.temp_mem + o;
    }
    *reinterpret_cast<f32x4*>(dp + c) = pos;
    *reinterpret_cast<f32x4*>(dm + c) = m;
}

// an act-dtype output [rows, ld] of `width` columns: bf16 rows as 8-byte pieces, f32 rows as 16-byte pieces, planes as whole 128-byte groups
const char* act_rows_problem(int dtype, const void* act, int64_t ld, int64_t width) {
    if (ld < width) return "leading dimension smaller than the row";
    if (dtype == TOC3D_BF16) return aligned(act, 8) && ld % 4 == 0 ? nullptr : "bf16 rows must be 8-byte aligned (leading dimension a multiple of 4)";
    if (dtype == TOC3D_F32) return aligned(act, 16) && ld % 4 == 0 ? nullptr : "f32 rows must be 16-byte aligned (leading dimension a multiple of 4)";
    if (dtype == TOC3D_F32X3P) return planes_rows_ok(act, ld) ? nullptr : "rows of (hi, lo) planes start on 128-byte boundaries (buffer aligned, leading dimension a multiple of 32)";
    return "dtype must be TOC3D_DTYPE_BF16, TOC3D_DTYPE_F32 or TOC3D_DTYPE_F32X3P";
}

}  // namespace

extern "C" {

int toc3d_head_query_inputs(int dtype, const float* reference_point, int64_t ref_stride, const float* velo, int64_t velo_stride, const double* timestamp,
                            int64_t ts_stride, const float* egopose, int64_t pose_stride, const float* pc_range, const float* dim_t3, const float* dim_t1,
                            void* pos3d, int64_t ld_pos, void* nerf, int64_t ld_nerf, void* t1d, int64_t ld_t1d, float* ref_out, int64_t ref_out_stride,
                            int64_t B, int64_t n, int64_t np, int64_t E, toc3d_stream_t stream) {
    TOC3D_REQUIRE(E == QE, "toc3d_head_query_inputs: E must be 256 (pos2posemb3d yields 3 * 128 columns, pos2posemb1d 256, MLN(180) has f_dim 256)");
    TOC3D_REQUIRE(reference_point && timestamp && pc_range && dim_t3 && dim_t1 && pos3d && t1d, "toc3d_head_query_inputs: null buffer");
    TOC3D_REQUIRE(!nerf || (velo && egopose), "toc3d_head_query_inputs: null buffer (the NeRF encoding reads velo and egopose)");
    TOC3D_REQUIRE(B >= 0 && n >= 0 && np >= 0 && np <= n, "toc3d_head_query_inputs: bad counts (B, n >= 0, 0 <= np <= n)");
    TOC3D_REQUIRE(np == 0 || (ref_out && ref_out_stride >= 3 * np), "toc3d_head_query_inputs: np > 0 needs ref_out with a sample stride of at least 3 np");
    TOC3D_REQUIRE(ref_stride >= 3 * n && ts_stride >= n && (!nerf || (velo_stride >= 2 * n && pose_stride >= 16 * n)),
                  "toc3d_head_query_inputs: sample stride smaller than the sample (3 n, 2 n, n, 16 n elements)");
    TOC3D_REQUIRE(aligned(dim_t3, 16) && aligned(dim_t1, 16) && aligned(reference_point, 4) && aligned(timestamp, 8), "toc3d_head_query_inputs: dim_t tables must be 16-byte aligned, timestamp 8-byte");
    if (const char* why = act_rows_problem(dtype, pos3d, ld_pos, POS_W)) { toc3d_set_error("toc3d_head_query_inputs: pos3d: %s", why); return TOC3D_ERR_ARG; }
    if (const char* why = act_rows_problem(dtype, t1d, ld_t1d, T1D_W)) { toc3d_set_error("toc3d_head_query_inputs: t1d: %s", why); return TOC3D_ERR_ARG; }
    if (nerf)
        if (const char* why = act_rows_problem(dtype, nerf, ld_nerf, NERF_WP)) { toc3d_set_error("toc3d_head_query_inputs: nerf: %s", why); return TOC3D_ERR_ARG; }
    TOC3D_REQUIRE(n < (1ll << 31) && (n == 0 || B <= ((1ll << 31) - 1) / n) && B * n <= ((1ll << 31) - 1) * 256 / QUADS_ROW, "toc3d_head_query_inputs: too many rows for one launch");
    const float span[3] = {pc_range[3] - pc_range[0], pc_range[4] - pc_range[1], pc_range[5] - pc_range[2]};
    TOC3D_REQUIRE(span[0] != 0.f && span[1] != 0.f && span[2] != 0.f, "toc3d_head_query_inputs: pc_range spans nothing");
    if (B * n == 0) return TOC3D_OK;
    QueryInArgs a;
    a.ref = reference_point; a.ref_stride = ref_stride; a.velo = velo; a.velo_stride = velo_stride; a.ts = timestamp; a.ts_stride = ts_stride;
    a.pose = egopose; a.pose_stride = pose_stride; a.dimt3 = dim_t3; a.dimt1 = dim_t1;
    a.lo0 = pc_range[0]; a.lo1 = pc_range[1]; a.lo2 = pc_range[2]; a.span0 = span[0]; a.span1 = span[1]; a.span2 = span[2];
    a.ld_pos = ld_pos; a.ld_nerf = ld_nerf; a.ld_t1d = ld_t1d; a.ref_out = ref_out; a.ref_out_stride = ref_out_stride;
    a.n = (int)n; a.np = (int)np; a.rows = B * n;
    const dim3 grid((unsigned)((a.rows * QUADS_ROW + 255) / 256));
    if (int rc = toc3d_dispatch_act<ACT_ANY>("toc3d_head_query_inputs", dtype, [&](auto tag) {
            using T = typename decltype(tag)::type;
            toc3d_launch(query_inputs_kernel<T>, grid, dim3(256), 0, as_stream(stream), a, (T*)pos3d, (T*)nerf, (T*)t1d);
        })) return rc;
    TOC3D_LAUNCH_CHECK("toc3d_head_query_inputs");
    return TOC3D_OK;
}

int toc3d_head_query_combine(const float* qe, int64_t ld_qe, const float* gb_pe, int64_t ld_gb_pe, const float* te, int64_t ld_te, const float* ln_weight,
                             const float* ln_bias, float ln_eps, const float* memory_embedding, int64_t mem_stride, int64_t ld_mem, const float* gb_mem,
                             int64_t ld_gb_mem, float* query_pos_tail, int64_t query_pos_stride, float* tgt_tail, int64_t tgt_stride, int64_t ld_tail,
                             float* temp_pos, float* temp_memory, int64_t ld_temp, int64_t B, int64_t n, int64_t np, int64_t E, toc3d_stream_t stream) {
    TOC3D_REQUIRE(E == QE, "toc3d_head_query_combine: E must be 256 (one wavefront holds a row as 4 columns per lane)");
    TOC3D_REQUIRE(qe && te && ln_weight && ln_bias && memory_embedding, "toc3d_head_query_combine: null buffer");
    TOC3D_REQUIRE(B >= 0 && n >= 0 && np >= 0 && np <= n, "toc3d_head_query_combine: bad counts (B, n >= 0, 0 <= np <= n)");
    TOC3D_REQUIRE(np == 0 || (query_pos_tail && tgt_tail), "toc3d_head_query_combine: null buffer (np > 0 needs the query_pos and tgt tails)");
    TOC3D_REQUIRE(np == n || (temp_pos && temp_memory), "toc3d_head_query_combine: null buffer (np < n needs temp_pos and temp_memory)");
    TOC3D_REQUIRE(ld_qe >= E && ld_te >= E && ld_mem >= E && (!gb_pe || ld_gb_pe >= 2 * E) && (!gb_mem || ld_gb_mem >= 2 * E),
                  "toc3d_head_query_combine: leading dimension smaller than the row (E; 2 E for gamma | beta)");
    TOC3D_REQUIRE(mem_stride >= n * ld_mem || n <= 1, "toc3d_head_query_combine: sample stride of memory_embedding smaller than the sample");
    TOC3D_REQUIRE(np == 0 || (ld_tail >= E && query_pos_stride >= np * ld_tail && tgt_stride >= np * ld_tail),
                  "toc3d_head_query_combine: tail leading dimension / sample stride smaller than the np rows written");
    TOC3D_REQUIRE(np == n || ld_temp >= E, "toc3d_head_query_combine: ld_temp smaller than the row");
    TOC3D_REQUIRE(ld_qe % 4 == 0 && ld_te % 4 == 0 && ld_mem % 4 == 0 && mem_stride % 4 == 0 && ld_gb_pe % 4 == 0 && ld_gb_mem % 4 == 0 && ld_tail % 4 == 0 &&
                      query_pos_stride % 4 == 0 && tgt_stride % 4 == 0 && ld_temp % 4 == 0,
                  "toc3d_head_query_combine: leading dimensions and sample strides must be multiples of 4");
    TOC3D_REQUIRE(aligned(qe, 16) && aligned(gb_pe, 16) && aligned(te, 16) && aligned(ln_weight, 16) && aligned(ln_bias, 16) && aligned(memory_embedding, 16) &&
                      aligned(gb_mem, 16) && aligned(query_pos_tail, 16) && aligned(tgt_tail, 16) && aligned(temp_pos, 16) && aligned(temp_memory, 16),
                  "toc3d_head_query_combine: buffers must be 16-byte aligned");
    TOC3D_REQUIRE(n < (1ll << 31) && (n == 0 || B <= ((1ll << 31) - 5) / n), "toc3d_head_query_combine: too many rows");
    if (B * n == 0) return TOC3D_OK;
    QueryCombineArgs a;
    a.qe = qe; a.ld_qe = ld_qe; a.gb_pe = gb_pe; a.ld_gb_pe = ld_gb_pe; a.te = te; a.ld_te = ld_te; a.ln_w = ln_weight; a.ln_b = ln_bias; a.eps = ln_eps;
    a.mem = memory_embedding; a.mem_stride = mem_stride; a.ld_mem = ld_mem; a.gb_mem = gb_mem; a.ld_gb_mem = ld_gb_mem;
    a.qpos_tail = query_pos_tail; a.tgt_tail = tgt_tail; a.qpos_stride = query_pos_stride; a.tgt_stride = tgt_stride; a.ld_tail = ld_tail;
    a.temp_pos = temp_pos; a.temp_mem = temp_memory; a.ld_temp = ld_temp; a.n = (int)n; a.np = (int)np; a.rows = (int)(B * n);
    toc3d_launch(query_combine_kernel, dim3((unsigned)((B * n + 3) / 4)), dim3(256), 0, as_stream(stream), a);
    TOC3D_LAUNCH_CHECK("toc3d_head_query_combine");
    return TOC3D_OK;
}

}  // extern "C"
