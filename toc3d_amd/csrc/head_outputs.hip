// Output side of StreamPETRHead (gfx950): what sits between the temporal decoder's outs_dec and the memory update / the detections.
//
// Reference: the second half of StreamPETRHead.get_transformer_outputs (dense_heads/streampetr_head.py:582-602: nan_to_num, cls_branches, reg_branches, the
// reference-point add, sigmoid, the pc_range de-normalisation) and StreamPETRHead.get_bboxes (:1051-1071) over NMSFreeCoder.decode
// (core/bbox/coders/nms_free_coder.py:39-111, denormalize_bbox core/bbox/util.py:24-51).
//
// The E -> E layers of the two towers are GEMMs (toc3d_linear_fused; the first layers of both towers read the same rows, so their weights are concatenated along
// N: the towers then live side by side in one [M, 2E] buffer, class tower in columns [0, E), box tower in [E, 2E)).  This file holds what a GEMM does badly:
//   * nan_to_num_kernel     the cleaned f32 rows (the reference returns and stores them) and the copy the first GEMM reads (act dtype, (hi, lo) planes on fp32x3);
//   * ln_relu_kernel        relu(LayerNorm(.)) on the class tower's columns and relu(.) on the box tower's, one wavefront per row, into the next GEMM's A operand;
//   * head_outputs_kernel   the towers' last LayerNorm + ReLU / ReLU on load, the two E -> 10 layers in f32 FMA from LDS-resident weights (a 10-column GEMM would pad
//                           an MFMA tile to 128 columns), + inverse_sigmoid(reference_points), sigmoid, pc_range, and the writes of all_cls_scores / all_bbox_preds;
//   * nms_free_decode_kernel  one workgroup per sample: sigmoid, the max_num best (query, class) pairs in descending order (ties: lowest flat index), box gather,
//                           denormalize_bbox, the post_center_range / score_threshold mask, compaction by a block prefix sum (no atomics: deterministic order).
// exp / log / atan2 are the libm forms (no fast-math intrinsics): scores decide a ranking.  A GEMM's A operand is stored in its three forms by put4 (act_rows.h).
#include "act_rows.h"

#include <float.h>

namespace {

// torch.nan_to_num with its defaults: NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX; everything else unchanged (bit tests: no dependence on fast-math settings)
TOC3D_DEV float nan_to_num(float x) {
    const unsigned u = __float_as_uint(x);
    if ((u & 0x7f800000u) != 0x7f800000u) return x;
    if (u & 0x007fffffu) return 0.f;
    return (u & 0x80000000u) ? -FLT_MAX : FLT_MAX;
}

template <typename T>
__global__ __launch_bounds__(256) void nan_to_num_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ out, int64_t ldo, T* __restrict__ act,
                                                         int64_t ld_act, int64_t M, int E4) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= M * E4) return;
    const int64_t row = id / E4;
    const int c = (int)(id % E4) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + row * ldx + c);
    const float y[4] = {nan_to_num(v[0]), nan_to_num(v[1]), nan_to_num(v[2]), nan_to_num(v[3])};
    if (out) store4(out + row * ldo + c, y);
    if (act) put4<T>(act + row * ld_act + c, y);
}

// One wavefront per row; a lane owns the 4 consecutive columns 4 lane + 256 i (i < 4: E <= 1024).  Statistics in f32, biased variance, two passes.
struct Row4 {
    f32x4 v[4];
};
TOC3D_DEV void load_row(const float* p, int E, int lane, Row4& r) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = 4 * lane + 256 * i;
        r.v[i] = c < E ? *reinterpret_cast<const f32x4*>(p + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
// r <- relu(LN(r; gamma, beta)) over the row's E valid columns (the others stay 0)
TOC3D_DEV void ln_relu(Row4& r, int E, int lane, const float* __restrict__ gamma, const float* __restrict__ beta, float eps) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += (r.v[i][0] + r.v[i][1]) + (r.v[i][2] + r.v[i][3]);
    const float mean = wave_sum(s) / (float)E;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (4 * lane + 256 * i < E) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = r.v[i][e] - mean; q += d * d; }
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)E + eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = 4 * lane + 256 * i;
        if (c < E) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c), b = *reinterpret_cast<const f32x4*>(beta + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) r.v[i][e] = fmaxf((r.v[i][e] - mean) * rstd * g[e] + b[e], 0.f);
        }
    }
}
TOC3D_DEV void relu(Row4& r) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) r.v[i][e] = fmaxf(r.v[i][e], 0.f);
}

// act[:, 0:E_ln] = relu(LN(x[:, 0:E_ln])), act[:, E_ln:E_ln + E_relu] = relu(x[:, E_ln:E_ln + E_relu])
template <typename T>
__global__ __launch_bounds__(256) void ln_relu_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                      T* __restrict__ act, int64_t ld_act, int M, int E_ln, int E_relu) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    if (row >= M) return;
    Row4 r;
    load_row(x + (int64_t)row * ldx, E_ln, lane, r);
    ln_relu(r, E_ln, lane, gamma, beta, eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = 4 * lane + 256 * i;
        if (c < E_ln) { const float y[4] = {r.v[i][0], r.v[i][1], r.v[i][2], r.v[i][3]}; put4<T>(act + (int64_t)row * ld_act + c, y); }
    }
    if (E_relu == 0) return;
    load_row(x + (int64_t)row * ldx + E_ln, E_relu, lane, r);
    relu(r);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = 4 * lane + 256 * i;
        if (c < E_relu) { const float y[4] = {r.v[i][0], r.v[i][1], r.v[i][2], r.v[i][3]}; put4<T>(act + (int64_t)row * ld_act + E_ln + c, y); }
    }
}

// ---- the two last layers and everything behind them -------------------------------------------------------------------------------------------------
TOC3D_DEV float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

struct HeadOutArgs {
    const float* h;                      // [M, ldh]: class tower in columns [0, E), box tower in [E, 2E), both BEFORE their last LayerNorm / ReLU
    int64_t ldh;
    const float *gamma, *beta;           // the class tower's last LayerNorm
    float eps;
    const float *w_cls, *b_cls, *w_reg, *b_reg, *ref;
    int ref_rows;                        // row m adds reference point m % ref_rows (the levels share the reference points)
    float lo[3], span[3];                // pc_range[0:3], pc_range[3:6] - pc_range[0:3]
    float* cls;
    int64_t ldc;
    float* box;
    int64_t ldb;
    int M, E, NC, CS;
};

__global__ __launch_bounds__(256) void head_outputs_kernel(const HeadOutArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_w[];                  // [NC][E] class weights, then [CS][E] box weights
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int E = a.E, nc4 = a.NC * E / 4, nr4 = a.CS * E / 4;
    for (int i = threadIdx.x; i < nc4; i += 256) reinterpret_cast<f32x4*>(s_w)[i] = reinterpret_cast<const f32x4*>(a.w_cls)[i];
    for (int i = threadIdx.x; i < nr4; i += 256) reinterpret_cast<f32x4*>(s_w)[nc4 + i] = reinterpret_cast<const f32x4*>(a.w_reg)[i];
    __syncthreads();
    const float* s_reg = s_w + a.NC * E;
    for (int64_t row64 = (int64_t)blockIdx.x * 4 + wave; row64 < a.M; row64 += (int64_t)gridDim.x * 4) {          // 64-bit: the stride may step past 2^31 near the row limit
        const int row = (int)row64;
        Row4 c, r;
        load_row(a.h + (int64_t)row * a.ldh, E, lane, c);
        load_row(a.h + (int64_t)row * a.ldh + E, E, lane, r);
        ln_relu(c, E, lane, a.gamma, a.beta, a.eps);
        relu(r);
        auto dot = [&](const Row4& v, const float* w) {                          // every lane returns the whole row's v . w
            float p = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int col = 4 * lane + 256 * i;
                if (col < E) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + col);
#pragma unroll
                    for (int e = 0; e < 4; ++e) p = fmaf(v.v[i][e], wv[e], p);
                }
            }
            return wave_sum(p);
        };
        float mine_c = 0.f, mine_r = 0.f;                                        // lane n keeps output column n
        for (int n = 0; n < a.NC; ++n) { const float p = dot(c, s_w + n * E); if (lane == n) mine_c = p; }
        for (int n = 0; n < a.CS; ++n) { const float p = dot(r, s_reg + n * E); if (lane == n) mine_r = p; }
        if (lane < a.NC) a.cls[(int64_t)row * a.ldc + lane] = mine_c + a.b_cls[lane];
        if (lane < a.CS) {
            float t = mine_r + a.b_reg[lane];
            if (lane < 3) {
                // tmp[..., 0:3] += inverse_sigmoid(reference_points); sigmoid; * (pc_range[3:6] - pc_range[0:3]) + pc_range[0:3]  (two roundings, as the reference's two ops)
                t += inverse_sigmoid(a.ref[(int64_t)(row % a.ref_rows) * 3 + lane]);
                t = __fadd_rn(__fmul_rn(sigmoidf_(t), a.span[lane]), a.lo[lane]);
            }
            a.box[(int64_t)row * a.ldb + lane] = t;
        }
    }
}

// ---- NMS-free decoding ------------------------------------------------------------------------------------------------------------------------------
// One 64-bit key per (query, class) slot whose unsigned order is the stable descending order (as the ranking kernels of tokens.hip): the score's bits made
// monotone (-0 folded onto +0), then the complemented flat index, so the lower index wins a tie.  Keys are unique.
TOC3D_DEV unsigned long long decode_key(float f, int i) {
    unsigned int u = __float_as_uint(f + 0.0f);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)i);
}

constexpr int DEC_THREADS = 1024, DEC_WAVES = DEC_THREADS / 64, DEC_SLOTS = 16;          // n = Q * num_classes <= 16384 keys, held in registers
constexpr int DEC_MAX_NUM = 2048;                                                       // two u64 lists of max_num entries in LDS

struct DecodeArgs {
    const float* cls;
    int64_t ld_cls;
    const float* bbox;
    int64_t ld_bbox;
    int Q, NC, CS, K;
    float pcr[6];
    int use_thr;
    float thr;
    int sub_half;
    float* boxes;
    float* scores;
    int64_t *labels, *qidx, *counts;
};

// exclusive prefix sum of v over the workgroup's threads (thread order), total in `total`; s_w: DEC_WAVES ints of LDS
TOC3D_DEV int block_excl_scan(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < DEC_WAVES; ++w) {
        const int t = s_w[w];
        off += w < wave ? t : 0;
        total += t;
    }
    __syncthreads();
    return off + incl - v;
}

__global__ __launch_bounds__(DEC_THREADS) void nms_free_decode_kernel(const DecodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_list[];            // cand[K] (selection order), sorted[K] (score order)
    __shared__ int s_part[2][DEC_WAVES];
    __shared__ int s_scan[DEC_WAVES];
    unsigned long long* cand = s_list;
    unsigned long long* sorted = s_list + a.K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int n = a.Q * a.NC, K = a.K;
    const float* cls = a.cls + (int64_t)b * a.Q * a.ld_cls;
    auto score_of = [&](int i) {
        const int q = i / a.NC;
        return sigmoidf_(cls[(int64_t)q * a.ld_cls + (i - q * a.NC)]);
    };
    // slot i = tid + 1024 s; absent slots get key 0, below every real key (a real key's low word is >= 0xFFFFC000)
    unsigned long long key[DEC_SLOTS];
#pragma unroll
    for (int s = 0; s < DEC_SLOTS; ++s) {
        const int i = tid + DEC_THREADS * s;
        key[s] = i < n ? decode_key(score_of(i), i) : 0ull;
    }
    // ---- the K-th largest key, bit by bit from the top: the largest T with #{key >= T} >= K.  Bits 14-31 are set in every real key.
    unsigned long long T = 0xFFFFC000ull;
    int pass = 0;
    for (int bit = 63; bit >= 0; --bit) {
        if (bit < 32 && bit >= 14) continue;
        const unsigned long long t = T | (1ull << bit);
        int c = 0;
#pragma unroll
        for (int s = 0; s < DEC_SLOTS; ++s) c += key[s] >= t ? 1 : 0;
        const float tot = wave_sum((float)c);                                     // counts <= 16384: exact in f32
        int* part = s_part[pass & 1];                                             // two buffers: one barrier per pass
        if (lane == 0) part[wave] = (int)tot;
        __syncthreads();
        int sum = 0;
#pragma unroll
        for (int w = 0; w < DEC_WAVES; ++w) sum += part[w];
        if (sum >= K) T = t;
        ++pass;
    }
    // ---- the K selected keys -> cand (thread order; the order is scratch: they are ranked next)
    {
        int c = 0;
#pragma unroll
        for (int s = 0; s < DEC_SLOTS; ++s) c += key[s] >= T ? 1 : 0;
        int total;
        int pos = block_excl_scan(c, s_scan, total);
#pragma unroll
        for (int s = 0; s < DEC_SLOTS; ++s)
            if (key[s] >= T && pos < K) cand[pos++] = key[s];
    }
    __syncthreads();
    for (int j = tid; j < K; j += DEC_THREADS) {
        const unsigned long long kj = cand[j];
        int r = 0;
        for (int m = 0; m < K; ++m) r += cand[m] > kj ? 1 : 0;
        sorted[r] = kj;
    }
    __syncthreads();
    // ---- gather, denormalize_bbox, mask, compaction in score order
    const int OW = a.CS > 8 ? 9 : 7;
    float* boxes = a.boxes + (int64_t)b * K * OW;
    float* scores = a.scores + (int64_t)b * K;
    int64_t* labels = a.labels + (int64_t)b * K;
    int64_t* qidx = a.qidx + (int64_t)b * K;
    int base = 0;
    for (int c0 = 0; c0 < K; c0 += DEC_THREADS) {
        const int r = c0 + tid;
        bool keep = false;
        float box[9], score = 0.f;
        int q = 0, label = 0;
        if (r < K) {
            const int i = (int)(0xFFFFFFFFu - (unsigned int)sorted[r]);
            q = i / a.NC;
            label = i - q * a.NC;
            score = score_of(i);
            const float* p = a.bbox + ((int64_t)b * a.Q + q) * a.ld_bbox;
            box[0] = p[0]; box[1] = p[1]; box[2] = p[2];
            box[3] = expf(p[3]); box[4] = expf(p[4]); box[5] = expf(p[5]);
            box[6] = atan2f(p[6], p[7]);
            if (OW == 9) { box[7] = p[8]; box[8] = p[9]; }
            keep = box[0] >= a.pcr[0] && box[1] >= a.pcr[1] && box[2] >= a.pcr[2] && box[0] <= a.pcr[3] && box[1] <= a.pcr[4] && box[2] <= a.pcr[5] &&
                   (!a.use_thr || score >= a.thr);
            if (a.sub_half) box[2] = box[2] - box[5] * 0.5f;                      // get_bboxes :1066, after the mask (x 0.5 is exact: one rounding either way)
        }
        int total;
        const int pos = base + block_excl_scan(keep ? 1 : 0, s_scan, total);
        if (keep) {
            for (int e = 0; e < OW; ++e) boxes[(int64_t)pos * OW + e] = box[e];
            scores[pos] = score;
            labels[pos] = label;
            qidx[pos] = q;
        }
        base += total;
    }
    for (int r = base + tid; r < K; r += DEC_THREADS) {                           // rows past the count: zeros, indices -1
        for (int e = 0; e < OW; ++e) boxes[(int64_t)r * OW + e] = 0.f;
        scores[r] = 0.f;
        labels[r] = -1;
        qidx[r] = -1;
    }
    if (tid == 0) a.counts[b] = base;
}

// the checks on an act-dtype output of a row kernel: bf16 rows as 8-byte pieces, f32 rows as 16-byte pieces, planes as whole 128-byte groups
const char* act_rows_problem(int dtype, const void* act, int64_t ld_act) {
    if (dtype == TOC3D_BF16) return aligned(act, 8) && ld_act % 4 == 0 ? nullptr : "bf16 rows must be 8-byte aligned (ld_act a multiple of 4)";
    if (dtype == TOC3D_F32) return aligned(act, 16) && ld_act % 4 == 0 ? nullptr : "f32 rows must be 16-byte aligned (ld_act a multiple of 4)";
    if (dtype == TOC3D_F32X3P) return planes_rows_ok(act, ld_act) ? nullptr : "rows of (hi, lo) planes start on 128-byte boundaries (out_act aligned, ld_act a multiple of 32)";
    return "dtype must be TOC3D_DTYPE_BF16, TOC3D_DTYPE_F32 or TOC3D_DTYPE_F32X3P";
}

}  // namespace

extern "C" {

int toc3d_head_nan_to_num_rows(int dtype, const float* x, int64_t ldx, float* out, int64_t ldo, void* out_act, int64_t ld_act, int64_t M, int64_t E,
                               toc3d_stream_t stream) {
    TOC3D_REQUIRE(x && (out || out_act) && M >= 0 && E > 0 && E % 4 == 0 && ldx >= E && ldx % 4 == 0 && aligned(x, 16),
                  "toc3d_head_nan_to_num_rows: bad arguments (E and ldx multiples of 4, x 16-byte aligned, at least one output)");
    TOC3D_REQUIRE(!out || (ldo >= E && ldo % 4 == 0 && aligned(out, 16)), "toc3d_head_nan_to_num_rows: out needs ldo >= E, a multiple of 4, 16-byte aligned rows");
    if (out_act) {
        TOC3D_REQUIRE(ld_act >= E, "toc3d_head_nan_to_num_rows: ld_act < E");
        if (const char* why = act_rows_problem(dtype, out_act, ld_act)) { toc3d_set_error("toc3d_head_nan_to_num_rows: %s", why); return TOC3D_ERR_ARG; }
        TOC3D_REQUIRE(dtype != TOC3D_F32X3P || E % 32 == 0, "toc3d_head_nan_to_num_rows: rows of (hi, lo) planes are whole 32-element groups (E a multiple of 32)");
    }
    // one thread per 4 elements on a one-dimensional grid of at most 2^31 - 1 workgroups
    TOC3D_REQUIRE(E < (1ll << 31) && M <= ((1ll << 31) - 1) * 256 / (E / 4), "toc3d_head_nan_to_num_rows: too many elements for one launch");
    if (M == 0) return TOC3D_OK;
    const dim3 grid((unsigned)((M * (E / 4) + 255) / 256));
    // (without out_act the dtype names nothing: the f32 kernel writes `out` alone)
    if (int rc = toc3d_dispatch_act<ACT_ANY>("toc3d_head_nan_to_num_rows", out_act ? dtype : TOC3D_F32, [&](auto tag) {
            using T = typename decltype(tag)::type;
            toc3d_launch(nan_to_num_kernel<T>, grid, dim3(256), 0, as_stream(stream), x, ldx, out, ldo, (T*)out_act, ld_act, M, (int)(E / 4));
        })) return rc;
    TOC3D_LAUNCH_CHECK("toc3d_head_nan_to_num_rows");
    return TOC3D_OK;
}

int toc3d_head_ln_relu_rows(int dtype, const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, void* out_act, int64_t ld_act,
                            int64_t M, int64_t E_ln, int64_t E_relu, toc3d_stream_t stream) {
    TOC3D_REQUIRE(x && gamma && beta && out_act && M >= 0 && E_ln > 0 && E_ln <= 1024 && E_relu >= 0 && E_relu <= 1024 && E_ln % 4 == 0 && E_relu % 4 == 0,
                  "toc3d_head_ln_relu_rows: bad arguments (0 < E_ln <= 1024, 0 <= E_relu <= 1024, both multiples of 4)");
    TOC3D_REQUIRE(ldx >= E_ln + E_relu && ldx % 4 == 0 && ld_act >= E_ln + E_relu, "toc3d_head_ln_relu_rows: leading dimension below E_ln + E_relu (ldx a multiple of 4)");
    TOC3D_REQUIRE(aligned(x, 16) && aligned(gamma, 16) && aligned(beta, 16), "toc3d_head_ln_relu_rows: x, gamma and beta must be 16-byte aligned");
    if (const char* why = act_rows_problem(dtype, out_act, ld_act)) { toc3d_set_error("toc3d_head_ln_relu_rows: %s", why); return TOC3D_ERR_ARG; }
    TOC3D_REQUIRE(dtype != TOC3D_F32X3P || (E_ln % 32 == 0 && E_relu % 32 == 0), "toc3d_head_ln_relu_rows: rows of (hi, lo) planes are whole 32-element groups (E_ln, E_relu multiples of 32)");
    TOC3D_REQUIRE(M < (1ll << 31) - 4, "toc3d_head_ln_relu_rows: too many rows");
    if (M == 0) return TOC3D_OK;
    const dim3 grid((unsigned)((M + 3) / 4));
    if (int rc = toc3d_dispatch_act<ACT_ANY>("toc3d_head_ln_relu_rows", dtype, [&](auto tag) {
            using T = typename decltype(tag)::type;
            toc3d_launch(ln_relu_kernel<T>, grid, dim3(256), 0, as_stream(stream), x, ldx, gamma, beta, eps, (T*)out_act, ld_act, (int)M, (int)E_ln, (int)E_relu);
        })) return rc;
    TOC3D_LAUNCH_CHECK("toc3d_head_ln_relu_rows");
    return TOC3D_OK;
}

int toc3d_head_outputs(const float* h, int64_t ldh, const float* gamma, const float* beta, float eps, const float* w_cls, const float* b_cls,
                       const float* w_reg, const float* b_reg, const float* reference_points, int64_t ref_rows, const float* pc_range,
                       float* cls_out, int64_t ld_cls, float* bbox_out, int64_t ld_bbox, int64_t M, int64_t E, int64_t num_cls, int64_t code_size,
                       toc3d_stream_t stream) {
    TOC3D_REQUIRE(h && gamma && beta && w_cls && b_cls && w_reg && b_reg && reference_points && pc_range && cls_out && bbox_out, "toc3d_head_outputs: null buffer");
    TOC3D_REQUIRE(M >= 0 && E > 0 && E <= 1024 && E % 4 == 0 && num_cls > 0 && num_cls <= 64 && code_size >= 3 && code_size <= 64 && ref_rows > 0,
                  "toc3d_head_outputs: bad dims (E <= 1024 and a multiple of 4, 1 <= num_cls <= 64, 3 <= code_size <= 64, ref_rows > 0)");
    TOC3D_REQUIRE((num_cls + code_size) * E * 4 <= 64 * 1024, "toc3d_head_outputs: the two weight blocks ((num_cls + code_size) * E floats) must fit 64 KB of LDS");
    TOC3D_REQUIRE(ldh >= 2 * E && ldh % 4 == 0 && ld_cls >= num_cls && ld_bbox >= code_size, "toc3d_head_outputs: leading dimension too small (ldh >= 2 E and a multiple of 4)");
    TOC3D_REQUIRE(aligned(h, 16) && aligned(gamma, 16) && aligned(beta, 16) && aligned(w_cls, 16) && aligned(w_reg, 16), "toc3d_head_outputs: h, gamma, beta and the weights must be 16-byte aligned");
    TOC3D_REQUIRE(M < (1ll << 31) - 4 && ref_rows < (1ll << 31), "toc3d_head_outputs: too many rows");
    if (M == 0) return TOC3D_OK;
    HeadOutArgs a;
    a.h = h; a.ldh = ldh; a.gamma = gamma; a.beta = beta; a.eps = eps; a.w_cls = w_cls; a.b_cls = b_cls; a.w_reg = w_reg; a.b_reg = b_reg;
    a.ref = reference_points; a.ref_rows = (int)ref_rows;
    for (int i = 0; i < 3; ++i) { a.lo[i] = pc_range[i]; a.span[i] = pc_range[3 + i] - pc_range[i]; }
    a.cls = cls_out; a.ldc = ld_cls; a.box = bbox_out; a.ldb = ld_bbox; a.M = (int)M; a.E = (int)E; a.NC = (int)num_cls; a.CS = (int)code_size;
    const int64_t groups = (M + 3) / 4;
    const dim3 grid((unsigned)(groups < 1024 ? groups : 1024));                   // a workgroup stages the weights once and walks its rows
    toc3d_launch(head_outputs_kernel, grid, dim3(256), (size_t)((num_cls + code_size) * E * 4), as_stream(stream), a);
    TOC3D_LAUNCH_CHECK("toc3d_head_outputs");
    return TOC3D_OK;
}

int toc3d_nms_free_decode(const float* cls_scores, int64_t ld_cls, const float* bbox_preds, int64_t ld_bbox, int64_t B, int64_t Q, int64_t num_classes,
                          int64_t code_size, int64_t max_num, const float* post_center_range, int use_threshold, float score_threshold, int sub_half_height,
                          float* boxes, float* scores, int64_t* labels, int64_t* query_index, int64_t* counts, toc3d_stream_t stream) {
    TOC3D_REQUIRE(cls_scores && bbox_preds && post_center_range && boxes && scores && labels && query_index && counts, "toc3d_nms_free_decode: null buffer");
    TOC3D_REQUIRE(B >= 0 && Q > 0 && num_classes > 0 && ld_cls >= num_classes, "toc3d_nms_free_decode: bad dims (ld_cls >= num_classes)");
    TOC3D_REQUIRE(code_size >= 8 && ld_bbox >= code_size && (code_size == 8 || code_size >= 10),
                  "toc3d_nms_free_decode: code_size must be 8 (no velocity) or >= 10 (velocity in columns 8, 9), ld_bbox >= code_size");
    TOC3D_REQUIRE(Q <= DEC_THREADS * DEC_SLOTS && num_classes <= DEC_THREADS * DEC_SLOTS && Q * num_classes <= DEC_THREADS * DEC_SLOTS,
                  "toc3d_nms_free_decode: num_query * num_classes = %lld exceeds the register-resident limit %d", (long long)(Q * num_classes), DEC_THREADS * DEC_SLOTS);
    TOC3D_REQUIRE(max_num > 0 && max_num <= DEC_MAX_NUM && max_num <= Q * num_classes,
                  "toc3d_nms_free_decode: max_num must be in [1, min(%d, num_query * num_classes)] (torch.topk refuses more than there are)", DEC_MAX_NUM);
    TOC3D_REQUIRE(B <= (1ll << 31) - 1, "toc3d_nms_free_decode: batch too large");
    if (B == 0) return TOC3D_OK;
    DecodeArgs a;
    a.cls = cls_scores; a.ld_cls = ld_cls; a.bbox = bbox_preds; a.ld_bbox = ld_bbox; a.Q = (int)Q; a.NC = (int)num_classes; a.CS = (int)code_size; a.K = (int)max_num;
    for (int i = 0; i < 6; ++i) a.pcr[i] = post_center_range[i];
    a.use_thr = use_threshold ? 1 : 0; a.thr = score_threshold; a.sub_half = sub_half_height ? 1 : 0;
    a.boxes = boxes; a.scores = scores; a.labels = labels; a.qidx = query_index; a.counts = counts;
    toc3d_launch(nms_free_decode_kernel, dim3((unsigned)B), dim3(DEC_THREADS), (size_t)(2 * max_num * 8), as_stream(stream), a);
    TOC3D_LAUNCH_CHECK("toc3d_nms_free_decode");
    return TOC3D_OK;
}

}  // extern "C"
