// Multi-head attention with STREAMED keys for the StreamPETR temporal decoder (gfx950), and the two row kernels around it.
//
// Reference: torch.nn.MultiheadAttention as PETRMultiheadAttention.forward calls it (utils/petr_transformer.py:327-332; mmcv's MultiheadAttention for
// self_attn has the same dataflow), at eval: no mask, no dropout; the decoder layer around it is PETRTemporalDecoderLayer._forward (:714-760).
// The window kernels (attention.hip, attention_rot.hip) hold a window's <= 400 keys of a 64-wide head whole in LDS.  The decoder is the opposite shape:
// head_dim 32, no RoPE, separate q and k / v row sets, 1668 (self) or 6000 (cross) keys -- more than LDS holds, so keys are streamed, flash-style.
//
// One workgroup = (a tile of 16 * QT queries, head, sample); its NW wavefronts SPLIT THE KEYS: wave w takes the 32-key chunks w, w + NW, w + 2 NW, ...
// and carries its own running (max, sum, O) per query; the partials meet in LDS and wave 0 adds them in wave order 0, 1, ..., so the result does not depend
// on timing (bit-stable from run to run).  900 queries x 8 heads are only 57 x 8 = 456 query tiles of 16: cutting the keys inside the workgroup is what
// fills the 256 CUs x 4 SIMDs without a second kernel or a global workspace (QT = 2, NW = 8: 232 workgroups x 8 wavefronts; DESIGN.md section 4b has the forms measured).
//
// Per chunk of 32 keys, as in attention_rot.hip: scores TRANSPOSED, S^T = K.Q^T -- one v_mfma_f32_16x16x32_bf16 per 16 keys with the whole head_dim as the
// K dimension (A = K rows, straight from global memory: lane (key, g) reads dims 8g .. 8g+7; B = Q, loaded once) -- so that a lane owns ONE query and
// its 8 keys sit in its own registers: the softmax statistics need one butterfly over the 4 lane groups, and P, rounded to bf16, is directly the B operand
// of O^T = V^T.P^T.  V^T (A operand: lane (dim, g) needs 8 KEYS of one dim) is the one operand that needs a transpose: the wave parks the chunk's V rows
// row-major in a private 2 KB LDS image ([key][32 dims], the two 32-byte halves of a row swapped for keys 4-7 mod 8, which makes the transposing read
// conflict-free) and reads it back with ds_read_b64_tr_b16.  The image is private to the wave: LDS operations of one wave execute in order, no barrier in the loop.
// The next chunk's K and V rows are loaded into registers before the current chunk is multiplied (register double buffer).
//
// fp32x3 (X3): q, k, v are f32; every operand is split into bf16 (hi, lo) in registers and each product is hi.hi + hi.lo + lo.hi (three MFMAs), P
// included -- P on ONE bf16 plane would put a 2^-9 relative rounding on every term of the P.V sum, the largest error of the whole layer; split, the kernel is at
// 2e-5 of f64 and six post-norm layers stay at 1.5e-5 of the reference (profiles/decoder_parity.txt).
// Softmax exp2-based on f32 scores scaled by scale * log2(e) after the MFMA (q itself is not re-rounded).
#include "act_rows.h"

namespace {

constexpr int HD = 32;
constexpr float NEG_BIG = -1.0e30f;
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lptr_t;

struct MhaArgs {
    const char *q, *k, *v, *k2, *v2;
    char* out;
    int64_t ldq, ldk, ldv, ldk2, ldv2, ldo;      // in elements
    int Nq, Nk, Nk2, heads;
    float sl2;                                   // scale * log2(e)
};

TOC3D_DEV void split8(const f32x4 a, const f32x4 b, bf16x8& hi, bf16x8& lo) {
    const float f[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const bf16_t h = (bf16_t)f[e];
        hi[e] = h;
        lo[e] = (bf16_t)(f[e] - (float)h);
    }
}

// 8 consecutive elements at p as MFMA fragment(s)
template <bool X3> TOC3D_DEV void load_frag(const char* p, bf16x8& hi, bf16x8& lo) {
    const f32x4* s = reinterpret_cast<const f32x4*>(p);
    if constexpr (X3) split8(s[0], s[1], hi, lo);
    else hi = __builtin_bit_cast(bf16x8, s[0]);
}

// the raw K / V rows of one 32-key chunk as a lane loads them: K = its two A fragments (keys r16 and 16 + r16, dims 8g ..), V = 16 dims of key lane >> 1
template <bool X3> struct RawKV {
    f32x4 k[X3 ? 4 : 2];
    f32x4 v[X3 ? 4 : 2];
};

template <bool X3, int QT, int NW>
__global__ __launch_bounds__(64 * NW) void mha_kernel(const MhaArgs a) {
    constexpr int ES = X3 ? 4 : 2;                         // bytes per element
    constexpr int VB = X3 ? 4096 : 2048;                   // V image(s) of one wave: [32 keys][64 B] hi (, lo)
    constexpr int NP = QT * 10;                            // floats of one lane's partial state: (max, sum, 8 x O) per query tile
    __shared__ __attribute__((aligned(16))) char vst[NW * VB];
    __shared__ float mrg[NW - 1][NP][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
    const int head = blockIdx.y, b = blockIdx.z, q0 = blockIdx.x * (16 * QT);
    const int NK = a.Nk + a.Nk2;
    const int64_t hoff = (int64_t)head * HD;

    bf16x8 qh[QT], ql[QT];
#pragma unroll
    for (int u = 0; u < QT; ++u) {
        int qi = q0 + u * 16 + r16;
        qi = qi < a.Nq ? qi : a.Nq - 1;                    // tail rows read a valid row; their results are not stored
        load_frag<X3>(a.q + (((int64_t)b * a.Nq + qi) * a.ldq + hoff + 8 * g) * ES, qh[u], ql[u]);
    }
    float mx[QT], sum[QT];
    f32x4 o[QT][2];
#pragma unroll
    for (int u = 0; u < QT; ++u) {
        mx[u] = NEG_BIG; sum[u] = 0.f;
        o[u][0] = f32x4{0.f, 0.f, 0.f, 0.f}; o[u][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // row j of the key list = row j of (k, v) for j < Nk, row j - Nk of (k2, v2) after that; indices past the list read its last row (masked below)
    auto krow = [&](int j) -> const char* {
        j = j < NK ? j : NK - 1;
        return j < a.Nk ? a.k + (((int64_t)b * a.Nk + j) * a.ldk + hoff) * ES : a.k2 + (((int64_t)b * a.Nk2 + (j - a.Nk)) * a.ldk2 + hoff) * ES;
    };
    auto vrow = [&](int j) -> const char* {
        j = j < NK ? j : NK - 1;
        return j < a.Nk ? a.v + (((int64_t)b * a.Nk + j) * a.ldv + hoff) * ES : a.v2 + (((int64_t)b * a.Nk2 + (j - a.Nk)) * a.ldv2 + hoff) * ES;
    };
    auto load_chunk = [&](const int c, RawKV<X3>& r) {
        const int kb = c * 32;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const f32x4* p = reinterpret_cast<const f32x4*>(krow(kb + 16 * t + r16) + 8 * g * ES);
            if constexpr (X3) { r.k[2 * t] = p[0]; r.k[2 * t + 1] = p[1]; }
            else r.k[t] = p[0];
        }
        const f32x4* p = reinterpret_cast<const f32x4*>(vrow(kb + (lane >> 1)) + 16 * (lane & 1) * ES);
#pragma unroll
        for (int i = 0; i < (X3 ? 4 : 2); ++i) r.v[i] = p[i];
    };

    char* const vw = vst + wave * VB;
    // V image: 16-byte piece ch (0..3) of key row r at piece ch ^ (((r >> 2) & 1) * 2)
    const int vr = lane >> 1;
    char* const vdst = vw + vr * 64 + ((((lane & 1) * 2) ^ (((vr >> 2) & 1) * 2)) << 4);          // this lane's two pieces are adjacent either way
    // transposing read of d-tile t: lane (i = r16, g) names row 4g + (i >> 2), dims 16t + 4 (i & 3) .. + 3, and receives keys 4g .. 4g+3 of dim 16t + i
    const int tr_row = 4 * g + (r16 >> 2);
    const char* const vsrc = vw + tr_row * 64 + ((r16 & 1) << 3);
    const int tr_piece = (r16 & 3) >> 1, tr_sw = ((tr_row >> 2) & 1) * 2;

    const int nchunks = (NK + 31) >> 5;
    RawKV<X3> cur{}, nxt{};
    if (wave < nchunks) load_chunk(wave, cur);
    for (int c = wave; c < nchunks; c += NW) {
        if (c + NW < nchunks) load_chunk(c + NW, nxt);
        const int kb = c * 32;
        // ---- V rows -> the wave's LDS image
        if constexpr (X3) {
            bf16x8 h0, l0, h1, l1;
            split8(cur.v[0], cur.v[1], h0, l0);
            split8(cur.v[2], cur.v[3], h1, l1);
            *reinterpret_cast<bf16x8*>(vdst) = h0; *reinterpret_cast<bf16x8*>(vdst + 16) = h1;
            *reinterpret_cast<bf16x8*>(vdst + 2048) = l0; *reinterpret_cast<bf16x8*>(vdst + 2048 + 16) = l1;
        } else {
            *reinterpret_cast<f32x4*>(vdst) = cur.v[0]; *reinterpret_cast<f32x4*>(vdst + 16) = cur.v[1];
        }
        __builtin_amdgcn_wave_barrier();
        Frag<bf16_t> vh[2], vl[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const char* p0 = vsrc + (((2 * t + tr_piece) ^ tr_sw) << 4);
            const s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(lptr_t)p0);
            const s16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(lptr_t)(p0 + 1024));
            vh[t].v = __builtin_bit_cast(bf16x8, __builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7));
            if constexpr (X3) {
                const s16x4 y0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(lptr_t)(p0 + 2048));
                const s16x4 y1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(lptr_t)(p0 + 2048 + 1024));
                vl[t].v = __builtin_bit_cast(bf16x8, __builtin_shufflevector(y0, y1, 0, 1, 2, 3, 4, 5, 6, 7));
            }
        }
        __builtin_amdgcn_wave_barrier();
        // ---- K fragments
        Frag<bf16_t> kh[2], kl[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if constexpr (X3) split8(cur.k[2 * t], cur.k[2 * t + 1], kh[t].v, kl[t].v);
            else kh[t].v = __builtin_bit_cast(bf16x8, cur.k[t]);
        }
        const bool tail = kb + 32 > NK;
#pragma unroll
        for (int u = 0; u < QT; ++u) {
            Frag<bf16_t> qfh, qfl;
            qfh.v = qh[u];
            f32x4 s[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (X3) {                         // small terms first
                    qfl.v = ql[u];
                    mma_step(s[t], kl[t], qfh);
                    mma_step(s[t], kh[t], qfl);
                }
                mma_step(s[t], kh[t], qfh);
            }
            float sv[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) { sv[r] = s[0][r] * a.sl2; sv[4 + r] = s[1][r] * a.sl2; }   // sv[r]: key kb + 4g + r, sv[4 + r]: key kb + 16 + 4g + r
            if (tail) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sv[r] = kb + 4 * g + r < NK ? sv[r] : NEG_BIG;
                    sv[4 + r] = kb + 16 + 4 * g + r < NK ? sv[4 + r] : NEG_BIG;
                }
            }
            const float cmax = g4_max(fmaxf(fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3])), fmaxf(fmaxf(sv[4], sv[5]), fmaxf(sv[6], sv[7]))));
            if (__builtin_amdgcn_ballot_w64(cmax > mx[u]) != 0ull) {       // wave-uniform: some query's maximum moved
                const float mnew = fmaxf(mx[u], cmax);
                const float sc = __builtin_amdgcn_exp2f(mx[u] - mnew);     // exactly 1 for a query whose maximum stayed
                sum[u] *= sc;
                o[u][0] *= sc; o[u][1] *= sc;
                mx[u] = mnew;
            }
            float pv[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) pv[r] = __builtin_amdgcn_exp2f(sv[r] - mx[u]);              // masked keys: exp2(-1e30) = 0
            sum[u] += ((pv[0] + pv[1]) + (pv[2] + pv[3])) + ((pv[4] + pv[5]) + (pv[6] + pv[7]));
            Frag<bf16_t> ph, pl;
            if constexpr (X3) {
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const bf16_t h = (bf16_t)pv[r];
                    ph.v[r] = h;
                    pl.v[r] = (bf16_t)(pv[r] - (float)h);
                }
            } else {
                ph = make_frag(pv, bf16_t());
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {                   // rows = head dims 16t + .., columns = queries
                if constexpr (X3) {
                    mma_step(o[u][t], vl[t], ph);
                    mma_step(o[u][t], vh[t], pl);
                }
                mma_step(o[u][t], vh[t], ph);
            }
        }
        cur = nxt;
    }

    // ---- the NW partial states of every query meet in LDS; wave 0 adds them in wave order
    if (wave > 0) {
#pragma unroll
        for (int u = 0; u < QT; ++u) {
            mrg[wave - 1][u * 10 + 0][lane] = mx[u];
            mrg[wave - 1][u * 10 + 1][lane] = sum[u];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) mrg[wave - 1][u * 10 + 2 + t * 4 + r][lane] = o[u][t][r];
        }
    }
    __syncthreads();
    if (wave != 0) return;
    using T = std::conditional_t<X3, float, bf16_t>;
#pragma unroll
    for (int u = 0; u < QT; ++u) {
#pragma unroll
        for (int w = 0; w < NW - 1; ++w) {
            const float mw = mrg[w][u * 10 + 0][lane];
            const float mnew = fmaxf(mx[u], mw);
            const float c0 = __builtin_amdgcn_exp2f(mx[u] - mnew), cw = __builtin_amdgcn_exp2f(mw - mnew);   // a wave without chunks: mw = -1e30, cw = 0
            sum[u] = sum[u] * c0 + mrg[w][u * 10 + 1][lane] * cw;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[u][t][r] = o[u][t][r] * c0 + mrg[w][u * 10 + 2 + t * 4 + r][lane] * cw;
            mx[u] = mnew;
        }
        const float inv = 1.f / g4_sum(sum[u]);
        const int qi = q0 + u * 16 + r16;
        if (qi < a.Nq) {
            T* dst = reinterpret_cast<T*>(a.out) + ((int64_t)b * a.Nq + qi) * a.ldo + hoff + 4 * g;
#pragma unroll
            for (int t = 0; t < 2; ++t) {                   // o[u][t][r] = O[query r16][dim 16t + 4g + r]
                T o4[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) o4[r] = to_act<T>(o[u][t][r] * inv);
                store4(dst + 16 * t, o4);
            }
        }
    }
}

// The one work split the library launches: 32 queries per workgroup, keys cut over 8 wavefronts.  Measured against 16 queries and / or 4 wavefronts at 900 queries x 8
// heads over 1668 and 6000 keys (profiles/decoder_mha_variants.txt): fastest at both key counts in both precisions.  A wave multiplies every K / V fragment it loads
// against two query tiles, and 232 workgroups x 8 waves put two waves on every SIMD of 232 CUs; key lists shorter than 8 chunks leave waves without work, at no cost.
constexpr int MHA_QT = 2, MHA_NW = 8;
template <bool X3> void launch_mha(const MhaArgs& a, int64_t B, hipStream_t s) {
    const unsigned qt = (unsigned)((a.Nq + 16 * MHA_QT - 1) / (16 * MHA_QT));
    toc3d_launch(mha_kernel<X3, MHA_QT, MHA_NW>, dim3(qt, (unsigned)a.heads, (unsigned)B), dim3(64 * MHA_NW), 0, s, a);
}

// ---- row kernels of the decoder layer: one wavefront per row, E <= 1024, statistics by DPP / permlane (common.h), two-pass variance ---------------------
// out = LN(x; gamma, beta) f32 (the residual stream); act = act(out); act_pos = act(out + pos); out2 = LN(out; gamma2, beta2) (the decoder's shared post_norm,
// written straight into the layer's slice of outs_dec).  Every output but `out` is optional.
template <typename T>
__global__ __launch_bounds__(256) void add_ln_pos_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float eps, const float* __restrict__ pos, int64_t ldp, float* __restrict__ out, int64_t ldo,
                                                         T* __restrict__ act, int64_t ld_act, T* __restrict__ act_pos, int64_t ld_act_pos,
                                                         const float* __restrict__ gamma2, const float* __restrict__ beta2, float* __restrict__ out2, int64_t ldo2,
                                                         int M, int E) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    if (row >= M) return;
    float v[16];
    auto normalise = [&](const float* g_, const float* b_) {          // v <- LN(v) over the row's E valid entries
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) s += v[i];
        const float mean = wave_sum(s) / (float)E;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) { const float d = lane + 64 * i < E ? v[i] - mean : 0.f; q += d * d; }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)E + eps);
#pragma unroll
        for (int i = 0; i < 16; ++i) { const int c = lane + 64 * i; v[i] = c < E ? (v[i] - mean) * rstd * g_[c] + b_[c] : 0.f; }
    };
#pragma unroll
    for (int i = 0; i < 16; ++i) { const int c = lane + 64 * i; v[i] = c < E ? x[(int64_t)row * ldx + c] : 0.f; }
    normalise(gamma, beta);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + 64 * i;
        if (c < E) {
            out[(int64_t)row * ldo + c] = v[i];
            if (act) act[(int64_t)row * ld_act + c] = to_act<T>(v[i]);
            if (act_pos) act_pos[(int64_t)row * ld_act_pos + c] = to_act<T>(v[i] + pos[(int64_t)row * ldp + c]);
        }
    }
    if (out2) {
        normalise(gamma2, beta2);
#pragma unroll
        for (int i = 0; i < 16; ++i) { const int c = lane + 64 * i; if (c < E) out2[(int64_t)row * ldo2 + c] = v[i]; }
    }
}

// act = act(x) and / or act_pos = act(x + pos), elementwise over [M, E] f32 rows: the decoder's inputs in the form the projections read
template <typename T>
__global__ __launch_bounds__(256) void add_pos_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ pos, int64_t ldp, T* __restrict__ act,
                                                      int64_t ld_act, T* __restrict__ act_pos, int64_t ld_act_pos, int64_t M, int E) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= M * E) return;
    const int64_t row = id / E;
    const int c = (int)(id % E);
    const float xv = x[row * ldx + c];
    if (act) act[row * ld_act + c] = to_act<T>(xv);
    if (act_pos) act_pos[row * ld_act_pos + c] = to_act<T>(xv + pos[row * ldp + c]);
}

}  // namespace

extern "C" {

int toc3d_mha_attention_ex(int dtype, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                           const void* k2, int64_t ldk2, const void* v2, int64_t ldv2, void* out, int64_t ldo,
                           int64_t B, int64_t Nq, int64_t Nk, int64_t Nk2, int64_t heads, int64_t head_dim, float scale, toc3d_stream_t stream) {
    if (head_dim != HD) { toc3d_set_error("toc3d_mha_attention: head_dim must be 32 (got %lld)", (long long)head_dim); return TOC3D_ERR_UNSUPPORTED; }
    if (dtype != TOC3D_BF16 && dtype != TOC3D_F32X3) {
        toc3d_set_error("toc3d_mha_attention: dtype must be TOC3D_DTYPE_BF16 or TOC3D_DTYPE_F32X3");
        return TOC3D_ERR_UNSUPPORTED;
    }
    TOC3D_REQUIRE(q && out && B > 0 && Nq > 0 && Nk >= 0 && Nk2 >= 0 && Nk + Nk2 > 0 && heads > 0, "toc3d_mha_attention: null buffer or empty dimension");
    TOC3D_REQUIRE((Nk == 0 || (k && v)) && (Nk2 == 0 || (k2 && v2)), "toc3d_mha_attention: null key / value buffer");
    TOC3D_REQUIRE(B <= 65535 && heads <= 65535 && Nq < (1 << 30) && Nk + Nk2 < (1 << 30), "toc3d_mha_attention: dimension too large");
    const int64_t W = heads * HD;
    TOC3D_REQUIRE(ldq >= W && ldo >= W && (Nk == 0 || (ldk >= W && ldv >= W)) && (Nk2 == 0 || (ldk2 >= W && ldv2 >= W)),
                  "toc3d_mha_attention: leading dimension below heads * 32");
    // fragments are read as 16-byte pieces: rows of 8 (bf16) / 4 (f32) element granularity on 16-byte aligned bases
    const int64_t gran = dtype == TOC3D_BF16 ? 8 : 4;
    TOC3D_REQUIRE(ldq % gran == 0 && ldo % 4 == 0 && (Nk == 0 || (ldk % gran == 0 && ldv % gran == 0)) && (Nk2 == 0 || (ldk2 % gran == 0 && ldv2 % gran == 0)),
                  "toc3d_mha_attention: leading dimensions must be multiples of 8 (bf16) / 4 (f32) elements");
    TOC3D_REQUIRE(aligned(q, 16) && aligned(out, 16) && aligned(k, 16) && aligned(v, 16) && aligned(k2, 16) && aligned(v2, 16), "toc3d_mha_attention: buffers must be 16-byte aligned");
    MhaArgs a;
    a.q = (const char*)q; a.k = (const char*)k; a.v = (const char*)v; a.k2 = (const char*)k2; a.v2 = (const char*)v2; a.out = (char*)out;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldk2 = ldk2; a.ldv2 = ldv2; a.ldo = ldo;
    a.Nq = (int)Nq; a.Nk = (int)Nk; a.Nk2 = (int)Nk2; a.heads = (int)heads;
    a.sl2 = scale * 1.4426950408889634f;
    if (dtype == TOC3D_BF16) launch_mha<false>(a, B, as_stream(stream));
    else launch_mha<true>(a, B, as_stream(stream));
    TOC3D_LAUNCH_CHECK("toc3d_mha_attention");
    return TOC3D_OK;
}

int toc3d_mha_attention(int dtype, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* out, int64_t ldo,
                        int64_t B, int64_t Nq, int64_t Nk, int64_t heads, int64_t head_dim, float scale, toc3d_stream_t stream) {
    return toc3d_mha_attention_ex(dtype, q, ldq, k, ldk, v, ldv, nullptr, 0, nullptr, 0, out, ldo, B, Nq, Nk, 0, heads, head_dim, scale, stream);
}

int toc3d_add_layernorm_pos(int dtype, const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, const float* pos, int64_t ldp,
                            float* out, int64_t ldo, void* out_act, int64_t ld_act, void* out_act_pos, int64_t ld_act_pos,
                            const float* gamma2, const float* beta2, float* out2, int64_t ldo2, int64_t M, int64_t E, toc3d_stream_t stream) {
    TOC3D_REQUIRE(x && gamma && beta && out && M >= 0 && E > 0 && E <= 1024 && ldx >= E && ldo >= E, "toc3d_add_layernorm_pos: bad arguments (E <= 1024)");
    TOC3D_REQUIRE((!out_act || ld_act >= E) && (!out_act_pos || (pos && ldp >= E && ld_act_pos >= E)) && (!out2 || (gamma2 && beta2 && ldo2 >= E)),
                  "toc3d_add_layernorm_pos: an optional output lacks its inputs");
    TOC3D_REQUIRE(M < (1ll << 31) - 4, "toc3d_add_layernorm_pos: too many rows");
    if (M == 0) return TOC3D_OK;
    dim3 grid((unsigned)((M + 3) / 4));
    if (int rc = toc3d_dispatch_act<ACT_BF16 | ACT_F32>("toc3d_add_layernorm_pos", dtype, [&](auto tag) {
            using T = typename decltype(tag)::type;
            toc3d_launch(add_ln_pos_kernel<T>, grid, dim3(256), 0, as_stream(stream), x, ldx, gamma, beta, eps, pos, ldp, out, ldo, (T*)out_act, ld_act,
                         (T*)out_act_pos, ld_act_pos, gamma2, beta2, out2, ldo2, (int)M, (int)E);
        })) return rc;
    TOC3D_LAUNCH_CHECK("toc3d_add_layernorm_pos");
    return TOC3D_OK;
}

int toc3d_add_pos_rows(int dtype, const float* x, int64_t ldx, const float* pos, int64_t ldp, void* out_act, int64_t ld_act, void* out_act_pos, int64_t ld_act_pos,
                       int64_t M, int64_t E, toc3d_stream_t stream) {
    TOC3D_REQUIRE(x && (out_act || out_act_pos) && M >= 0 && E > 0 && ldx >= E, "toc3d_add_pos_rows: bad arguments");
    TOC3D_REQUIRE((!out_act || ld_act >= E) && (!out_act_pos || (pos && ldp >= E && ld_act_pos >= E)), "toc3d_add_pos_rows: an output lacks its inputs");
    // one thread per element on a one-dimensional grid of at most 2^31 - 1 workgroups (a larger count would wrap in the cast below and cover a part of the rows only)
    TOC3D_REQUIRE(E < (1ll << 31) && M <= ((1ll << 31) - 1) * 256 / E, "toc3d_add_pos_rows: too many elements for one launch");
    if (M == 0) return TOC3D_OK;
    dim3 grid((unsigned)((M * E + 255) / 256));
    if (int rc = toc3d_dispatch_act<ACT_BF16 | ACT_F32>("toc3d_add_pos_rows", dtype, [&](auto tag) {
            using T = typename decltype(tag)::type;
            toc3d_launch(add_pos_kernel<T>, grid, dim3(256), 0, as_stream(stream), x, ldx, pos, ldp, (T*)out_act, ld_act, (T*)out_act_pos, ld_act_pos, M, (int)E);
        })) return rc;
    TOC3D_LAUNCH_CHECK("toc3d_add_pos_rows");
    return TOC3D_OK;
}

}  // extern "C"
