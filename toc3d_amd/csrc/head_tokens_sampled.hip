// Token side of StreamPETRHead.forward on the tokens an index list names (include/toc3d_sampled.h): what the reference does with topk_indexes before any
// arithmetic -- topk_gather of the per-token geometry inside position_embeding (dense_heads/streampetr_head.py:379-422) and of the feature rows in forward
// (:627-639; models/utils/misc.py:13-23).  Two kernels: the frustum points of the listed tokens (frustum_point.h: the full kernel's body, hence its bits), and a
// row gather of act rows.  Both clamp every index into [0, LEN - 1]: whatever the list holds, nothing outside the source buffers is read.
#include "../../include/toc3d_sampled.h"
#include "act_rows.h"
#include "frustum_point.h"

namespace {

TOC3D_DEV int clamp_index(int64_t i, int len) { return (int)(i < 0 ? 0 : i > (int64_t)len - 1 ? (int64_t)len - 1 : i); }

// one thread per (output row, depth bin): row r = b*K + j holds token i = index[r] of sample b -- view b*N + i / hw, pixel i % hw, camera i % N (frustum_point)
template <typename T>
__global__ __launch_bounds__(256) void frustum_sampled_kernel(FrustumArgs a, const int64_t* __restrict__ index, int K, T* __restrict__ pin, int64_t ld_pin,
                                                              T* __restrict__ cone_act, int64_t ld_cone, float* __restrict__ cone) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int hw = a.h * a.w;
    const int64_t total = (int64_t)a.B * K * a.D;
    if (id >= total) return;
    const int d = (int)(id % a.D);
    const int64_t row = id / a.D;
    const int b = (int)(row / K);
    const int i = clamp_index(index[row], a.N * hw);
    frustum_point(a, b * a.N + i / hw, i % hw, i, d, row, pin, ld_pin, cone_act, ld_cone, cone);
}

// Row gather, as bytes: one wavefront per destination row, each lane moving units of U (16 bytes; 2 bytes where the host found no 16-byte form).  PLANES: the
// valid columns of a (hi, lo) planes row are two byte streams, the hi halves and the lo halves, cut into 64-byte pieces that alternate in 128-byte groups
// (common.h, planes_addr): unit u of half-plane p sits at byte (u*|U| / 64) * 128 + p * 64 + (u*|U|) % 64.  Otherwise the valid columns are the row's first bytes.
// The wave's row, and with it the index, is wave-uniform: the index is one scalar load per wavefront.  No LDS, no atomics.
template <typename U, bool PLANES>
__global__ __launch_bounds__(256) void gather_rows_kernel(const char* __restrict__ src, int64_t src_row_bytes, const int64_t* __restrict__ index, int K, int LEN,
                                                          int64_t rows, int units, char* __restrict__ dst, int64_t dst_row_bytes) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const int64_t b = row / K;
    const int i = clamp_index(index[row], LEN);
    const char* s = src + (b * LEN + i) * src_row_bytes;
    char* o = dst + row * dst_row_bytes;
    const int half = units / 2;                                          // PLANES: units of one half-plane
    for (int q = lane; q < units; q += 64) {
        int64_t off;
        if (PLANES) {
            const int p = q >= half ? 1 : 0;
            const int byte = (q - p * half) * (int)sizeof(U);
            off = (int64_t)(byte / 64) * 128 + p * 64 + byte % 64;
        } else {
            off = (int64_t)q * (int)sizeof(U);
        }
        *reinterpret_cast<U*>(o + off) = *reinterpret_cast<const U*>(s + off);
    }
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

}  // namespace

extern "C" {

int toc3d_sampled_abi(void) { return TOC3D_SAMPLED_ABI; }

int toc3d_head_frustum_inputs_sampled(int dtype, const float* img2lidar, const float* intrinsics, const float* coords_d, const float* position_range,
                                      const int64_t* index, int64_t B, int64_t N, int64_t h, int64_t w, int64_t K, int64_t D, int64_t stride, int64_t pad_h,
                                      int64_t pad_w, void* pos_in, int64_t ld_pos, void* cone_act, int64_t ld_cone, float* cone, toc3d_stream_t stream) {
    TOC3D_REQUIRE(img2lidar && intrinsics && coords_d && position_range && index && pos_in && cone_act && cone, "toc3d_head_frustum_inputs_sampled: null buffer");
    TOC3D_REQUIRE(act_served(ACT_ANY, dtype), "toc3d_head_frustum_inputs_sampled: bad dtype");
    TOC3D_REQUIRE(B > 0 && N > 0 && h > 0 && w > 0 && stride > 0 && pad_h > 0 && pad_w > 0, "toc3d_head_frustum_inputs_sampled: bad dims (B, N, h, w, stride, pad_h, pad_w must be positive)");
    TOC3D_REQUIRE(D >= 30 && D <= 65535, "toc3d_head_frustum_inputs_sampled: bad dims (30 <= depth_num <= 65535)");
    const int64_t I32 = 0x7fffffffll;
    TOC3D_REQUIRE(B <= I32 && N <= I32 && h <= I32 && w <= I32 && stride <= 65535 && pad_h <= I32 && pad_w <= I32 && h * w <= I32 && N * h * w <= I32 &&
                  B * N <= I32 && h * stride <= I32 && w * stride <= I32, "toc3d_head_frustum_inputs_sampled: bad dims (the token count of a sample and the padded image size must fit 31 bits)");
    TOC3D_REQUIRE(K > 0 && K <= N * h * w, "toc3d_head_frustum_inputs_sampled: bad K (0 < K <= N*h*w tokens of a sample)");
    TOC3D_REQUIRE(ld_pos >= 3 * D && ld_cone >= 8, "toc3d_head_frustum_inputs_sampled: bad leading dimensions (ld_pos >= 3*depth_num, ld_cone >= 8)");
    TOC3D_PLANES_ROWS("toc3d_head_frustum_inputs_sampled", "pos_in", pos_in, ld_pos);
    TOC3D_PLANES_ROWS("toc3d_head_frustum_inputs_sampled", "cone_act", cone_act, ld_cone);
    TOC3D_REQUIRE(B * K <= I32 * 256 / D, "toc3d_head_frustum_inputs_sampled: too many rows for one launch's grid");
    FrustumArgs a;
    a.img2lidar = img2lidar; a.intrinsics = intrinsics; a.coords_d = coords_d;
    for (int i = 0; i < 6; ++i) a.pr[i] = position_range[i];              // host pointer
    a.B = (int)B; a.N = (int)N; a.h = (int)h; a.w = (int)w; a.D = (int)D; a.stride = (int)stride; a.pad_h = (int)pad_h; a.pad_w = (int)pad_w;
    const int64_t total = B * K * D;
    dim3 grid((unsigned)((total + 255) / 256));
    if (int rc = toc3d_dispatch_act<ACT_ANY>("toc3d_head_frustum_inputs_sampled", dtype, [&](auto tag) {
            using T = typename decltype(tag)::type;
            toc3d_launch(frustum_sampled_kernel<T>, grid, dim3(256), 0, as_stream(stream), a, index, (int)K, (T*)pos_in, ld_pos, (T*)cone_act, ld_cone, cone);
        })) return rc;
    TOC3D_LAUNCH_CHECK("toc3d_head_frustum_inputs_sampled");
    return TOC3D_OK;
}

int toc3d_gather_token_rows(int dtype, const void* src, int64_t ld_src, const int64_t* index, int64_t B, int64_t LEN, int64_t K, int64_t C, void* dst,
                            int64_t ld_dst, toc3d_stream_t stream) {
    TOC3D_REQUIRE(src && index && dst, "toc3d_gather_token_rows: null buffer");
    TOC3D_REQUIRE(act_served(ACT_ANY, dtype), "toc3d_gather_token_rows: bad dtype");
    const int64_t I32 = 0x7fffffffll;
    TOC3D_REQUIRE(B > 0 && LEN > 0 && C > 0 && B <= I32 && LEN <= I32 && C <= (1 << 24), "toc3d_gather_token_rows: bad dims (B, LEN, C must be positive; LEN within 31 bits, C <= 2^24)");
    TOC3D_REQUIRE(K > 0 && K <= LEN, "toc3d_gather_token_rows: bad K (0 < K <= LEN rows of a sample)");
    TOC3D_REQUIRE(ld_src >= C && ld_dst >= C, "toc3d_gather_token_rows: bad leading dimensions (ld_src >= C, ld_dst >= C)");
    TOC3D_PLANES_ROWS("toc3d_gather_token_rows", "src", src, ld_src);
    TOC3D_PLANES_ROWS("toc3d_gather_token_rows", "dst", dst, ld_dst);
    TOC3D_REQUIRE(B * K <= I32 * 4, "toc3d_gather_token_rows: too many rows for one launch's grid");
    const bool planes = dtype == TOC3D_F32X3P;
    const int64_t esz = dtype == TOC3D_BF16 ? 2 : 4;                     // bytes of an element in a row (a planes element: its two halves)
    const int64_t per16 = planes ? 8 : 16 / esz;                         // columns a 16-byte unit covers (planes: of one half)
    // the 16-byte form: every unit of every row on a 16-byte boundary -- valid width a whole number of units, rows 16-byte multiples from aligned buffers
    const bool vec = C % per16 == 0 && (ld_src * esz) % 16 == 0 && (ld_dst * esz) % 16 == 0 && aligned(src, 16) && aligned(dst, 16);
    const int64_t rows = B * K, bytes = C * esz;                         // valid bytes of a row; the scalar form moves 2-byte units
    const int units = (int)(vec ? bytes / 16 : bytes / 2);
    dim3 grid((unsigned)((rows + 3) / 4));
    auto launch = [&](auto kernel) {
        toc3d_launch(kernel, grid, dim3(256), 0, as_stream(stream), (const char*)src, ld_src * esz, index, (int)K, (int)LEN, rows, units, (char*)dst, ld_dst * esz);
    };
    if (planes) { if (vec) launch(gather_rows_kernel<u32x4, true>); else launch(gather_rows_kernel<unsigned short, true>); }
    else { if (vec) launch(gather_rows_kernel<u32x4, false>); else launch(gather_rows_kernel<unsigned short, false>); }
    TOC3D_LAUNCH_CHECK("toc3d_gather_token_rows");
    return TOC3D_OK;
}

}  // extern "C"
