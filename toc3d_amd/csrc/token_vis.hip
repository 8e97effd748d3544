// Token selection overlays (include/toc3d_vis.h): the reference's token_selection_vis (models/utils/token_select_vis.py:27-80) as uint8 pixels made on the device.
// toc3d_token_alpha turns a stage's mask and keep list into one alpha byte per token (a workgroup per view, the keep list scattered into an LDS table);
// toc3d_token_vis_render reads every source pixel once, denormalises it (or takes the raw byte) and stores it into the ori image and, with the token's alpha, into
// every RGBA plane.  Every float product and sum is rounded on its own (contraction switched off where they are formed: the reference's two ops, no FMA).
#include "../../include/toc3d_vis.h"
#include "capi.h"
#include "common.h"
#include "vis_pixel.h"                                   // sat_u8, mul_then_add, denorm_byte: the image byte; group_byte, store_group: four pixels in three dwords -- shared with box_vis.hip

namespace {

constexpr int MAXT = TOC3D_VIS_MAX_TOKENS;
static_assert(MAXT % 4 == 0 && MAXT >= 5000, "the membership table is cleared in dwords and covers 1600 x 800 at patch 16");

TOC3D_DEV uint32_t alpha_byte(float m, float lo, float span) {
#pragma clang fp contract(off)
    return sat_u8(255.f * mul_then_add(m, span, lo));
}

__global__ __launch_bounds__(256) void token_alpha_kernel(const float* mask, const int64_t* keep, int64_t keep_stride, int K, int T, float lo, float span,
                                                          uint8_t* alpha_mask, uint8_t* alpha_keep) {
    __shared__ __attribute__((aligned(16))) uint8_t member[MAXT];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * T;
    for (int i = tid; i < T; i += 256) alpha_mask[base + i] = (uint8_t)alpha_byte(mask[base + i], lo, span);
    if (alpha_keep == nullptr) return;                                   // (the same for every thread of the launch)
    uint32_t* m32 = reinterpret_cast<uint32_t*>(member);
    for (int i = tid; i < (T + 3) / 4; i += 256) m32[i] = 0u;            // (T + 3) / 4 * 4 <= MAXT
    __syncthreads();
    const int64_t* row = keep + (int64_t)blockIdx.x * keep_stride;
    for (int j = tid; j < K; j += 256) {
        const int64_t t = row[j];
        if (t >= 0 && t < T) member[t] = 1;                              // an index out of range is ignored; a duplicate stores the same byte again
    }
    __syncthreads();
    const uint8_t in = (uint8_t)alpha_byte(1.f, lo, span), out = (uint8_t)alpha_byte(0.f, lo, span);
    for (int i = tid; i < T; i += 256) alpha_keep[base + i] = member[i] ? in : out;
}

struct VisArgs {
    const void* src; const uint8_t* alpha; uint8_t* ori; uint8_t* rgba;
    int64_t src_stride;
    int V, H0, W0, H, W, patch, wp, T, A, to_rgb;
    float mean[3], sd[3];
};

// the three array bytes of pixel (v, y, x), one element at a time
template <bool U8>
TOC3D_DEV void pixel_bytes(const VisArgs& a, int v, int y, int x, uint32_t b[3]) {
    if (U8) {
        if (y < a.H0 && x < a.W0) {
            const uint8_t* p = static_cast<const uint8_t*>(a.src) + ((int64_t)v * a.H0 + y) * a.src_stride + (int64_t)x * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) b[c] = p[a.to_rgb ? 2 - c : c];
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) b[c] = sat_u8(a.mean[c]);
        }
    } else {
        const float* p = static_cast<const float*>(a.src) + ((int64_t)v * 3 * a.H + y) * a.W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) b[c] = denorm_byte(p[(int64_t)c * a.H * a.W], a.sd[c], a.mean[c]);
    }
}

// Wide form (W % 4 == 0, rgba 16-byte aligned, ori 4-byte aligned): a thread owns pixels [x, x + 4) of row y of view v.  SRCW: the source in wide units (f32:
// 16-byte loads, src 16-byte aligned; u8: dwords, src and src_stride multiples of 4) where the four pixels lie in the source.
template <bool U8, bool SRCW>
__global__ __launch_bounds__(256) void vis_render_wide_kernel(VisArgs a) {
    const int W4 = a.W >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)a.H * W4) return;
    const int y = (int)(idx / W4), x = (int)(idx % W4) * 4, v = blockIdx.y;
    uint32_t b[4][3];
    bool done = false;
    if (SRCW) {
        if (U8) {
            if (y < a.H0 && x + 4 <= a.W0) {
                // byte 3x of a row that starts on a dword: a multiple of 12
                const uint32_t* p = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(a.src) + ((int64_t)v * a.H0 + y) * a.src_stride + (int64_t)x * 3);
                const uint32_t d[3] = {p[0], p[1], p[2]};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const uint32_t plain = group_byte(d, 3 * q + c), swapped = group_byte(d, 3 * q + 2 - c);
                        b[q][c] = a.to_rgb ? swapped : plain;
                    }
                }
                done = true;
            }
        } else {
            const float* p = static_cast<const float*>(a.src) + ((int64_t)v * 3 * a.H + y) * a.W + x;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 f = *reinterpret_cast<const float4*>(p + (int64_t)c * a.H * a.W);
                b[0][c] = denorm_byte(f.x, a.sd[c], a.mean[c]); b[1][c] = denorm_byte(f.y, a.sd[c], a.mean[c]);
                b[2][c] = denorm_byte(f.z, a.sd[c], a.mean[c]); b[3][c] = denorm_byte(f.w, a.sd[c], a.mean[c]);
            }
            done = true;
        }
    }
    if (!done) {
#pragma unroll
        for (int q = 0; q < 4; ++q) pixel_bytes<U8>(a, v, y, x + q, b[q]);
    }
    const int64_t pix = ((int64_t)v * a.H + y) * a.W + x;
    store_group(a.ori + pix * 3, b);
    uint32_t rgb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) rgb[q] = b[q][0] | b[q][1] << 8 | b[q][2] << 16;
    // the tokens of the four pixels: x / patch, stepped (patch may be smaller than 4)
    int t[4];
    {
        int tx = x / a.patch, r = x - tx * a.patch;
        const int trow = (y / a.patch) * a.wp;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            t[q] = trow + tx;
            if (++r == a.patch) { r = 0; ++tx; }
        }
    }
    for (int pl = 0; pl < a.A; ++pl) {
        const uint8_t* al = a.alpha + ((int64_t)pl * a.V + v) * a.T;
        uint4 px;
        px.x = rgb[0] | (uint32_t)al[t[0]] << 24; px.y = rgb[1] | (uint32_t)al[t[1]] << 24;
        px.z = rgb[2] | (uint32_t)al[t[2]] << 24; px.w = rgb[3] | (uint32_t)al[t[3]] << 24;
        *reinterpret_cast<uint4*>(a.rgba + (((int64_t)pl * a.V + v) * a.H * a.W + (int64_t)y * a.W + x) * 4) = px;
    }
}

// Narrow form: a thread owns one pixel.  RGBA4: rgba 4-byte aligned, a pixel of a plane is one dword; bytes otherwise.  ori in bytes.
template <bool U8, bool RGBA4>
__global__ __launch_bounds__(256) void vis_render_narrow_kernel(VisArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)a.H * a.W) return;
    const int y = (int)(idx / a.W), x = (int)(idx % a.W), v = blockIdx.y;
    uint32_t b[3];
    pixel_bytes<U8>(a, v, y, x, b);
    const int64_t pix = ((int64_t)v * a.H + y) * a.W + x;
    uint8_t* o = a.ori + pix * 3;
    o[0] = (uint8_t)b[0]; o[1] = (uint8_t)b[1]; o[2] = (uint8_t)b[2];
    const int t = (y / a.patch) * a.wp + x / a.patch;
    for (int pl = 0; pl < a.A; ++pl) {
        const uint32_t al = a.alpha[((int64_t)pl * a.V + v) * a.T + t];
        uint8_t* r = a.rgba + (((int64_t)pl * a.V + v) * a.H * a.W + (int64_t)y * a.W + x) * 4;
        if (RGBA4) {
            *reinterpret_cast<uint32_t*>(r) = b[0] | b[1] << 8 | b[2] << 16 | al << 24;
        } else {
            r[0] = (uint8_t)b[0]; r[1] = (uint8_t)b[1]; r[2] = (uint8_t)b[2]; r[3] = (uint8_t)al;
        }
    }
}

}  // namespace

extern "C" {

int toc3d_vis_abi(void) { return TOC3D_VIS_ABI; }

int toc3d_token_alpha(const float* mask, const int64_t* keep, int64_t keep_stride, int64_t K, int64_t V, int64_t T, double min_alpha, double max_alpha,
                      uint8_t* alpha_mask, uint8_t* alpha_keep, toc3d_stream_t stream) {
    TOC3D_REQUIRE(mask && alpha_mask, "toc3d_token_alpha: null buffer");
    TOC3D_REQUIRE(V > 0 && T > 0 && K >= 0, "toc3d_token_alpha: bad dims (V and T must be positive, K not negative)");
    TOC3D_REQUIRE(V <= 0x7fffffffll, "toc3d_token_alpha: bad dims (V must fit one launch's grid)");
    TOC3D_REQUIRE(T <= MAXT, "toc3d_token_alpha: bad dims (T <= %d = TOC3D_VIS_MAX_TOKENS: a view's membership table must fit the kernel's LDS)", MAXT);
    const bool with_keep = alpha_keep != nullptr;
    const int64_t Kk = with_keep ? K : 0;
    TOC3D_REQUIRE(!with_keep || keep || K == 0, "toc3d_token_alpha: null buffer (keep, with alpha_keep given and K > 0)");
    TOC3D_REQUIRE(Kk == 0 || keep_stride >= K, "toc3d_token_alpha: bad strides (keep_stride >= K elements: a stride smaller than a row)");
    TOC3D_REQUIRE(Kk <= 0x7fffffffll, "toc3d_token_alpha: bad dims (K must fit 31 bits)");
    TOC3D_REQUIRE(toc3d_device_memory(mask) && toc3d_device_memory(alpha_mask) && (!with_keep || toc3d_device_memory(alpha_keep)) && (Kk == 0 || toc3d_device_memory(keep)),
                  "toc3d_token_alpha: host pointer (every buffer must be device memory)");
    toc3d_launch(token_alpha_kernel, dim3((unsigned)V), dim3(256), 0, as_stream(stream), mask, Kk ? keep : nullptr, keep_stride, (int)Kk, (int)T, (float)min_alpha,
                 (float)(max_alpha - min_alpha), alpha_mask, alpha_keep);
    TOC3D_LAUNCH_CHECK("toc3d_token_alpha");
    return TOC3D_OK;
}

int toc3d_token_vis_render(const void* src, int src_u8, int64_t src_stride, int64_t V, int64_t H0, int64_t W0, int64_t H, int64_t W, int64_t patch,
                           const uint8_t* alpha, int64_t A, float mean0, float mean1, float mean2, float std0, float std1, float std2, int to_rgb,
                           uint8_t* ori, uint8_t* rgba, toc3d_stream_t stream) {
    TOC3D_REQUIRE(src && alpha && ori && rgba, "toc3d_token_vis_render: null buffer");
    TOC3D_REQUIRE(A > 0 && V > 0 && H0 > 0 && W0 > 0 && H > 0 && W > 0 && patch > 0, "toc3d_token_vis_render: bad dims (A, V, H0, W0, H, W and patch must be positive)");
    TOC3D_REQUIRE(V <= 65535 && A <= 65535 && H <= 0x7fffffffll && W <= 0x7fffffffll && H * W <= 0x7fffffffll,
                  "toc3d_token_vis_render: bad dims (V and A at most 65535, H * W below 2^31: one launch's grid)");
    TOC3D_REQUIRE(H % patch == 0 && W % patch == 0, "toc3d_token_vis_render: bad dims (H and W must be multiples of patch)");
    if (src_u8) TOC3D_REQUIRE(H0 <= H && W0 <= W, "toc3d_token_vis_render: bad dims (the source H0 x W0 must lie inside the padded H x W)");
    else TOC3D_REQUIRE(H0 == H && W0 == W, "toc3d_token_vis_render: bad dims (an f32 source has the padded size: H0 == H and W0 == W)");
    const int64_t T = (H / patch) * (W / patch);
    TOC3D_REQUIRE(T <= MAXT, "toc3d_token_vis_render: bad dims ((H/patch)*(W/patch) <= %d = TOC3D_VIS_MAX_TOKENS)", MAXT);
    TOC3D_REQUIRE(!src_u8 || src_stride >= 3 * W0, "toc3d_token_vis_render: bad strides (src_stride >= 3*W0 bytes: a stride smaller than a row)");
    TOC3D_REQUIRE(src_u8 || ((uintptr_t)src & 3) == 0, "toc3d_token_vis_render: bad alignment (an f32 source starts on a 4-byte boundary)");
    TOC3D_REQUIRE(toc3d_device_memory(src) && toc3d_device_memory(alpha) && toc3d_device_memory(ori) && toc3d_device_memory(rgba),
                  "toc3d_token_vis_render: host pointer (every buffer must be device memory)");
    VisArgs a;
    a.src = src; a.alpha = alpha; a.ori = ori; a.rgba = rgba; a.src_stride = src_stride;
    a.V = (int)V; a.H0 = (int)H0; a.W0 = (int)W0; a.H = (int)H; a.W = (int)W; a.patch = (int)patch; a.wp = (int)(W / patch); a.T = (int)T; a.A = (int)A;
    a.to_rgb = to_rgb ? 1 : 0;
    a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2; a.sd[0] = std0; a.sd[1] = std1; a.sd[2] = std2;
    // the access widths, from pointers, strides and W
    const bool wide = W % 4 == 0 && ((uintptr_t)rgba & 15) == 0 && ((uintptr_t)ori & 3) == 0;
    const bool srcw = src_u8 ? ((uintptr_t)src & 3) == 0 && src_stride % 4 == 0 : ((uintptr_t)src & 15) == 0;
    const bool rgba4 = ((uintptr_t)rgba & 3) == 0;
    const int64_t threads = wide ? H * (W / 4) : H * W;
    dim3 grid((unsigned)((threads + 255) / 256), (unsigned)V);
    auto launch = [&](auto kernel) { toc3d_launch(kernel, grid, dim3(256), 0, as_stream(stream), a); };
    if (wide) {
        if (src_u8) { if (srcw) launch(vis_render_wide_kernel<true, true>); else launch(vis_render_wide_kernel<true, false>); }
        else { if (srcw) launch(vis_render_wide_kernel<false, true>); else launch(vis_render_wide_kernel<false, false>); }
    } else {
        if (src_u8) { if (rgba4) launch(vis_render_narrow_kernel<true, true>); else launch(vis_render_narrow_kernel<true, false>); }
        else { if (rgba4) launch(vis_render_narrow_kernel<false, true>); else launch(vis_render_narrow_kernel<false, false>); }
    }
    TOC3D_LAUNCH_CHECK("toc3d_token_vis_render");
    return TOC3D_OK;
}

}  // extern "C"
