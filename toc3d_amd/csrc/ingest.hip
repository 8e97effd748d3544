// Camera ingest (include/toc3d_ingest.h): Pillow's 8-bit resize (ImagingResample: integer coefficients, a horizontal pass rounded to uint8, then a vertical
// pass) and crop of raw HWC frames, bit for bit, in one launch.  A workgroup owns a 64 x 32 output tile: it stages its slices of the coefficient and bounds tables
// in LDS (one barrier), writes the horizontal pass of the source rows its vertical taps span into LDS as bytes, synchronises, and finishes the tile from LDS.  Every source
// index, tap count and intermediate row is clamped: whatever the tables hold, nothing outside the source rows is read, nothing outside the destination rows written.
#include "../../include/toc3d_ingest.h"
#include "capi.h"
#include "common.h"

namespace {

constexpr int TW = TOC3D_INGEST_TILE_W, TH = TOC3D_INGEST_TILE_H, ROWS = TOC3D_INGEST_LDS_ROWS, KMAX = TOC3D_INGEST_MAX_KSIZE;
constexpr int RPS = 4;                                                   // source rows a thread of the horizontal pass works on at a time (1, 2 and 4 measured alike)
constexpr int PITCH = TW * 3;                                            // bytes of an intermediate row: a multiple of 4
static_assert(TW == 64 && PITCH % 4 == 0, "the index arithmetic below takes 64-pixel rows");

struct IngestArgs {
    const uint8_t* src; uint8_t* dst;
    const int32_t *coef_h, *bounds_h, *coef_v, *bounds_v;
    int64_t src_stride, dst_stride;
    int H0, W0, fH, fW, ksh, ksv, max_span;
};

// bytes of the intermediate in LDS for `rows` rows, kept a multiple of 16 so that the tables behind it stay aligned
__host__ __device__ inline int inter_bytes(int rows) { return (rows * PITCH + 15) & ~15; }

TOC3D_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
// Pillow's clip8 of its 32-bit accumulator (which the sums of a resampling table never overflow; kept unsigned here so that any other table wraps, defined)
// pixel * coefficient on the full-rate 24-bit multiplier (a 32-bit integer multiply runs at a quarter of it): exact for a byte times a coefficient within
// signed 24 bits, which every resampling table's are (the host asserts it; |k| <= 2^22 up to rounding).  Of any other value its low 24 bits count.
TOC3D_DEV uint32_t mulk(uint32_t pixel, uint32_t k) { return (uint32_t)__mul24((int)pixel, (int)k); }
TOC3D_DEV uint32_t clip8(uint32_t acc) { return (uint32_t)clampi((int)acc >> 22, 0, 255); }

// DST4: the destination in 4-byte units -- dst and dst_stride multiples of 4 (the host's choice); a thread then owns 4 pixels = 12 bytes of an output row.
// KS: the source in 4-byte units for ksize_h == KS (below); 0: in bytes
template <bool DST4, int KS>
__global__ __launch_bounds__(256) void resize_crop_kernel(IngestArgs a) {
    // dynamic LDS, sized by the host from max_span and the two ksizes (at most ROWS rows and KMAX taps: 45,312 bytes): the intermediate, then the table slices
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t* inter = lds;
    int32_t* kh = reinterpret_cast<int32_t*>(lds + inter_bytes(a.max_span));
    int32_t* kv = kh + TW * a.ksh;
    int32_t* bh = kv + TH * a.ksv;
    int32_t* bv = bh + TW * 2;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, v = blockIdx.z;
    const int tw = min(TW, a.fW - x0), th = min(TH, a.fH - y0);
    for (int i = tid; i < tw * a.ksh; i += 256) kh[i] = a.coef_h[(int64_t)x0 * a.ksh + i];
    for (int i = tid; i < th * a.ksv; i += 256) kv[i] = a.coef_v[(int64_t)y0 * a.ksv + i];
    for (int i = tid; i < tw * 2; i += 256) bh[i] = a.bounds_h[(int64_t)x0 * 2 + i];
    for (int i = tid; i < th * 2; i += 256) bv[i] = a.bounds_v[(int64_t)y0 * 2 + i];
    // the source rows of this tile: from the first tap of its first output row to the last tap of its last (the bounds of a resampling table do not decrease)
    const int r0 = clampi(a.bounds_v[(int64_t)y0 * 2], 0, a.H0 - 1);
    const int64_t yl = (int64_t)(y0 + th - 1) * 2;
    const int nrows = clampi(clampi(a.bounds_v[yl], 0, a.H0 - 1) + clampi(a.bounds_v[yl + 1], 0, a.ksv) - r0, 1, min(a.max_span, a.H0 - r0));
    __syncthreads();

    // horizontal pass, bytes into LDS: a thread owns one output column (its taps and coefficients are read once) and every fourth source row, four rows at a
    // time.  Taps beyond the image are dropped (a resampling table has none), so every tap's pixel lies in its row.
    const uint8_t* src = a.src + ((int64_t)v * a.H0 + r0) * a.src_stride;
    const int hc = tid & 63, g = tid >> 6;
    if (hc < tw) {
        const int xmin = clampi(bh[2 * hc], 0, a.W0 - 1), cnt = clampi(bh[2 * hc + 1], 0, min(a.ksh, a.W0 - xmin));
        const int32_t* k = kh + hc * a.ksh;
        // KS > 0 (the host's choice: ksize_h == KS, src, src_stride and 3*W0 multiples of 4): the 3*KS bytes of a column's taps are read as the aligned dwords
        // that hold them -- a third of the load instructions -- and shifted into place; a tap past the count has weight zero.  KS == 0: byte loads.
        constexpr int NE = (3 * KS + 3) / 4, ND = NE + 1;
        const int i0 = (3 * xmin) >> 2, sh = 8 * ((3 * xmin) & 3), last = (3 * a.W0) / 4 - 1;
        uint32_t w[KS > 0 ? KS : 1];
#pragma unroll
        for (int t = 0; t < KS; ++t) w[t] = t < cnt ? (uint32_t)k[t] : 0u;
        for (int rb = g; rb < nrows; rb += 4 * RPS) {
            const uint8_t* row[RPS];
            uint32_t s[RPS][3];
#pragma unroll
            for (int u = 0; u < RPS; ++u) {
                row[u] = src + (int64_t)min(rb + 4 * u, nrows - 1) * a.src_stride;          // a row past the tile's last: that last row again, not stored
                s[u][0] = s[u][1] = s[u][2] = 1u << 21;
            }
            if (KS > 0) {
#pragma unroll
                for (int u = 0; u < RPS; ++u) {
                    const uint32_t* r32 = reinterpret_cast<const uint32_t*>(row[u]);
                    uint32_t d[ND], e[NE > 0 ? NE : 1];
#pragma unroll
                    for (int j = 0; j < ND; ++j) d[j] = r32[min(i0 + j, last)];
#pragma unroll
                    for (int j = 0; j < NE; ++j) e[j] = (uint32_t)((((uint64_t)d[j + 1] << 32) | d[j]) >> sh);
#pragma unroll
                    for (int t = 0; t < KS; ++t) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) s[u][ch] += mulk((e[(3 * t + ch) >> 2] >> (8 * ((3 * t + ch) & 3))) & 255u, w[t]);
                    }
                }
            } else {
                for (int t = 0; t < cnt; ++t) {
                    const int off = 3 * (xmin + t);
                    const uint32_t wt = (uint32_t)k[t];
#pragma unroll
                    for (int u = 0; u < RPS; ++u) {
                        const uint8_t* p = row[u] + off;
                        s[u][0] += mulk(p[0], wt); s[u][1] += mulk(p[1], wt); s[u][2] += mulk(p[2], wt);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < RPS; ++u) {
                if (rb + 4 * u < nrows) {
                    uint8_t* o = inter + (rb + 4 * u) * PITCH + hc * 3;
                    o[0] = (uint8_t)clip8(s[u][0]); o[1] = (uint8_t)clip8(s[u][1]); o[2] = (uint8_t)clip8(s[u][2]);
                }
            }
        }
    }
    __syncthreads();

    // vertical pass, from LDS
    uint8_t* dst = a.dst + ((int64_t)v * a.fH + y0) * a.dst_stride + (int64_t)x0 * 3;
    if (DST4) {
        for (int idx = tid; idx < th * (TW / 4); idx += 256) {
            const int y = idx >> 4, c = (idx & 15) * 4;
            if (c >= tw) continue;
            const int ymin = clampi(bv[2 * y], 0, a.H0 - 1) - r0, cnt = clampi(bv[2 * y + 1], 0, a.ksv);
            const int32_t* k = kv + y * a.ksv;
            uint32_t s[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) s[j] = 1u << 21;
            for (int t = 0; t < cnt; ++t) {
                const uint32_t* p = reinterpret_cast<const uint32_t*>(inter + clampi(ymin + t, 0, nrows - 1) * PITCH + c * 3);      // c % 4 == 0: 4-byte aligned
                const uint32_t w = (uint32_t)k[t];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const uint32_t d = p[q];
#pragma unroll
                    for (int b = 0; b < 4; ++b) s[q * 4 + b] += mulk((d >> (8 * b)) & 255u, w);
                }
            }
            uint8_t* o = dst + (int64_t)y * a.dst_stride + c * 3;
            if (c + 4 <= tw) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    reinterpret_cast<uint32_t*>(o)[q] = clip8(s[q * 4]) | clip8(s[q * 4 + 1]) << 8 | clip8(s[q * 4 + 2]) << 16 | clip8(s[q * 4 + 3]) << 24;
            } else {                                                     // the row's last, partial group: its valid bytes one at a time
#pragma unroll
                for (int j = 0; j < 12; ++j)
                    if (j < (tw - c) * 3) o[j] = (uint8_t)clip8(s[j]);
            }
        }
    } else {
        for (int idx = tid; idx < th * TW; idx += 256) {
            const int y = idx >> 6, c = idx & 63;
            if (c >= tw) continue;
            const int ymin = clampi(bv[2 * y], 0, a.H0 - 1) - r0, cnt = clampi(bv[2 * y + 1], 0, a.ksv);
            const int32_t* k = kv + y * a.ksv;
            uint32_t s0 = 1u << 21, s1 = 1u << 21, s2 = 1u << 21;
            for (int t = 0; t < cnt; ++t) {
                const uint8_t* p = inter + clampi(ymin + t, 0, nrows - 1) * PITCH + c * 3;
                const uint32_t w = (uint32_t)k[t];
                s0 += mulk(p[0], w); s1 += mulk(p[1], w); s2 += mulk(p[2], w);
            }
            uint8_t* o = dst + (int64_t)y * a.dst_stride + c * 3;
            o[0] = (uint8_t)clip8(s0); o[1] = (uint8_t)clip8(s1); o[2] = (uint8_t)clip8(s2);
        }
    }
}

}  // namespace

extern "C" {

int toc3d_ingest_abi(void) { return TOC3D_INGEST_ABI; }

int toc3d_resize_crop_u8(const uint8_t* src, int64_t src_stride, int64_t V, int64_t H0, int64_t W0, uint8_t* dst, int64_t dst_stride, int64_t fH, int64_t fW,
                         const int32_t* coef_h, const int32_t* bounds_h, int64_t ksize_h, const int32_t* coef_v, const int32_t* bounds_v, int64_t ksize_v,
                         int64_t max_span, toc3d_stream_t stream) {
    TOC3D_REQUIRE(src && dst && coef_h && bounds_h && coef_v && bounds_v, "toc3d_resize_crop_u8: null buffer");
    const int64_t I32 = 0x7fffffffll;
    TOC3D_REQUIRE(V > 0 && H0 > 0 && W0 > 0 && fH > 0 && fW > 0, "toc3d_resize_crop_u8: bad dims (V, H0, W0, fH, fW must be positive)");
    TOC3D_REQUIRE(V <= 65535 && H0 <= I32 / 3 && W0 <= I32 / 3 && fH <= I32 / 3 && fW <= I32 / 3 && (fH + TH - 1) / TH <= 65535,
                  "toc3d_resize_crop_u8: bad dims (image sizes must fit 31 bits as bytes, V and the tile rows one launch's grid)");
    TOC3D_REQUIRE(src_stride >= 3 * W0 && dst_stride >= 3 * fW, "toc3d_resize_crop_u8: bad strides (src_stride >= 3*W0, dst_stride >= 3*fW bytes: a stride smaller than a row)");
    TOC3D_REQUIRE(ksize_h >= 1 && ksize_h <= KMAX && ksize_v >= 1 && ksize_v <= KMAX,
                  "toc3d_resize_crop_u8: bad ksize (1 <= ksize_h, ksize_v <= %d: the coefficients of a tile must fit the kernel's LDS budget)", KMAX);
    TOC3D_REQUIRE(max_span >= 1 && max_span <= ROWS, "toc3d_resize_crop_u8: bad max_span (1 <= max_span <= %d rows of the intermediate fit the kernel's LDS budget)", ROWS);
    TOC3D_REQUIRE(toc3d_device_memory(src) && toc3d_device_memory(dst) && toc3d_device_memory(coef_h) && toc3d_device_memory(bounds_h) && toc3d_device_memory(coef_v) && toc3d_device_memory(bounds_v),
                  "toc3d_resize_crop_u8: host pointer (every buffer must be device memory)");
    IngestArgs a;
    a.src = src; a.dst = dst; a.coef_h = coef_h; a.bounds_h = bounds_h; a.coef_v = coef_v; a.bounds_v = bounds_v;
    a.src_stride = src_stride; a.dst_stride = dst_stride;
    a.H0 = (int)H0; a.W0 = (int)W0; a.fH = (int)fH; a.fW = (int)fW; a.ksh = (int)ksize_h; a.ksv = (int)ksize_v; a.max_span = (int)max_span;
    dim3 grid((unsigned)((fW + TW - 1) / TW), (unsigned)((fH + TH - 1) / TH), (unsigned)V);
    // the access width of the destination, from its pointer and stride: a tile's rows start at byte 192 tx of a row, so 4-byte units need only these two
    const size_t lds = (size_t)inter_bytes(a.max_span) + sizeof(int32_t) * (TW * a.ksh + TH * a.ksv + TW * 2 + TH * 2);       // <= 45,312 bytes: within the budget every kernel has
    // the access widths, from pointers and strides.  Destination: a tile's rows start at byte 192 tx of a row, so 4-byte units need only dst and dst_stride.
    // Source: rows of whole dwords that start on a dword, for the ksizes a bicubic resize by 0.4 or more has (1: an axis of unchanged size).
    const bool dst4 = ((uintptr_t)dst & 3) == 0 && dst_stride % 4 == 0;
    const bool src4 = ((uintptr_t)src & 3) == 0 && src_stride % 4 == 0 && (3 * W0) % 4 == 0;
    auto launch = [&](auto kernel) { toc3d_launch(kernel, grid, dim3(256), lds, as_stream(stream), a); };
    auto pick = [&](auto ks) {
        constexpr int KS = decltype(ks)::value;
        if (dst4) launch(resize_crop_kernel<true, KS>); else launch(resize_crop_kernel<false, KS>);
    };
    switch (src4 ? a.ksh : 0) {
        case 1: pick(std::integral_constant<int, 1>{}); break;
        case 5: pick(std::integral_constant<int, 5>{}); break;
        case 7: pick(std::integral_constant<int, 7>{}); break;
        case 9: pick(std::integral_constant<int, 9>{}); break;
        case 11: pick(std::integral_constant<int, 11>{}); break;
        default: pick(std::integral_constant<int, 0>{}); break;
    }
    TOC3D_LAUNCH_CHECK("toc3d_resize_crop_u8");
    return TOC3D_OK;
}

}  // extern "C"
