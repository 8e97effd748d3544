// Predicted 3-D boxes on the camera views and a top-down panel (include/toc3d_boxes.h): what mmdet3d's draw_lidar_bbox3d_on_img (core/visualizer/image_vis.py:61-126)
// draws with cv2.line on the host, as uint8 pixels made on the device.  toc3d_box_segments / toc3d_box_segments_bev turn the decoded boxes into integer segment
// tables (corners of lidar_box3d.py:50-90, near-plane clip before the division, Liang-Barsky against the guarded image rectangle); toc3d_segments_render writes
// every pixel once: TokenVis's image byte (vis_pixel.h) unless a segment covers it, by a rule stated in integers.
#include "../../include/toc3d_boxes.h"
#include "capi.h"
#include "common.h"
#include "vis_pixel.h"

namespace {

constexpr int EC = TOC3D_BOXES_CAMERA_EDGES, EB = TOC3D_BOXES_BEV_EDGES, TW = TOC3D_BOXES_TILE_W, TH = TOC3D_BOXES_TILE_H, CHUNK = 256;
constexpr int MAX_SIDE = TOC3D_BOXES_MAX_SIDE, MAX_GUARD = TOC3D_BOXES_MAX_GUARD, MAX_T = TOC3D_BOXES_MAX_THICKNESS;
static_assert(TW * TH == 4 * CHUNK && TW % 4 == 0, "256 threads, four consecutive pixels of a row each");
// the twelve edges of image_vis.py:77, a nibble each, edge 0 lowest: (0,1) (0,3) (0,4) (1,2) (1,5) (3,2) (3,7) (4,5) (4,7) (2,6) (5,6) (6,7)
constexpr unsigned long long EDGE_A = 0x652443311000ull, EDGE_B = 0x766757252431ull;
constexpr int NONE = 0x7fffffff;

// corner k of lidar_box3d.py:50-90, before the rotation: the unit offset (k >> 2, (k >> 1) & 1, (k ^ k >> 1) & 1) minus (0.5, 0.5, 0), times the size
TOC3D_DEV void box_corner_xy(int k, float x, float y, float dx, float dy, float sn, float cs, float& cx, float& cy) {
    const float lx = (k >> 2) ? 0.5f * dx : -0.5f * dx, ly = ((k >> 1) & 1) ? 0.5f * dy : -0.5f * dy;
    cx = (lx * cs - ly * sn) + x;                                        // structures/utils.py:79-106
    cy = (lx * sn + ly * cs) + y;
}

// Liang-Barsky against [xmin, xmax] x [ymin, ymax]; false: nothing inside, or a coordinate that is not finite.  The ends of a kept segment are set into the
// rectangle, which absorbs the rounding of x0 + t * dx.
TOC3D_DEV bool clip_rect(float& x0, float& y0, float& x1, float& y1, float xmin, float ymin, float xmax, float ymax) {
    if (!(isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1))) return false;
    const float dx = x1 - x0, dy = y1 - y0;
    const float p[4] = {-dx, dx, -dy, dy}, q[4] = {x0 - xmin, xmax - x0, y0 - ymin, ymax - y0};
    float t0 = 0.f, t1 = 1.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (p[i] == 0.f) {
            if (q[i] < 0.f) return false;
        } else {
            const float r = q[i] / p[i];
            if (p[i] < 0.f) {
                if (r > t1) return false;
                t0 = fmaxf(t0, r);
            } else {
                if (r < t0) return false;
                t1 = fminf(t1, r);
            }
        }
    }
    const float ax = t0 > 0.f ? x0 + t0 * dx : x0, ay = t0 > 0.f ? y0 + t0 * dy : y0;
    const float bx = t1 < 1.f ? x0 + t1 * dx : x1, by = t1 < 1.f ? y0 + t1 * dy : y1;
    if (!(isfinite(ax) && isfinite(ay) && isfinite(bx) && isfinite(by))) return false;
    x0 = fminf(fmaxf(ax, xmin), xmax); y0 = fminf(fmaxf(ay, ymin), ymax);
    x1 = fminf(fmaxf(bx, xmin), xmax); y1 = fminf(fmaxf(by, ymin), ymax);
    return true;
}

TOC3D_DEV void store_segment(float* segf, int32_t* segi, uint8_t* cidx, int64_t s, bool drawn, float x0, float y0, float x1, float y1, uint8_t colour) {
    if (!drawn) x0 = y0 = x1 = y1 = 0.f;
    float* f = segf + s * 4;
    int32_t* i = segi + s * 4;
    f[0] = x0; f[1] = y0; f[2] = x1; f[3] = y1;
    i[0] = (int32_t)rintf(x0); i[1] = (int32_t)rintf(y0); i[2] = (int32_t)rintf(x1); i[3] = (int32_t)rintf(y1);
    cidx[s] = drawn ? colour : (uint8_t)255;
}

struct BoxRow {
    float x, y, z, dx, dy, dz, yaw;
    bool live;                                                           // score, label and the seven columns allow drawing
    uint8_t colour;
};

TOC3D_DEV BoxRow load_box(const float* boxes, int64_t box_stride, const float* scores, const int64_t* labels, int b, float score_thr, int num_colors) {
    const float* r = boxes + (int64_t)b * box_stride;
    BoxRow o;
    o.x = r[0]; o.y = r[1]; o.z = r[2]; o.dx = r[3]; o.dy = r[4]; o.dz = r[5]; o.yaw = r[6];
    const int64_t lab = labels[b];
    const bool finite = isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(o.dx) && isfinite(o.dy) && isfinite(o.dz) && isfinite(o.yaw);
    o.live = finite && !(scores[b] < score_thr) && lab >= 0 && lab < num_colors;
    o.colour = (uint8_t)(o.live ? lab : 255);
    return o;
}

// one thread per (view, box)
__global__ __launch_bounds__(256) void box_segments_kernel(const float* boxes, int64_t box_stride, const float* scores, const int64_t* labels, int n, float score_thr,
                                                           int num_colors, const float* proj, int V, float near, float xmin, float ymin, float xmax, float ymax,
                                                           float* segf, int32_t* segi, uint8_t* cidx) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)V * n) return;
    const int v = (int)(idx / n), b = (int)(idx % n);
    const BoxRow o = load_box(boxes, box_stride, scores, labels, b, score_thr, num_colors);
    float P[16];
    bool live = o.live;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        P[i] = proj[(int64_t)v * 16 + i];
        live = live && isfinite(P[i]);
    }
    float sn, cs;
    sincosf(o.yaw, &sn, &cs);
    float hx[8], hy[8], hz[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float cx, cy;
        box_corner_xy(k, o.x, o.y, o.dx, o.dy, sn, cs, cx, cy);
        const float cz = ((k ^ (k >> 1)) & 1) ? o.z + o.dz : o.z;
        hx[k] = P[0] * cx + P[1] * cy + P[2] * cz + P[3];
        hy[k] = P[4] * cx + P[5] * cy + P[6] * cz + P[7];
        hz[k] = P[8] * cx + P[9] * cy + P[10] * cz + P[11];
    }
    const int64_t s0 = idx * EC;
#pragma unroll
    for (int e = 0; e < EC; ++e) {
        const int ka = (int)((EDGE_A >> (4 * e)) & 15), kb = (int)((EDGE_B >> (4 * e)) & 15);
        float ax = hx[ka], ay = hy[ka], az = hz[ka], bx = hx[kb], by = hy[kb], bz = hz[kb];
        const bool a_behind = az < near, b_behind = bz < near;
        bool drawn = live && !(a_behind && b_behind);
        if (a_behind != b_behind) {                                      // the point of depth `near` on the 3-D edge: h interpolated before the division
            const float t = (near - az) / (bz - az);
            const float mx = ax + t * (bx - ax), my = ay + t * (by - ay);
            if (a_behind) { ax = mx; ay = my; az = near; }
            else { bx = mx; by = my; bz = near; }
        }
        float x0 = ax / az, y0 = ay / az, x1 = bx / bz, y1 = by / bz;
        drawn = drawn && clip_rect(x0, y0, x1, y1, xmin, ymin, xmax, ymax);
        store_segment(segf, segi, cidx, s0 + e, drawn, x0, y0, x1, y1, o.colour);
    }
}

// one thread per box: the footprint (0,3) (3,7) (7,4) (4,0) and the heading stroke from the centre to the middle of edge (4,7)
__global__ __launch_bounds__(256) void box_segments_bev_kernel(const float* boxes, int64_t box_stride, const float* scores, const int64_t* labels, int n,
                                                               float score_thr, int num_colors, float half, float scale, float xmin, float xmax, float* segf,
                                                               int32_t* segi, uint8_t* cidx) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    const BoxRow o = load_box(boxes, box_stride, scores, labels, b, score_thr, num_colors);
    float sn, cs;
    sincosf(o.yaw, &sn, &cs);
    float col[6], row[6];                                                // corners 0, 3, 7, 4, the centre, the middle of (4,7)
    const int order[4] = {0, 3, 7, 4};
    float wx[4], wy[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        box_corner_xy(order[j], o.x, o.y, o.dx, o.dy, sn, cs, wx[j], wy[j]);
        col[j] = half - wy[j] * scale;
        row[j] = half - wx[j] * scale;
    }
    col[4] = half - o.y * scale;
    row[4] = half - o.x * scale;
    col[5] = half - (0.5f * (wy[2] + wy[3])) * scale;
    row[5] = half - (0.5f * (wx[2] + wx[3])) * scale;
    const int ea[EB] = {0, 1, 2, 3, 4}, eb[EB] = {1, 2, 3, 0, 5};
#pragma unroll
    for (int e = 0; e < EB; ++e) {
        float x0 = col[ea[e]], y0 = row[ea[e]], x1 = col[eb[e]], y1 = row[eb[e]];
        const bool drawn = o.live && clip_rect(x0, y0, x1, y1, xmin, xmin, xmax, xmax);
        store_segment(segf, segi, cidx, (int64_t)b * EB + e, drawn, x0, y0, x1, y1, o.colour);
    }
}

// the coverage rule of the header; tt = t * t.  First-level products in int32, second-level in int64 (bounds: the header)
TOC3D_DEV bool covers(int px, int py, int x0, int y0, int x1, int y1, int tt) {
    const int dx = x1 - x0, dy = y1 - y0, qx = px - x0, qy = py - y0;
    const int dd = dx * dx + dy * dy, u = qx * dx + qy * dy;
    if (dd == 0 || u <= 0) return 4 * (qx * qx + qy * qy) <= tt;
    if (u >= dd) {
        const int rx = qx - dx, ry = qy - dy;
        return 4 * (rx * rx + ry * ry) <= tt;
    }
    const int64_t c = qx * dy - qy * dx;
    return 4 * c * c <= (int64_t)tt * dd;
}

struct RenderArgs {
    const void* src; const int32_t* segi; const uint8_t* cidx; const uint8_t* palette; uint8_t* out;
    int64_t src_stride;
    int V, H, W, nseg, ncol, t, guard, to_rgb, tiles_x;
    uint32_t bg[3];
    float mean[3], sd[3];
};

// KIND: 0 f32 NCHW, 1 u8 HWC, 2 none.  SRCW: the source in wide units where the thread's four pixels lie in it.  OUTW: three dwords a thread (W % 4 == 0, out
// 4-byte aligned); bytes otherwise.
template <int KIND, bool SRCW, bool OUTW>
__global__ __launch_bounds__(256) void segments_render_kernel(RenderArgs a) {
    __shared__ int4 s_seg[CHUNK];
    __shared__ unsigned long long s_hit[CHUNK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int X0 = (int)(blockIdx.x % a.tiles_x) * TW, Y0 = (int)(blockIdx.x / a.tiles_x) * TH, v = blockIdx.y;
    const int y = Y0 + tid / (TW / 4), x = X0 + (tid % (TW / 4)) * 4;
    const int grow = (a.t + 1) / 2, tt = a.t * a.t;
    const int32_t* segv = a.segi + (int64_t)v * a.nseg * 4;
    const uint8_t* cv = a.cidx + (int64_t)v * a.nseg;
    int best[4] = {NONE, NONE, NONE, NONE};
    for (int base = 0; base < a.nseg; base += CHUNK) {                   // (nseg < 2^31 - 256: base + tid does not wrap)
        const int s = base + tid;
        bool hit = false;
        int4 g = make_int4(0, 0, 0, 0);
        if (s < a.nseg && cv[s] < a.ncol) {
            const int32_t* p = segv + (int64_t)s * 4;
            g = make_int4(p[0], p[1], p[2], p[3]);
            const int lox = min(g.x, g.z), hix = max(g.x, g.z), loy = min(g.y, g.w), hiy = max(g.y, g.w);
            if (lox >= -a.guard && hix <= a.W - 1 + a.guard && loy >= -a.guard && hiy <= a.H - 1 + a.guard)      // (which also bounds the sums below)
                hit = hix + grow >= X0 && lox - grow <= X0 + TW - 1 && hiy + grow >= Y0 && loy - grow <= Y0 + TH - 1;
        }
        s_seg[tid] = g;
        const unsigned long long m = __ballot(hit);
        if (lane == 0) s_hit[wave] = m;
        __syncthreads();
        // the hits in rising index: the first segment that covers a pixel is its smallest
#pragma unroll
        for (int h = 0; h < CHUNK / 32; ++h) {
            const unsigned long long mm = s_hit[h >> 1];
            uint32_t bits = __builtin_amdgcn_readfirstlane((uint32_t)(h & 1 ? mm >> 32 : mm));
            while (bits) {
                const int j = h * 32 + __builtin_ctz(bits);
                bits &= bits - 1;
                const int4 q = s_seg[j];
                if (y < min(q.y, q.w) - grow || y > max(q.y, q.w) + grow) continue;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (best[k] == NONE && covers(x + k, y, q.x, q.y, q.z, q.w, tt)) best[k] = base + j;
            }
        }
        __syncthreads();
    }
    if (y >= a.H || x >= a.W) return;
    // the base: TokenVis's image byte, red first
    uint32_t b[4][3];
    if (KIND == 2) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) b[k][c] = a.bg[c];
    } else if (KIND == 1) {
        const uint8_t* p = static_cast<const uint8_t*>(a.src) + ((int64_t)v * a.H + y) * a.src_stride + (int64_t)x * 3;
        if (SRCW && x + 4 <= a.W) {                                      // byte 3x of a row that starts on a dword: a multiple of 12
            const uint32_t* pw = reinterpret_cast<const uint32_t*>(p);
            const uint32_t d[3] = {pw[0], pw[1], pw[2]};
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) b[k][c] = group_byte(d, 3 * k + 2 - c);          // raw frames hold blue first
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) b[k][c] = x + k < a.W ? p[3 * k + 2 - c] : 0u;
        }
    } else {
        const float* p = static_cast<const float*>(a.src) + ((int64_t)v * 3 * a.H + y) * a.W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* pc = p + (int64_t)c * a.H * a.W;
            const int oc = a.to_rgb ? c : 2 - c;                         // array channel c is red-first channel oc
            if (SRCW) {
                const float4 f = *reinterpret_cast<const float4*>(pc);
                b[0][oc] = denorm_byte(f.x, a.sd[c], a.mean[c]); b[1][oc] = denorm_byte(f.y, a.sd[c], a.mean[c]);
                b[2][oc] = denorm_byte(f.z, a.sd[c], a.mean[c]); b[3][oc] = denorm_byte(f.w, a.sd[c], a.mean[c]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) b[k][oc] = x + k < a.W ? denorm_byte(pc[k], a.sd[c], a.mean[c]) : 0u;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (best[k] != NONE) {
            const uint8_t* pal = a.palette + 3 * (int)cv[best[k]];       // cv[best] < ncol: tested when the segment was staged
            b[k][0] = pal[0]; b[k][1] = pal[1]; b[k][2] = pal[2];
        }
    uint8_t* o = a.out + (((int64_t)v * a.H + y) * a.W + x) * 3;
    if (OUTW) {
        store_group(o, b);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x + k < a.W) {
                o[3 * k] = (uint8_t)b[k][0]; o[3 * k + 1] = (uint8_t)b[k][1]; o[3 * k + 2] = (uint8_t)b[k][2];
            }
    }
}

}  // namespace

// what the two geometry entry points check alike
#define BOXES_COMMON_CHECKS(name)                                                                                                                          \
    TOC3D_REQUIRE(n >= 0, name ": bad dims (n must not be negative)");                                                                                     \
    TOC3D_REQUIRE(n == 0 || (boxes && scores && labels && segf && segi && cidx), name ": null buffer");                                                    \
    TOC3D_REQUIRE(thickness >= 1 && thickness <= MAX_T, name ": bad thickness (1 <= thickness <= %d)", MAX_T);                                              \
    TOC3D_REQUIRE(guard >= (thickness + 1) / 2 && guard <= MAX_GUARD, name ": bad guard ((thickness + 1) / 2 <= guard <= %d)", MAX_GUARD);                  \
    TOC3D_REQUIRE(n == 0 || box_stride >= 7, name ": bad strides (box_stride >= 7 elements: a stride smaller than a row)");                                 \
    TOC3D_REQUIRE(num_colors >= 1 && num_colors <= 254, name ": bad num_colors (1 <= num_colors <= 254: 255 marks a segment that is not drawn)")

extern "C" {

int toc3d_boxes_abi(void) { return TOC3D_BOXES_ABI; }

int toc3d_box_segments(const float* boxes, int64_t box_stride, const float* scores, const int64_t* labels, int64_t n, float score_thr, int64_t num_colors,
                       const float* proj, int64_t V, float near, int64_t H, int64_t W, int64_t guard, int64_t thickness, float* segf, int32_t* segi, uint8_t* cidx,
                       toc3d_stream_t stream) {
    BOXES_COMMON_CHECKS("toc3d_box_segments");
    TOC3D_REQUIRE(n == 0 || proj, "toc3d_box_segments: null buffer (proj)");
    TOC3D_REQUIRE(V > 0 && H > 0 && W > 0, "toc3d_box_segments: bad dims (V, H and W must be positive)");
    TOC3D_REQUIRE(H <= MAX_SIDE && W <= MAX_SIDE, "toc3d_box_segments: bad dims (H and W at most %d)", MAX_SIDE);
    TOC3D_REQUIRE(V <= 65535 && n <= 0x7fffffffll && V * n <= 0x7fffffffll / EC,"toc3d_box_segments: bad dims (V at most 65535, V * n * 12 below 2^31: one launch's grid)");
    if (n == 0) return TOC3D_OK;
    TOC3D_REQUIRE(toc3d_device_memory(boxes) && toc3d_device_memory(scores) && toc3d_device_memory(labels) && toc3d_device_memory(proj) && toc3d_device_memory(segf) && toc3d_device_memory(segi) &&
                      toc3d_device_memory(cidx),
                  "toc3d_box_segments: host pointer (every buffer must be device memory)");
    const int64_t threads = V * n;
    toc3d_launch(box_segments_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, as_stream(stream), boxes, box_stride, scores, labels, (int)n, score_thr,
                 (int)num_colors, proj, (int)V, near, -(float)guard, -(float)guard, (float)(W - 1 + guard), (float)(H - 1 + guard), segf, segi, cidx);
    TOC3D_LAUNCH_CHECK("toc3d_box_segments");
    return TOC3D_OK;
}

int toc3d_box_segments_bev(const float* boxes, int64_t box_stride, const float* scores, const int64_t* labels, int64_t n, float score_thr, int64_t num_colors,
                           int64_t S, float range_m, int64_t guard, int64_t thickness, float* segf, int32_t* segi, uint8_t* cidx, toc3d_stream_t stream) {
    BOXES_COMMON_CHECKS("toc3d_box_segments_bev");
    TOC3D_REQUIRE(S > 0, "toc3d_box_segments_bev: bad dims (S must be positive)");
    TOC3D_REQUIRE(S <= MAX_SIDE, "toc3d_box_segments_bev: bad dims (S at most %d)", MAX_SIDE);
    TOC3D_REQUIRE(range_m > 0.f && range_m <= 3.0e38f, "toc3d_box_segments_bev: bad range_m (a positive finite number of metres)");
    TOC3D_REQUIRE(n <= 0x7fffffffll / EB, "toc3d_box_segments_bev: bad dims (n * 5 below 2^31: one launch's grid)");
    if (n == 0) return TOC3D_OK;
    TOC3D_REQUIRE(toc3d_device_memory(boxes) && toc3d_device_memory(scores) && toc3d_device_memory(labels) && toc3d_device_memory(segf) && toc3d_device_memory(segi) && toc3d_device_memory(cidx),
                  "toc3d_box_segments_bev: host pointer (every buffer must be device memory)");
    const float half = 0.5f * (float)S, scale = (float)S / (2.f * range_m);
    toc3d_launch(box_segments_bev_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), boxes, box_stride, scores, labels, (int)n, score_thr,
                 (int)num_colors, half, scale, -(float)guard, (float)(S - 1 + guard), segf, segi, cidx);
    TOC3D_LAUNCH_CHECK("toc3d_box_segments_bev");
    return TOC3D_OK;
}

int toc3d_segments_render(const void* src, int src_kind, int64_t src_stride, int64_t V, int64_t H, int64_t W, float mean0, float mean1, float mean2,
                          float std0, float std1, float std2, int to_rgb, int bg_r, int bg_g, int bg_b, const int32_t* segi, const uint8_t* cidx, int64_t nseg,
                          const uint8_t* palette, int64_t num_colors, int64_t thickness, int64_t guard, uint8_t* out, toc3d_stream_t stream) {
    TOC3D_REQUIRE(src_kind >= 0 && src_kind <= 2, "toc3d_segments_render: bad src_kind (0 f32 NCHW, 1 u8 HWC, 2 none)");
    TOC3D_REQUIRE(out && palette && (src || src_kind == 2), "toc3d_segments_render: null buffer");
    TOC3D_REQUIRE(nseg >= 0 && nseg < 0x7fffffffll - CHUNK, "toc3d_segments_render: bad dims (nseg must not be negative and stays below 2^31 - 256)");
    TOC3D_REQUIRE(nseg == 0 || (segi && cidx), "toc3d_segments_render: null buffer (segi and cidx, with nseg > 0)");
    TOC3D_REQUIRE(V > 0 && H > 0 && W > 0, "toc3d_segments_render: bad dims (V, H and W must be positive)");
    TOC3D_REQUIRE(H <= MAX_SIDE && W <= MAX_SIDE, "toc3d_segments_render: bad dims (H and W at most %d)", MAX_SIDE);
    TOC3D_REQUIRE(V <= 65535, "toc3d_segments_render: bad dims (V at most 65535: one launch's grid)");
    TOC3D_REQUIRE(thickness >= 1 && thickness <= MAX_T, "toc3d_segments_render: bad thickness (1 <= thickness <= %d)", MAX_T);
    TOC3D_REQUIRE(guard >= (thickness + 1) / 2 && guard <= MAX_GUARD, "toc3d_segments_render: bad guard ((thickness + 1) / 2 <= guard <= %d)", MAX_GUARD);
    TOC3D_REQUIRE(src_kind != 1 || src_stride >= 3 * W, "toc3d_segments_render: bad strides (src_stride >= 3*W bytes: a stride smaller than a row)");
    TOC3D_REQUIRE(src_kind != 0 || ((uintptr_t)src & 3) == 0, "toc3d_segments_render: bad alignment (an f32 source starts on a 4-byte boundary)");
    TOC3D_REQUIRE(((uintptr_t)segi & 3) == 0, "toc3d_segments_render: bad alignment (segi starts on a 4-byte boundary)");
    TOC3D_REQUIRE(num_colors >= 1 && num_colors <= 254, "toc3d_segments_render: bad num_colors (1 <= num_colors <= 254: 255 marks a segment that is not drawn)");
    TOC3D_REQUIRE(bg_r >= 0 && bg_r <= 255 && bg_g >= 0 && bg_g <= 255 && bg_b >= 0 && bg_b <= 255, "toc3d_segments_render: bad background (three bytes, 0..255)");
    TOC3D_REQUIRE(toc3d_device_memory(out) && toc3d_device_memory(palette) && (src_kind == 2 || toc3d_device_memory(src)) && (nseg == 0 || (toc3d_device_memory(segi) && toc3d_device_memory(cidx))),
                  "toc3d_segments_render: host pointer (every buffer must be device memory)");
    RenderArgs a;
    a.src = src; a.segi = segi; a.cidx = cidx; a.palette = palette; a.out = out; a.src_stride = src_stride;
    a.V = (int)V; a.H = (int)H; a.W = (int)W; a.nseg = (int)nseg; a.ncol = (int)num_colors; a.t = (int)thickness; a.guard = (int)guard; a.to_rgb = to_rgb ? 1 : 0;
    a.tiles_x = (int)((W + TW - 1) / TW);
    a.bg[0] = (uint32_t)bg_r; a.bg[1] = (uint32_t)bg_g; a.bg[2] = (uint32_t)bg_b;
    a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2; a.sd[0] = std0; a.sd[1] = std1; a.sd[2] = std2;
    // the access widths, from pointers, strides and W
    const bool outw = W % 4 == 0 && ((uintptr_t)out & 3) == 0;
    const bool srcw = src_kind == 1 ? ((uintptr_t)src & 3) == 0 && src_stride % 4 == 0 : src_kind == 0 && W % 4 == 0 && ((uintptr_t)src & 15) == 0;
    dim3 grid((unsigned)(a.tiles_x * ((H + TH - 1) / TH)), (unsigned)V);     // at most 128 * 512 tiles
    auto launch = [&](auto kernel) { toc3d_launch(kernel, grid, dim3(256), 0, as_stream(stream), a); };
    if (src_kind == 2) {
        if (outw) launch(segments_render_kernel<2, false, true>); else launch(segments_render_kernel<2, false, false>);
    } else if (src_kind == 1) {
        if (srcw) { if (outw) launch(segments_render_kernel<1, true, true>); else launch(segments_render_kernel<1, true, false>); }
        else { if (outw) launch(segments_render_kernel<1, false, true>); else launch(segments_render_kernel<1, false, false>); }
    } else {
        if (srcw) { if (outw) launch(segments_render_kernel<0, true, true>); else launch(segments_render_kernel<0, true, false>); }
        else { if (outw) launch(segments_render_kernel<0, false, true>); else launch(segments_render_kernel<0, false, false>); }
    }
    TOC3D_LAUNCH_CHECK("toc3d_segments_render");
    return TOC3D_OK;
}

}  // extern "C"
