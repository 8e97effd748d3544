// Decoded boxes to nuScenes submission records in the global frame (include/toc3d_results.h): what mmdet3d's output_to_nusc_box, lidar_nusc_box_to_global and the
// attribute branch of _format_bbox (mmdet3d/datasets/nuscenes_dataset.py:576-657, :327-346) do in a Python loop over pyquaternion objects, as one launch over the
// fixed-capacity tensors of NMSFreeCoder.decode_fixed: a workgroup per sample, a thread per box, the kept boxes compacted stably with wave ballots and an LDS prefix.
#include "../../include/toc3d_results.h"
#include "capi.h"
#include "common.h"

#include <cmath>

// every float64 operation below is rounded once, in the order the header states: no fused multiply-adds
#pragma clang fp contract(off)

namespace {

constexpr int CHUNK = 256, WAVES = CHUNK / 64, REC = TOC3D_RESULTS_REC;
constexpr int MAX_K = TOC3D_RESULTS_MAX_BOXES, MAX_CLASSES = TOC3D_RESULTS_MAX_CLASSES;

struct ResultsArgs {
    const float* boxes; const float* scores; const int64_t* labels; const int64_t* counts;
    const double* poses; const double* class_range; const int32_t* attr_moving; const int32_t* attr_still;
    double* rec; float* score; int32_t* name; int32_t* attr; int32_t* src; int64_t* kept;
    int64_t box_stride, sample_stride;
    double speed_thr;
    int K, ncls, with_vel;
};

struct Pose {
    double w, x, y, z, t[3], R[9];
};

TOC3D_DEV Pose load_pose(const double* p) {
    Pose o;
    o.w = p[0]; o.x = p[1]; o.y = p[2]; o.z = p[3]; o.t[0] = p[4]; o.t[1] = p[5]; o.t[2] = p[6];
    const double w = o.w, x = o.x, y = o.y, z = o.z;
    o.R[0] = 1.0 - 2.0 * (y * y + z * z); o.R[1] = 2.0 * (x * y - w * z);       o.R[2] = 2.0 * (x * z + w * y);
    o.R[3] = 2.0 * (x * y + w * z);       o.R[4] = 1.0 - 2.0 * (x * x + z * z); o.R[5] = 2.0 * (y * z - w * x);
    o.R[6] = 2.0 * (x * z - w * y);       o.R[7] = 2.0 * (y * z + w * x);       o.R[8] = 1.0 - 2.0 * (x * x + y * y);
    return o;
}

// v = R v (+ t): each row ((R0 v0 + R1 v1) + R2 v2) + t
TOC3D_DEV void rotate(const Pose& p, double* v, bool translate) {
    const double a = v[0], b = v[1], c = v[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double s = (p.R[3 * i] * a + p.R[3 * i + 1] * b) + p.R[3 * i + 2] * c;
        v[i] = translate ? s + p.t[i] : s;
    }
}

// q = p (x) q: the Hamilton product, the pose on the left
TOC3D_DEV void hamilton(const Pose& p, double* q) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    q[0] = ((p.w * w - p.x * x) - p.y * y) - p.z * z;
    q[1] = ((p.w * x + p.x * w) + p.y * z) - p.z * y;
    q[2] = ((p.w * y - p.x * z) + p.y * w) + p.z * x;
    q[3] = ((p.w * z + p.x * y) - p.y * x) + p.z * w;
}

__global__ __launch_bounds__(CHUNK) void boxes_to_global_kernel(ResultsArgs a) {
    __shared__ int s_cnt[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, K = a.K;
    const int64_t cnt = a.counts[b];
    const int n = cnt < 0 ? 0 : cnt > K ? K : (int)cnt;
    const float* boxes = a.boxes + (int64_t)b * a.sample_stride;
    const float* scores = a.scores + (int64_t)b * K;
    const int64_t* labels = a.labels + (int64_t)b * K;
    double* rec = a.rec + (int64_t)b * K * REC;
    float* score = a.score + (int64_t)b * K;
    int32_t* name = a.name + (int64_t)b * K;
    int32_t* attr = a.attr + (int64_t)b * K;
    int32_t* src = a.src + (int64_t)b * K;
    const Pose ego = load_pose(a.poses + (int64_t)b * 14), glob = load_pose(a.poses + (int64_t)b * 14 + 7);
    int base = 0;                                                            // kept boxes of the chunks before this one: the same in every thread
    for (int c0 = 0; c0 < n; c0 += CHUNK) {                                  // (n is the workgroup's: every thread makes the same trips)
        const int i = c0 + tid;
        bool keep = false;
        double c[3] = {}, size[3] = {}, q[4] = {}, v[3] = {};
        float sc = 0.f;
        int lab = -1, at = -1;
        if (i < n) {
            const float* r = boxes + (int64_t)i * a.box_stride;
            const float x = r[0], y = r[1], zb = r[2], dx = r[3], dy = r[4], dz = r[5], yaw = r[6];
            const float vx = a.with_vel ? r[7] : 0.f, vy = a.with_vel ? r[8] : 0.f;
            sc = scores[i];
            const int64_t l = labels[i];
            keep = l >= 0 && l < a.ncls && isfinite(x) && isfinite(y) && isfinite(zb) && isfinite(dx) && isfinite(dy) && isfinite(dz) && isfinite(yaw) &&
                   isfinite(vx) && isfinite(vy) && isfinite(sc);
            if (keep) {
                lab = (int)l;
                const float zg = zb + dz * 0.5f;                             // float32, as lidar_box3d.py:41-47 (the product is exact: nothing to fuse)
                keep = isfinite(zg);                                         // (z_bottom + dz / 2 may overflow float32 where neither column does)
                c[0] = (double)x; c[1] = (double)y; c[2] = (double)zg;
                size[0] = (double)dy; size[1] = (double)dx; size[2] = (double)dz;
                const double half = (double)yaw * 0.5;
                q[0] = cos(half); q[1] = 0.0; q[2] = 0.0; q[3] = sin(half);
                v[0] = (double)vx; v[1] = (double)vy; v[2] = 0.0;
                rotate(ego, c, true);
                hamilton(ego, q);
                rotate(ego, v, false);
                const double radius = sqrt(c[0] * c[0] + c[1] * c[1]);
                keep = keep && !(radius > a.class_range[lab]);
                rotate(glob, c, true);
                hamilton(glob, q);
                rotate(glob, v, false);
                at = sqrt(v[0] * v[0] + v[1] * v[1]) > a.speed_thr ? a.attr_moving[lab] : a.attr_still[lab];
            }
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int before = base, total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const int k = s_cnt[w];
            if (w < wave) before += k;
            total += k;
        }
        if (keep) {                                                          // pos <= i < n <= K
            const int pos = before + __popcll(m & ((1ull << lane) - 1ull));
            double* o = rec + (int64_t)pos * REC;
            o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = size[0]; o[4] = size[1]; o[5] = size[2];
            o[6] = q[0]; o[7] = q[1]; o[8] = q[2]; o[9] = q[3]; o[10] = v[0]; o[11] = v[1];
            score[pos] = sc; name[pos] = lab; attr[pos] = at; src[pos] = i;
        }
        base += total;
        __syncthreads();                                                     // s_cnt is rewritten by the next chunk
    }
    for (int i = base + tid; i < K; i += CHUNK) {                            // the tail: every row at or beyond kept[b]
        double* o = rec + (int64_t)i * REC;
#pragma unroll
        for (int k = 0; k < REC; ++k) o[k] = 0.0;
        score[i] = 0.f; name[i] = -1; attr[i] = -1; src[i] = -1;
    }
    if (tid == 0) a.kept[b] = base;
}

}  // namespace

extern "C" {

int toc3d_results_abi(void) { return TOC3D_RESULTS_ABI; }

int toc3d_boxes_to_global(const float* boxes, int64_t box_stride, int64_t sample_stride, const float* scores, const int64_t* labels, const int64_t* counts,
                          int64_t B, int64_t K, int with_velocity, const double* poses, const double* class_range, const int32_t* attr_moving,
                          const int32_t* attr_still, int64_t num_classes, double speed_thr, double* rec, float* score, int32_t* name, int32_t* attr, int32_t* src,
                          int64_t* kept, toc3d_stream_t stream) {
    const char* fn = "toc3d_boxes_to_global";
    const int64_t row = with_velocity ? 9 : 7;
    TOC3D_REQUIRE(B >= 0 && K >= 0, "%s: bad dims (B and K must not be negative)", fn);
    TOC3D_REQUIRE(K <= MAX_K, "%s: bad dims (K at most %d, the decoder's own cap)", fn, MAX_K);
    TOC3D_REQUIRE(B <= 65535, "%s: bad dims (B at most 65535: one launch's grid)", fn);
    const bool work = B > 0 && K > 0;
    TOC3D_REQUIRE(!work || (boxes && scores && labels && counts && poses && class_range && attr_moving && attr_still && rec && score && name && attr && src && kept),
                  "%s: null buffer", fn);
    TOC3D_REQUIRE(box_stride >= row, "%s: bad strides (box_stride >= %d elements: a stride smaller than a row)", fn, (int)row);
    TOC3D_REQUIRE(K == 0 || sample_stride / K >= box_stride, "%s: bad strides (sample_stride >= K * box_stride elements: samples that overlap)", fn);
    TOC3D_REQUIRE(num_classes >= 1 && num_classes <= MAX_CLASSES, "%s: bad num_classes (1 <= num_classes <= %d)", fn, MAX_CLASSES);
    TOC3D_REQUIRE(std::isfinite(speed_thr), "%s: bad speed_thr (a finite number of metres per second)", fn);
    TOC3D_REQUIRE(((uintptr_t)boxes & 3) == 0, "%s: bad alignment (boxes starts on a 4-byte boundary)", fn);
    TOC3D_REQUIRE(((uintptr_t)rec & 7) == 0 && ((uintptr_t)poses & 7) == 0, "%s: bad alignment (rec and poses start on an 8-byte boundary)", fn);
    if (!work) return TOC3D_OK;
    const void* buffers[] = {boxes, scores, labels, counts, poses, class_range, attr_moving, attr_still, rec, score, name, attr, src, kept};
    for (const void* p : buffers) TOC3D_REQUIRE(toc3d_device_memory(p), "%s: host pointer (every buffer must be device memory)", fn);
    ResultsArgs a;
    a.boxes = boxes; a.scores = scores; a.labels = labels; a.counts = counts; a.poses = poses; a.class_range = class_range;
    a.attr_moving = attr_moving; a.attr_still = attr_still; a.rec = rec; a.score = score; a.name = name; a.attr = attr; a.src = src; a.kept = kept;
    a.box_stride = box_stride; a.sample_stride = sample_stride; a.speed_thr = speed_thr;
    a.K = (int)K; a.ncls = (int)num_classes; a.with_vel = with_velocity ? 1 : 0;
    toc3d_launch(boxes_to_global_kernel, dim3((unsigned)B), dim3(CHUNK), 0, as_stream(stream), a);
    TOC3D_LAUNCH_CHECK(fn);
    return TOC3D_OK;
}

}  // extern "C"
