// Greedy centre-distance tracking of the submission records (include/toc3d_tracks.h): what nusc_tracking/pub_tracker.py:41-186 and track_utils.py:3-12 do on the
// host with an N x M float64 matrix and one argmin per detection, as one launch over the tensors toc3d_boxes_to_global leaves on the device: a workgroup per
// stream, a wavefront per tracking label walking its own detections in order, the tracks of a step in device memory from frame to frame.
#include "../../include/toc3d_tracks.h"
#include "capi.h"
#include "common.h"

#include <climits>
#include <cmath>

// every float64 and float32 operation below is rounded once, in the order the header states: no fused multiply-adds
#pragma clang fp contract(off)

#include "tracks_steps.h"                          // the steps shared with tracking_hungarian.hip: the state, the filter, the write of the new state

namespace {

using namespace tracks;

constexpr int THREADS = 512, WAVES = THREADS / 64;
constexpr int MAX_K = TOC3D_TRACKS_MAX_BOXES, MAX_CAP = TOC3D_TRACKS_MAX_TRACKS;
constexpr unsigned long long NONE = ~0ull;

// dynamic LDS of a launch: float32 positions of the tracks (per label) and the detections, the match of each detection, and the index lists
size_t lds_bytes(int64_t cap, int64_t K) { return (size_t)(4 * (2 * cap + 3 * K) + 2 * (cap + K) + (cap + K)); }

__global__ __launch_bounds__(THREADS) void tracks_step_kernel(TracksArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int s_cnt[WAVES], s_lcount[MAX_LABELS], s_tstart[MAX_LABELS + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, K = a.K, cap = a.cap, nl = a.nl;
    float* tqx = reinterpret_cast<float*>(smem);                            // [cap] the tracks' float32 positions, label by label, track order inside a label
    float* tqy = tqx + cap;
    float* dpx = tqy + cap;                                                  // [K] the surviving detections' float32 positions, detection order
    float* dpy = dpx + K;
    int* dmatch = reinterpret_cast<int*>(dpy + K);                           // [K] the track a detection took, -1 none
    unsigned short* tidx = reinterpret_cast<unsigned short*>(dmatch + K);    // [cap] position in tqx -> track
    unsigned short* drow = tidx + cap;                                       // [K] surviving detection -> input row
    unsigned char* tmatch = reinterpret_cast<unsigned char*>(drow + K);      // [cap] 1: the track was taken
    unsigned char* dlab = tmatch + cap;                                      // [K] a surviving detection's label

    const Stream s = stream_of(a, b);                                        // 0. the state read, or an empty one
    const State& in = s.in;
    const int M = s.M;
    const int N = filter_compact<THREADS>(a, s, dpx, dpy, drow, dlab, dmatch, s_cnt);     // 1, 2.
    for (int t = tid; t < M; t += THREADS) tmatch[t] = 0;
    __syncthreads();                                                         // the last chunk's detections and the flags are read by other threads from here on

    if (N > 0 && M > 0) {
        // the tracks label by label: wavefront w counts, then places, the tracks of labels w, w + 8, ...
        for (int L = wave; L < nl; L += WAVES) {
            int c = 0;
            for (int t0 = 0; t0 < M; t0 += 64) {
                const int t = t0 + lane;
                c += __popcll(__ballot(t < M && in.label[t] == L));
            }
            if (lane == 0) s_lcount[L] = c;
        }
        __syncthreads();
        if (tid == 0) {
            int s = 0;
            for (int L = 0; L < nl; ++L) { s_tstart[L] = s; s += s_lcount[L]; }      // s <= M <= cap
            s_tstart[nl] = s;
        }
        __syncthreads();
        for (int L = wave; L < nl; L += WAVES) {
            int pos = s_tstart[L];
            for (int t0 = 0; t0 < M; t0 += 64) {
                const int t = t0 + lane;
                const bool f = t < M && in.label[t] == L;
                const unsigned long long m = __ballot(f);
                if (f) {
                    const int j = pos + __popcll(m & ((1ull << lane) - 1ull));
                    tqx[j] = (float)in.ct[2 * t]; tqy[j] = (float)in.ct[2 * t + 1]; tidx[j] = (unsigned short)t;
                }
                pos += __popcll(m);
            }
        }
        __syncthreads();
        // 3, 4. the greedy chains: one per label, the detections of the label in order.  The key (distance bits, position) orders by distance and then by track
        // index: a distance is not negative, so its bits order as it does, and positions inside a label are in track order.  A taken track's x becomes NaN, written
        // by the one lane that ever reads that position: its distance is then NaN, which is never valid.
        for (int L = wave; L < nl; L += WAVES) {
            const int j0 = s_tstart[L], j1 = s_tstart[L + 1];
            if (j0 == j1) continue;
            const float gate = a.max_diff[L];
            for (int c0 = 0; c0 < N; c0 += 64) {
                const int i = c0 + lane;
                unsigned long long m = __ballot(i < N && dlab[i] == L);
                while (m) {                                                  // (m is the wavefront's: every lane makes the same trips)
                    const int d = c0 + __builtin_ctzll(m);
                    m &= m - 1;
                    const float px = dpx[d], py = dpy[d];
                    unsigned long long best = NONE;
                    for (int j = j0 + lane; j < j1; j += 64) {
                        // plain operators under this file's contract(off) (the __f*_rn wrappers are compiled with the headers' contraction and fuse once inlined);
                        // sqrtf is the correctly rounded one: the Makefile passes no fast-math flag
                        const float dx = tqx[j] - px, dy = tqy[j] - py;
                        const float xx = dx * dx, yy = dy * dy;
                        const float dist = sqrtf(xx + yy);
                        if (dist <= gate) {
                            const unsigned long long key = ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned)j;
                            best = key < best ? key : best;
                        }
                    }
                    best = wave_min_u64(best);
                    if (best != NONE) {
                        const int j = (int)(unsigned)best;
                        if (((j - j0) & 63) == lane) {
                            const int t = tidx[j];
                            tqx[j] = __builtin_nanf("");
                            tmatch[t] = 1; dmatch[d] = t;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }

    write_state<THREADS, 2>(a, s, N, dmatch, nullptr, drow, dlab, tmatch, s_cnt);      // 5, 6.
}

}  // namespace

extern "C" {

int toc3d_tracks_abi(void) { return TOC3D_TRACKS_ABI; }

int toc3d_tracks_state_bytes(int64_t capacity, int64_t* bytes) {
    const char* fn = "toc3d_tracks_state_bytes";
    TOC3D_REQUIRE(capacity >= 0 && capacity <= MAX_CAP, "%s: bad capacity (0 <= capacity <= %d)", fn, MAX_CAP);
    TOC3D_REQUIRE(bytes != nullptr, "%s: null buffer", fn);
    *bytes = TOC3D_TRACKS_STATE_BYTES(capacity);
    return TOC3D_OK;
}

int toc3d_tracks_step(const double* rec, const float* score, const int32_t* name, const int64_t* kept, int64_t B, int64_t K, const int32_t* track_label,
                      int64_t num_classes, const float* max_diff, int64_t num_track_labels, double score_thr, int64_t max_age, const double* timestamp,
                      const int32_t* first, const void* state_in, void* state_out, int64_t capacity, int32_t* track_id, int32_t* active, int32_t* order,
                      int64_t* num_out, toc3d_stream_t stream) {
    const char* fn = "toc3d_tracks_step";
    TOC3D_TRACKS_STEP_CHECKS(fn, MAX_K, "the decoder's own cap", MAX_CAP, num_out);
    TracksArgs a;
    a.rec = rec; a.score = score; a.name = name; a.kept = kept; a.track_label = track_label; a.max_diff = max_diff; a.timestamp = timestamp; a.first = first;
    a.state_in = static_cast<const char*>(state_in); a.state_out = static_cast<char*>(state_out);
    a.track_id = track_id; a.active = active; a.order = order; a.num_out = num_out; a.score_thr = score_thr;
    a.K = (int)K; a.ncls = (int)num_classes; a.nl = (int)num_track_labels; a.max_age = max_age > INT_MAX ? INT_MAX : (int)max_age; a.cap = (int)capacity;
    const size_t lds = lds_bytes(capacity, K);                               // at most 11 * 8192 + 15 * 2048 = 120832 bytes of the CU's 160 KiB
    static Toc3dLdsAttr attr;
    if (lds > 48 * 1024) attr.ensure(reinterpret_cast<const void*>(&tracks_step_kernel), (int)lds_bytes(MAX_CAP, MAX_K));
    toc3d_launch(tracks_step_kernel, dim3((unsigned)B), dim3(THREADS), lds, as_stream(stream), a);
    TOC3D_LAUNCH_CHECK(fn);
    return TOC3D_OK;
}

}  // extern "C"
