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

namespace {

constexpr int THREADS = 512, WAVES = THREADS / 64, REC = TOC3D_TRACKS_REC;
constexpr int MAX_K = TOC3D_TRACKS_MAX_BOXES, MAX_CAP = TOC3D_TRACKS_MAX_TRACKS, MAX_LABELS = TOC3D_TRACKS_MAX_CLASSES;
constexpr int HEADER = TOC3D_TRACKS_HEADER_BYTES;
constexpr unsigned long long NONE = ~0ull;

struct TracksArgs {
    const double* rec; const float* score; const int32_t* name; const int64_t* kept;
    const int32_t* track_label; const float* max_diff; const double* timestamp; const int32_t* first;
    const char* state_in; char* state_out;
    int32_t* track_id; int32_t* active; int32_t* order; int64_t* num_out;
    double score_thr;
    int K, ncls, nl, max_age, cap;
};

// dynamic LDS of a launch: float32 positions of the tracks (per label) and the detections, the match of each detection, and the index lists
size_t lds_bytes(int64_t cap, int64_t K) { return (size_t)(4 * (2 * cap + 3 * K) + 2 * (cap + K) + (cap + K)); }

struct State {
    double* ct; double* tracking; int32_t* label; int32_t* id; int32_t* age; int32_t* active;
};

TOC3D_DEV State rows_of(char* s, int cap) {
    State o;
    o.ct = reinterpret_cast<double*>(s + HEADER); o.tracking = o.ct + 2 * (int64_t)cap;
    o.label = reinterpret_cast<int32_t*>(o.tracking + 2 * (int64_t)cap); o.id = o.label + cap; o.age = o.id + cap; o.active = o.age + cap;
    return o;
}

// the smallest key of the wavefront in every lane: l ^ 32 and l ^ 16 by permlane swaps, the row by DPP moves; all 64 lanes are active
TOC3D_DEV unsigned long long wave_min_u64(unsigned long long k) {
    const auto pack = [](unsigned lo, unsigned hi) { return ((unsigned long long)hi << 32) | lo; };
    {
        const unsigned lo = (unsigned)k, hi = (unsigned)(k >> 32);
        const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false), h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        const unsigned long long k0 = pack(a[0], h[0]), k1 = pack(a[1], h[1]);
        k = k0 < k1 ? k0 : k1;
    }
    {
        const unsigned lo = (unsigned)k, hi = (unsigned)(k >> 32);
        const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        const unsigned long long k0 = pack(a[0], h[0]), k1 = pack(a[1], h[1]);
        k = k0 < k1 ? k0 : k1;
    }
    unsigned long long o;
    o = pack((unsigned)dpp_mov_i<DPP_ROW_ROR8>((int)(unsigned)k), (unsigned)dpp_mov_i<DPP_ROW_ROR8>((int)(unsigned)(k >> 32))); k = o < k ? o : k;
    o = pack((unsigned)lane_xor4_i((int)(unsigned)k), (unsigned)lane_xor4_i((int)(unsigned)(k >> 32))); k = o < k ? o : k;
    o = pack((unsigned)dpp_mov_i<DPP_QUAD_XOR2>((int)(unsigned)k), (unsigned)dpp_mov_i<DPP_QUAD_XOR2>((int)(unsigned)(k >> 32))); k = o < k ? o : k;
    o = pack((unsigned)dpp_mov_i<DPP_QUAD_XOR1>((int)(unsigned)k), (unsigned)dpp_mov_i<DPP_QUAD_XOR1>((int)(unsigned)(k >> 32))); k = o < k ? o : k;
    return k;
}

// flags of the workgroup's 512 threads -> (set flags in the threads before this one, set flags in all); two barriers, s_cnt is free again on return
TOC3D_DEV int block_prefix(bool flag, int* s_cnt, int lane, int wave, int& total) {
    const unsigned long long m = __ballot(flag);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int k = s_cnt[w];
        if (w < wave) before += k;
        total += k;
    }
    __syncthreads();
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

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

    const int64_t sbytes = TOC3D_TRACKS_STATE_BYTES(cap);
    const char* sin = a.state_in + (int64_t)b * sbytes;
    char* sout = a.state_out + (int64_t)b * sbytes;
    const State in = rows_of(const_cast<char*>(sin), cap), out = rows_of(sout, cap);
    const double* rec = a.rec + (int64_t)b * K * REC;
    const float* score = a.score + (int64_t)b * K;
    const int32_t* name = a.name + (int64_t)b * K;
    int32_t* track_id = a.track_id + (int64_t)b * K;
    int32_t* active = a.active + (int64_t)b * K;
    int32_t* order = a.order + (int64_t)b * K;

    // 0. the state read, or an empty one
    const bool fresh = a.first[b] != 0;
    const double ts = a.timestamp[b];
    const int count = reinterpret_cast<const int32_t*>(sin)[0];
    const int M = fresh ? 0 : count < 0 ? 0 : count > cap ? cap : count;
    const int id_count = fresh ? 0 : reinterpret_cast<const int32_t*>(sin)[1];
    const double last = fresh ? ts : *reinterpret_cast<const double*>(sin + 8);
    const double lag = ts - last;
    const int64_t cnt = a.kept[b];
    const int n = cnt < 0 ? 0 : cnt > K ? K : (int)cnt;

    // 1, 2. filter, compacted stably; a row that does not survive gets its zeros here
    int N = 0;
    for (int c0 = 0; c0 < n; c0 += THREADS) {                                // (n is the workgroup's: every thread makes the same trips)
        const int i = c0 + tid;
        bool keep = false;
        int lab = -1;
        float px = 0.f, py = 0.f;
        if (i < n) {
            const int nm = name[i];
            if (nm >= 0 && nm < a.ncls) {
                lab = a.track_label[nm];
                if (lab < 0 || lab >= nl) lab = -1;
            }
            keep = lab >= 0 && !((double)score[i] < a.score_thr);
            if (keep) {
                const double* r = rec + (int64_t)i * REC;
                const double tx = (r[10] * -1.0) * lag, ty = (r[11] * -1.0) * lag;
                px = (float)(r[0] + (double)(float)tx);
                py = (float)(r[1] + (double)(float)ty);
            } else {
                track_id[i] = 0; active[i] = 0;
            }
        }
        int total;
        const int pos = N + block_prefix(keep, s_cnt, lane, wave, total);
        if (keep) {                                                          // pos <= i < n <= K
            dpx[pos] = px; dpy[pos] = py; drow[pos] = (unsigned short)i; dlab[pos] = (unsigned char)lab; dmatch[pos] = -1;
        }
        N += total;
    }
    for (int i = n + tid; i < K; i += THREADS) { track_id[i] = 0; active[i] = 0; }
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

    int held;                                                                // tracks in the new state
    int new_id_count = id_count;
    if (N > 0) {
        // 5. matches, then unmatched detections, then the unmatched tracks young enough
        int nm = 0;
        for (int c0 = 0; c0 < N; c0 += THREADS) {
            const int f = c0 + tid;
            int total;
            block_prefix(f < N && dmatch[f] >= 0, s_cnt, lane, wave, total);
            nm += total;
        }
        int mbase = 0;
        for (int c0 = 0; c0 < N; c0 += THREADS) {
            const int f = c0 + tid;
            const bool live = f < N;
            const int t = live ? dmatch[f] : -1;
            int total;
            const int rm = mbase + block_prefix(t >= 0, s_cnt, lane, wave, total);      // matches before f
            mbase += total;
            if (live) {
                const int ru = f - rm;                                       // unmatched detections before f
                const int pos = t >= 0 ? rm : nm + ru;                       // pos < N <= K <= cap
                const int row = drow[f];
                const double* r = rec + (int64_t)row * REC;
                const int id = t >= 0 ? in.id[t] : id_count + ru + 1;
                const int act = t >= 0 ? in.active[t] + 1 : 1;
                out.ct[2 * pos] = r[0]; out.ct[2 * pos + 1] = r[1];
                out.tracking[2 * pos] = (r[10] * -1.0) * lag; out.tracking[2 * pos + 1] = (r[11] * -1.0) * lag;
                out.label[pos] = dlab[f]; out.id[pos] = id; out.age[pos] = 1; out.active[pos] = act;
                order[pos] = row; track_id[row] = id; active[row] = act;
            }
        }
        new_id_count = id_count + (N - nm);
        int kbase = N;
        for (int t0 = 0; t0 < M; t0 += THREADS) {
            const int t = t0 + tid;
            const bool stay = t < M && !tmatch[t] && in.age[t] < a.max_age;
            int total;
            const int pos = kbase + block_prefix(stay, s_cnt, lane, wave, total);
            kbase += total;
            if (stay && pos < cap) {                                         // (capacity >= K * (max_age + 1) holds every step's tracks: the bound is never met)
                out.ct[2 * pos] = in.ct[2 * t] + in.tracking[2 * t] * -1.0; out.ct[2 * pos + 1] = in.ct[2 * t + 1] + in.tracking[2 * t + 1] * -1.0;
                out.tracking[2 * pos] = in.tracking[2 * t]; out.tracking[2 * pos + 1] = in.tracking[2 * t + 1];
                out.label[pos] = in.label[t]; out.id[pos] = in.id[t]; out.age[pos] = in.age[t] + 1; out.active[pos] = 0;
            }
        }
        held = kbase < cap ? kbase : cap;
    } else {
        // 6. the empty frame: every track stays where it is; the old ones are left as they are
        for (int t = tid; t < M; t += THREADS) {
            const bool young = in.age[t] < a.max_age;
            const double tx = in.tracking[2 * t], ty = in.tracking[2 * t + 1];
            out.ct[2 * t] = young ? in.ct[2 * t] + tx * -1.0 : in.ct[2 * t]; out.ct[2 * t + 1] = young ? in.ct[2 * t + 1] + ty * -1.0 : in.ct[2 * t + 1];
            out.tracking[2 * t] = tx; out.tracking[2 * t + 1] = ty;
            out.label[t] = in.label[t]; out.id[t] = in.id[t]; out.age[t] = young ? in.age[t] + 1 : in.age[t]; out.active[t] = young ? 0 : in.active[t];
        }
        held = M;
    }
    for (int t = held + tid; t < cap; t += THREADS) {                        // the rest of the new state
        out.ct[2 * t] = 0.0; out.ct[2 * t + 1] = 0.0; out.tracking[2 * t] = 0.0; out.tracking[2 * t + 1] = 0.0;
        out.label[t] = 0; out.id[t] = 0; out.age[t] = 0; out.active[t] = 0;
    }
    for (int i = N + tid; i < K; i += THREADS) order[i] = -1;
    if (tid == 0) {
        int32_t* h = reinterpret_cast<int32_t*>(sout);
        h[0] = held; h[1] = new_id_count;
        *reinterpret_cast<double*>(sout + 8) = ts;
        h[4] = 0; h[5] = 0; h[6] = 0; h[7] = 0;
        a.num_out[b] = N;
    }
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
    TOC3D_REQUIRE(B >= 0 && K >= 0, "%s: bad dims (B and K must not be negative)", fn);
    TOC3D_REQUIRE(K <= MAX_K, "%s: bad dims (K at most %d, the decoder's own cap)", fn, MAX_K);
    TOC3D_REQUIRE(B <= 65535, "%s: bad dims (B at most 65535: one launch's grid)", fn);
    TOC3D_REQUIRE(max_age >= 0, "%s: bad max_age (must not be negative)", fn);
    TOC3D_REQUIRE(capacity >= 0 && capacity <= MAX_CAP, "%s: bad capacity (at most %d tracks a stream)", fn, MAX_CAP);
    TOC3D_REQUIRE(K == 0 || max_age < capacity / K, "%s: bad capacity (capacity >= K * (max_age + 1): what a step can hold)", fn);
    const bool work = B > 0;
    TOC3D_REQUIRE(!work || (kept && track_label && max_diff && timestamp && first && state_in && state_out && num_out), "%s: null buffer", fn);
    TOC3D_REQUIRE(!work || K == 0 || (rec && score && name && track_id && active && order), "%s: null buffer", fn);
    TOC3D_REQUIRE(num_classes >= 1 && num_classes <= MAX_LABELS, "%s: bad num_classes (1 <= num_classes <= %d)", fn, MAX_LABELS);
    TOC3D_REQUIRE(num_track_labels >= 1 && num_track_labels <= MAX_LABELS, "%s: bad num_track_labels (1 <= num_track_labels <= %d)", fn, MAX_LABELS);
    TOC3D_REQUIRE(std::isfinite(score_thr), "%s: bad score_thr (a finite number)", fn);
    TOC3D_REQUIRE(((uintptr_t)rec & 7) == 0 && ((uintptr_t)timestamp & 7) == 0, "%s: bad alignment (rec and timestamp start on an 8-byte boundary)", fn);
    TOC3D_REQUIRE(((uintptr_t)state_in & 7) == 0 && ((uintptr_t)state_out & 7) == 0, "%s: bad alignment (state_in and state_out start on an 8-byte boundary)", fn);
    if (!work) return TOC3D_OK;
    const uintptr_t si = (uintptr_t)state_in, so = (uintptr_t)state_out, span = (uintptr_t)(B * TOC3D_TRACKS_STATE_BYTES(capacity));
    TOC3D_REQUIRE(si + span <= so || so + span <= si, "%s: state_in and state_out overlap (a step reads one and writes the other)", fn);
    const void* always[] = {kept, track_label, max_diff, timestamp, first, state_in, state_out, num_out};
    for (const void* p : always) TOC3D_REQUIRE(toc3d_device_memory(p), "%s: host pointer (every buffer must be device memory)", fn);
    const void* rows[] = {rec, score, name, track_id, active, order};
    for (const void* p : rows) TOC3D_REQUIRE(K == 0 || toc3d_device_memory(p), "%s: host pointer (every buffer must be device memory)", fn);
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
