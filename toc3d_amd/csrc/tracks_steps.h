// The steps the two tracking kernels share (tracking.hip: greedy, include/toc3d_tracks.h; tracking_hungarian.hip: scipy's solver replayed, include/toc3d_assign.h):
// the state's layout, a stream's view of the arguments (point 0), the filter and stable compaction of the detections (points 1 and 2) and the write of the new state
// and the outputs (points 5 and 6), parametrised by the order of the detections (two or three groups) -- which tracks stay is the flag array the kernel hands in.
// Included after capi.h and common.h by files that set `#pragma clang fp contract(off)` first: every float64 operation here is rounded once.
#pragma once
#include "../../include/toc3d_tracks.h"

namespace tracks {

constexpr int REC = TOC3D_TRACKS_REC, MAX_LABELS = TOC3D_TRACKS_MAX_CLASSES, HEADER = TOC3D_TRACKS_HEADER_BYTES;

struct TracksArgs {
    const double* rec; const float* score; const int32_t* name; const int64_t* kept;
    const int32_t* track_label; const float* max_diff; const double* timestamp; const int32_t* first;
    const char* state_in; char* state_out;
    int32_t* track_id; int32_t* active; int32_t* order; int64_t* num_out;
    double score_thr;
    int K, ncls, nl, max_age, cap;
};

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

// flags of the workgroup's THREADS threads -> (set flags in the threads before this one, set flags in all); two barriers, s_cnt is free again on return
template <int THREADS>
TOC3D_DEV int block_prefix(bool flag, int* s_cnt, int lane, int wave, int& total) {
    const unsigned long long m = __ballot(flag);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
        const int k = s_cnt[w];
        if (w < wave) before += k;
        total += k;
    }
    __syncthreads();
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

// 0. one stream's view of a launch: its rows, its two states, the state read (or an empty one) and the time lag
struct Stream {
    const char* sin; char* sout;
    State in, out;
    const double* rec; const float* score; const int32_t* name;
    int32_t* track_id; int32_t* active; int32_t* order;
    double ts, lag;
    int M, id_count, n;
};

TOC3D_DEV Stream stream_of(const TracksArgs& a, int b) {
    Stream s;
    const int K = a.K, cap = a.cap;
    const int64_t sbytes = TOC3D_TRACKS_STATE_BYTES(cap);
    s.sin = a.state_in + (int64_t)b * sbytes;
    s.sout = a.state_out + (int64_t)b * sbytes;
    s.in = rows_of(const_cast<char*>(s.sin), cap); s.out = rows_of(s.sout, cap);
    s.rec = a.rec + (int64_t)b * K * REC;
    s.score = a.score + (int64_t)b * K;
    s.name = a.name + (int64_t)b * K;
    s.track_id = a.track_id + (int64_t)b * K;
    s.active = a.active + (int64_t)b * K;
    s.order = a.order + (int64_t)b * K;
    const bool fresh = a.first[b] != 0;
    s.ts = a.timestamp[b];
    const int count = reinterpret_cast<const int32_t*>(s.sin)[0];
    s.M = fresh ? 0 : count < 0 ? 0 : count > cap ? cap : count;
    s.id_count = fresh ? 0 : reinterpret_cast<const int32_t*>(s.sin)[1];
    const double last = fresh ? s.ts : *reinterpret_cast<const double*>(s.sin + 8);
    s.lag = s.ts - last;
    const int64_t cnt = a.kept[b];
    s.n = cnt < 0 ? 0 : cnt > K ? K : (int)cnt;
    return s;
}

// 1, 2. filter, compacted stably -> N; a row that does not survive, or lies at or beyond kept, gets its zeros here.  No barrier after the last chunk: the caller
// places one before another thread reads what was compacted.
template <int THREADS>
TOC3D_DEV int filter_compact(const TracksArgs& a, const Stream& s, float* dpx, float* dpy, unsigned short* drow, unsigned char* dlab, int* dmatch, int* s_cnt) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = s.n;
    int N = 0;
    for (int c0 = 0; c0 < n; c0 += THREADS) {                                // (n is the workgroup's: every thread makes the same trips)
        const int i = c0 + tid;
        bool keep = false;
        int lab = -1;
        float px = 0.f, py = 0.f;
        if (i < n) {
            const int nm = s.name[i];
            if (nm >= 0 && nm < a.ncls) {
                lab = a.track_label[nm];
                if (lab < 0 || lab >= a.nl) lab = -1;
            }
            keep = lab >= 0 && !((double)s.score[i] < a.score_thr);
            if (keep) {
                const double* r = s.rec + (int64_t)i * REC;
                const double tx = (r[10] * -1.0) * s.lag, ty = (r[11] * -1.0) * s.lag;
                px = (float)(r[0] + (double)(float)tx);
                py = (float)(r[1] + (double)(float)ty);
            } else {
                s.track_id[i] = 0; s.active[i] = 0;
            }
        }
        int total;
        const int pos = N + block_prefix<THREADS>(keep, s_cnt, lane, wave, total);
        if (keep) {                                                          // pos <= i < n <= K
            dpx[pos] = px; dpy[pos] = py; drow[pos] = (unsigned short)i; dlab[pos] = (unsigned char)lab; dmatch[pos] = -1;
        }
        N += total;
    }
    for (int i = n + tid; i < a.K; i += THREADS) { s.track_id[i] = 0; s.active[i] = 0; }
    return N;
}

// 5, 6. the new state and the outputs.  dmatch[f]: the track detection f continues (the groups' first), else -1.  GROUPS == 2: the matches in detection order, then
// the other detections in detection order.  GROUPS == 3: `late[f] != 0` puts an unmatched detection into a third group, after the second; the second and third
// together take the new ids in that sequence.  A track t stays when tmatch[t] == 0 and its age is below max_age.
template <int THREADS, int GROUPS>
TOC3D_DEV void write_state(const TracksArgs& a, const Stream& s, int N, const int* dmatch, const unsigned char* late, const unsigned short* drow,
                           const unsigned char* dlab, const unsigned char* tmatch, int* s_cnt) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = a.K, cap = a.cap, M = s.M, id_count = s.id_count;
    const State &in = s.in, &out = s.out;
    const double lag = s.lag;
    int held;                                                                // tracks in the new state
    int new_id_count = id_count;
    if (N > 0) {
        // 5. matches, then unmatched detections, then the unmatched tracks young enough
        int nm = 0, nearly = 0;                                              // matches; unmatched detections that are not late
        for (int c0 = 0; c0 < N; c0 += THREADS) {
            const int f = c0 + tid;
            int total;
            block_prefix<THREADS>(f < N && dmatch[f] >= 0, s_cnt, lane, wave, total);
            nm += total;
            if (GROUPS == 3) {
                block_prefix<THREADS>(f < N && dmatch[f] < 0 && !late[f], s_cnt, lane, wave, total);
                nearly += total;
            }
        }
        int mbase = 0, ebase = 0;
        for (int c0 = 0; c0 < N; c0 += THREADS) {
            const int f = c0 + tid;
            const bool live = f < N;
            const int t = live ? dmatch[f] : -1;
            int total;
            const int rm = mbase + block_prefix<THREADS>(t >= 0, s_cnt, lane, wave, total);      // matches before f
            mbase += total;
            bool is_late = false;
            int re = 0;                                                      // unmatched detections before f that are not late
            if (GROUPS == 3) {
                is_late = live && t < 0 && late[f];
                re = ebase + block_prefix<THREADS>(live && t < 0 && !is_late, s_cnt, lane, wave, total);
                ebase += total;
            }
            if (live) {
                int ru = f - rm;                                             // unmatched detections before f
                if (GROUPS == 3) ru = is_late ? nearly + (ru - re) : re;     // ... in the order of the second and third group
                const int pos = t >= 0 ? rm : nm + ru;                       // pos < N <= K <= cap
                const int row = drow[f];
                const double* r = s.rec + (int64_t)row * REC;
                const int id = t >= 0 ? in.id[t] : id_count + ru + 1;
                const int act = t >= 0 ? in.active[t] + 1 : 1;
                out.ct[2 * pos] = r[0]; out.ct[2 * pos + 1] = r[1];
                out.tracking[2 * pos] = (r[10] * -1.0) * lag; out.tracking[2 * pos + 1] = (r[11] * -1.0) * lag;
                out.label[pos] = dlab[f]; out.id[pos] = id; out.age[pos] = 1; out.active[pos] = act;
                s.order[pos] = row; s.track_id[row] = id; s.active[row] = act;
            }
        }
        new_id_count = id_count + (N - nm);
        int kbase = N;
        for (int t0 = 0; t0 < M; t0 += THREADS) {
            const int t = t0 + tid;
            const bool stay = t < M && !tmatch[t] && in.age[t] < a.max_age;
            int total;
            const int pos = kbase + block_prefix<THREADS>(stay, s_cnt, lane, wave, total);
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
    for (int i = N + tid; i < K; i += THREADS) s.order[i] = -1;
    if (tid == 0) {
        int32_t* h = reinterpret_cast<int32_t*>(s.sout);
        h[0] = held; h[1] = new_id_count;
        *reinterpret_cast<double*>(s.sout + 8) = s.ts;
        h[4] = 0; h[5] = 0; h[6] = 0; h[7] = 0;
        a.num_out[blockIdx.x] = N;
    }
}

}  // namespace tracks

// the argument checks of a step, before any launch: the refusals include/toc3d_tracks.h lists, with the caller's caps (k_note: what its K cap is)
#define TOC3D_TRACKS_STEP_CHECKS(fn, max_k, k_note, max_cap, extra_out)                                                                                              \
    TOC3D_REQUIRE(B >= 0 && K >= 0, "%s: bad dims (B and K must not be negative)", fn);                                                                              \
    TOC3D_REQUIRE(K <= (max_k), "%s: bad dims (K at most %d, %s)", fn, (int)(max_k), k_note);                                                                        \
    TOC3D_REQUIRE(B <= 65535, "%s: bad dims (B at most 65535: one launch's grid)", fn);                                                                              \
    TOC3D_REQUIRE(max_age >= 0, "%s: bad max_age (must not be negative)", fn);                                                                                       \
    TOC3D_REQUIRE(capacity >= 0 && capacity <= (max_cap), "%s: bad capacity (at most %d tracks a stream)", fn, (int)(max_cap));                                      \
    TOC3D_REQUIRE(K == 0 || max_age < capacity / K, "%s: bad capacity (capacity >= K * (max_age + 1): what a step can hold)", fn);                                   \
    const bool work = B > 0;                                                                                                                                         \
    TOC3D_REQUIRE(!work || (kept && track_label && max_diff && timestamp && first && state_in && state_out && num_out && (extra_out)), "%s: null buffer", fn);       \
    TOC3D_REQUIRE(!work || K == 0 || (rec && score && name && track_id && active && order), "%s: null buffer", fn);                                                  \
    TOC3D_REQUIRE(num_classes >= 1 && num_classes <= tracks::MAX_LABELS, "%s: bad num_classes (1 <= num_classes <= %d)", fn, tracks::MAX_LABELS);                    \
    TOC3D_REQUIRE(num_track_labels >= 1 && num_track_labels <= tracks::MAX_LABELS, "%s: bad num_track_labels (1 <= num_track_labels <= %d)", fn, tracks::MAX_LABELS); \
    TOC3D_REQUIRE(std::isfinite(score_thr), "%s: bad score_thr (a finite number)", fn);                                                                              \
    TOC3D_REQUIRE(((uintptr_t)rec & 7) == 0 && ((uintptr_t)timestamp & 7) == 0, "%s: bad alignment (rec and timestamp start on an 8-byte boundary)", fn);            \
    TOC3D_REQUIRE(((uintptr_t)state_in & 7) == 0 && ((uintptr_t)state_out & 7) == 0, "%s: bad alignment (state_in and state_out start on an 8-byte boundary)", fn);  \
    if (!work) return TOC3D_OK;                                                                                                                                      \
    {                                                                                                                                                                \
        const uintptr_t si = (uintptr_t)state_in, so = (uintptr_t)state_out, span = (uintptr_t)(B * TOC3D_TRACKS_STATE_BYTES(capacity));                             \
        TOC3D_REQUIRE(si + span <= so || so + span <= si, "%s: state_in and state_out overlap (a step reads one and writes the other)", fn);                         \
        const void* always[] = {kept, track_label, max_diff, timestamp, first, state_in, state_out, num_out, (extra_out)};                                           \
        for (const void* p : always) TOC3D_REQUIRE(toc3d_device_memory(p), "%s: host pointer (every buffer must be device memory)", fn);                             \
        const void* rows[] = {rec, score, name, track_id, active, order};                                                                                            \
        for (const void* p : rows) TOC3D_REQUIRE(K == 0 || toc3d_device_memory(p), "%s: host pointer (every buffer must be device memory)", fn);                     \
    }
