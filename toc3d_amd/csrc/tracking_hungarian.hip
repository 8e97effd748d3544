// The tracking step with the reference's hungarian=True (include/toc3d_assign.h): scipy's rectangular shortest-augmenting-path solver replayed operation for
// operation on the matrix nusc_tracking/pub_tracker.py:119-129 builds, one workgroup per stream, the matrix never materialised, the solver's state in LDS.  The
// filter and the write of the new state are tracking.hip's (tracks_steps.h).
#include "../../include/toc3d_assign.h"
#include "capi.h"
#include "common.h"

#include <climits>
#include <cmath>

// every float64 and float32 operation below is rounded once, in the order the header states: no fused multiply-adds
#pragma clang fp contract(off)

#include "tracks_steps.h"

namespace {

using namespace tracks;

// Four wavefronts, one per SIMD.  The kernel is its dependent chain: rounds x (a walk over the list + the pick).  One wavefront would need no barrier but walks
// nc / 64 positions a lane and round (19 at 1200 tracks, 32 at the caps), each a float32 distance and three float64 operations behind LDS reads; four walk a
// quarter of that and pay one barrier and four 16-byte LDS reads a round.  DESIGN.md 4n has the figures.
#ifndef TOC3D_ASSIGN_THREADS
#define TOC3D_ASSIGN_THREADS 256           // (a development build may set 64, 128 or 512: make EXTRA=-DTOC3D_ASSIGN_THREADS=64 ..., for tools/tracking_hungarian_time.py)
#endif
constexpr int THREADS = TOC3D_ASSIGN_THREADS, WAVES = THREADS / 64;
static_assert(THREADS >= 64 && THREADS <= 512 && (THREADS & (THREADS - 1)) == 0, "a power of two of whole wavefronts");
constexpr int MAX_K = TOC3D_ASSIGN_MAX_BOXES, MAX_CAP = TOC3D_ASSIGN_MAX_TRACKS;
constexpr unsigned long long NONE = ~0ull;
constexpr double INVALID = 1e18, SHOWN_BELOW = 1e16;                         // pub_tracker.py:126-128, :146
constexpr unsigned LATE = 2048u, POS = 2047u;                                // the pick's second key: 12 bits, bit 11 set when the column is assigned

// dynamic LDS of a launch, per column (cap) and per row or detection (K): see the kernel's carve-up
size_t lds_bytes(int64_t cap, int64_t K) { return (size_t)(cap * (8 + 8 + 4 + 4 + 2 + 2 + 2 + 1 + 1) + K * (8 + 4 + 4 + 4 + 2 + 2 + 1 + 1)); }

// float64 -> uint64 that orders as the numbers do, negative ones included (+0.0 and -0.0 are made one value first); and back
TOC3D_DEV unsigned long long image_of(double x) {
    if (x == 0.0) x = 0.0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : b | (1ull << 63);
}
TOC3D_DEV double number_of(unsigned long long k) { return __longlong_as_double((long long)((k >> 63) ? k & ~(1ull << 63) : ~k)); }

TOC3D_DEV unsigned wave_min_u32(unsigned k) {
    {
        const auto a = __builtin_amdgcn_permlane32_swap(k, k, false, false);
        k = a[0] < a[1] ? a[0] : a[1];
    }
    {
        const auto a = __builtin_amdgcn_permlane16_swap(k, k, false, false);
        k = a[0] < a[1] ? a[0] : a[1];
    }
    unsigned o;
    o = (unsigned)dpp_mov_i<DPP_ROW_ROR8>((int)k); k = o < k ? o : k;
    o = (unsigned)lane_xor4_i((int)k); k = o < k ? o : k;
    o = (unsigned)dpp_mov_i<DPP_QUAD_XOR2>((int)k); k = o < k ? o : k;
    o = (unsigned)dpp_mov_i<DPP_QUAD_XOR1>((int)k); k = o < k ? o : k;
    return k;
}

struct Pick { unsigned long long key; unsigned second, pad; };              // 16 bytes: one LDS read

__global__ __launch_bounds__(THREADS) void tracks_step_hungarian_kernel(TracksArgs a, int32_t* rounds_out) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int s_cnt[WAVES];
    __shared__ float s_gate[MAX_LABELS];                                     // max_diff: read once a round, on the chain
    __shared__ __align__(16) Pick s_pick[2][WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, K = a.K, cap = a.cap;
    // per column (a column is a track, or a detection when N > M: at most max(cap, K) = cap of them whenever there is something to solve)
    double* spc = reinterpret_cast<double*>(smem);                           // [cap] the shortest path cost to a column in this row's search
    double* v = spc + cap;                                                   // [cap] a column's dual
    double* u = v + cap;                                                     // [K]   a row's dual
    float* tqx = reinterpret_cast<float*>(u + K);                            // [cap] the tracks' float32 positions, track order
    float* tqy = tqx + cap;
    float* dpx = tqy + cap;                                                  // [K] the surviving detections' float32 positions, detection order
    float* dpy = dpx + K;
    int* dmatch = reinterpret_cast<int*>(dpy + K);                           // [K] the track a detection continues, -1 none
    short* path = reinterpret_cast<short*>(dmatch + K);                      // [cap] the row a column's shortest path comes from
    short* row4col = path + cap;                                             // [cap]
    unsigned short* remaining = reinterpret_cast<unsigned short*>(row4col + cap);      // [cap] the list of a row's search; its tail holds the columns scanned off it
    short* col4row = reinterpret_cast<short*>(remaining + cap);             // [K]
    unsigned short* drow = reinterpret_cast<unsigned short*>(col4row + K);   // [K] surviving detection -> input row
    unsigned char* tlab = reinterpret_cast<unsigned char*>(drow + K);        // [cap] a track's label (255: none a detection can have)
    unsigned char* tmatch = tlab + cap;                                      // [cap] 1: the track is in a match, valid or not
    unsigned char* dlab = tmatch + cap;                                      // [K] a surviving detection's label
    unsigned char* late = dlab + K;                                          // [K] 1: the detection is in a match that costs more than 1e16

    const Stream s = stream_of(a, b);                                        // 0.
    const int M = s.M;
    const int N = filter_compact<THREADS>(a, s, dpx, dpy, drow, dlab, dmatch, s_cnt);     // 1, 2.
    for (int t = tid; t < M; t += THREADS) {
        tmatch[t] = 0;
        const int lab = s.in.label[t];
        tqx[t] = (float)s.in.ct[2 * t]; tqy[t] = (float)s.in.ct[2 * t + 1]; tlab[t] = lab >= 0 && lab < a.nl ? (unsigned char)lab : (unsigned char)255;
    }
    for (int f = tid; f < N; f += THREADS) late[f] = 0;
    if (tid < a.nl) s_gate[tid] = a.max_diff[tid];                           // nl <= 64 <= THREADS
    __syncthreads();

    int rounds = 0;
    if (N > 0 && M > 0) {
        // 3, 4h.  Rows are detections, or tracks when N > M; (q - p) * (q - p) is (p - q) * (p - q) bit for bit, so a cost reads the same from either side.
        const bool transposed = N > M;
        const int nr = transposed ? M : N, nc = transposed ? N : M;          // nr <= nc <= cap, nr <= K
        const float *rx = transposed ? tqx : dpx, *ry = transposed ? tqy : dpy, *cx = transposed ? dpx : tqx, *cy = transposed ? dpy : tqy;
        const unsigned char *rlab = transposed ? tlab : dlab, *clab = transposed ? dlab : tlab;
        const auto cost = [&](float px, float py, int lab, float gate, int j) {
            // plain operators under this file's contract(off); sqrtf is the correctly rounded one: the Makefile passes no fast-math flag
            const float dx = cx[j] - px, dy = cy[j] - py;
            const float xx = dx * dx, yy = dy * dy;
            const float dist = sqrtf(xx + yy);
            return clab[j] == lab && dist <= gate ? (double)dist : INVALID;  // (a NaN distance compares false: invalid)
        };
        for (int j = tid; j < nc; j += THREADS) { v[j] = 0.0; row4col[j] = -1; path[j] = -1; spc[j] = INFINITY; remaining[j] = (unsigned short)(nc - 1 - j); }
        for (int i = tid; i < nr; i += THREADS) { u[i] = 0.0; col4row[i] = -1; }
        __syncthreads();
        for (int cur = 0; cur < nr; ++cur) {
            double min_val = 0.0;
            int i = cur, nrem = nc, sink = -1;
            for (int round = 0; round <= cur && sink < 0; ++round, ++rounds) {       // (uniform: every thread holds the same cur, sink, nrem, i, min_val)
                const float px = rx[i], py = ry[i];
                const int lab = rlab[i];
                const float gate = lab < a.nl ? s_gate[lab] : 0.f;       // (lab == 255 equals no column's label)
                const double ui = u[i];
                unsigned long long best = NONE;
                unsigned second = ~0u;
                for (int it = tid; it < nrem; it += THREADS) {
                    const int j = remaining[it];
                    const double r = ((min_val + cost(px, py, lab, gate, j)) - ui) - v[j];
                    double sp = spc[j];
                    if (r < sp) { path[j] = (short)i; spc[j] = r; sp = r; }
                    // the last unassigned position among the smallest, else the first position among them
                    const unsigned long long key = image_of(sp);
                    const unsigned sec = ((row4col[j] < 0 ? POS - (unsigned)it : LATE | (unsigned)it) << 16) | (unsigned)j;
                    if (key < best || (key == best && sec < second)) { best = key; second = sec; }
                }
                const unsigned long long wbest = wave_min_u64(best);
                const unsigned wsecond = wave_min_u32(best == wbest ? second : ~0u);
                Pick* slot = s_pick[round & 1];                              // (read until the next barrier, written again after it: two slots)
                if (lane == 0) { slot[wave].key = wbest; slot[wave].second = wsecond; }
                __syncthreads();
                Pick p = slot[0];
#pragma unroll
                for (int w = 1; w < WAVES; ++w) {
                    const Pick o = slot[w];
                    if (o.key < p.key || (o.key == p.key && o.second < p.second)) p = o;
                }
                if (p.key == NONE) break;                                    // (nrem >= nc - cur > 0: some thread had a position; never taken)
                min_val = number_of(p.key);
                const int j = (int)(p.second & 0xffffu);
                const unsigned sec = p.second >> 16;
                const bool unassigned = !(sec & LATE);
                const int pick = unassigned ? (int)(POS - sec) : (int)(sec & POS);
                --nrem;
                if ((pick & (THREADS - 1)) == tid) {                         // the owner of the picked position: no other thread reads or writes it before the next barrier
                    const unsigned short tail = remaining[nrem];
                    remaining[pick] = tail; remaining[nrem] = (unsigned short)j;      // the column scanned off the list is kept in its tail: SC
                }
                if (unassigned) sink = j;
                else i = row4col[j];
            }
            __syncthreads();                                                 // the list's tail and spc, as the last round left them
            if (sink >= 0) {
                // duals: the columns of SC are the list's tail; the rows of SR are cur and the rows those columns are assigned to (col4row[row4col[j]] == j)
                for (int p = nrem + tid; p < nc; p += THREADS) {
                    const int j = remaining[p];
                    const double d = min_val - spc[j];
                    v[j] -= d;
                    const int r = row4col[j];
                    if (j != sink && r >= 0) u[r] += d;                      // (a column scanned off the list that is not the sink is assigned)
                }
                if (tid == 0) u[cur] += min_val;
            }
            __syncthreads();
            if (sink >= 0 && tid == 0) {                                     // augment: at most cur + 1 steps
                int j = sink;
                for (int step = 0; step <= cur; ++step) {
                    const int r = path[j];
                    if (r < 0 || r >= nr) break;                             // (every column on the path was reached from a row: never taken)
                    row4col[j] = (short)r;
                    const int next = col4row[r];
                    col4row[r] = (short)j;
                    j = next;
                    if (r == cur || j < 0) break;
                }
            }
            for (int j = tid; j < nc; j += THREADS) { spc[j] = INFINITY; remaining[j] = (unsigned short)(nc - 1 - j); }
            __syncthreads();
        }
        // the matches: valid ones continue a track; a detection in an invalid one is late; a track in either is taken
        for (int r = tid; r < nr; r += THREADS) {
            const int c = col4row[r];
            if (c < 0) continue;                                             // (every row is assigned: never taken)
            const int lab = rlab[r];
            const float gate = lab < a.nl ? s_gate[lab] : 0.f;
            const bool good = cost(rx[r], ry[r], lab, gate, c) <= SHOWN_BELOW;
            const int f = transposed ? c : r, t = transposed ? r : c;
            tmatch[t] = 1;
            if (good) dmatch[f] = t;
            else late[f] = 1;
        }
        __syncthreads();
    }
    write_state<THREADS, 3>(a, s, N, dmatch, late, drow, dlab, tmatch, s_cnt);          // 5h, 6.
    if (tid == 0) rounds_out[b] = rounds;
}

}  // namespace

extern "C" {

int toc3d_assign_abi(void) { return TOC3D_ASSIGN_ABI; }

int toc3d_tracks_step_hungarian(const double* rec, const float* score, const int32_t* name, const int64_t* kept, int64_t B, int64_t K, const int32_t* track_label,
                                int64_t num_classes, const float* max_diff, int64_t num_track_labels, double score_thr, int64_t max_age, const double* timestamp,
                                const int32_t* first, const void* state_in, void* state_out, int64_t capacity, int32_t* track_id, int32_t* active, int32_t* order,
                                int64_t* num_out, int32_t* rounds, toc3d_stream_t stream) {
    const char* fn = "toc3d_tracks_step_hungarian";
    TOC3D_TRACKS_STEP_CHECKS(fn, MAX_K, "TOC3D_ASSIGN_MAX_BOXES", MAX_CAP, rounds);
    TracksArgs a;
    a.rec = rec; a.score = score; a.name = name; a.kept = kept; a.track_label = track_label; a.max_diff = max_diff; a.timestamp = timestamp; a.first = first;
    a.state_in = static_cast<const char*>(state_in); a.state_out = static_cast<char*>(state_out);
    a.track_id = track_id; a.active = active; a.order = order; a.num_out = num_out; a.score_thr = score_thr;
    a.K = (int)K; a.ncls = (int)num_classes; a.nl = (int)num_track_labels; a.max_age = max_age > INT_MAX ? INT_MAX : (int)max_age; a.cap = (int)capacity;
    const size_t lds = lds_bytes(capacity, K);                               // at most 32 * 2048 + 26 * 512 = 78848 bytes of the CU's 160 KiB
    static Toc3dLdsAttr attr;
    if (lds > 48 * 1024) attr.ensure(reinterpret_cast<const void*>(&tracks_step_hungarian_kernel), (int)lds_bytes(MAX_CAP, MAX_K));
    toc3d_launch(tracks_step_hungarian_kernel, dim3((unsigned)B), dim3(THREADS), lds, as_stream(stream), a, rounds);
    TOC3D_LAUNCH_CHECK(fn);
    return TOC3D_OK;
}

}  // extern "C"
