// The host side of toc3d_tracks_step_hungarian (include/toc3d_assign.h) under the host sanitizers: a stand-alone program that compiles
// csrc/tracking_hungarian.hip itself, with stand-ins for the three symbols it takes from capi.cpp and plan.cpp, and walks the argument checks -- the caps of its own, every refusal it
// shares with toc3d_tracks_step, the no-work form, and real host buffers, which must be refused as "host pointer" and left untouched.  Nothing is launched: every call ends in the checks.
// Needs no GPU.
//
//   cd toc3d_amd/csrc && hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -x hip tracking_hungarian.hip ../../tools/sanitize/tracking_hungarian_args.cpp -o /tmp/tracking_hungarian_args && /tmp/tracking_hungarian_args
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/toc3d_assign.h"
#include "../../toc3d_amd/csrc/capi.h"

static char g_error[512];
void toc3d_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}
thread_local Toc3dPlan* toc3d_tls_recording = nullptr;
void toc3d_plan_record(Toc3dPlan*, const void*, dim3, dim3, size_t, hipStream_t, const void* const*, const size_t*, const size_t*, int) {
    fprintf(stderr, "a launch was recorded: the checks let a call through\n");
    abort();
}

namespace {

struct Args {
    const double* rec; const float* score; const int32_t* name; const int64_t* kept; int64_t B, K; const int32_t* label; int64_t ncls; const float* gate; int64_t nl;
    double thr; int64_t max_age; const double* ts; const int32_t* first; const void* sin; void* sout; int64_t cap;
    int32_t* track_id; int32_t* active; int32_t* order; int64_t* num_out; int32_t* rounds;
};

int call(const Args& a) {
    g_error[0] = 0;
    return toc3d_tracks_step_hungarian(a.rec, a.score, a.name, a.kept, a.B, a.K, a.label, a.ncls, a.gate, a.nl, a.thr, a.max_age, a.ts, a.first, a.sin, a.sout, a.cap, a.track_id,
                                       a.active, a.order, a.num_out, a.rounds, nullptr);
}

int failures = 0;
void expect(const char* what, const Args& a, int rc_want, const char* reason) {
    const int rc = call(a);
    const bool ok = rc == rc_want && (reason == nullptr || strstr(g_error, reason) != nullptr);
    printf("%-52s rc %2d %s%s\n", what, rc, g_error, ok ? "" : "   <-- UNEXPECTED");
    failures += !ok;
}

}  // namespace

int main() {
    constexpr int64_t B = 2, K = 5, AGE = 3, CAP = K * (AGE + 1);
    const int64_t sbytes = TOC3D_TRACKS_STATE_BYTES(CAP);
    std::vector<double> rec(B * K * 12, 1.0), ts(B, 10.0);
    std::vector<float> score(B * K, 0.5f), gate(7, 2.5f);
    std::vector<int32_t> name(B * K, 0), label(10, 0), first(B, 1), track_id(B * K, 7), active(B * K, 7), order(B * K, 7), rounds(B, 7);
    std::vector<int64_t> kept(B, K), num_out(B, 7);
    std::vector<double> sin(B * sbytes / 8, 7.0), sout(B * sbytes / 8, 7.0);                // (doubles: on an 8-byte boundary)
    const Args good{rec.data(), score.data(), name.data(), kept.data(), B, K, label.data(), 10, gate.data(), 7, 0.25, AGE, ts.data(), first.data(), sin.data(), sout.data(),
                    CAP, track_id.data(), active.data(), order.data(), num_out.data(), rounds.data()};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const int64_t big = std::numeric_limits<int64_t>::max(), small = std::numeric_limits<int64_t>::min();
    Args a = good;
    expect("host buffers", a, TOC3D_ERR_ARG, "host pointer");
    a = good; a.B = -1; expect("B < 0", a, TOC3D_ERR_ARG, "must not be negative");
    a = good; a.K = small; expect("K = INT64_MIN", a, TOC3D_ERR_ARG, "must not be negative");
    a = good; a.K = 513; a.cap = 2048; a.max_age = 0; expect("K > 512", a, TOC3D_ERR_ARG, "K at most 512");
    a = good; a.K = 2048; expect("K = 2048, the greedy step's cap", a, TOC3D_ERR_ARG, "K at most 512");
    a = good; a.K = big; expect("K = INT64_MAX", a, TOC3D_ERR_ARG, "K at most 512");
    a = good; a.B = 65536; expect("B > 65535", a, TOC3D_ERR_ARG, "at most 65535");
    a = good; a.B = big; expect("B = INT64_MAX", a, TOC3D_ERR_ARG, "at most 65535");
    a = good; a.max_age = -1; expect("max_age < 0", a, TOC3D_ERR_ARG, "bad max_age");
    a = good; a.max_age = small; expect("max_age = INT64_MIN", a, TOC3D_ERR_ARG, "bad max_age");
    a = good; a.cap = 2049; expect("capacity > 2048", a, TOC3D_ERR_ARG, "bad capacity (at most 2048");
    a = good; a.cap = 8192; expect("capacity 8192, the greedy step's cap", a, TOC3D_ERR_ARG, "bad capacity (at most 2048");
    a = good; a.cap = big; expect("capacity = INT64_MAX", a, TOC3D_ERR_ARG, "bad capacity");
    a = good; a.cap = -1; expect("capacity < 0", a, TOC3D_ERR_ARG, "bad capacity");
    a = good; a.cap = CAP - 1; expect("capacity < K * (max_age + 1)", a, TOC3D_ERR_ARG, "capacity >= K * (max_age + 1)");
    a = good; a.max_age = big; expect("max_age = INT64_MAX (max_age + 1 would wrap)", a, TOC3D_ERR_ARG, "capacity >= K * (max_age + 1)");
    a = good; a.K = 512; a.cap = 2048; a.max_age = 4; expect("K 512, max_age 4: 2560 tracks", a, TOC3D_ERR_ARG, "capacity >= K * (max_age + 1)");
    a = good; a.rec = nullptr; expect("rec NULL", a, TOC3D_ERR_ARG, "null buffer");
    a = good; a.kept = nullptr; expect("kept NULL", a, TOC3D_ERR_ARG, "null buffer");
    a = good; a.sin = nullptr; expect("state_in NULL", a, TOC3D_ERR_ARG, "null buffer");
    a = good; a.sout = nullptr; expect("state_out NULL", a, TOC3D_ERR_ARG, "null buffer");
    a = good; a.num_out = nullptr; expect("num_out NULL", a, TOC3D_ERR_ARG, "null buffer");
    a = good; a.order = nullptr; expect("order NULL", a, TOC3D_ERR_ARG, "null buffer");
    a = good; a.rounds = nullptr; expect("rounds NULL", a, TOC3D_ERR_ARG, "null buffer");
    a = good; a.ncls = 0; expect("num_classes 0", a, TOC3D_ERR_ARG, "bad num_classes");
    a = good; a.ncls = 65; expect("num_classes 65", a, TOC3D_ERR_ARG, "bad num_classes");
    a = good; a.nl = 0; expect("num_track_labels 0", a, TOC3D_ERR_ARG, "bad num_track_labels");
    a = good; a.nl = big; expect("num_track_labels = INT64_MAX", a, TOC3D_ERR_ARG, "bad num_track_labels");
    a = good; a.thr = nan; expect("score_thr NaN", a, TOC3D_ERR_ARG, "bad score_thr");
    a = good; a.thr = inf; expect("score_thr inf", a, TOC3D_ERR_ARG, "bad score_thr");
    a = good; a.rec = reinterpret_cast<const double*>(reinterpret_cast<const char*>(rec.data()) + 4); expect("rec off an 8-byte boundary", a, TOC3D_ERR_ARG, "8-byte boundary");
    a = good; a.ts = reinterpret_cast<const double*>(reinterpret_cast<const char*>(ts.data()) + 4); expect("timestamp off an 8-byte boundary", a, TOC3D_ERR_ARG, "8-byte boundary");
    a = good; a.sout = reinterpret_cast<char*>(sout.data()) + 4; expect("state_out off an 8-byte boundary", a, TOC3D_ERR_ARG, "8-byte boundary");
    a = good; a.sout = sin.data(); expect("state_out == state_in", a, TOC3D_ERR_ARG, "overlap");
    a = good; a.sout = reinterpret_cast<char*>(sin.data()) + sbytes; expect("state_out inside state_in", a, TOC3D_ERR_ARG, "overlap");
    a = good; a.B = 0; expect("B == 0: no work", a, TOC3D_OK, nullptr);
    a = Args{nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 10, nullptr, 7, 0.25, 3, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr};
    expect("B == K == 0, every pointer NULL", a, TOC3D_OK, nullptr);
    a = good; a.K = 0; a.cap = 0; a.rec = nullptr; a.score = nullptr; a.name = nullptr; a.track_id = nullptr; a.active = nullptr; a.order = nullptr;
    expect("K == 0 without row buffers: host state refused", a, TOC3D_ERR_ARG, "host pointer");
    bool untouched = true;
    for (double v : sin) untouched = untouched && v == 7.0;
    for (double v : sout) untouched = untouched && v == 7.0;
    for (size_t i = 0; i < track_id.size(); ++i) untouched = untouched && track_id[i] == 7 && active[i] == 7 && order[i] == 7;
    for (int64_t v : num_out) untouched = untouched && v == 7;
    for (int32_t v : rounds) untouched = untouched && v == 7;
    for (double v : rec) untouched = untouched && v == 1.0;
    printf("host buffers untouched: %s\n", untouched ? "yes" : "NO");
    failures += !untouched;
    if (toc3d_assign_abi() != TOC3D_ASSIGN_ABI) ++failures;
    printf("%s\n", failures ? "FAILED" : "all refusals as the header states");
    return failures ? 1 : 0;
}
