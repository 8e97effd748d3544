// The host side of toc3d_boxes_to_global (include/toc3d_results.h) under the host sanitizers: a stand-alone program that compiles csrc/nusc_results.hip itself,
// with stand-ins for the three symbols it takes from capi.cpp and plan.cpp, and walks the argument checks -- every refusal of the header, the two no-work forms, and
// real host buffers, which must be refused as "host pointer" and left untouched.  Nothing is launched: every call ends in the checks.  Needs no GPU.
//
//   cd toc3d_amd/csrc && hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -x hip nusc_results.hip ../../tools/sanitize/nusc_results_args.cpp -o /tmp/nusc_results_args && /tmp/nusc_results_args
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/toc3d_results.h"
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
    const float* boxes; int64_t box_stride, sample_stride; const float* scores; const int64_t* labels; const int64_t* counts; int64_t B, K; int vel;
    const double* poses; const double* range; const int32_t* mov; const int32_t* still; int64_t ncls; double thr;
    double* rec; float* score; int32_t* name; int32_t* attr; int32_t* src; int64_t* kept;
};

int call(const Args& a) {
    g_error[0] = 0;
    return toc3d_boxes_to_global(a.boxes, a.box_stride, a.sample_stride, a.scores, a.labels, a.counts, a.B, a.K, a.vel, a.poses, a.range, a.mov, a.still, a.ncls, a.thr,
                                 a.rec, a.score, a.name, a.attr, a.src, a.kept, nullptr);
}

int failures = 0;
void expect(const char* what, const Args& a, int rc_want, const char* reason) {
    const int rc = call(a);
    const bool ok = rc == rc_want && (reason == nullptr || strstr(g_error, reason) != nullptr);
    printf("%-44s rc %2d %s%s\n", what, rc, g_error, ok ? "" : "   <-- UNEXPECTED");
    failures += !ok;
}

}  // namespace

int main() {
    constexpr int64_t B = 2, K = 5;
    std::vector<float> boxes(B * K * 9, 1.f), scores(B * K, 0.5f), score(B * K, 7.f);
    std::vector<int64_t> labels(B * K, 0), counts(B, K), kept(B, 7);
    std::vector<double> poses(B * 14, 0.0), range(10, 50.0), rec(B * K * 12, 7.0);
    std::vector<int32_t> mov(10, 5), still(10, 6), name(B * K, 7), attr(B * K, 7), src(B * K, 7);
    for (int64_t b = 0; b < 2 * B; ++b) poses[b * 7] = 1.0;
    const Args good{boxes.data(), 9, K * 9, scores.data(), labels.data(), counts.data(), B, K, 1, poses.data(), range.data(), mov.data(), still.data(), 10, 0.2,
                    rec.data(), score.data(), name.data(), attr.data(), src.data(), kept.data()};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const int64_t big = std::numeric_limits<int64_t>::max(), small = std::numeric_limits<int64_t>::min();
    Args a = good;
    expect("host buffers", a, TOC3D_ERR_ARG, "host pointer");
    a = good; a.B = -1; expect("B < 0", a, TOC3D_ERR_ARG, "must not be negative");
    a = good; a.K = small; expect("K = INT64_MIN", a, TOC3D_ERR_ARG, "must not be negative");
    a = good; a.K = 2049; expect("K > 2048", a, TOC3D_ERR_ARG, "at most 2048");
    a = good; a.K = big; expect("K = INT64_MAX", a, TOC3D_ERR_ARG, "at most 2048");
    a = good; a.B = 65536; expect("B > 65535", a, TOC3D_ERR_ARG, "at most 65535");
    a = good; a.B = big; expect("B = INT64_MAX", a, TOC3D_ERR_ARG, "at most 65535");
    a = good; a.boxes = nullptr; expect("boxes NULL", a, TOC3D_ERR_ARG, "null buffer");
    a = good; a.kept = nullptr; expect("kept NULL", a, TOC3D_ERR_ARG, "null buffer");
    a = good; a.poses = nullptr; expect("poses NULL", a, TOC3D_ERR_ARG, "null buffer");
    a = good; a.box_stride = 8; expect("box_stride 8 with the velocity", a, TOC3D_ERR_ARG, "smaller than a row");
    a = good; a.vel = 0; a.box_stride = 6; expect("box_stride 6 without", a, TOC3D_ERR_ARG, "smaller than a row");
    a = good; a.box_stride = small; expect("box_stride = INT64_MIN", a, TOC3D_ERR_ARG, "smaller than a row");
    a = good; a.sample_stride = K * 9 - 1; expect("sample_stride < K * box_stride", a, TOC3D_ERR_ARG, "samples that overlap");
    a = good; a.box_stride = big; a.sample_stride = big; expect("box_stride = INT64_MAX (K * box_stride wraps)", a, TOC3D_ERR_ARG, "samples that overlap");
    a = good; a.sample_stride = small; expect("sample_stride = INT64_MIN", a, TOC3D_ERR_ARG, "samples that overlap");
    a = good; a.ncls = 0; expect("num_classes 0", a, TOC3D_ERR_ARG, "bad num_classes");
    a = good; a.ncls = 65; expect("num_classes 65", a, TOC3D_ERR_ARG, "bad num_classes");
    a = good; a.thr = nan; expect("speed_thr NaN", a, TOC3D_ERR_ARG, "bad speed_thr");
    a = good; a.thr = -inf; expect("speed_thr -inf", a, TOC3D_ERR_ARG, "bad speed_thr");
    a = good; a.boxes = reinterpret_cast<const float*>(reinterpret_cast<const char*>(boxes.data()) + 2); expect("boxes off a 4-byte boundary", a, TOC3D_ERR_ARG, "4-byte boundary");
    a = good; a.rec = reinterpret_cast<double*>(reinterpret_cast<char*>(rec.data()) + 4); expect("rec off an 8-byte boundary", a, TOC3D_ERR_ARG, "8-byte boundary");
    a = good; a.poses = reinterpret_cast<const double*>(reinterpret_cast<const char*>(poses.data()) + 4); expect("poses off an 8-byte boundary", a, TOC3D_ERR_ARG, "8-byte boundary");
    a = good; a.B = 0; expect("B == 0: no work", a, TOC3D_OK, nullptr);
    a = good; a.K = 0; a.sample_stride = 0; expect("K == 0: no work", a, TOC3D_OK, nullptr);
    a = Args{nullptr, 9, 0, nullptr, nullptr, nullptr, 0, 0, 1, nullptr, nullptr, nullptr, nullptr, 10, 0.2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    expect("B == K == 0, every pointer NULL", a, TOC3D_OK, nullptr);
    bool untouched = true;
    for (double v : rec) untouched = untouched && v == 7.0;
    for (float v : score) untouched = untouched && v == 7.f;
    for (size_t i = 0; i < name.size(); ++i) untouched = untouched && name[i] == 7 && attr[i] == 7 && src[i] == 7;
    for (int64_t v : kept) untouched = untouched && v == 7;
    for (float v : boxes) untouched = untouched && v == 1.f;
    printf("host buffers untouched: %s\n", untouched ? "yes" : "NO");
    failures += !untouched;
    if (toc3d_results_abi() != TOC3D_RESULTS_ABI) ++failures;
    printf("%s\n", failures ? "FAILED" : "all refusals as the header states");
    return failures ? 1 : 0;
}
