// What the row kernels (tokens, scorer, mha's row kernels, head_tokens / head_queries / head_outputs) share: stores of an act-dtype row in its three forms
// (f32, bf16, f32 as (hi, lo) planes -- f32p_t and the layout, common.h), mmdet's inverse_sigmoid, and on the host the dispatch of an entry point's dtype
// onto the kernel's element type and the alignment / planes-rows refusals.  A new act form or a change of the planes layout starts here.
#pragma once
#include "capi.h"
#include "common.h"

// ---- device: stores ---------------------------------------------------------------------------------------------------------------------------------
// one element of an act row: the act dtype's rounding, or -- f32p_t -- the element's (hi, lo) pair at planes_addr
template <typename T> TOC3D_DEV void put1(T* p, float v) { *p = to_act<T>(v); }
template <> TOC3D_DEV void put1<f32p_t>(f32p_t* p, float v) {
    const bf16_t h = (bf16_t)v;
    char* g = planes_addr(p);
    *reinterpret_cast<bf16_t*>(g) = h;
    *reinterpret_cast<bf16_t*>(g + 64) = (bf16_t)(v - (float)h);
}
// 4 consecutive elements, the first at a multiple of 4 columns of an aligned row: per element the bits of put1, as one 16-byte (f32) or 8-byte (bf16; each
// plane of f32p_t) store
template <typename T> TOC3D_DEV void put4(T* p, const float (&v)[4]);
template <> TOC3D_DEV void put4<float>(float* p, const float (&v)[4]) { store4(p, v); }
template <> TOC3D_DEV void put4<bf16_t>(bf16_t* p, const float (&v)[4]) {
    const bf16_t b[4] = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
    store4(p, b);
}
template <> TOC3D_DEV void put4<f32p_t>(f32p_t* p, const float (&v)[4]) { store4_planes(p, v); }

// mmdet's inverse_sigmoid: clamp to [0, 1], eps = 1e-5 on numerator and denominator
TOC3D_DEV float inverse_sigmoid(float x) {
    x = fminf(fmaxf(x, 0.f), 1.f);
    return logf(fmaxf(x, 1e-5f) / fmaxf(1.f - x, 1e-5f));
}

// (The one-wavefront-per-row LayerNorm statistics are NOT here.  Each row kernel keeps its own: the order of its additions is part of its result -- tokens.hip
// pairs the squares of a float4, the head's kernels add them one by one, head_queries.hip starts its sum without a 0.f -- and where two kernels do spell the
// same sums (add_ln_pos_kernel, mln_kernel) a common helper still changed their schedules and register counts.)

// ---- host: refusals and dtype dispatch ------------------------------------------------------------------------------------------------------------------
inline bool aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }      // bytes: a power of two
// rows of (hi, lo) planes are whole 128-byte groups: the host half of planes_addr
inline bool planes_rows_ok(const void* p, int64_t ld) { return aligned(p, 128) && ld % 32 == 0; }

// The act dtypes an entry point serves, as a set; toc3d_dispatch_act calls fn(ActTag<T>()) with the element type of `dtype` when the set holds it (fn is
// instantiated for the set's types only), and otherwise refuses with "<entry>: bad dtype".
constexpr unsigned ACT_F32 = 1u << TOC3D_F32, ACT_BF16 = 1u << TOC3D_BF16, ACT_PLANES = 1u << TOC3D_F32X3P, ACT_ANY = ACT_F32 | ACT_BF16 | ACT_PLANES;
template <typename T> struct ActTag { using type = T; };
inline bool act_served(unsigned allowed, int dtype) { return dtype >= 0 && dtype < 32 && ((allowed >> dtype) & 1u); }
template <unsigned ALLOWED, typename F>
int toc3d_dispatch_act(const char* entry, int dtype, F&& fn) {
    if (!act_served(ALLOWED, dtype)) { toc3d_set_error("%s: bad dtype", entry); return TOC3D_ERR_ARG; }
    if constexpr ((ALLOWED & ACT_BF16) != 0) if (dtype == TOC3D_BF16) fn(ActTag<bf16_t>());
    if constexpr ((ALLOWED & ACT_F32) != 0) if (dtype == TOC3D_F32) fn(ActTag<float>());
    if constexpr ((ALLOWED & ACT_PLANES) != 0) if (dtype == TOC3D_F32X3P) fn(ActTag<f32p_t>());
    return TOC3D_OK;
}
