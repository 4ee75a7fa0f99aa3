// rt_cull.h — the certificate arithmetic of the conservative float32 cull (rt_device.h has the derivation of its error budget and the
// loops that run it per wave), and the guard that decides which direction a query's cull reads.  HIP-free C++17 in the style of
// rt_math.h / rt_facing.h: the kernel and the CPU check (tests/algo/cull_direction_check.cpp) compile this same text.
#pragma once
#include "rt_math.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace rt {

constexpr float CULL_K_ANCHOR = 0x1p-19f * 1.0001f;
constexpr float CULL_K_ORIGIN = 0x1p-18f;
constexpr float CULL_K_S = 0x1p-21f;
constexpr float CULL_K_FLOOR = 0x1p-40f;

#ifdef __clang__
typedef float f4 __attribute__((ext_vector_type(4)));
#else
typedef float f4 __attribute__((vector_size(16)));
#endif

struct RayF {              // float32 shadow of a query, for the cull only
    F3 o, R;
    float mgq, esq;        // per-ray parts of the origin form's margins: K_O |o|² + floor,  K_S (1 + |o|²)
};

// The anchored form needs the direction only; the origin terms are added where the origin form is used.
RT_MATH_FN F3 cull_dir32(const V3 &v) { return F3{(float)v.x, (float)v.y, (float)v.z}; }
RT_MATH_FN RayF make_rayf_dir(const F3 &dir)
{
    RayF q;
    q.o = F3{0.0f, 0.0f, 0.0f};
    q.R = dir;
    q.mgq = 0.0f; q.esq = 0.0f;
    return q;
}
RT_MATH_FN RayF make_rayf_dir(const V3 &R) { return make_rayf_dir(cull_dir32(R)); }
RT_MATH_FN void add_origin(RayF &q, const V3 &o, float extent2)
{
    q.o = F3{(float)o.x, (float)o.y, (float)o.z};
    const float oo = __builtin_fmaf(q.o.z, q.o.z, __builtin_fmaf(q.o.y, q.o.y, q.o.x * q.o.x));
    q.mgq = __builtin_fmaf(CULL_K_ORIGIN, oo, CULL_K_FLOOR * (oo + extent2));
    q.esq = __builtin_fmaf(CULL_K_S, oo, CULL_K_S);
}

// tau of one (anchor, sphere) pair: the line through the anchor with unit direction R misses the sphere by more
// than every error the budget allows when |(A-c).R32| < tau.  ll = |A-c|² (float64).
RT_MATH_FN float anchored_tau(double ll, double r2, float floor_anch)
{
    const double W = ((ll - r2) - (ll + r2) * (double)CULL_K_ANCHOR) - (double)floor_anch;
    if (!(W > 0.0)) return 0.0f;                              // anchor inside or too close (or NaN): never certified
    return (float)(__builtin_sqrt(W) * (1.0 - 0x1p-20));      // rounded down: the float32 rounding is within 2^-24
}

// true = this lane holds a certificate that sphere k reports a miss for this ray (anchored form)
RT_MATH_FN bool cull_anchored(const f4 e, const RayF &q)
{
    const float s = __builtin_fmaf(e[2], q.R.z, __builtin_fmaf(e[1], q.R.y, e[0] * q.R.x));
    return __builtin_fabsf(s) < e[3];                         // e[3] = tau (0: never, +inf: padding, always)
}

// origin form: line-miss or behind certificate
RT_MATH_FN bool cull_origin(const f4 c, const RayF &q)
{
    const float lx = q.o.x - c[0], ly = q.o.y - c[1], lz = q.o.z - c[2];
    const float s = __builtin_fmaf(lz, q.R.z, __builtin_fmaf(ly, q.R.y, lx * q.R.x));
    const float ll = __builtin_fmaf(lz, lz, __builtin_fmaf(ly, ly, lx * lx));
    const float cc = ll - c[3];
    const float D = __builtin_fmaf(s, s, -cc);
    const float mg = __builtin_fmaf(CULL_K_ORIGIN, ll + c[3], q.mgq);
    const float es = __builtin_fmaf(CULL_K_S, ll, q.esq);
    // no short-circuit: a divergent branch here costs an exec-mask region plus a select and a compare to get the
    // result back into a lane mask
    return (bool)((int)(D < -mg) | ((int)(s > es) & (int)(cc > mg)));
}

// ---------------------------------------------------------------------------------------------
// Which direction a query's cull reads.  The float64 sphere tests work on R = normalize(d) and a = R.R; the cull needs only a
// float32 direction, and when it leaves no sphere R and a are never read.  So a wave-uniform query (rt_device.h: closest_spheres,
// any_spheres_masks) forms nn = |d|² and e = nn - 1 (the first part of renormalize_unit), and
//   * if EVERY live lane has |e| < UNIT_WINDOW: culls on float32(d) and calls renormalize_unit_fast(d, e) only in front of a
//     float64 sphere test (a chunk whose mask is not empty);
//   * otherwise (one lane outside the window, a NaN included): the former order for the whole wave — R = normalize3_generic(d)
//     first, the cull on float32(R).
// Soundness of the first case.  |e| < 2^-33 puts |d| within a relative 2^-34 (1 + 2^-35) of 1, and R = d / RN(sqrt(nn)) rounded
// per component: d = R (1 + δ) with |δ| <= 2^-34 + 2^-52 per component.  The certificates are evaluated on d32 = float32(d) where
// the budget assumes float32(R): every term that is linear in the direction moves by the relative |δ| < 2^-33.9 = 2^-9.9 u
// (u = 2^-24), before the same float32 roundings as before:
//     s' = (A-c).d32 or L.d32:   |s'| grows by at most 2^-9.9 u Λ  (|s| <= Λ for a unit direction)
//     anchored |D' - D|:         D' = s'² + w; s'² moves by 2 |s| 2^-9.9 u Λ <= 2^-8.9 u Λ²:  13u Λ² -> 13.003u Λ²   (32u used)
//     origin   |D' - D|:         the same term:                                               19u Λ² -> 19.003u Λ²   (64u used)
//     origin   |s' - s|:         u(|o| + 5Λ) -> u(|o| + 5.002Λ)                                 (8u(1 + Λ² + |o|²) used)
//     origin   |c' - c|:         c = |L|² - r2 does not read the direction: unchanged.
// The reference's own D is taken with a = R.R, within 2^-51 of 1 (floor covers it, as before).  Outside the window none of this
// holds: a direction shortened by 2^-12 lowers |s'| by 2^-12 Λ = 2^12 u Λ, far beyond the margins, and a grazing line would be
// certified a miss (tests/algo/cull_direction_check.cpp finds such false certificates at 1 ± 2^-12, and none inside the window
// in 10^7 near-grazing triples).  A NaN component of d makes nn and e NaN: the lane fails the window.  An infinite one makes
// nn infinite: likewise.
// ---------------------------------------------------------------------------------------------
RT_MATH_FN double unit_excess(const V3 &d) { return (d.x * d.x + d.y * d.y + d.z * d.z) - 1.0; }   // e of renormalize_unit (exact subtraction)
RT_MATH_FN bool outside_unit_window(double e) { return !(__builtin_fabs(e) < UNIT_WINDOW); }       // per lane; NaN: outside
// lanes_outside: the wave's ballot of outside_unit_window over its live lanes
RT_MATH_FN bool cull_reads_d(unsigned long long lanes_outside) { return lanes_outside == 0ull; }

}  // namespace rt
