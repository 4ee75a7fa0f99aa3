// rt_math.h — the exact-arithmetic routines of the render kernel (rt_device.h) that need nothing of the GPU: the vector type,
// the normalizes, the scene queries' division and square root, the counter hashes and the colour clip.  Every bit of them
// reaches the frames, and each shortcut is justified by a CPU check over 10^7 to 10^8 operands, so the kernel and the checks
// (tests/algo/normalize_check.cpp, renorm_check.cpp, divsqrt_check.cpp, plane_sign_check.cpp, hash_check.cpp) compile this same
// text.  HIP-free C++17: no HIP type or builtin.  What the hardware supplies — the v_rsq_f64 / v_rcp_f64 seed of an iteration —
// is an argument: rt_device.h's wrappers pass the instruction's result, the checks a stand-in that is 2^-24 off, which bounds the
// instructions' own error with little to spare (measured on an MI355X over the operands of tests/device_math_cases.py: v_rcp_f64 at
// most 2^-24.39 off, v_rsq_f64 2^-24.18; profiles/device_math_seeds.json;
// tests/test_gpu_device_math.py asserts the bound and runs the wrappers on the device against IEEE).  The
// wave-uniform guards (a ballot) stay with the wrappers; their constants are named here.
// No multiply-add may be fused and none split: clang is told below, other compilers need -ffp-contract=off.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define RT_MATH_FN __host__ __device__ __forceinline__
#else
#define RT_MATH_FN static inline
#endif

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace rt {

struct V3 { double x, y, z; };
struct F3 { float x, y, z; };

RT_MATH_FN double dot3(const V3 &a, const V3 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }   // common.py:35-37

// common.py:28-32 — sqrt and three true divisions, as the compiler lowers them (correctly rounded).
RT_MATH_FN V3 normalize3_generic(const V3 &v)
{
    double n = __builtin_sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
    return V3{v.x / n, v.y / n, v.z / n};
}

// The same normalize with the work the three divisions have in common done once.  The AMDGPU backend lowers
//   sqrt(x):  y = rsq(x); g = x*y; h = y/2; r = fma(-h,g,1/2); g = fma(g,r,g); h = fma(h,r,h);
//             twice { d = fma(-g,g,x); g = fma(d,h,g); }                      (+ range scaling of x)
//   a / b:    r = rcp(b); twice { e = fma(-b,r,1); r = fma(r,e,r); }  q = a*r; res = fma(fma(-b,q,a), r, q)
//                                                                             (+ div_scale / div_fixup)
// both correctly rounded.  For operands well inside the exponent range the scaling steps are identities, so
// the sequences below return bit-identical results while the reciprocal (5 of a division's 11 instructions) is
// shared by x/n, y/n, z/n and the sqrt skips its range handling.  The reciprocal itself needs no v_rcp_f64
// (a quarter-rate instruction): the sqrt iteration's h already approximates 1/(2g) to ~2^-50, so one Newton
// step from 2h lands where the backend's two steps from the rcp seed land — within half an ulp (+2^-47) of
// 1/g, which is what the final fma correction of each quotient requires.  26 instructions instead of 55.  Guard (wave-uniform): every component's magnitude >= 2^-200 (hence nonzero, and |v|² >= 2^-400) and
// |v|² <= 2^400, so no intermediate leaves the normal range and no signed-zero case arises; otherwise the
// generic path.  tests/test_algorithms.py runs this on the CPU against sqrt()/division on 10^8 vectors
// with seeds 2^-24 off (the bound of v_rsq_f64 / v_rcp_f64 measured above), and once more with seeds 2^-16 off: only from there does a
// sample show whether the reciprocal's Newton step is present (tests/algo/normalize_check.cpp has the arithmetic).
constexpr double NORMALIZE_MIN_COMPONENT = 0x1p-200, NORMALIZE_MAX_NN = 0x1p400;   // the guard (rt_device.h: normalize3)
// The square root's iteration on its own: g = RN(sqrt(x)) and h ~ 1/(2g) (relative error ~2^-50), from y = rsq(x).
struct SqrtIter { double g, h; };
RT_MATH_FN SqrtIter sqrt_iter(double x, double y)
{
    double g = x * y, h = 0.5 * y;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g); h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x); g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x); g = __builtin_fma(d, h, g);
    return SqrtIter{g, h};
}
// nn = |v|² as normalize3 forms it, y = rsq(nn).
RT_MATH_FN V3 normalize3_seeded(const V3 &v, double nn, double y)
{
    const SqrtIter s = sqrt_iter(nn, y);
    const double g = s.g;
    double rc = 2.0 * s.h;
    const double e = __builtin_fma(-g, rc, 1.0); rc = __builtin_fma(rc, e, rc);   // within 1/2 ulp(1 + 2^-47) of 1/g
    const double qx = v.x * rc, qy = v.y * rc, qz = v.z * rc;
    return V3{__builtin_fma(__builtin_fma(-g, qx, v.x), rc, qx),
              __builtin_fma(__builtin_fma(-g, qy, v.y), rc, qy),
              __builtin_fma(__builtin_fma(-g, qz, v.z), rc, qz)};
}

// The scene queries' own division and square root (t = num/den of a plane, t = n/a of the closest sphere, sqrt of a sphere's
// discriminant), as the backend lowers them minus the range handling (see normalize3 above): v_div_scale x2 / v_div_fixup
// and the sqrt's ldexp scaling are identities for operands well inside the exponent range, and there they are: scene values
// are float32 (magnitudes 2^-149 .. 2^128 or zero), a plane's denominator is at least 0.001 in magnitude where the quotient is
// formed (intersections.py:55), a is within rounding of 1, numerators and discriminants are sums of a few products of such
// values (zero, or above 2^-600), while the backend scales below 2^-767 (sqrt) / numerators below 2^-969, denominators of
// extreme exponent, exponent differences beyond 2^768 (division).  Outside that range (a camera at 1e300, infinities) both
// forms end in an infinity, a NaN or a value whose comparison with (0, 999) has the same outcome: no hit.  3 of 11
// instructions per division, 7 of 21 per square root.  tests/algo/divsqrt_check.cpp runs both on the CPU, with seeds 2^-24 off
// and with seeds 2^-16 off (where a sample can tell two Newton steps from one).
RT_MATH_FN double div_seeded(double a, double b, double r)     // r = rcp(b)
{
    double e = __builtin_fma(-b, r, 1.0); r = __builtin_fma(r, e, r);
    e = __builtin_fma(-b, r, 1.0); r = __builtin_fma(r, e, r);
    const double q = a * r;
    // q has the quotient's sign (r has b's), a zero q included; the correction's sum of zeros has not: fma(-b, q, a) is +0 for either
    // zero numerator, and -0 / b with b > 0 came out +0.  One v_bfi_b32 puts q's sign on the result (it has it already wherever the
    // result is not zero), so a zero quotient is IEEE's as well (tests/test_gpu_device_math.py compares signed zeros on the device).
    return __builtin_copysign(__builtin_fma(__builtin_fma(-b, q, a), r, q), q);
}
RT_MATH_FN double sqrt_seeded(double x, double y)              // x >= 0 (or NaN), y = rsq(x)
{
    const double g = sqrt_iter(x, y).g;
    return x > 0.0 ? g : x;                                   // sqrt(+0) = +0 (the iteration yields NaN there: 0 * inf)
}

// ---------------------------------------------------------------------------------------------
// normalize() of a vector that is ALREADY unit length (every direction a scene query receives is
// the output of a normalize) — bit-identical to normalize3(), without the generic sqrt and divides.
//
//   nn = fl(x²+y²+z²) lies within a few ulp of 1; e = nn - 1 is exact.  With eps = 2^-52:
//     e = k·eps    (k >= 0):  sqrt = 1 + e/2 - e²/8 ..  ->  RN = 1 + floor(k/2)·eps
//     e = -j·eps/2 (j >= 1):  sqrt = 1 + e/2 - e²/8 ..  ->  RN = 1 - ceil(j/2)·eps/2
//   i.e. RN(sqrt(nn)) is 1 + e/2 rounded to nearest with every tie (odd k, odd j) resolved downward, because
//   the second-order term is negative.  One fma rounds exactly once, so nudging e toward -inf by a relative
//   2^-30 first (e2 = e - |e|·2^-30, far below half a grid step, far above e²/8) makes
//   nrm = fma(e2, 1/2, 1) that value: the nudge decides the ties and moves nothing else.
//   y = RN(1/nrm) likewise: with dl = nrm - 1 (exact), 1/nrm = 1 - dl + dl² .., ties (dl = -i·eps/2, i odd)
//   resolved upward: y = fma(-dl, 1 + 2^-30, 1).
//   Each quotient x/nrm is then  q1 = fma(-x, dl, x)  (faithful: off by |x|·dl² at most),
//   r = fma(-q1, nrm, x) (the exact remainder),  q = fma(r, y, q1)  — Markstein's final correction,
//   which returns the correctly rounded quotient RN(x/nrm) given y = RN(1/nrm) and a faithful q1.
// The caller falls back to the generic path (wave-uniformly) if any live lane's nn is not within 2^-33 of 1.
// tests/test_algorithms.py runs this routine on the CPU: nrm and y against sqrt and division for EVERY double
// within 2^-33 of 1 (1.57 million), the whole routine against sqrt-and-divide on 10^7 vectors.
// (The same values used to be derived from the IEEE bit pattern with 64-bit integer arithmetic: ~25 more
// instructions per call, 13 calls per tile — one in seven of all the kernel's VALU instructions.)
// ---------------------------------------------------------------------------------------------
constexpr double UNIT_WINDOW = 0x1p-33;                             // the guard (rt_device.h: renormalize_unit): |e| < this
struct UnitNorm { double nrm, dl, y; };                             // RN(sqrt(nn)), nrm - 1, RN(1/nrm)
RT_MATH_FN UnitNorm unit_norm(double e)                             // e = nn - 1 (exact), |e| < UNIT_WINDOW
{
    const double e2 = __builtin_fma(-__builtin_fabs(e), 0x1p-30, e);
    const double nrm = __builtin_fma(e2, 0.5, 1.0);                // RN(sqrt(nn))
    const double dl = nrm - 1.0;                                   // exact
    return UnitNorm{nrm, dl, __builtin_fma(-dl, 1.0 + 0x1p-30, 1.0)};   // RN(1/nrm)
}
RT_MATH_FN V3 renormalize_unit_fast(const V3 &d, double e)
{
    const UnitNorm u = unit_norm(e);
    V3 q{__builtin_fma(-d.x, u.dl, d.x), __builtin_fma(-d.y, u.dl, d.y), __builtin_fma(-d.z, u.dl, d.z)};
    const V3 r{__builtin_fma(-q.x, u.nrm, d.x), __builtin_fma(-q.y, u.nrm, d.y), __builtin_fma(-q.z, u.nrm, d.z)};
    q = V3{__builtin_fma(r.x, u.y, q.x), __builtin_fma(r.y, u.y, q.y), __builtin_fma(r.z, u.y, q.z)};
    return q;
}

// The counter hashes (no state, any launch tiling gives the same frame).  One hash, jitter_hash(x, y, t, seed), in two parts:
// hash_xy is its first two rounds, on the seed and the pixel, scatter_hash the last two, on the counter t.
// tests/algo/hash_check.cpp runs the keys below against the one-part form and jitter_hash against the oracle's.
RT_MATH_FN unsigned hash_xy(unsigned seed, unsigned x, unsigned y)
{
    unsigned h = seed ^ 0x9E3779B9u;
    h = (h ^ x) * 0x85EBCA6Bu; h ^= h >> 13;
    h = (h ^ y) * 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
RT_MATH_FN unsigned scatter_hash(unsigned key, unsigned t)
{
    unsigned h = (key ^ t) * 0x27D4EB2Fu; h ^= h >> 15;
    h *= 0x165667B1u; h ^= h >> 13;
    return h;
}

// Sub-pixel jitter of sample s of pixel (x,y) for the stochastic mode.  u = ((h & 0xFFFF) + 1/2)/65536 - 1/2, v likewise from
// the high half: exact.
RT_MATH_FN unsigned jitter_hash(unsigned x, unsigned y, unsigned s, unsigned seed) { return scatter_hash(hash_xy(seed, x, y), s); }

// The scatter hash (rt_set_scene_materials_scatter, mi355rt.h): jitter_hash(X, Y, ((s*16 + b)*8 + j)*4 + c, seed ^ 0x5CA77E12)
// in two parts.  scatter_key is its first two rounds, on (X, Y), with s folded in: for b <= 15 the third argument is the bit
// pattern s << 9 | b << 5 | j << 2 | c, so XOR-ing s << 9 into the state before the third round is the same as XOR-ing it in
// there.  scatter_hash finishes it for the low nine bits t = b << 5 | j << 2 | c.
RT_MATH_FN unsigned scatter_key(unsigned x, unsigned y, unsigned s, unsigned seed) { return hash_xy(seed ^ 0x5CA77E12u, x, y) ^ (s << 9); }

// The area-light hash (rt_set_scene_area_lights, mi355rt.h): jitter_hash(X, Y, t, seed ^ 0x50F7117E) with
// t = ((((s*32 + b)*64 + m)*16 + i)*8 + j)*4 + c, the bit pattern s << 20 | b << 15 | m << 9 | i << 5 | j << 2 | c (s < 64,
// b <= 16, m < 64, i < 16).  soft_key is its first two rounds on (X, Y) with s folded in (as scatter_key); scatter_hash
// finishes it for t without s.
RT_MATH_FN unsigned soft_key(unsigned x, unsigned y, unsigned s, unsigned seed) { return hash_xy(seed ^ 0x50F7117Eu, x, y) ^ (s << 20); }

// The lens hash (rt_set_lens, mi355rt.h): jitter_hash(X, Y, (s*8 + j)*2 + c, seed ^ 0x1E45D0F5), the bit pattern s << 4 | j << 1 | c.
// lens_key is its first two rounds on (X, Y) with s folded in (as scatter_key); scatter_hash finishes it for t = j << 1 | c.
RT_MATH_FN unsigned lens_key(unsigned x, unsigned y, unsigned s, unsigned seed) { return hash_xy(seed ^ 0x1E45D0F5u, x, y) ^ (s << 4); }

// Component t of a hashed candidate in the unit ball or disk: (h >> 8) 2^-23 + 2^-24 - 1, in (-1, 1), exact.
RT_MATH_FN double hash_unit(unsigned key, unsigned t) { return (double)(scatter_hash(key, t) >> 8) * 0x1p-23 + (0x1p-24 - 1.0); }

// common.py:52-57: min(max(0, int(round(c))), 255), round half to even (v_rndne_f64).
// Straight-line: round, clamp to [0, 255] as a double, convert; four instructions a channel.  The same byte for every double as the
// rule spelled out with its tests (NaN -> 0, c <= -0.5 -> 0, c >= 255.5 -> 255, else rint(c) clamped to 0..255): that rule clamps
// the rounded value as an int, this clamps it before the conversion, which then sees an integer of 0..255 whatever c was, a NaN
// included (clamp_lo sends it to 0).  c in (-0.5, 0) rounds to -0: either zero converts to 0.
// clamp_lo(c, k) is c > k ? c : k, so a NaN goes to k; clamp_hi(c, k) the same with <.  On the device they are fmax and fmin
// (v_max_f64 / v_min_f64, one instruction each: rint's result is never a signalling NaN, so the backend adds no canonicalize, as
// it does when it clamps first).  A host's libm may hand a signalling NaN through rint and fmax, and the conversion to int must
// never see one, so the host spells the selects out.
// tests/algo/fixed_path_check.cpp compares the host's text with the rule on the specials, every tie and 10^7 bit patterns;
// tests/test_gpu_fixed_path.py puts a frame's values on the ties and bounds on the device.
RT_MATH_FN double clamp_lo(double c, double k)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_fmax(c, k);
#else
    return c > k ? c : k;
#endif
}
RT_MATH_FN double clamp_hi(double c, double k)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_fmin(c, k);
#else
    return c < k ? c : k;
#endif
}
// The rule as written, with its branches: what every kernel but the trimmed ones (rt_device.h: RT_TRIM_STORE) keeps compiling.
RT_MATH_FN uint8_t clip_color_branches(double c)
{
    if (!(c == c)) return 0;
    if (c <= -0.5) return 0;
    if (c >= 255.5) return 255;
    const int i = (int)__builtin_rint(c);
    return (uint8_t)(i < 0 ? 0 : (i > 255 ? 255 : i));
}
RT_MATH_FN uint8_t clip_color(double c)
{
    return (uint8_t)(int)clamp_hi(clamp_lo(__builtin_rint(c), 0.0), 255.0);
}

}  // namespace rt
