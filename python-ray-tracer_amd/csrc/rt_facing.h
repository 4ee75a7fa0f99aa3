/*
 * rt_facing.h — the facing certificate of the point-light loop (rt_device.h, trace_bounce): a per-lane test that proves,
 * before the light's direction is normalised, that the Lambert term k = lamb * dot3(normalize3(v), N) of v = light - Pt will
 * not be positive, and the host-side formula of its margin.  A wave in which every live lane holds the certificate goes to
 * the next light without forming normalize3(v).  No HIP: the kernel includes it, and tests/algo/facing_check.c evaluates the
 * same expression on the CPU against sqrt and division.  Valid C99 and C++.
 *
 * The predicate.  With v = (vx, vy, vz) the three differences normalize3 consumes and N the shading normal,
 *     u = fma(vz, nz, fma(vy, ny, vx * nx))              (float64, this order, three roundings)
 * and the lane is certified when  u < -tau.
 *
 * The theorem.  Let reach >= |v| / (1 + 2^-10) and tau = rt_facing_tau(reach, lamb).  If the lane is certified and !(lamb < 0),
 * then the kernel's own  lamb * dot3(normalize3(v), N) > 0.0  is false, and so is  dot3(normalize3(v), N) > 0.0.
 *
 * Proof.  eps = 2^-53.  Three facts about the operands:
 *   (a) normalize3(v) returns q_i = RN(v_i / g), all three by the same g = RN(sqrt(RN(v.v))) (rt_device.h: the fast path is
 *       bit-identical to sqrt and three divisions).  The proof uses nothing of g but g > 0 or g = +inf: a certified lane has
 *       |v| |N| >= |u| / (1 + 3 eps) > tau / 2 >= 2^-48 reach, hence |v| > 2^-50 reach, far from where v.v underflows to 0.
 *   (b) dot3 is RN(RN(RN(q_x N_x) + RN(q_y N_y)) + RN(q_z N_z)).
 *   (c) |N| <= 2 for every finite normal.  A sphere's is a normalize3 output (|N| <= 1 + 2^-51).  A plane's is
 *       rt_scene.h's plane_normal_f32: n_i / RN32(sqrt(s)), s the float32 sum of the float32 squares.  Where s is a normal
 *       float32, |N|^2 is within a few 2^-24 of 1.  Where s is subnormal, s is at least 2^-149 and the true sum is below
 *       2.5 * 2^-149 (two squares that round to 0 and one that rounds to 2^-149), so |N|^2 < 2.5.  Where s rounds to 0 or
 *       overflows, the components are inf, NaN or 0: see the special values below.
 * Finite case, g finite.  Each q_i = (v_i / g)(1 + d), |d| <= eps, or q_i is subnormal with an absolute error below 2^-1075;
 * each product and each sum adds a factor (1 + d) (sums of subnormals are exact, a subnormal product errs by 2^-1075 at most).
 * So the computed dot is  (v.N + E) / g  with  |E| <= ((1 + eps)^4 - 1) sum |v_i N_i| + 6 * 2^-1075 * g  <=  4.01 eps |v| |N| +
 * 2^-1072 reach.  Likewise u = v.N + E',  |E'| <= 3.01 eps |v| |N| + 2^-1073.  A certified lane therefore has
 *     v.N + E  <  -tau + |E| + |E'|  <=  -tau + 7.02 eps * 1.001 reach * 2 + 2^-1071 reach  <  -tau + 15 eps reach  <  0
 * since tau = 2^-47 reach = 64 eps reach.  g > 0, so the computed dot is negative or -0, and with lamb >= +0 the product k is
 * negative, -0 or (lamb = inf, dot = -0) NaN: not > 0.
 * g = +inf (v.v overflows, v finite): every q_i is +-0, the dot is +-0 or NaN, k likewise.  Certified or not, k > 0 is false.
 * g = 0 (v.v underflows to 0: only with a reach below 2^-480, which no launch has, since reach >= 999): q_i is v_i's sign times
 * inf, or NaN where v_i = 0; a dot > 0 would need every term +inf, hence every v_i N_i > 0 and u > 0: not certified.
 *
 * Special values, none with a case of its own:
 *   - a NaN in v or N makes u NaN: u < -tau is false, nothing is certified.
 *   - an infinite component of v: reach is then inf and tau = inf, nothing is certified (and q is NaN: k > 0 is false anyway).
 *   - an infinite component of N (a plane whose raw normal underflows in float32): u = -inf certifies, and only where k > 0 is
 *     false anyway: u = -inf needs a term v_i N_i = -inf and none that is +inf or NaN; q_i has the sign of v_i or is 0, so the
 *     dot's term i is -inf or NaN, no other is +inf, and the dot is -inf or NaN.
 *   - v overflowing in v.v or in u (components near 1e300): covered by g = +inf above; u = -inf or a huge negative u certifies
 *     only where k > 0 is false anyway.
 *   - lamb < 0: k > 0 happens exactly where the dot is negative.  rt_facing_tau returns +inf for it (wave-uniform lamb), and
 *     rt_facing_certified_lamb refuses it per lane: certifies nothing.
 *   - lamb = +-0: k is +-0 or NaN, never > 0; lamb = NaN: k is NaN.  Both may certify, only where k > 0 is false anyway.
 *     (-0.0 < 0 is false: -0 counts as zero, and lamb * negative = +0 is not > 0.)
 *   - lamb = +inf: certified lanes have a dot that is negative, -0 or NaN: k is -inf or NaN.
 *   - reach NaN or inf (a camera at infinity): tau is NaN or inf, nothing is certified.
 *
 * The LIT loop's condition  k > 0 || (spec > 0 && dot > 0)  is false under the same certificate, since the theorem also gives
 * dot > 0 false.
 */
#ifndef RT_FACING_H
#define RT_FACING_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_FACING_FN __host__ __device__ static inline
#else
#define RT_FACING_FN static inline
#endif

/* The launch constant tau.  reach bounds |light - Pt| for every hit of the launch: |cam| (+ aperture) + 999 (depth + 1) + the
 * scene's extent, the sum the host forms for floor_anch (each segment of a path is shorter than 999; the 0.0002 biases and the
 * strictness of t < 999 stay inside the factor 1 + 2^-10 the theorem allows).  lamb is the launch's Lambert coefficient where
 * it is wave-uniform (PLAIN), 0.0 where it is per lane (rt_facing_certified_lamb then looks at the lane's own). */
RT_FACING_FN double rt_facing_tau(double reach, double lamb)
{
    return lamb < 0.0 ? __builtin_inf() : 0x1p-47 * reach;
}

RT_FACING_FN double rt_facing_u(double vx, double vy, double vz, double nx, double ny, double nz)
{
    return __builtin_fma(vz, nz, __builtin_fma(vy, ny, vx * nx));
}

/* 1 if the lane is certified: three multiply-adds and one compare. */
RT_FACING_FN int rt_facing_certified(double vx, double vy, double vz, double nx, double ny, double nz, double tau)
{
    return rt_facing_u(vx, vy, vz, nx, ny, nz) < -tau;
}

/* The same with a Lambert coefficient of the lane's own (material tables): a negative one certifies nothing. */
RT_FACING_FN int rt_facing_certified_lamb(double vx, double vy, double vz, double nx, double ny, double nz, double tau, double lamb)
{
    return rt_facing_certified(vx, vy, vz, nx, ny, nz, tau) && !(lamb < 0.0);
}

#endif
