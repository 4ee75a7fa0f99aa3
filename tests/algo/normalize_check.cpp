/* rt_math.h's normalize3_seeded() (rt_device.h: normalize3's fast path) against sqrt() and three divisions: sqrt by one rsq seed
 * + Goldschmidt/Newton steps (the sequence the AMDGPU backend emits for f64 sqrt, without its range scaling), the reciprocal of
 * the norm taken from that iteration's own 1/(2g) estimate plus one Newton step and shared by the three quotients, one fma
 * correction per quotient (the backend's f64 division without div_scale/div_fixup).  The routine is the header's, the text the
 * kernel compiles; only the seed is this program's.
 * Seeds carry a relative error of up to 2^-24 here: no better than v_rsq_f64 / v_rcp_f64, whose measured maxima on an MI355X are
 * 2^-24.18 (rsq) and 2^-24.39 (rcp) (profiles/device_math_seeds.json; tests/test_gpu_device_math.py asserts <= 2^-24), so agreement
 * with the correctly rounded / and sqrt() on every sample covers the hardware's seeds; the pass at 2^-16 below shows the margin.  One sample in four sits at the edges of the guard
 * (components down to 2^-200, |v|^2 up to 2^400).
 * A second pass on a quarter as many vectors (the stream goes on) has seeds 2^-16 off.  At 2^-24 the iteration's 2h is already
 * within 2^-47 of 1/g and a quotient formed without the Newton step is 2^-94 off: no sample count sees that.  From 2^-16, h is
 * 2^-31 off: with the step the reciprocal still ends at rounding level, without it a quotient is 2^-62 off, wrong once in about
 * 2^9 components.  Built and run by tests/test_algorithms.py. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../python-ray-tracer_amd/csrc/rt_math.h"

static uint64_t s[2] = {0x9E3779B97F4A7C15ull, 0xD1B54A32D192ED03ull};
static inline uint64_t rnd(void) { uint64_t a = s[0], b = s[1]; s[0] = b; a ^= a << 23; s[1] = a ^ b ^ (a >> 17) ^ (b >> 26); return s[1] + b; }
static inline double urand(void) { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }

static void normalize_ref(const double v[3], double out[3])
{
    double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    out[0] = v[0] / n; out[1] = v[1] / n; out[2] = v[2] / n;
}

static double seed_err = 0x1p-24;
static void normalize_fast(const double v[3], double out[3], double *norm)
{
    const double nn = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    const double y = (1.0 / sqrt(nn)) * (1.0 + (urand() * 2 - 1) * seed_err);   /* stand-in for v_rsq_f64 */
    *norm = rt::sqrt_iter(nn, y).g;                        /* the iteration normalize3_seeded takes its norm from */
    const rt::V3 q = rt::normalize3_seeded(rt::V3{v[0], v[1], v[2]}, nn, y);
    out[0] = q.x; out[1] = q.y; out[2] = q.z;
}

/* n vectors with seeds up to seed_err off */
static void pass(long n, long *badsqrt_out, long *bad_out)
{
    long bad = 0, badsqrt = 0;
    for (long it = 0; it < n; ++it) {
        double v[3], a[3], b[3], nr;
        int mode = it & 7;
        double sc = mode == 0 ? 1.0 : exp((urand() - 0.5) * (mode == 1 ? 8 : 60));   /* magnitudes 1e-13 .. 1e13 */
        if (mode == 4) sc = ldexp(1.0, 190 + (int)(rnd() % 9));                      /* |v|^2 just below 2^400 */
        if (mode == 5) sc = ldexp(1.0, -(185 + (int)(rnd() % 14)));                  /* components around 2^-200 */
        for (int c = 0; c < 3; ++c) v[c] = (urand() * 2 - 1) * sc;
        if (mode == 3) v[(int)(rnd() % 3)] *= exp(-urand() * 60);                    /* one component much smaller */
        if (mode == 6) v[(int)(rnd() % 3)] = ldexp(0.5 + urand() * 0.5, -199);        /* one component at the guard, others O(1) */
        {   /* the guard of rt_device.h (rt_math.h names its constants): outside it the kernel takes the generic path */
            const double cmin = fmin(fmin(fabs(v[0]), fabs(v[1])), fabs(v[2]));
            if (!(cmin >= rt::NORMALIZE_MIN_COMPONENT && v[0] * v[0] + v[1] * v[1] + v[2] * v[2] <= rt::NORMALIZE_MAX_NN)) continue;
        }
        normalize_ref(v, a);
        normalize_fast(v, b, &nr);
        if (nr != sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])) badsqrt++;
        if (memcmp(a, b, sizeof a) != 0) {
            if (bad++ < 5) fprintf(stderr, "MISMATCH v=(%a,%a,%a) ref=(%a,%a,%a) got=(%a,%a,%a)\n", v[0], v[1], v[2], a[0], a[1], a[2], b[0], b[1], b[2]);
        }
    }
    *badsqrt_out = badsqrt; *bad_out = bad;
}

int main(int argc, char **argv)
{
    long n = argc > 1 ? atol(argv[1]) : 10000000, bad, badsqrt, cbad, csqrt;
    if (argc > 2) { s[0] ^= (uint64_t)atoll(argv[2]) * 0x9E3779B97F4A7C15ull; s[1] += (uint64_t)atoll(argv[2]); }
    pass(n, &badsqrt, &bad);
    printf("checked=%ld sqrt_mismatches=%ld mismatches=%ld\n", n, badsqrt, bad);
    seed_err = 0x1p-16;
    pass(n / 4, &csqrt, &cbad);
    printf("coarse_seeds=%ld sqrt_wrong=%ld wrong=%ld\n", n / 4, csqrt, cbad);
    return (bad || badsqrt || cbad || csqrt) ? 1 : 0;
}
