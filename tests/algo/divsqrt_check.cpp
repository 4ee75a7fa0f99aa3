/* rt_math.h's div_seeded() and sqrt_seeded() (rt_device.h: div_inrange, sqrt_inrange), the text the kernel compiles, against the
 * correctly rounded / and sqrt(): the AMDGPU backend's f64 division and square root without their range handling (v_div_scale /
 * v_div_fixup, ldexp scaling), which are identities inside the exponent range the scene queries work in.  The sequences are
 * written out above rt_math.h's normalize3_seeded; only the seeds are this program's.
 * Seeds carry a relative error of up to 2^-24 here: no better than v_rcp_f64 / v_rsq_f64, whose measured maxima on an MI355X are
 * 2^-24.18 (rsq) and 2^-24.39 (rcp) (profiles/device_math_seeds.json; tests/test_gpu_device_math.py asserts <= 2^-24), so agreement
 * with the correctly rounded / and sqrt() on every sample covers the hardware's seeds; the pass at 2^-16 below shows the margin.
 * Operand ranges: denominators 1e-3 .. 1e40 and
 * within an ulp of 1 (t = n/a), numerators 0 and 1e-130 .. 1e80, radicands 0 and 1e-130 .. 1e80 — wider than what
 * float32 scenes produce (see rt_device.h).
 * A second pass on a quarter as many operands (the stream goes on) has seeds 2^-16 off.  At 2^-24 a Newton step too few leaves the
 * reciprocal 2^-48 off and the corrected quotient 2^-96: no sample count sees that.  From 2^-16 the sequence as written still ends
 * at rounding level (2^-64 after two steps), while one step fewer leaves 2^-32 and a quotient 2^-64 off, wrong once in about 2^11
 * operands.  Built and run by tests/test_algorithms.py. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../python-ray-tracer_amd/csrc/rt_math.h"

static uint64_t s[2] = {0x9E3779B97F4A7C15ull, 0xD1B54A32D192ED03ull};
static inline uint64_t rnd(void) { uint64_t a = s[0], b = s[1]; s[0] = b; a ^= a << 23; s[1] = a ^ b ^ (a >> 17) ^ (b >> 26); return s[1] + b; }
static inline double urand(void) { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }
static double seed_err = 0x1p-24;
static inline double noise(void) { return 1.0 + (urand() * 2 - 1) * seed_err; }

static double div_inrange(double a, double b) { return rt::div_seeded(a, b, (1.0 / b) * noise()); }   /* stand-in for v_rcp_f64 */
static double sqrt_inrange(double x) { return rt::sqrt_seeded(x, (x > 0.0 ? 1.0 / sqrt(x) : INFINITY) * noise()); }   /* for v_rsq_f64 */

static double magnitude(int wide) { return exp((urand() - 0.5) * (wide ? 480.0 : 40.0)); }   /* 1e-104..1e104 / 2e-9..5e8 */

/* n operand pairs and radicands with seeds up to seed_err off */
static void pass(long n, long *baddiv_out, long *badsqrt_out)
{
    long baddiv = 0, badsqrt = 0;
    for (long it = 0; it < n; ++it) {
        const int mode = it & 7;
        double a = (urand() * 2 - 1) * magnitude(mode & 1), b;
        if (mode < 3) b = 1.0 + ((double)(rnd() % 33) - 16.0) * 0x1p-52;            /* t = n / a: a = R.R of a unit vector */
        else {
            b = (urand() < 0.5 ? -1.0 : 1.0) * (0.001 + urand()) * (mode == 7 ? exp(urand() * 92.0) : exp(urand() * 8.0));   /* |den| >= 0.001, up to 1e40 */
        }
        if (mode == 6) a = (it & 8) ? -0.0 : 0.0;                                     /* either zero: the quotient's sign is compared */
        if (fabs(a) < 1e-130 && a != 0.0) a = 1e-130;
        if (fabs(a) > 1e80) a = copysign(1e80, a);
        const double want = a / b, got = div_inrange(a, b);
        if (want != got || signbit(want) != signbit(got)) { if (baddiv++ < 5) fprintf(stderr, "DIV a=%a b=%a want=%a got=%a\n", a, b, want, got); }
        double x = mode == 6 ? 0.0 : fabs(a) * magnitude(0);
        if (x != 0.0 && x < 1e-130) x = 1e-130;
        if (x > 1e80) x = 1e80;
        if (mode == 5) { const double q = floor(urand() * 1e6) + 1.0; x = q * q; }   /* perfect squares */
        const double ws = sqrt(x), gs = sqrt_inrange(x);
        if (ws != gs) { if (badsqrt++ < 5) fprintf(stderr, "SQRT x=%a want=%a got=%a\n", x, ws, gs); }
    }
    *baddiv_out = baddiv; *badsqrt_out = badsqrt;
}

int main(int argc, char **argv)
{
    long n = argc > 1 ? atol(argv[1]) : 10000000, baddiv, badsqrt, cdiv, csqrt;
    if (argc > 2) { s[0] ^= (uint64_t)atoll(argv[2]) * 0x9E3779B97F4A7C15ull; s[1] += (uint64_t)atoll(argv[2]); }
    pass(n, &baddiv, &badsqrt);
    printf("checked=%ld div_mismatches=%ld sqrt_mismatches=%ld\n", n, baddiv, badsqrt);
    seed_err = 0x1p-16;
    pass(n / 4, &cdiv, &csqrt);
    printf("coarse_seeds=%ld div_wrong=%ld sqrt_wrong=%ld\n", n / 4, cdiv, csqrt);
    return (baddiv || badsqrt || cdiv || csqrt) ? 1 : 0;
}
