/* rt_facing.h under UndefinedBehaviorSanitizer: every function of the header on a lattice of combinations of special values (zeros,
 * denormals, huge values, infinities, NaN) for each argument, and the properties that need no reference: a NaN in v, N or tau
 * certifies nothing, an infinite tau certifies nothing, a negative lamb gives an infinite tau and no per-lane certificate, and
 * a larger tau never certifies more.  Built with -fsanitize=undefined and run by tests/test_facing_skip.py. */
#include <math.h>
#include <stdio.h>

#include "../../python-ray-tracer_amd/csrc/rt_facing.h"

int main(void)
{
    const double sp[] = {0.0, -0.0, 0x1p-1074, -0x1p-1074, 0x1p-1022, 1e-30, -0.3, 1.0, -1.0, 9191.0, 1e300, -1e300,
                         0x1.fffffffffffffp1023, INFINITY, -INFINITY, NAN};
    const double reach[] = {0.0, 999.0, 9191.0, 1e300, INFINITY, NAN};
    const double lamb[] = {-0.6, -0.0, 0.0, 0.6, NAN, INFINITY};
    const int n = sizeof sp / sizeof *sp, nr = sizeof reach / sizeof *reach, nl = sizeof lamb / sizeof *lamb;
    long calls = 0, bad = 0;
    for (int r = 0; r < nr; ++r) for (int l = 0; l < nl; ++l) {
        const double tau = rt_facing_tau(reach[r], lamb[l]), tau0 = rt_facing_tau(reach[r], 0.0);
        if (lamb[l] < 0.0 && !(isinf(tau) && tau > 0)) ++bad;
        for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) for (int c = (a + b) % 3; c < n; c += 3)
            for (int d = (a + c) % 3; d < n; d += 3) for (int e = b % 3; e < n; e += 3) for (int f = (a + d) % 2; f < n; f += 2) {
                const double u = rt_facing_u(sp[a], sp[b], sp[c], sp[d], sp[e], sp[f]);
                const int c0 = rt_facing_certified(sp[a], sp[b], sp[c], sp[d], sp[e], sp[f], tau);
                const int c1 = rt_facing_certified_lamb(sp[a], sp[b], sp[c], sp[d], sp[e], sp[f], tau0, lamb[l]);
                const int c2 = rt_facing_certified(sp[a], sp[b], sp[c], sp[d], sp[e], sp[f], 2.0 * tau + 1.0);
                calls += 4;
                const int any_nan = sp[a] != sp[a] || sp[b] != sp[b] || sp[c] != sp[c] || sp[d] != sp[d] || sp[e] != sp[e] || sp[f] != sp[f];
                if ((c0 | c1 | c2) & ~1) ++bad;
                if ((any_nan || u != u) && (c0 || c1 || c2)) ++bad;
                if ((tau != tau || (isinf(tau) && tau > 0)) && c0) ++bad;
                if (lamb[l] < 0.0 && (c0 || c1)) ++bad;
                if (c2 && !c0 && tau >= 0.0) ++bad;
            }
    }
    printf("calls=%ld violations=%ld\n", calls, bad);
    return bad ? 1 : 0;
}
