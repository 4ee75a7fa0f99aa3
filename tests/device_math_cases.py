"""Operands, plain references and property checkers for the device harness of the kernels' exact-arithmetic primitives
(tests/algo/device_math_kat.hip).  numpy only, seeded.  tests/test_device_math_cases.py checks this module on the CPU (every class
is populated as named, the references agree with rt_math.h's text run on the host, the checkers reject planted faults);
tests/test_gpu_device_math.py runs the operands through the device.

The references are numpy float64 operations, which are IEEE correctly rounded: a / b, np.sqrt(x), and v / np.sqrt(x*x + y*y + z*z)
with every multiplication, addition, square root and division rounded on its own.  Results are compared as bit patterns: signed
zeros count, a NaN matches any NaN.

The in-range set, on which div_inrange / sqrt_inrange claim bit equality, is read off the comment above rt_math.h's div_seeded:
    scene values are float32 (magnitudes 2^-149 .. 2^128 or zero);
    a denominator is a plane's den with 0.001 <= |den| (< 2^130: a dot product of a unit direction and a float32 normal), or the
      a = R.R of a unit vector, 1 + k 2^-52 with |k| <= 16;
    numerators and discriminants are sums of a few products of such values: zero (either sign for a numerator), or of magnitude
      2^-600 .. 2^300 (a NaN discriminant passes through).
Everything else is the out-of-range class (cameras at 1e300, denormal and huge numerators and radicands, exponent differences beyond
2^768, infinities, NaN and zero denominators), on which the comment claims only that the comparisons the kernel makes of the result
come out as with the correctly rounded value: `999 > t && t > 0` of a quotient (closest_hit's sphere and plane tests), and for a
square root q the same of the t that sphere_closest forms from it, n = -s - q, or -s + q where that is not positive.  Denormal
denominators are left out of it: the kernel divides by a (within rounding of 1, or 0 / NaN for a degenerate direction) and by a den
it has compared with 0.001, never by a denormal."""
import numpy as np

F64 = np.float64
NORMALIZE_MIN_COMPONENT = 2.0 ** -200      # rt_math.h
NORMALIZE_MAX_NN = 2.0 ** 400
UNIT_WINDOW = 2.0 ** -33
SENTINEL = np.uint64(0xC0DEC0DEC0DEC0DE)
SENTINEL32 = np.uint32(0xC0DEC0DE)
IN_RANGE_MIN, IN_RANGE_MAX = 2.0 ** -600, 2.0 ** 300

# K operands and the types of the result words of every harness function (device_math_kat.hip)
FUNCTIONS = {
    "div_seeded": (3, "d"), "sqrt_seeded": (2, "ddd"), "normalize3_seeded": (5, "ddd"), "normalize3_generic": (3, "dddd"),
    "renormalize_unit_fast": (4, "dddddd"), "unit_window": (3, "du"), "anchored_tau": (3, "f"), "cull_anchored": (7, "u"),
    "cull_origin": (11, "uff"), "facing": (8, "dduu"), "hashes": (4, "uuuuuudd"), "clip_color": (1, "u"),
    "seed_rcp": (1, "d"), "seed_rsq": (1, "d"), "seed_rcpf": (1, "f"), "normalize3": (3, "ddd"), "renormalize_unit": (3, "ddd"),
    "div_inrange": (2, "d"), "sqrt_inrange": (1, "d"), "raybox": (13, "uuu"),
}
HOST_FUNCTIONS = ("div_seeded", "sqrt_seeded", "normalize3_seeded", "normalize3_generic", "renormalize_unit_fast", "unit_window",
                  "anchored_tau", "cull_anchored", "cull_origin", "facing", "hashes", "clip_color")


# ---- files ------------------------------------------------------------------------------------------------------------------
def write_operands(path, cols):
    """K columns of n float64, column after column."""
    a = np.ascontiguousarray(np.stack([np.asarray(c, F64) for c in cols]))
    a.tofile(path)
    return a.shape[1]


def read_results(path, name, n):
    """The M result words of function `name` for n rows: a list of uint64 arrays."""
    m = len(FUNCTIONS[name][1])
    w = np.fromfile(path, np.uint64)
    assert w.size == m * n, (path, w.size, m, n)
    return list(w.reshape(m, n))


def as_f64(words):
    return np.asarray(words, np.uint64).view(F64)


def as_f32(words):
    return np.asarray(words, np.uint64).astype(np.uint32).view(np.float32)


def bit_mismatches(got_words, want):
    """Rows where the float64 whose bits are got_words differs from `want`: bit patterns, any NaN matching any NaN."""
    got = as_f64(got_words)
    want = np.asarray(want, F64)
    same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    return np.flatnonzero(~same)


def shape_rows(n, shape):
    """How many of n rows a launch shape takes: whole waves, or a last wave of 37 lanes."""
    if shape == "tail":
        return n - ((n - 37) % 64)
    return n - n % 64


def pow2(e):
    return np.ldexp(1.0, np.asarray(e, np.int64).astype(np.int32))


def _rand_mant(rng, n):
    return 1.0 + rng.integers(0, 1 << 52, n).astype(F64) * 2.0 ** -52       # [1, 2), every mantissa bit random


def _sign(rng, n):
    return np.where(rng.integers(0, 2, n) == 1, -1.0, 1.0)


def _f32(rng, n, lo=-20, hi=20):
    """float32 scene values of either sign, log-uniform magnitude."""
    return (_sign(rng, n) * _rand_mant(rng, n) * pow2(rng.integers(lo, hi, n))).astype(np.float32).astype(F64)


def _few_products(rng, n):
    """A sum of three products of float32 values, as a plane's or a sphere's numerator is formed."""
    return _f32(rng, n) * _f32(rng, n) + _f32(rng, n) * _f32(rng, n) + _f32(rng, n) * _f32(rng, n)


class Classes:
    """Named operand classes laid end to end: cols (a tuple of arrays) and, per class, the slice it occupies."""

    def __init__(self):
        self.parts, self.where, self.n = [], {}, 0

    def add(self, name, *cols):
        cols = [np.asarray(c, F64) for c in cols]
        k = cols[0].size
        assert all(c.size == k for c in cols)
        self.where[name] = slice(self.n, self.n + k)
        self.parts.append(cols)
        self.n += k

    def cols(self):
        return tuple(np.concatenate([p[c] for p in self.parts]) for c in range(len(self.parts[0])))

    def counts(self):
        return {k: s.stop - s.start for k, s in self.where.items()}


# ---- division -----------------------------------------------------------------------------------------------------------------
def division_cases(seed=1, scale=1):
    """(a, b) of the in-range set.  scale shrinks the bulk classes (the CPU test runs 10^5 rows per class)."""
    rng = np.random.default_rng(seed)
    c = Classes()
    n = (1 << 18) // scale
    k = rng.integers(-16, 17, n).astype(F64)
    k[:33] = np.arange(-16, 17)
    c.add("near_one", _few_products(rng, n), 1.0 + k * 2.0 ** -52)                       # t = n / a, a = R.R
    n = (1 << 19) // scale
    b = _sign(rng, n) * np.maximum(_rand_mant(rng, n) * pow2(rng.integers(-10, 128, n)), 0.001)
    b[:4] = [0.001, -0.001, 2.0 ** 128, -2.0 ** 128]
    c.add("plane_t", _few_products(rng, n), b)                                           # a plane's t = num / den
    n = (1 << 20) // scale                                                               # evenly spaced mantissas x every exponent
    mant = 1.0 + (np.arange(n, dtype=F64) + 0.5) / n
    b = _sign(rng, n) * mant * pow2(np.arange(n) % 138 - 9)                              # 2^-9 .. 2^128: all >= 0.001
    a = _sign(rng, n) * _rand_mant(rng, n) * pow2(rng.integers(-600, 300, n))
    c.add("mantissa_sweep", a, b)
    n = (1 << 12) // min(scale, 4)
    b = _sign(rng, n) * np.maximum(_rand_mant(rng, n) * pow2(rng.integers(-10, 128, n)), 0.001)
    b[: n // 4] = 1.0 + rng.integers(-16, 17, n // 4) * 2.0 ** -52
    c.add("zero_numerators", np.where(rng.integers(0, 2, n) == 1, -0.0, 0.0), b)
    n = (1 << 19) // scale
    b = _sign(rng, n) * np.maximum(_rand_mant(rng, n) * pow2(rng.integers(-10, 128, n)), 0.001)
    c.add("random", _sign(rng, n) * _rand_mant(rng, n) * pow2(rng.integers(-600, 300, n)), b)
    return c


def division_in_range(a, b):
    a, b = np.abs(a), np.abs(b)
    return ((a == 0) | ((a >= IN_RANGE_MIN) & (a <= IN_RANGE_MAX))) & (((b >= 0.001) & (b <= 2.0 ** 130)) | (np.abs(b - 1.0) <= 2.0 ** -48))


def division_out_of_range_cases(seed=2):
    rng = np.random.default_rng(seed)
    c = Classes()
    n = 1 << 14
    inb = _sign(rng, n) * np.maximum(_rand_mant(rng, n) * pow2(rng.integers(-10, 128, n)), 0.001)
    inb[::3] = 1.0 + rng.integers(-16, 17, inb[::3].size) * 2.0 ** -52
    c.add("camera_1e300", _sign(rng, n) * 1e300 * _rand_mant(rng, n) * _f32(rng, n, -4, 12), inb)
    c.add("denormal_numerators", _sign(rng, n) * rng.integers(1, 1 << 52, n).astype(F64) * 5e-324, inb)
    a = _sign(rng, n) * _rand_mant(rng, n) * np.where(rng.integers(0, 2, n) == 1, pow2(rng.integers(780, 1023, n)), pow2(rng.integers(-1022, -780, n)))
    c.add("exponent_difference", a, inb)
    sp = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1.0, -3.0, 1e300, -1e-300, 5e-324])
    aa, bb = np.meshgrid(sp, np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1.0, -0.001, 2.0 ** 128]))
    c.add("specials", aa.ravel(), bb.ravel())
    return c


def ref_div(a, b):
    with np.errstate(all="ignore"):
        return np.asarray(a, F64) / np.asarray(b, F64)


def hit_of_t(t):
    """closest_hit's test of a quotient against the far limit: best > t && t > 0 with best = 999."""
    with np.errstate(invalid="ignore"):
        return (999.0 > t) & (t > 0.0)


# ---- square root ----------------------------------------------------------------------------------------------------------------
def _scale_even(rng, x):
    """x times a random even power of two that keeps it inside the in-range set (x in [1, 16))."""
    return x * pow2(2 * rng.integers(-299, 148, x.size))


def sqrt_cases(seed=3, scale=1):
    rng = np.random.default_rng(seed)
    c = Classes()
    c.add("zeros", np.array([0.0, -0.0] * 32))
    n = (1 << 18) // scale
    g = _rand_mant(rng, n) * pow2(rng.integers(0, 2, n))                                 # [1, 4)
    c.add("squares", _scale_even(rng, g * g))
    sq = g * g
    for steps, name in ((1, "squares_1_step"), (2, "squares_2_steps")):
        up, dn = sq.copy(), sq.copy()
        for _ in range(steps):
            up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
        c.add(name, _scale_even(rng, np.concatenate([up[: n // 2], dn[n // 2:]])))
    # the midpoint between a root r and its upper neighbour is m = r + ulp/2; m² = r² + r ulp + ulp²/4 sits within an ulp of
    # RN(r² + r ulp), so that double and its four nearest neighbours are the radicands adjacent to the midpoint
    r = _rand_mant(rng, n) * pow2(rng.integers(0, 2, n))
    ulp = np.spacing(r)
    m2 = (r.astype(np.longdouble) * r + r.astype(np.longdouble) * ulp).astype(F64)
    near = m2.copy()
    j = np.arange(n) % 5 - 2
    for s in (1, 2):
        near = np.where(j >= s, np.nextafter(near, np.inf), np.where(j <= -s, np.nextafter(near, -np.inf), near))
    c.add("near_midpoints", _scale_even(rng, near))
    n = (1 << 19) // scale
    e = np.arange(n) % 901 - 600                                                         # 2^-600 (the smallest discriminant) .. 2^300
    x = _rand_mant(rng, n) * pow2(e)
    x[:2] = [IN_RANGE_MIN, IN_RANGE_MAX]
    c.add("exponent_sweep", x)
    c.add("nan", np.full(64, np.nan))
    n = (1 << 18) // scale
    c.add("few_products", np.abs(_few_products(rng, n)) + 2.0 ** -600)
    return c


def sqrt_in_range(x):
    return np.isnan(x) | (x == 0) | ((x >= IN_RANGE_MIN) & (x <= IN_RANGE_MAX * 2))


def sqrt_out_of_range_cases(seed=4):
    rng = np.random.default_rng(seed)
    c = Classes()
    n = 1 << 14
    c.add("infinity", np.full(64, np.inf))
    c.add("camera_1e300", 1e300 * _rand_mant(rng, n) * pow2(rng.integers(0, 26, n)))
    c.add("denormals", rng.integers(1, 1 << 52, n).astype(F64) * 5e-324)
    c.add("tiny", _rand_mant(rng, n) * pow2(rng.integers(-1022, -601, n)))
    c.add("huge", _rand_mant(rng, n) * pow2(rng.integers(302, 1023, n)))
    return c


def ref_sqrt(x):
    with np.errstate(all="ignore"):
        return np.sqrt(np.asarray(x, F64))


def hit_of_root(q, s):
    """sphere_closest's use of q = sqrt(D): n = -s - q, or -s + q where that is not positive; then closest_hit's test of t = n / a
    (a = 1 here)."""
    with np.errstate(invalid="ignore"):
        n = -s - q
        n = np.where(n > 0.0, n, -s + q)
        return hit_of_t(n / 1.0)


ROOT_S = (-1e3, -1.0, -0.0, 0.0, 1.0, 1e3, -1e200, 1e200)


# ---- normalize3 -----------------------------------------------------------------------------------------------------------------
def normalize_guard(x, y, z):
    """The per-lane predicate of normalize3's guard (rt_device.h)."""
    with np.errstate(all="ignore"):
        nn = x * x + y * y + z * z
        cmin = np.fmin(np.fmin(np.abs(x), np.abs(y)), np.abs(z))
        return (cmin >= NORMALIZE_MIN_COMPONENT) & (nn <= NORMALIZE_MAX_NN)


def _inside_vectors(rng, n):
    m = pow2(rng.integers(-190, 191, n))
    return tuple(_sign(rng, n) * m * (0.25 + 0.75 * rng.random(n)) for _ in range(3))


def _outside_vectors(rng, n):
    """Vectors that fail the guard, every kind in turn."""
    x, y, z = (np.array(v) for v in _inside_vectors(rng, n))
    kind = np.arange(n) % 8
    below = np.nextafter(NORMALIZE_MIN_COMPONENT, 0.0)
    x = np.where(kind == 0, below, x); y = np.where(kind == 0, 1.0, y); z = np.where(kind == 0, -3.0, z)
    x = np.where(kind == 1, 2.0 ** 200, x); y = np.where(kind == 1, 2.0 ** 174, y); z = np.where(kind == 1, 2.0 ** 100, z)   # nn one ulp above
    y = np.where(kind == 2, 0.0, y)
    z = np.where(kind == 3, -0.0, z)
    x = np.where(kind == 4, np.nan, x)
    y = np.where(kind == 5, np.inf, y)
    z = np.where(kind == 6, -np.inf, z)
    x = np.where(kind == 7, 1e250, x)
    return x, y, z


def normalize_cases(seed=5, scale=1):
    """Every class is a whole number of 64-lane waves, so a class's rows share waves only with their own kind."""
    rng = np.random.default_rng(seed)
    c = Classes()
    n = (1 << 17) // scale
    d = [_f32(rng, n, -30, 30) - _f32(rng, n, -30, 30) for _ in range(3)]
    d = [np.where(np.abs(v) < NORMALIZE_MIN_COMPONENT, 1.0, v) for v in d]
    c.add("float32_differences", *d)
    n = (1 << 19) // scale
    c.add("magnitudes", *_inside_vectors(rng, n))
    n = 1 << 10
    x, y, z = (np.array(v) for v in _inside_vectors(rng, n))
    x = _sign(rng, n) * NORMALIZE_MIN_COMPONENT
    y, z = np.abs(y) * 2.0 ** -10 + 2.0 ** -199, z * 2.0 ** -10
    z = np.where(np.abs(z) < 2.0 ** -199, 2.0 ** -199, z)
    perm = np.arange(n) % 3
    c.add("min_component_exact", np.where(perm == 0, x, np.where(perm == 1, y, z)), np.where(perm == 0, y, np.where(perm == 1, z, x)),
          np.where(perm == 0, z, np.where(perm == 1, x, y)))
    big = 2.0 ** 200 * _sign(rng, n)
    sm = pow2(rng.integers(-200, 173, n))
    c.add("nn_exact_max", np.where(perm == 0, big, sm), np.where(perm == 1, big, sm), np.where(perm == 2, big, sm))
    below = np.nextafter(NORMALIZE_MIN_COMPONENT, 0.0)
    c.add("min_component_below", np.where(perm == 0, below, 1.5), np.where(perm == 1, -below, -2.0 ** -100), np.where(perm == 2, below, 2.0 ** 100))
    nxt = (perm + 1) % 3                                                                 # 2^400 + (2^174)² is one ulp above 2^400
    c.add("nn_above_max", *(np.where(perm == i, big, np.where(nxt == i, 2.0 ** 174, 2.0 ** 100)) for i in range(3)))
    sp = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -2.5, 1e-300, 1e300, 5e-324])
    gx, gy, gz = np.meshgrid(sp, sp, sp)
    k = gx.size - gx.size % 64
    c.add("specials", gx.ravel()[:k], gy.ravel()[:k], gz.ravel()[:k])
    waves = 1 << 10                                                                      # 63 lanes inside the guard, one outside
    x, y, z = (np.array(v) for v in _inside_vectors(rng, waves * 64))
    ox, oy, oz = _outside_vectors(rng, waves)
    at = np.arange(waves) * 64 + rng.integers(0, 64, waves)
    at[:64] = np.arange(64) * 64 + np.arange(64)                                         # every lane position once
    x[at], y[at], z[at] = ox, oy, oz
    c.add("one_lane_outside", x, y, z)
    c.add("inside_tail", *_inside_vectors(rng, 128))                                     # what the launch shapes trim is of this class
    return c


def ref_normalize(x, y, z):
    with np.errstate(all="ignore"):
        n = np.sqrt(x * x + y * y + z * z)
        return x / n, y / n, z / n


# ---- renormalize_unit -------------------------------------------------------------------------------------------------------------
def unit_excess(x, y, z):
    with np.errstate(all="ignore"):
        return (x * x + y * y + z * z) - 1.0


def _units(rng, n):
    v = [rng.standard_normal(n) for _ in range(3)]
    v[0][: n // 8] *= 2.0 ** -20                                                          # near-axis directions too
    v[1][n // 16: n // 8] *= 2.0 ** -30
    return ref_normalize(*v)


def _window_edge(rng, n, target_e):
    """Vectors whose e = fl(x² + y² + z²) - 1 is exactly target_e: candidates around the solution, kept where it comes out so."""
    y = rng.random(4 * n) * 0.7
    z = rng.random(4 * n) * 0.1
    x = np.sqrt((1.0 + target_e) - y * y - z * z)
    for _ in range(3):
        x = x + rng.integers(-2, 3, x.size) * np.spacing(x)
    s = [_sign(rng, x.size) for _ in range(3)]
    perm = np.arange(x.size) % 3
    a, b, cc = x * s[0], y * s[1], z * s[2]
    v = (np.where(perm == 0, a, np.where(perm == 1, b, cc)), np.where(perm == 0, b, np.where(perm == 1, cc, a)),
         np.where(perm == 0, cc, np.where(perm == 1, a, b)))
    keep = unit_excess(*v) == target_e                                                   # in the order the kernel sums the squares
    return tuple(c[keep][:n] for c in v)


def _pad_waves(rng, cols, waves):
    """Exactly `waves` whole waves: cols repeated or cut."""
    n = waves * 64
    idx = np.arange(n) % cols[0].size
    return tuple(c[idx] for c in cols)


def renormalize_cases(seed=6, scale=1):
    rng = np.random.default_rng(seed)
    c = Classes()
    n = (1 << 18) // scale
    c.add("unit", *_units(rng, n))
    n = (1 << 19) // scale
    u = _units(rng, n)
    delta = (rng.random(n) * 2 - 1) * 2.0 ** -34
    delta[:2] = [2.0 ** -34, -2.0 ** -34]
    c.add("scaled", *(v * (1.0 + delta) for v in u))
    W, ulp1 = UNIT_WINDOW, 2.0 ** -52
    for name, e in (("window_exact_above", W), ("window_inside_above", W - ulp1), ("window_outside_above", W + ulp1),
                    ("window_exact_below", -W), ("window_inside_below", -W + ulp1 / 2), ("window_outside_below", -W - ulp1 / 2)):
        c.add(name, *_pad_waves(rng, _window_edge(rng, 256, e), 8))
    waves = 256                                                                          # one NaN lane in an in-window wave
    x, y, z = (np.array(v) for v in _units(rng, waves * 64))
    at = np.arange(waves) * 64 + rng.integers(0, 64, waves)
    at[:64] = np.arange(64) * 64 + np.arange(64)
    which = np.arange(waves) % 3
    x[at[which == 0]] = np.nan; y[at[which == 1]] = np.nan; z[at[which == 2]] = np.nan
    c.add("one_nan_lane", x, y, z)
    c.add("unit_tail", *_units(rng, 128))
    return c


# ---- the seeds --------------------------------------------------------------------------------------------------------------------
def seed_operands(scale=1):
    """What the kernels feed the f64 seed instructions: every in-range denominator, every in-range radicand and every |v|² the seeded
    normalize meets.  And float32 operands for rcpf as raybox_axis feeds it: 2^-40 <= |R_i|, an even mantissa sweep and random."""
    b = division_cases(scale=scale).cols()[1]
    x = sqrt_cases(scale=scale).cols()[0]
    x = x[(x > 0) & np.isfinite(x)]
    nx, ny, nz = normalize_cases(scale=scale).cols()
    ok = normalize_guard(nx, ny, nz)
    with np.errstate(all="ignore"):
        nn = (nx * nx + ny * ny + nz * nz)[ok]
    rng = np.random.default_rng(7)
    n = (1 << 21) // scale
    m = 1.0 + np.arange(n, dtype=F64) / n
    f = np.concatenate([_sign(rng, n) * m * pow2(np.arange(n) % 81 - 40), _sign(rng, n) * _rand_mant(rng, n) * pow2(rng.integers(-40, 41, n))])
    return b, np.concatenate([x, nn]), f.astype(np.float32).astype(F64)


def seed_error(got, exact_inverse_ld):
    """max |got x - 1| in long double, x = b for rcp(b) and sqrt(x) for rsq(x); and where."""
    err = np.abs(got.astype(np.longdouble) * exact_inverse_ld - 1.0)
    k = int(np.argmax(err))
    return float(err[k]), k


def rcpf_ulps(x32, got32):
    """|got - 1/x| in units of the ulp of the correctly rounded float32 reciprocal."""
    exact = 1.0 / x32.astype(F64)
    rn = exact.astype(np.float32)
    return np.abs(got32.astype(F64) - exact) / np.spacing(np.abs(rn)).astype(F64)


# ---- host against device: operands of the HIP-free functions ---------------------------------------------------------------------------
def _noisy(rng, exact, level=2.0 ** -24):
    out = exact * (1.0 + (rng.random(exact.size) * 2 - 1) * level)
    out[::4] = exact[::4]
    return out


def hostdev_operands(name, n=1 << 20, seed=8):
    """n rows of operands for one HIP-free function: what the kernel feeds it (seeds with up to 2^-24 of noise), and special values."""
    rng = np.random.default_rng(seed + sorted(FUNCTIONS).index(name))
    take = lambda cols: tuple(np.resize(c, n) for c in cols)
    sp = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -1.0, 1e300, -1e300, 5e-324, 2.0 ** -1022, 0.5, 255.5, -0.5])
    if name == "div_seeded":
        a, b = take([np.concatenate(p) for p in zip(division_cases().cols(), division_out_of_range_cases().cols())])
        with np.errstate(all="ignore"):
            return a, b, _noisy(rng, 1.0 / b)
    if name == "sqrt_seeded":
        x, = take([np.concatenate([sqrt_cases().cols()[0], sqrt_out_of_range_cases().cols()[0]])])
        with np.errstate(all="ignore"):
            return x, _noisy(rng, 1.0 / np.sqrt(x))
    if name in ("normalize3_seeded", "normalize3_generic"):
        x, y, z = take(normalize_cases().cols())
        if name == "normalize3_generic":
            return x, y, z
        with np.errstate(all="ignore"):
            nn = x * x + y * y + z * z
            return x, y, z, nn, _noisy(rng, 1.0 / np.sqrt(nn))
    if name in ("renormalize_unit_fast", "unit_window"):
        x, y, z = take(renormalize_cases().cols())
        return (x, y, z) if name == "unit_window" else (x, y, z, unit_excess(x, y, z))
    if name == "anchored_tau":
        ll = np.abs(_few_products(rng, n))
        r2 = np.where(rng.integers(0, 4, n) == 0, ll * (1.0 + (rng.random(n) - 0.5) * 2.0 ** -17), np.abs(_f32(rng, n)))
        fl = np.abs(_f32(rng, n, -40, 10))
        for c in (ll, r2, fl):
            c[: sp.size] = sp
        return ll, r2, np.roll(fl, 3)
    if name == "cull_anchored":
        e = [_f32(rng, n, -8, 12) for _ in range(3)] + [np.abs(_f32(rng, n, -8, 12))]
        R = list(_units(rng, n))
        near = rng.integers(0, 2, n) == 1                                                # tau next to |s|: the compare is the product
        with np.errstate(all="ignore"):
            e[3] = np.where(near, np.abs(e[0] * R[0] + e[1] * R[1] + e[2] * R[2]) * (1.0 + (rng.random(n) - 0.5) * 2.0 ** -20), e[3]).astype(np.float32).astype(F64)
        e[3][: sp.size] = np.abs(sp); R[0][sp.size: 2 * sp.size] = sp
        return (*e, *R)
    if name == "cull_origin":
        c = [_f32(rng, n, -8, 12) for _ in range(3)] + [np.abs(_f32(rng, n, -8, 12))]
        R = list(_units(rng, n))
        o = [_few_products(rng, n) * 2.0 ** -10 for _ in range(3)]
        graze = rng.integers(0, 2, n) == 1                                               # r2 next to the squared distance from the line
        L = [o[i] - c[i] for i in range(3)]
        s = L[0] * R[0] + L[1] * R[1] + L[2] * R[2]
        c[3] = np.where(graze, np.abs(L[0] ** 2 + L[1] ** 2 + L[2] ** 2 - s * s) * (1.0 + (rng.random(n) - 0.5) * 2.0 ** -14), c[3]).astype(np.float32).astype(F64)
        ext = np.abs(_f32(rng, n, 0, 30))
        o[1][: sp.size] = sp; c[3][sp.size: 2 * sp.size] = np.abs(sp); R[2][2 * sp.size: 3 * sp.size] = sp
        return (*c, *R, *o, ext)
    if name == "facing":
        v = [_few_products(rng, n) for _ in range(3)]
        N = list(_units(rng, n))
        reach = np.abs(_f32(rng, n, 8, 14))
        lamb = np.where(rng.integers(0, 8, n) == 0, -0.25, rng.random(n))
        edge = rng.integers(0, 2, n) == 1                                                # u next to -tau
        N[2] = np.where(edge, -(v[0] * N[0] + v[1] * N[1] + 2.0 ** -47 * reach * (1.0 + (rng.random(n) - 0.5) * 2.0 ** -30)) / v[2], N[2])
        v[0][: sp.size] = sp; N[1][sp.size: 2 * sp.size] = sp; reach[2 * sp.size: 3 * sp.size] = sp; lamb[3 * sp.size: 4 * sp.size] = sp
        return (*v, *N, reach, lamb)
    if name == "hashes":
        cols = [rng.integers(0, 1 << 32, n).astype(F64) for _ in range(4)]
        edge = np.array([0, 1, 2, 255, 256, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xFFFFFFFE, 63, 64, 1 << 20, (1 << 23) - 1], F64)
        g = np.meshgrid(edge, edge, edge, edge)
        for c, e in zip(cols, g):
            c[: e.size] = e.ravel()
        cols[2][e.size: 2 * e.size] = np.arange(e.size) % 64                            # sample counters as the kernels pass them
        return tuple(cols)
    if name == "clip_color":
        return (np.resize(clip_operands(rng), n),)
    raise KeyError(name)


def clip_operands(rng):
    halves = np.arange(-4, 517) * 0.5                                                    # every half in [-2, 258]
    near = np.concatenate([np.nextafter(halves, np.inf), np.nextafter(halves, -np.inf)])
    sp = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e300, -1e300, 2147483648.0, -2147483649.0, 4294967296.0, 5e-324])
    return np.concatenate([halves, near, sp, (rng.random(1 << 16) * 300 - 20)])


def ref_clip(c):
    """common.py: min(max(0, int(round(c))), 255), round half to even; NaN gives 0 (rt_math.h)."""
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(np.where(np.isnan(c), 0.0, c)), 0, 255)
    return r.astype(np.uint64)


# ---- the dispatch order (rt::order_kernel) ------------------------------------------------------------------------------------------
ORDER_XCDS = 8
ORDER_NBLOCKS = (1, 7, 8, 63, 64, 65, 1000, 16200, (1 << 20) - 1)
ORDER_COSTS = ("equal", "zero", "max", "increasing", "random")


def order_bucket(c):
    """rt_device.h's order_bucket: the logarithmic cost key, monotone in c, < 1024."""
    c = np.asarray(c, np.uint64)
    msb = np.zeros(c.shape, np.int64)
    v = c.copy()
    for s in (16, 8, 4, 2, 1):
        big = v >= (np.uint64(1) << np.uint64(s))
        msb += np.where(big, s, 0)
        v = np.where(big, v >> np.uint64(s), v)
    sh = np.maximum(msb - 5, 0).astype(np.uint64)
    log = ((msb - 4) << 5) | ((c >> sh) & np.uint64(31)).astype(np.int64)
    return np.where(c < 32, c.astype(np.int64), log)


def order_shapes(nblocks):
    """(gshift, wshift, nvalid): gshift 0..6, wshift 0 or 2 with gshift >= wshift; nvalid = nblocks, and nblocks - 3 with wshift 2."""
    out = [(g, 0, nblocks) for g in range(7)]
    for g in range(2, 7):
        out += [(g, 2, nblocks), (g, 2, max(nblocks - 3, 0))]
    return out


def order_costs(kind, nvalid, seed=9):
    rng = np.random.default_rng(seed + nvalid)
    if kind == "equal":
        return np.full(nvalid, 5000, np.uint32)
    if kind == "zero":
        return np.zeros(nvalid, np.uint32)
    if kind == "max":
        return np.full(nvalid, 0xFFFFFFFF, np.uint32)
    if kind == "increasing":
        return (np.arange(nvalid, dtype=np.uint64) * 37 + 1).astype(np.uint32)
    return np.minimum(np.exp(rng.random(nvalid) * 22.0), 4.0e9).astype(np.uint32)        # log-uniform, 1 .. 3.6e9


def write_order_cases(path, cases):
    """cases: (nblocks, gshift, wshift, nvalid, cost)."""
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], np.int64).tobytes())
        for nb, g, w, nv, cost in cases:
            assert cost.dtype == np.uint32 and cost.size == max(nv, 0)
            f.write(np.array([nb, g, w, nv], np.int64).tobytes())
            f.write(cost.tobytes())


def read_order_results(path, cases):
    w = np.fromfile(path, np.uint32)
    assert w.size == sum(2 * c[0] for c in cases)
    out, pos = [], 0
    for c in cases:
        out.append(w[pos: pos + 2 * c[0]])
        pos += 2 * c[0]
    return out


def _cost_of(cost, nblocks, nvalid):
    full = np.zeros(nblocks, np.uint64)
    full[: max(nvalid, 0)] = cost[: max(nvalid, 0)]
    return full


def _place(x, t, wshift):
    return ((ORDER_XCDS * (t >> wshift) + x) << wshift) | (t & ((1 << wshift) - 1))


def valid_order(nblocks, gshift, wshift, nvalid, cost):
    """A numpy construction of what order_kernel's comment describes, ties in index order.  Both permutations, end to end."""
    c = _cost_of(cost, nblocks, nvalid)
    gb, full = 1 << gshift, nblocks >> gshift
    rows = full // ORDER_XCDS
    tail = ORDER_XCDS * rows * gb
    mean = c[: full * gb].reshape(full, gb).sum(axis=1) >> np.uint64(gshift) if full else np.zeros(0, np.uint64)
    rank = np.empty(full, np.int64)
    rank[np.argsort(-order_bucket(mean), kind="stable")] = np.arange(full)
    q, col = rank // ORDER_XCDS, rank % ORDER_XCDS
    xcd = np.where(q < rows, np.where(q & 1, ORDER_XCDS - 1 - col, col), ORDER_XCDS)
    item_x = np.full(nblocks, ORDER_XCDS, np.int64)
    item_x[: full * gb] = np.repeat(xcd, gb)
    first, second = np.full(nblocks, -1, np.int64), np.full(nblocks, -1, np.int64)
    bk = order_bucket(c)
    for x in range(ORDER_XCDS + 1):
        items = np.flatnonzero(item_x == x)
        t = np.arange(items.size)
        by_cost = items[np.argsort(-bk[items], kind="stable")]
        if x < ORDER_XCDS:
            first[_place(x, t, wshift)] = by_cost
            second[_place(x, t, wshift)] = items
        else:
            first[tail + t] = by_cost
            grouped = items[items < full * gb]
            second[tail + np.arange(grouped.size)] = grouped
            short = items[items >= full * gb]
            second[short] = short
    return np.concatenate([first, second]).astype(np.uint32)


def order_violations(order, nblocks, gshift, wshift, nvalid, cost):
    """The properties order_kernel's comment promises, checked on its output.  Returns the list of those that fail (ties are
    ordered by atomics on the device, so the bytes of two valid orders differ)."""
    bad = []
    order = np.asarray(order, np.int64)
    if order.size != 2 * nblocks:
        return ["size"]
    first, second = order[:nblocks], order[nblocks:]
    ident = np.arange(nblocks)
    for name, h in (("first", first), ("second", second)):
        if not np.array_equal(np.sort(h), ident):
            bad.append(f"{name} half is no permutation of [0, nblocks)")
    if bad:
        return bad
    c = _cost_of(cost, nblocks, nvalid)
    gb, full = 1 << gshift, nblocks >> gshift
    rows = full // ORDER_XCDS
    tail = ORDER_XCDS * rows * gb
    pos = np.arange(tail)
    px = (pos >> wshift) % ORDER_XCDS                                                    # place()'s inverse on the rows region
    pt = (((pos >> wshift) // ORDER_XCDS) << wshift) | (pos & ((1 << wshift) - 1))
    gx = []
    for name, h in (("first", first), ("second", second)):
        if np.any(h[:tail] >= full * gb):
            bad.append(f"{name} half: an item of the short group in the rows region")
            return bad
        at = np.empty(nblocks, np.int64)
        at[h] = ident                                                                    # where every item sits
        at = at[: full * gb].reshape(full, gb)
        xs = np.where(at < tail, px[np.minimum(at, max(tail - 1, 0))] if tail else ORDER_XCDS, ORDER_XCDS)
        lo, hi, cnt = xs.min(axis=1), xs.max(axis=1), (at < tail).sum(axis=1)
        if np.any((cnt != 0) & (cnt != gb)):
            bad.append(f"{name} half: a group is partly in the rows region")
        if np.any((cnt == gb) & (lo != hi)):
            bad.append(f"{name} half: a group is split over two XCD classes")
        gx.append(np.where(cnt != 0, lo, ORDER_XCDS))
        if np.any(np.bincount(gx[-1], minlength=ORDER_XCDS + 1)[:ORDER_XCDS] != rows):
            bad.append(f"{name} half: an XCD class does not have `rows` groups")
    if bad:
        return bad
    if not np.array_equal(gx[0], gx[1]):
        bad.append("a group's XCD class differs between the halves")
    bk = order_bucket(c)
    for x in range(ORDER_XCDS):
        sel = np.flatnonzero(px == x)
        sel = sel[np.argsort(pt[sel], kind="stable")]
        if np.any(np.diff(bk[first[sel]]) > 0):
            bad.append(f"first half: the cost bucket increases along XCD {x}'s list")
        want = (np.repeat(np.flatnonzero(gx[1] == x), gb) << gshift) + np.tile(np.arange(gb), rows)
        if not np.array_equal(second[sel], want):
            bad.append(f"second half: XCD {x}'s list is not its groups in tile order, items back to back")
    left = np.concatenate([(np.repeat(np.flatnonzero(gx[0] == ORDER_XCDS), gb) << gshift) + np.tile(np.arange(gb), int(np.sum(gx[0] == ORDER_XCDS))),
                           np.arange(full * gb, nblocks)]).astype(np.int64)
    if not np.array_equal(np.sort(first[tail:]), np.sort(left)):
        bad.append("first half: the positions behind `tail` do not hold exactly the leftover groups and the short group")
    if np.any(np.diff(bk[first[tail:]]) > 0):
        bad.append("first half: the cost bucket increases behind `tail`")
    if not np.array_equal(second[tail:], left):
        bad.append("second half: behind `tail` the leftover groups in tile order, then the short group in place, are expected")
    return bad


# ---- the cluster box test (make_raybox + box_open) ------------------------------------------------------------------------------------
def _boxes(rng, n):
    """Boxes of float32 corners inside a scene of extent `ext` (the square root of what the kernel gets as extent2)."""
    ext = pow2(rng.integers(-2, 11, n)).astype(F64)
    ctr = (rng.random((3, n)) * 2 - 1) * 0.5 * ext
    half = rng.random((3, n)) * 0.25 * ext * pow2(-rng.integers(0, 12, (3, n)))          # flat and elongated ones among them
    lo = (ctr - half).astype(np.float32).astype(F64)
    hi = np.maximum((ctr + half).astype(np.float32).astype(F64), np.nextafter(lo.astype(np.float32), np.float32(np.inf)).astype(F64))
    return ext, lo, hi


def raybox_hitting_rays(n=1 << 18, seed=10):
    """Rays whose float64 half-line provably enters the box: through a point at least 2^-30 extent inside it (near faces, edges
    and corners), from origins inside and outside, axis-parallel directions (R_i = 0 and |R_i| < 2^-40) among them.
    Returns the 13 operand columns of the harness's raybox function."""
    rng = np.random.default_rng(seed)
    ext, lo, hi = _boxes(rng, n)
    inset = np.minimum(2.0 ** -30 * ext * (1.0 + rng.random((3, n)) * pow2(rng.integers(0, 20, (3, n)))), 0.5 * (hi - lo))
    side = rng.integers(0, 3, (3, n))                                                    # per axis: near lo, near hi, anywhere
    p = np.where(side == 0, lo + inset, np.where(side == 1, hi - inset, lo + rng.random((3, n)) * (hi - lo)))
    p = np.clip(p, lo + np.minimum(2.0 ** -30 * ext, 0.5 * (hi - lo)), hi - np.minimum(2.0 ** -30 * ext, 0.5 * (hi - lo)))
    o = p + (rng.random((3, n)) * 2 - 1) * ext * pow2(-rng.integers(0, 8, n))
    kind = np.arange(n) % 8
    ax = rng.integers(0, 3, n)
    for i in range(3):
        o[i] = np.where((kind == 0) & (ax != i), p[i], o[i])                             # parallel to axis `ax`: two R_i = 0
        o[i] = np.where((kind == 1) & (ax == i), p[i], o[i])                             # one R_i = 0
        o[i] = np.where((kind == 2) & (ax == i), p[i] + (rng.random(n) - 0.5) * 2.0 ** -41 * ext, o[i])   # |R_i| < 2^-40
    d = p - o
    nrm = np.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2)
    ok = nrm > 2.0 ** -20 * ext
    R = d / np.where(ok, nrm, 1.0)
    cols = (*o, *R, (ext * ext * 1.0001).astype(np.float32).astype(F64), *lo, *hi)
    return tuple(c[ok] for c in cols)


def provably_enters(cols):
    """The float64 slab test with room to spare: the half-line o + tR, t >= 0, is inside the box over a parameter interval longer
    than 2^-40 of the scene (float64 rounding moves the interval's ends by 2^-50 of it at most)."""
    o, R, ext2, lo, hi = np.array(cols[0:3]), np.array(cols[3:6]), cols[6], np.array(cols[7:10]), np.array(cols[10:13])
    with np.errstate(all="ignore"):
        t1, t2 = (lo - o) / R, (hi - o) / R
        par = R == 0
        inside = (lo < o) & (o < hi)
        tn = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t1, t2)).max(axis=0)
        tf = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t1, t2)).min(axis=0)
        scale = np.sqrt(ext2) + np.abs(o).sum(axis=0)
        return (tf - np.maximum(tn, 0.0)) > 2.0 ** -40 * scale


def raybox_false_certificates(cols, cert):
    """Rows that hold a certificate although the ray provably enters the box."""
    return np.flatnonzero((np.asarray(cert) != 0) & provably_enters(cols))


def raybox_missing_rays(n=1 << 18, seed=11):
    """A family every ray of which the box test must certify: all |R_i| >= 2^-4, and the half-line stays at least
    2^-10 (extent + |o|_1) away from the box (the float64 slab test on the box grown by that much, with room to spare)."""
    rng = np.random.default_rng(seed)
    ext, lo, hi = _boxes(rng, n)
    o = (rng.random((3, n)) * 2 - 1) * ext * 0.9
    R = np.array(_units(rng, n))
    R = np.where(np.abs(R) < 2.0 ** -3, np.copysign(2.0 ** -3, R), R)
    R = np.array(ref_normalize(*R))
    grow = 2.0 ** -10 * (ext * 1.01 + np.abs(o).sum(axis=0)) * 1.01
    with np.errstate(all="ignore"):
        t1, t2 = ((lo - grow) - o) / R, ((hi + grow) - o) / R
        tn, tf = np.minimum(t1, t2).max(axis=0), np.maximum(t1, t2).min(axis=0)
        miss = (tf < np.maximum(tn, 0.0) * (1.0 - 2.0 ** -30) - 2.0 ** -30 * ext) & np.all(np.abs(R) >= 2.0 ** -4, axis=0)
    cols = (*o, *R, (ext * ext * 1.0001).astype(np.float32).astype(F64), *lo, *hi)
    return tuple(c[miss] for c in cols)


def raybox_special_rays():
    """NaN and infinite operands: none may certify."""
    sp = [np.nan, np.inf, -np.inf]
    rows = []
    base = [5.0, 6.0, 7.0, 0.6, 0.0, 0.8, 100.0, -1.0, -1.0, -1.0, 1.0, 1.0, 1.0]       # points away from the box: certified as it is
    for k in range(6):
        for v in sp:
            r = list(base); r[k] = v; rows.append(r)
    rows.append(base)
    return tuple(np.array(rows, F64).T.copy())


def raybox_reference(cols, rcp=None):
    """make_raybox + box_open + sane restated in float32 numpy, the reciprocal correctly rounded (or `rcp`)."""
    f = np.float32
    with np.errstate(all="ignore"):
        o, R = [np.asarray(c, F64).astype(f) for c in cols[0:3]], [np.asarray(c, F64).astype(f) for c in cols[3:6]]
        ext2 = np.asarray(cols[6]).astype(f)
        lo, hi = [np.asarray(c).astype(f) for c in cols[7:10]], [np.asarray(c).astype(f) for c in cols[10:13]]
        m = f(2.0 ** -18) * (np.sqrt(ext2) + ((np.abs(o[0]) + np.abs(o[1])) + np.abs(o[2])))
        fma = lambda a, b, c: (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(f)    # (the product is exact in float64; the sum's second rounding is far below the test's margins)
        tn, tf = None, None
        for i in range(3):
            Rs = np.where(np.abs(R[i]) < f(2.0 ** -40), np.copysign(f(2.0 ** -40), R[i]), R[i])
            inv = (f(1.0) / Rs) if rcp is None else rcp(Rs)
            a, b = -((o[i] + m) * inv), -((o[i] - m) * inv)
            da, db = np.abs(a) * f(2.0 ** -21), np.abs(b) * f(2.0 ** -21)
            clo = np.where(inv > 0, a - da, a + da)
            chi = np.where(inv > 0, b + db, b - db)
            ta, tb = fma(lo[i], inv, clo), fma(hi[i], inv, chi)
            tn = np.fmin(ta, tb) if tn is None else np.fmax(tn, np.fmin(ta, tb))
            tf = np.fmax(ta, tb) if tf is None else np.fmin(tf, np.fmax(ta, tb))
        open_ = ~(tf < np.fmax(tn * (f(1.0) - f(2.0 ** -18)), f(0.0)))
        chk = ((o[0] + o[1]) + o[2]) + ((R[0] + R[1]) + R[2])
        sane = (chk == chk) & (np.abs(chk) < f(2.0 ** 100))
    return (~open_ & sane).astype(np.uint64)
