"""Variance-guided denoiser — the film's second moment and the a-trous filter whose colour tolerance is each pixel's estimated variance
of the mean (rt_film_accumulate_moments, rt_film_denoise_variance of include/mi355rt.h) in numpy: accumulate_moments_reference and
denoise_variance_reference are the contract's second statement, as film.accumulate_reference and denoise.denoise_reference are their
parents'.  denoise_variance_reference is the header's loop, vectorised per tap, in the header's order of operations.  Nothing here
touches the device: Film(moments=True), Film.denoise(variance=True) and Film.variance do.
"""
import numpy as np

from .denoise import B3, GUIDE_PLANES, MAX_LEVELS, NORMAL_SHININESS

VAR_PLANES = 4
G3 = (0.25, 0.5, 0.25)

# Film.denoise(variance=True)'s default kappa: the colour tolerance in standard deviations of the mean.  The choice of the sweep
# 0.5, 0.75, 1, 1.5, 2, 3, 4 at levels 4, normal_shininess 32 with demodulation and the variance prefilter on the soft_default_64_d4
# scene (one shadow sample) against its 1024-pass mean: the lowest RMSE at 4 passes among the values that beat the raw mean at 2, 4, 8
# and 16 passes (tools/variance_sweep.py, profiles/variance_sweep.json; DESIGN.md, Variance-guided denoiser)
KAPPA = 1.5


def check_denoise_variance(levels, normal_shin, kappa, var_floor, demodulate, prefilter):
    """(levels, normal_shin, kappa, var_floor, demodulate, prefilter) as Python numbers, or ValueError: what rt_film_denoise_variance
    would refuse."""
    if isinstance(levels, float) and not levels.is_integer():
        raise ValueError(f"levels must be an integer 0..{MAX_LEVELS}, not {levels!r}")
    levels = int(levels)
    if not 0 <= levels <= MAX_LEVELS:
        raise ValueError(f"levels must be 0..{MAX_LEVELS}, not {levels}")
    if normal_shin not in NORMAL_SHININESS:
        raise ValueError(f"normal_shin must be one of 1, 2, 4, ..., 1024, not {normal_shin!r}")
    kappa, var_floor = float(kappa), float(var_floor)
    if not (np.isfinite(kappa) and kappa >= 0.0):
        raise ValueError(f"kappa must be finite and >= 0, not {kappa!r}")
    if not (np.isfinite(var_floor) and var_floor >= 0.0):
        raise ValueError(f"var_floor must be finite and >= 0, not {var_floor!r}")
    if demodulate not in (0, 1, False, True):
        raise ValueError(f"demodulate must be 0 or 1, not {demodulate!r}")
    if prefilter not in (0, 1, False, True):
        raise ValueError(f"prefilter must be 0 or 1, not {prefilter!r}")
    return levels, int(normal_shin), kappa, var_floor, int(demodulate), int(prefilter)


def accumulate_moments_reference(total, total_sq, frames):
    """The sum rules of rt_film_accumulate_moments in numpy.  total, total_sq: float64 (3, ws, h), or both None (reset: start from
    +0.0); frames: an iterable of float32 (3, ws, h) pass frames, in pass order.  The sum is film.accumulate_reference's (s = s +
    (double)f_i[e]); the sum of squares per element, float64, in pass order:
        q = reset ? +0.0 : sq[e];  for i: g = (double)f_i[e]; q = q + g*g;  sq[e] = q
    Returns (sum, sum of squares), new float64 arrays."""
    if (total is None) != (total_sq is None):
        raise ValueError("the sum and the sum of squares are reset together")
    s = None if total is None else np.array(total, dtype=np.float64)
    q = None if total_sq is None else np.array(total_sq, dtype=np.float64)
    for f in frames:
        f = np.asarray(f)
        if f.dtype != np.float32:
            raise ValueError(f"pass frames are float32, not {f.dtype}")
        g = f.astype(np.float64)
        if s is None:
            s, q = np.zeros(g.shape, np.float64), np.zeros(g.shape, np.float64)
        with np.errstate(all="ignore"):
            s = s + g
            q = q + g * g
    if s is None:
        raise ValueError("no sums and no pass frame")
    return s, q


def denoise_variance_reference(total, total_sq, n, guides, levels, normal_shin, kappa, var_floor, demodulate, prefilter):
    """rt_film_denoise_variance in numpy.  total, total_sq: float64 (3, ws, h), the sum and the sum of squares of n >= 2 passes; guides:
    float32 (8, ws, h).  Returns float64 (4, ws, h): the filtered mean and, in plane 3, its propagated variance.  Per pixel p in
    float64, no fused multiply-add, in this order (k[] is the B3 spline of denoise_reference):
        m_0[c][p] = s[c][p] / (double)n;    r = sq[c][p] / (double)n - m_0[c][p]*m_0[c][p];    r > 0 ? r : 0   (NaN: 0)
        var_c = r / (double)(n - 1)                                   (the variance of the MEAN, per channel)
        demodulate:  a[c][p] = max((double)albedo_c[p], 1.0);   m_0[c][p] = m_0[c][p] / a[c][p];   var_c = var_c / (a[c][p]*a[c][p])
        v_0[p] = (var_0 + var_1) + var_2
        levels == 0:  out[c][p] = s[c][p] / (double)n;  out[3][p] = v_0[p] computed WITHOUT demodulation;  nothing else is evaluated
        for i = 0 .. levels-1:    step = 1 << i
            prefilter:  gw = gv = +0.0;  for dx = -1..1 (outer), dy = -1..1 (inner):  q = (p.x+dx, p.y+dy)   (step 1 at every level)
                            q outside the frame, or id[q] != id[p]:  skip
                            t = g[dx]*g[dy]   g = (1/4, 1/2, 1/4);    gw = gw + t;   gv = gv + t * v_i[q]
                        vp = gv / gw                                   (the centre contributes 1/4, so gw > 0)
            else:       vp = v_i[p]
            den = (kappa*kappa) * vp + var_floor
            W = +0.0; A_c = +0.0; V = +0.0
            for dx = -2..2 (outer), dy = -2..2 (inner):   q = (p.x + step*dx, p.y + step*dy)
                outside, id, normal test and cn:  exactly the lines of rt_film_denoise
                e_c = m_i[c][q] - m_i[c][p];   d2 = (e_0*e_0 + e_1*e_1) + e_2*e_2
                den > 0:  wc = 1.0 / (1.0 + d2 / den)        else:  wc = d2 > 0 ? 0.0 : 1.0
                w = ((k[dx] * k[dy]) * cn) * wc
                W = W + w;   A_c = A_c + w * m_i[c][q];   V = V + (w*w) * v_i[q]
            m_{i+1}[c][p] = A_c / W;     v_{i+1}[p] = V / (W*W)
        out[c][p] = demodulate ? m_levels[c][p] * a[c][p] : m_levels[c][p];     out[3][p] = v_levels[p]   (filter units)"""
    levels, normal_shin, kappa, var_floor, demodulate, prefilter = check_denoise_variance(levels, normal_shin, kappa, var_floor, demodulate, prefilter)
    n = int(n)
    if n < 2:
        raise ValueError(f"n must be >= 2 (a variance needs two passes), not {n}")
    s, sq = np.asarray(total, dtype=np.float64), np.asarray(total_sq, dtype=np.float64)
    g = np.asarray(guides)
    if s.ndim != 3 or s.shape[0] != 3:
        raise ValueError(f"total must have shape (3, ws, h), got {s.shape}")
    if sq.shape != s.shape:
        raise ValueError(f"total_sq must have the shape of total, {s.shape}, got {sq.shape}")
    if g.dtype != np.float32 or g.shape != (GUIDE_PLANES,) + s.shape[1:]:
        raise ValueError(f"guides must be float32 of shape {(GUIDE_PLANES,) + s.shape[1:]}, got {g.dtype} {g.shape}")
    ws, h = s.shape[1:]
    nsq = normal_shin.bit_length() - 1
    with np.errstate(all="ignore"):
        m = s / np.float64(n)
        r = sq / np.float64(n) - m * m
        r = np.where(r > 0.0, r, 0.0)
        var = r / np.float64(n - 1)
        if levels == 0:
            return np.concatenate([m, ((var[0] + var[1]) + var[2])[None]])
        a = None
        if demodulate:
            alb = g[4:7].astype(np.float64)
            a = np.where(alb > 1.0, alb, 1.0)
            m = m / a
            var = var / (a * a)
        v = (var[0] + var[1]) + var[2]
        k2 = np.float64(kappa) * np.float64(kappa)
        ident = g[7]
        surface = ident >= 0
        N = g[0:3].astype(np.float64)

        def windows(o, size):
            p = slice(max(0, -o), min(size, size - o))
            return (p, slice(p.start + o, p.stop + o)) if p.start < p.stop else (None, None)

        for i in range(levels):
            step = 1 << i
            if prefilter:
                gw, gv = np.zeros((ws, h)), np.zeros((ws, h))
                for dx in range(-1, 2):
                    px, qx = windows(dx, ws)
                    if px is None:
                        continue
                    for dy in range(-1, 2):
                        py, qy = windows(dy, h)
                        if py is None:
                            continue
                        ok = ident[qx, qy] == ident[px, py]
                        t = np.float64(G3[dx + 1]) * np.float64(G3[dy + 1])
                        gw[px, py] = np.where(ok, gw[px, py] + t, gw[px, py])
                        gv[px, py] = np.where(ok, gv[px, py] + t * v[qx, qy], gv[px, py])
                vp = gv / gw
            else:
                vp = v
            den = k2 * vp + np.float64(var_floor)
            W = np.zeros((ws, h))
            A = np.zeros((3, ws, h))
            V = np.zeros((ws, h))
            for dx in range(-2, 3):
                px, qx = windows(step * dx, ws)
                if px is None:
                    continue
                for dy in range(-2, 3):
                    py, qy = windows(step * dy, h)
                    if py is None:
                        continue
                    ok = ident[qx, qy] == ident[px, py]
                    cn = ((N[0][px, py] * N[0][qx, qy]) + (N[1][px, py] * N[1][qx, qy])) + (N[2][px, py] * N[2][qx, qy])
                    sp = surface[px, py]
                    ok &= np.where(sp, cn > 0.0, True)
                    for _ in range(nsq):
                        cn = cn * cn
                    cn = np.where(sp, cn, 1.0)
                    mq, mp = m[:, qx, qy], m[:, px, py]
                    e = mq - mp
                    d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
                    dn = den[px, py]
                    wc = np.where(dn > 0.0, 1.0 / (1.0 + d2 / dn), np.where(d2 > 0.0, 0.0, 1.0))
                    w = ((np.float64(B3[dx + 2]) * np.float64(B3[dy + 2])) * cn) * wc
                    W[px, py] = np.where(ok, W[px, py] + w, W[px, py])
                    A[:, px, py] = np.where(ok, A[:, px, py] + w * mq, A[:, px, py])
                    V[px, py] = np.where(ok, V[px, py] + (w * w) * v[qx, qy], V[px, py])
            m = A / W
            v = V / (W * W)
        return np.concatenate([m * a if demodulate else m, v[None]])
