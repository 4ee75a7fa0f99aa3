"""Variance-guided denoiser — the film's second moment and the a-trous filter whose colour tolerance is each pixel's estimated variance
of the mean (rt_film_accumulate_moments, rt_film_denoise_variance of include/mi355rt.h) in numpy: accumulate_moments_reference and
denoise_variance_reference are the contract's second statement, as film.accumulate_reference and denoise.denoise_reference are their
parents'.  denoise_variance_reference is the header's loop, vectorised per tap, in the header's order of operations.  Nothing here
touches the device: Film(moments=True), Film.denoise(variance=True) and Film.variance do.  denoise_variance_temporal_reference is
rt_film_denoise_variance_temporal's: the same filter on a temporal mean, its mean of squares and its per-pixel length.
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


def _filter(m, var, g, levels, normal_shin, kappa, var_floor, demodulate, prefilter):
    """The lines both filters share, from the prepare pass's demodulation on: m float64 (3, ws, h) the mean and var float64 (3, ws, h)
    the variance of the mean per channel, before demodulation."""
    ws, h = m.shape[1:]
    nsq = normal_shin.bit_length() - 1
    with np.errstate(all="ignore"):
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
    with np.errstate(all="ignore"):
        m = s / np.float64(n)
        r = sq / np.float64(n) - m * m
        r = np.where(r > 0.0, r, 0.0)
        var = r / np.float64(n - 1)
    return _filter(m, var, g, levels, normal_shin, kappa, var_floor, demodulate, prefilter)


# Film.denoise(variance=True, temporal=True)'s default spatial_below: pixels whose history is shorter than this many passes take their
# variance from their object's neighbours.  The choice of tools/temporal_variance_sweep.py (profiles/temporal_variance_sweep.json;
# DESIGN.md, Variance under a history) among 0, 2, 4 and 8 on the orbit of tests/temporal_cases.py at kappa = KAPPA: the lowest matte-pixel
# RMSE at 4 passes per frame among the values that do not lose to the unfiltered temporal mean at 1, 2 and 4 passes per frame (all four
# qualify; at 4 passes per frame they lie within 0.1 % of each other, at 1 pass per frame pooling gains 3 % over none).  KAPPA stays: over
# every kappa the sweep's best is kappa 1 by 0.5 % at 4 passes per frame, which one orbit does not resolve, so there is no KAPPA_TEMPORAL
SPATIAL_BELOW = 8.0


def check_spatial_below(spatial_below):
    """spatial_below as a Python float, or ValueError: what rt_film_denoise_variance_temporal would refuse."""
    spatial_below = float(spatial_below)
    if not (np.isfinite(spatial_below) and spatial_below >= 0.0):
        raise ValueError(f"spatial_below must be finite and >= 0, not {spatial_below!r}")
    return spatial_below


def denoise_variance_temporal_reference(mean, msq, length, guides, levels, normal_shin, kappa, var_floor, demodulate, prefilter,
                                        spatial_below=SPATIAL_BELOW, pooled=False):
    """rt_film_denoise_variance_temporal in numpy: denoise_variance_reference on what rt_film_temporal_moments wrote.  mean, msq: float64
    (3, ws, h), the temporal mean and mean of squares; length: float32 (ws, h), the per-pixel length; guides: float32 (8, ws, h).
    Returns float64 (4, ws, h) as denoise_variance_reference; pooled=True returns (that, bool (ws, h): which pixels pooled).  Per pixel
    p, float64, no fused multiply-add, in this order:
        Lp = (double)len[p];   m_c = mean[c][p]
        Lp >= spatial_below  (own):
            r_c = msq[c][p] - m_c*m_c;  r_c > 0 ? r_c : 0 (NaN: 0)
            Lp > 1:  var_c = r_c / (Lp - 1.0)        else:  var_c = 0
        else  (pooled; a NaN length lands here):
            SL = M_c = Q_c = +0.0
            for dx = -2..2 (outer), dy = -2..2 (inner), step 1:   q = (p.x+dx, p.y+dy)
                q outside the frame, or id[q] != id[p]:  skip
                lq = (double)len[q];   !(lq > 0):  skip
                SL = SL + lq;   M_c = M_c + lq * mean[c][q];   Q_c = Q_c + lq * msq[c][q]
            !(SL > 1) or !(Lp > 0):  var_c = 0
            else:  pm = M_c / SL;   r_c = Q_c / SL - pm*pm  (clamped as above);   var_c = (r_c / (SL - 1.0)) * (SL / Lp)
        demodulate, v_0, levels == 0 (out = mean, out[3] = v_0 without demodulation), the levels and the output:
            exactly rt_film_denoise_variance's lines"""
    levels, normal_shin, kappa, var_floor, demodulate, prefilter = check_denoise_variance(levels, normal_shin, kappa, var_floor, demodulate, prefilter)
    spatial_below = check_spatial_below(spatial_below)
    m, q = np.asarray(mean, dtype=np.float64), np.asarray(msq, dtype=np.float64)
    ln, g = np.asarray(length), np.asarray(guides)
    if m.ndim != 3 or m.shape[0] != 3:
        raise ValueError(f"mean must have shape (3, ws, h), got {m.shape}")
    if q.shape != m.shape:
        raise ValueError(f"msq must have the shape of mean, {m.shape}, got {q.shape}")
    if ln.dtype != np.float32 or ln.shape != m.shape[1:]:
        raise ValueError(f"length must be float32 of shape {m.shape[1:]}, got {ln.dtype} {ln.shape}")
    if g.dtype != np.float32 or g.shape != (GUIDE_PLANES,) + m.shape[1:]:
        raise ValueError(f"guides must be float32 of shape {(GUIDE_PLANES,) + m.shape[1:]}, got {g.dtype} {g.shape}")
    ws, h = m.shape[1:]
    with np.errstate(all="ignore"):
        Lp = ln.astype(np.float64)
        own = Lp >= np.float64(spatial_below)
        r = q - m * m
        r = np.where(r > 0.0, r, 0.0)
        var_own = np.where(Lp > 1.0, r / (Lp - 1.0), 0.0)
        ident = g[7]
        SL, M, Q = np.zeros((ws, h)), np.zeros((3, ws, h)), np.zeros((3, ws, h))

        def windows(o, size):
            p = slice(max(0, -o), min(size, size - o))
            return (p, slice(p.start + o, p.stop + o)) if p.start < p.stop else (None, None)

        for dx in range(-2, 3):
            px, qx = windows(dx, ws)
            if px is None:
                continue
            for dy in range(-2, 3):
                py, qy = windows(dy, h)
                if py is None:
                    continue
                lq = Lp[qx, qy]
                ok = (ident[qx, qy] == ident[px, py]) & (lq > 0.0)
                SL[px, py] = np.where(ok, SL[px, py] + lq, SL[px, py])
                M[:, px, py] = np.where(ok, M[:, px, py] + lq * m[:, qx, qy], M[:, px, py])
                Q[:, px, py] = np.where(ok, Q[:, px, py] + lq * q[:, qx, qy], Q[:, px, py])
        pm = M / SL
        rp = Q / SL - pm * pm
        rp = np.where(rp > 0.0, rp, 0.0)
        var_pool = np.where((SL > 1.0) & (Lp > 0.0), (rp / (SL - 1.0)) * (SL / Lp), 0.0)
        var = np.where(own, var_own, var_pool)
    out = _filter(m, var, g, levels, normal_shin, kappa, var_floor, demodulate, prefilter)
    return (out, ~own) if pooled else out
