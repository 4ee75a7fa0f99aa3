"""Denoiser — the first-hit guides and the edge-stopping film filter (rt_render_guides, rt_film_denoise of include/mi355rt.h) in
numpy: guides_reference and denoise_reference are the contract's second statement, as film.tone_reference is the resolve's.
guides_reference is built from leaf restatements of the reference's functions (normalize, plane_normal_f32, intersect_ray_sphere,
intersect_ray_plane, get_intersection, all vectorised over rays) and scene.texture.texel_index; denoise_reference is the header's
loop, vectorised per tap, in the header's order of operations.  Nothing here touches the device: Film.guides and Film.denoise do.
"""
import numpy as np

from .scene.texture import texel_index

GUIDE_PLANES = 8
NORMAL_SHININESS = tuple(1 << i for i in range(11))          # 1, 2, 4, ..., 1024
MAX_LEVELS = 6
B3 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
MISS_DISC, MISS_BEHIND = -999.9, -999.0
HIT_SPHERE, HIT_PLANE, HIT_NONE = 0, 1, 404


def check_denoise(levels, normal_shin, sigma, demodulate):
    """(levels, normal_shin, sigma, demodulate) as Python numbers, or ValueError: what rt_film_denoise would refuse."""
    if isinstance(levels, float) and not levels.is_integer():
        raise ValueError(f"levels must be an integer 0..{MAX_LEVELS}, not {levels!r}")
    levels = int(levels)
    if not 0 <= levels <= MAX_LEVELS:
        raise ValueError(f"levels must be 0..{MAX_LEVELS}, not {levels}")
    if normal_shin not in NORMAL_SHININESS:
        raise ValueError(f"normal_shin must be one of 1, 2, 4, ..., 1024, not {normal_shin!r}")
    sigma = float(sigma)
    if not (sigma == 0.0 or (np.isfinite(sigma) and sigma > 0.0)):
        raise ValueError(f"sigma must be 0 (no colour weight), or finite and > 0, not {sigma!r}")
    if demodulate not in (0, 1, False, True):
        raise ValueError(f"demodulate must be 0 or 1, not {demodulate!r}")
    return levels, int(normal_shin), sigma, int(demodulate)


# ---------------------------------------------------------------------------------------------------------------------
# The filter

def denoise_reference(total, n, guides, levels, normal_shin, sigma, demodulate):
    """rt_film_denoise in numpy.  total: float64 (3, ws, h), the sum of n passes; guides: float32 (8, ws, h).  Returns the filtered
    mean, float64 (3, ws, h).  Per pixel p in float64, no fused multiply-add, in this order:
        m_0[c][p] = s[c][p] / (double)n
        demodulate:  a[c][p] = max((double)albedo_c[p], 1.0);   m_0[c][p] = m_0[c][p] / a[c][p]
        levels == 0 (with or without demodulate):  out[c][p] = s[c][p] / (double)n, and nothing else is evaluated
        for i = 0 .. levels-1:      step = 1 << i;   q_i = sigma / 2^i  (exact)
            W = +0.0; A_c = +0.0
            for dx = -2..2 (outer), dy = -2..2 (inner):   q = (p.x + step*dx, p.y + step*dy)
                q outside [0,ws) x [0,h):  skip
                id[q] != id[p]:            skip
                id[p] >= 0:  cn = ((nx_p*nx_q) + (ny_p*ny_q)) + (nz_p*nz_q)   (float32 normals widened to double)
                             !(cn > 0):  skip;    log2(normal_shin) times:  cn = cn*cn
                id[p] <  0:  cn = 1.0                                          (sky pixels: the colour weight alone)
                sigma > 0:   e_c = (m_i[c][q] - m_i[c][p]) / q_i;  d2 = (e_0*e_0 + e_1*e_1) + e_2*e_2;  wc = 1.0 / (1.0 + d2)
                else:        wc = 1.0
                w = ((k[dx] * k[dy]) * cn) * wc          k = (1/16, 1/4, 3/8, 1/4, 1/16)  (the B3 spline)
                W = W + w;   A_c = A_c + w * m_i[c][q]
            m_{i+1}[c][p] = A_c / W                       (the centre tap always contributes 9/64, so W > 0)
        out[c][p] = demodulate ? m_levels[c][p] * a[c][p] : m_levels[c][p]"""
    levels, normal_shin, sigma, demodulate = check_denoise(levels, normal_shin, sigma, demodulate)
    n = int(n)
    if n < 1:
        raise ValueError(f"n must be >= 1 (the number of passes accumulated), not {n}")
    s = np.asarray(total, dtype=np.float64)
    g = np.asarray(guides)
    if s.ndim != 3 or s.shape[0] != 3:
        raise ValueError(f"total must have shape (3, ws, h), got {s.shape}")
    if g.dtype != np.float32 or g.shape != (GUIDE_PLANES,) + s.shape[1:]:
        raise ValueError(f"guides must be float32 of shape {(GUIDE_PLANES,) + s.shape[1:]}, got {g.dtype} {g.shape}")
    ws, h = s.shape[1:]
    nsq = normal_shin.bit_length() - 1
    with np.errstate(all="ignore"):
        m = s / np.float64(n)
        if levels == 0:
            return m
        a = None
        if demodulate:
            alb = g[4:7].astype(np.float64)
            a = np.where(alb > 1.0, alb, 1.0)
            m = m / a
        ident = g[7]
        surface = ident >= 0
        N = g[0:3].astype(np.float64)
        for i in range(levels):
            step = 1 << i
            q = np.float64(sigma) / np.float64(2.0 ** i)
            W = np.zeros((ws, h))
            A = np.zeros((3, ws, h))
            for dx in range(-2, 3):
                ox = step * dx
                px = slice(max(0, -ox), min(ws, ws - ox))
                if px.start >= px.stop:
                    continue
                qx = slice(px.start + ox, px.stop + ox)
                for dy in range(-2, 3):
                    oy = step * dy
                    py = slice(max(0, -oy), min(h, h - oy))
                    if py.start >= py.stop:
                        continue
                    qy = slice(py.start + oy, py.stop + oy)
                    ok = ident[qx, qy] == ident[px, py]
                    cn = ((N[0][px, py] * N[0][qx, qy]) + (N[1][px, py] * N[1][qx, qy])) + (N[2][px, py] * N[2][qx, qy])
                    sp = surface[px, py]
                    ok &= np.where(sp, cn > 0.0, True)
                    for _ in range(nsq):
                        cn = cn * cn
                    cn = np.where(sp, cn, 1.0)
                    mq, mp = m[:, qx, qy], m[:, px, py]
                    if sigma > 0.0:
                        e = (mq - mp) / q
                        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
                        wc = 1.0 / (1.0 + d2)
                    else:
                        wc = 1.0
                    w = ((np.float64(B3[dx + 2]) * np.float64(B3[dy + 2])) * cn) * wc
                    W[px, py] = np.where(ok, W[px, py] + w, W[px, py])
                    A[:, px, py] = np.where(ok, A[:, px, py] + w * mq, A[:, px, py])
            m = A / W
        return m * a if demodulate else m


# ---------------------------------------------------------------------------------------------------------------------
# Leaf restatements of the reference's functions, vectorised over rays: arrays of shape (n, 3) and (n,)

def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def normalize(v):
    """common.py:28-32: v / sqrt(v.v), float64."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        return v / np.sqrt(_dot(v, v))[..., None]


def plane_normal_f32(n):
    """common.py:104-110 on a float32 normal: float32 squares and sums, the float32 square root of the sum, float32 divisions."""
    n = np.asarray(n, dtype=np.float32)
    with np.errstate(all="ignore"):
        s = n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1] + n[..., 2] * n[..., 2]
        norm = np.sqrt(s.astype(np.float64)).astype(np.float32)
        return n / norm[..., None]


def intersect_ray_sphere(o, d, c, r):
    """intersections.py:6-38 for rays (o (3,) or (n, 3), d (n, 3)) and one float32 sphere (c (3,), r): distances (n,)."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    c, r = np.asarray(c, dtype=np.float32), np.float32(r)
    with np.errstate(all="ignore"):
        R = normalize(d)
        Lv = o - c.astype(np.float64)
        a = _dot(R, R)
        b = 2 * _dot(Lv, R)
        cc = _dot(Lv, Lv) - np.float64(r * r)                     # (a float32 product)
        disc = b * b - 4 * a * cc
        sq = np.sqrt(np.where(disc < 0.0, 0.0, disc))
        n1, n2 = -b - sq, -b + sq
        t = np.where(n1 > 0.0, n1 / (2 * a), np.where(n2 > 0.0, n2 / (2 * a), MISS_BEHIND))
        return np.where(disc < 0.0, MISS_DISC, t)


def intersect_ray_plane(o, d, po, pn):
    """intersections.py:41-68 for rays and one float32 plane (origin po, raw normal pn): distances (n,)."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    po, n = np.asarray(po, dtype=np.float32).astype(np.float64), np.asarray(pn, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        den = d[..., 0] * n[0] + d[..., 1] * n[1] + d[..., 2] * n[2]
        LP = po - o
        LP = np.broadcast_to(LP, d.shape)
        nom = LP[..., 0] * n[0] + LP[..., 1] * n[1] + LP[..., 2] * n[2]
        dist = nom / den
        return np.where(np.abs(den) < 0.001, MISS_DISC, np.where(dist > 0, dist, MISS_BEHIND))


def get_intersection(o, d, spheres, planes):
    """trace.py:7-41 for rays: (t (n,) float64, idx (n,) int, type (n,) int) with type 0 a sphere, 1 a plane, 404 nothing (then
    t = 999.0 and idx = -999).  spheres float32 (7, S), planes float32 (9, P), in the caller's order: the first of equal distances
    wins, spheres before planes."""
    spheres, planes = np.asarray(spheres, dtype=np.float32), np.asarray(planes, dtype=np.float32)
    d = np.asarray(d, dtype=np.float64)
    n = d.shape[0]
    best = np.full(n, 999.0)
    idx = np.full(n, -999, dtype=np.int64)
    typ = np.full(n, HIT_NONE, dtype=np.int64)
    for k in range(spheres.shape[1]):
        dist = intersect_ray_sphere(o, d, spheres[0:3, k], spheres[3, k])
        take = (best > dist) & (dist > 0)
        best, idx, typ = np.where(take, dist, best), np.where(take, k, idx), np.where(take, HIT_SPHERE, typ)
    for k in range(planes.shape[1]):
        dist = intersect_ray_plane(o, d, planes[0:3, k], planes[3:6, k])
        take = (best > dist) & (dist > 0)
        best, idx, typ = np.where(take, dist, best), np.where(take, k, idx), np.where(take, HIT_PLANE, typ)
    return best, idx, typ


# ---------------------------------------------------------------------------------------------------------------------
# The guides

def primary_rays(cam_origin, cam_rot, w, h, raygen=None, pixel_loc=None, x0=0, x1=None):
    """The RT_AA_NONE primary rays of columns [x0, x1) without a lens: (o (3,), d ((x1-x0)*h, 3)), x slow and y fast.
    P = (px, x*dy + y0, y*dz + z0) from raygen = (px, y0, dy, z0, dz), or pixel_loc[:, x, y]; d = normalize(R P)."""
    x1 = w if x1 is None else x1
    o = np.asarray(cam_origin, dtype=np.float64).reshape(3)
    R = np.asarray(cam_rot, dtype=np.float64).reshape(3, 3)
    xs, ys = np.meshgrid(np.arange(x0, x1), np.arange(h), indexing="ij")
    if pixel_loc is not None:
        pl = np.asarray(pixel_loc, dtype=np.float64)
        if pl.shape != (3, w, h):
            raise ValueError(f"pixel_loc must have shape (3, {w}, {h}), got {pl.shape}")
        P = pl[:, x0:x1, :].reshape(3, -1).T
    else:
        px, y0, dy, z0, dz = (np.float64(v) for v in raygen)
        P = np.stack([np.full(xs.size, px), xs.reshape(-1).astype(np.float64) * dy + y0, ys.reshape(-1).astype(np.float64) * dz + z0], axis=1)
    v = np.stack([R[i, 0] * P[:, 0] + R[i, 1] * P[:, 1] + R[i, 2] * P[:, 2] for i in range(3)], axis=1)
    return o, normalize(v)


def guides_reference(spheres, planes, cam_origin, cam_rot, w, h, raygen=None, pixel_loc=None, x0=0, x1=None, textures=None):
    """rt_render_guides in numpy: float32 (8, x1-x0, h).  Per pixel, with (t, idx, type) = get_intersection(cam_origin, d) for the
    pinhole primary ray d (primary_rays):
        planes 0..2  (float)N: a sphere's normalize(Pt - c) with Pt = o + t d, a plane's plane_normal_f32(n);   miss: +0.0
        plane  3     (float)t;                                                                                  miss: +0.0
        planes 4..6  the object's float32 colour, or with textures = (records, sphere_ids, plane_ids, texels) and the object's
                     id k >= 0 the texel texels[texel_index(Pt, *records[k])];                                  miss: +0.0
        plane  7     the caller's sphere index k, or S + k for plane k;                                         miss: -1.0"""
    spheres, planes = np.asarray(spheres, dtype=np.float32), np.asarray(planes, dtype=np.float32)
    x1 = w if x1 is None else x1
    S = spheres.shape[1]
    o, d = primary_rays(cam_origin, cam_rot, w, h, raygen, pixel_loc, x0, x1)
    t, idx, typ = get_intersection(o, d, spheres, planes)
    n = d.shape[0]
    out = np.zeros((GUIDE_PLANES, n), np.float32)
    out[7] = -1.0
    with np.errstate(all="ignore"):
        Pt = o + t[:, None] * d
    sph, pln = np.flatnonzero(typ == HIT_SPHERE), np.flatnonzero(typ == HIT_PLANE)
    if sph.size:
        k = idx[sph]
        N = normalize(Pt[sph] - spheres[0:3, k].T.astype(np.float64))
        out[0:3, sph] = N.T.astype(np.float32)
        out[4:7, sph] = spheres[4:7, k]
        out[7, sph] = k.astype(np.float32)
    if pln.size:
        k = idx[pln]
        out[0:3, pln] = plane_normal_f32(planes[3:6, k].T).T
        out[4:7, pln] = planes[6:9, k]
        out[7, pln] = (S + k).astype(np.float32)
    hit = typ != HIT_NONE
    with np.errstate(all="ignore"):
        out[3, hit] = t[hit].astype(np.float32)
    if textures is not None:
        records, tsid, tpid, texels = textures
        tsid, tpid = np.asarray(tsid, dtype=np.int64).reshape(-1), np.asarray(tpid, dtype=np.int64).reshape(-1)
        texels = np.asarray(texels, dtype=np.float32).reshape(-1, 3)
        tex = np.full(n, -1, dtype=np.int64)
        tex[sph] = tsid[idx[sph]]
        tex[pln] = tpid[idx[pln]]
        for k, (origin, axes, dims, first) in enumerate(records):
            sel = np.flatnonzero(tex == k)
            if sel.size:
                out[4:7, sel] = texels[texel_index(Pt[sel], origin, axes, dims, first)].T
    return out.reshape(GUIDE_PLANES, x1 - x0, h)
