"""Lighting: a colour and strength per light and a Blinn-Phong highlight per material
(include/mi355rt.h: rt_set_scene_lighting).  light_terms() is the per-light arithmetic of the header, word for word, in
numpy float64; the kernel (rt_device.h: trace_bounce) must agree with it bit for bit."""
import numpy as np

SHININESS = tuple(1 << i for i in range(11))    # 1, 2, 4, ..., 1024


def squarings(shin):
    """log2(shin) for a shininess of SHININESS; ValueError for any other value."""
    f = float(shin)
    for i, v in enumerate(SHININESS):
        if f == float(v):
            return i
    raise ValueError(f"shin must be one of 1, 2, 4, ..., 1024, got {shin}")


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _xyz(v):
    v = np.asarray(v, dtype=np.float64)
    return v[..., 0], v[..., 1], v[..., 2]


def light_wants(Ld, N, lamb_n, spec):
    """(cN, k, wantL, wantS) of one light for each trace: which terms ask for the shadow query.
    Ld, N (..., 3) float64 unit vectors; lamb_n and spec scalars or arrays of shape (...)."""
    Ld, N = _xyz(Ld), _xyz(N)
    with np.errstate(invalid="ignore", over="ignore"):
        cN = _dot(Ld, N)
        k = np.asarray(lamb_n, dtype=np.float64) * cN
        wantL = k > 0.0
        wantS = (np.asarray(spec, dtype=np.float64) > 0.0) & (cN > 0.0)
    return cN, k, wantL, wantS


def light_terms(rgb, d, N, Ld, col, e, lamb_n, spec, spec_n, shin, occluded):
    """The colour of each trace after one light: rgb (..., 3) float64 plus that light's Lambert and highlight terms.
    d incoming unit direction, N outward normal, Ld unit vector to the light (or to its sample point), col the object's colour
    or texel, all (..., 3) float64; e (3,) the light's colour times strength; lamb_n = lamb / n, spec, spec_n = spec / n
    (n: the scene's shadow_samples under area lights, else 1) and shin scalars or arrays of shape (...); occluded (...) bool,
    the shadow query's answer (read only where a term asked for the query).  float64, no fused multiply-add, in this order:
        cN = dot(Ld, N);  k = lamb_n * cN
        wantL = k > 0;  wantS = spec > 0 and cN > 0
        neither, or occluded: rgb unchanged
        wantL:  rgb_c = rgb_c + ((k * e_c) * col_c)
        wantS:  Hs = Ld + (-d);  H = Hs / sqrt(dot(Hs, Hs));  s = dot(N, H)
                s > 0:  q = s, log2(shin) times q = q * q;  a = spec_n * q;  rgb_c = rgb_c + (a * e_c)
    A NaN compares false: Hs == 0 gives s = NaN and no highlight."""
    rgb = np.array(rgb, dtype=np.float64)
    col = np.asarray(col, dtype=np.float64)
    e = np.asarray(e, dtype=np.float64).reshape(3)
    dx, dy, dz = _xyz(d)
    Nv, Lv = _xyz(N), _xyz(Ld)
    shape = rgb.shape[:-1]
    nsq = np.broadcast_to(np.vectorize(squarings, otypes=[np.int64])(np.asarray(shin, dtype=np.float64)), shape)
    spec_n = np.broadcast_to(np.asarray(spec_n, dtype=np.float64), shape)
    cN, k, wantL, wantS = light_wants(Ld, N, lamb_n, spec)
    k = np.broadcast_to(k, shape)
    lit = ~np.asarray(occluded, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        addL = np.broadcast_to(wantL & lit, shape)
        for c in range(3):
            rgb[..., c] = np.where(addL, rgb[..., c] + ((k * e[c]) * col[..., c]), rgb[..., c])
        Hs = (Lv[0] + (-dx), Lv[1] + (-dy), Lv[2] + (-dz))
        nrm = np.sqrt(Hs[0] * Hs[0] + Hs[1] * Hs[1] + Hs[2] * Hs[2])
        H = (Hs[0] / nrm, Hs[1] / nrm, Hs[2] / nrm)
        s = _dot(Nv, H)
        q = np.array(np.broadcast_to(s, shape), dtype=np.float64)
        for i in range(10):
            q = np.where(i < nsq, q * q, q)
        a = spec_n * q
        addS = np.broadcast_to(wantS & lit & (s > 0.0), shape)
        for c in range(3):
            rgb[..., c] = np.where(addS, rgb[..., c] + (a * e[c]), rgb[..., c])
    return rgb
