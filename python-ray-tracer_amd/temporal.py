"""Temporal accumulation — the film through a camera move (rt_film_temporal of include/mi355rt.h) in numpy: temporal_reference is
the contract's second statement, as film.tone_reference is the resolve's and denoise.denoise_reference the filter's;
temporal_moments_reference is rt_film_temporal_moments', the same call with a second moment carried beside the mean.  It is the
header's loop, vectorised over the frame with the four taps in the header's order; the primary ray is denoise.primary_rays, the one
guides_reference forms.  Nothing here touches the device: Film.next_frame and Film.temporal do.
"""
import numpy as np

from .denoise import GUIDE_PLANES, primary_rays

MAX_N = 1 << 24
SNAP = 2.0 ** -20

# Film.temporal's defaults: the best whole-frame RMSE of the sweep recorded in DESIGN.md (Temporal accumulation; tools/temporal_sweep.py)
# on an 8-step orbit of the soft_default_64_d4 scene with a matte floor, 4 passes per frame with one shadow sample, against the
# 1024-pass mean at the last camera.  A longer history keeps lowering the noise of matte pixels but not their error (resampling
# blur at edges takes over) and makes mirrors and highlights lag further; a normal_cos of 0.999 throws away curved surfaces.
DEPTH_TOL = 0.1
NORMAL_COS = 0.99
MAX_HISTORY = 8.0


def orbit(cam, pivot, degrees):
    """The camera (origin (3,), rotation (3, 3)) turned by `degrees` about the vertical (z) axis through `pivot`: it keeps looking at
    what it looked at.  Returns (origin, rotation), float64."""
    o, R = np.asarray(cam[0], dtype=np.float64).reshape(3), np.asarray(cam[1], dtype=np.float64).reshape(3, 3)
    c = np.asarray(pivot, dtype=np.float64).reshape(3)
    a = np.deg2rad(float(degrees))
    Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return c + Rz @ (o - c), Rz @ R


def check_temporal(depth_tol, normal_cos, max_history, n=1):
    """(depth_tol, normal_cos, max_history, n) as Python numbers, or ValueError: what rt_film_temporal would refuse."""
    depth_tol, normal_cos, max_history = float(depth_tol), float(normal_cos), float(max_history)
    if isinstance(n, float) and not n.is_integer():
        raise ValueError(f"n must be an integer 1..2^24, not {n!r}")
    n = int(n)
    if not 1 <= n <= MAX_N:
        raise ValueError(f"n must be 1..2^24 (the number of passes in the sum), not {n}")
    if not (np.isfinite(depth_tol) and depth_tol >= 0.0):
        raise ValueError(f"depth_tol must be finite and >= 0, not {depth_tol!r}")
    if not -1.0 <= normal_cos <= 1.0:
        raise ValueError(f"normal_cos must lie in [-1, 1], not {normal_cos!r}")
    if not (np.isfinite(max_history) and max_history >= 0.0):
        raise ValueError(f"max_history must be finite and >= 0, not {max_history!r}")
    return depth_tol, normal_cos, max_history, n


def _camera(cam, what):
    o = np.asarray(cam[0], dtype=np.float64).reshape(-1)
    R = np.asarray(cam[1], dtype=np.float64).reshape(-1)
    if o.size != 3 or R.size != 9:
        raise ValueError(f"{what} must be (origin (3,), rotation (3, 3))")
    if not (np.isfinite(o).all() and np.isfinite(R).all()):
        raise ValueError(f"{what} has an entry that is not finite")
    return o, R


def temporal_taps_reference(guides, hist, hist_len, hist_guides, cam, prev_cam, raygen, w, h, depth_tol, normal_cos, max_history,
                            taps=False):
    """The history's part of temporal_reference: (hm, L, valid) with hm float64 (3, w, h) the surviving taps' weighted mean, L
    float64 (w, h) their length after the cap and valid bool (w, h): some tap survived (elsewhere hm and L are 0 and the pixel is
    fresh).  taps=True adds a dict: "Pt" (3, w, h) the world point of each pixel's first hit, "qx", "qy" (4, w, h) the taps'
    pixel indices clipped into the frame, "used" bool (4, w, h) which taps contributed, "bw" (4, w, h) their bilinear weights, in
    the order (a, b) = (0, 0), (0, 1), (1, 0), (1, 1)."""
    return _taps(guides, hist, hist_len, hist_guides, cam, prev_cam, raygen, w, h, depth_tol, normal_cos, max_history, taps, None)[0]


def _taps(guides, hist, hist_len, hist_guides, cam, prev_cam, raygen, w, h, depth_tol, normal_cos, max_history, taps, hist_sq):
    """(what temporal_taps_reference returns, hq): hq float64 (3, w, h) is the surviving taps' weighted mean of hist_sq (None
    without one), summed in the taps' order beside hm."""
    hsq = None if hist_sq is None else np.asarray(hist_sq, dtype=np.float64)
    if hsq is not None and hsq.shape != (3, int(w), int(h)):
        raise ValueError(f"hist_sq must have shape {(3, int(w), int(h))}, got {hsq.shape}")
    depth_tol, normal_cos, max_history, _ = check_temporal(depth_tol, normal_cos, max_history)
    w, h = int(w), int(h)
    g, hg = np.asarray(guides), np.asarray(hist_guides)
    hs, hl = np.asarray(hist, dtype=np.float64), np.asarray(hist_len)
    for name, a in (("guides", g), ("hist_guides", hg)):
        if a.dtype != np.float32 or a.shape != (GUIDE_PLANES, w, h):
            raise ValueError(f"{name} must be float32 of shape {(GUIDE_PLANES, w, h)}, got {a.dtype} {a.shape}")
    if hs.shape != (3, w, h):
        raise ValueError(f"hist must have shape {(3, w, h)}, got {hs.shape}")
    if hl.dtype != np.float32 or hl.shape != (w, h):
        raise ValueError(f"hist_len must be float32 of shape {(w, h)}, got {hl.dtype} {hl.shape}")
    o, R = _camera(cam, "cam")
    po, pR = _camera(prev_cam, "prev_cam")
    px, y0, dy, z0, dz = (np.float64(v) for v in raygen)
    if dy == 0.0 or dz == 0.0:
        raise ValueError("the grid's dy or dz is 0")
    with np.errstate(all="ignore"):
        idp = g[7]
        live = ~(idp < 0)
        if max_history == 0.0:
            live = np.zeros((w, h), bool)
        _, d = primary_rays(o, R.reshape(3, 3), w, h, raygen)
        d = d.T.reshape(3, w, h)
        t = g[3].astype(np.float64)
        Pt = np.stack([o[k] + t * d[k] for k in range(3)])
        u = np.stack([Pt[k] - po[k] for k in range(3)])
        q = [(pR[j] * u[0] + pR[3 + j] * u[1]) + pR[6 + j] * u[2] for j in range(3)]
        live &= q[0] > 0.0
        r2 = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
        sc = px / q[0]
        fx = (q[1] * sc - y0) / dy
        fy = (q[2] * sc - z0) / dz
        rx, ry = np.floor(fx + 0.5), np.floor(fy + 0.5)
        fx = np.where(np.abs(fx - rx) <= SNAP, rx, fx)
        fy = np.where(np.abs(fy - ry) <= SNAP, ry, fy)
        live &= (fx > -1.0) & (fx < w) & (fy > -1.0) & (fy < h)
        fx, fy = np.where(live, fx, 0.0), np.where(live, fy, 0.0)           # (fresh pixels: any index inside the frame)
        flx, fly = np.floor(fx), np.floor(fy)
        ax, ay = fx - flx, fy - fly
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        N = g[0:3].astype(np.float64)
        HN = hg[0:3].astype(np.float64)
        HT = hg[3].astype(np.float64)
        HL = hl.astype(np.float64)
        W, Lh, H = np.zeros((w, h)), np.zeros((w, h)), np.zeros((3, w, h))
        Q = np.zeros((3, w, h))
        info = dict(Pt=Pt, qx=[], qy=[], used=[], bw=[])
        for a in (0, 1):
            for b in (0, 1):
                qx, qy = ix + a, iy + b
                bw = (ax if a else 1.0 - ax) * (ay if b else 1.0 - ay)
                ok = live & (bw != 0.0) & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                ok &= hg[7][cx, cy] == idp
                tq = HT[cx, cy]
                ok &= np.abs(tq * tq - r2) <= depth_tol * r2
                cn = ((N[0] * HN[0][cx, cy]) + (N[1] * HN[1][cx, cy])) + (N[2] * HN[2][cx, cy])
                ok &= cn >= normal_cos
                lq = HL[cx, cy]
                ok &= lq > 0.0
                W = np.where(ok, W + bw, W)
                H = np.where(ok, H + bw * hs[:, cx, cy], H)
                if hsq is not None:
                    Q = np.where(ok, Q + bw * hsq[:, cx, cy], Q)
                Lh = np.where(ok, Lh + bw * lq, Lh)
                info["qx"].append(cx); info["qy"].append(cy); info["used"].append(ok); info["bw"].append(bw)
        valid = W > 0.0
        Ws = np.where(valid, W, 1.0)
        hm = np.where(valid, H / Ws, 0.0)
        L = np.where(valid, Lh / Ws, 0.0)
        L = np.where(L > max_history, max_history, L)
        hq = None if hsq is None else np.where(valid, Q / Ws, 0.0)
    if taps:
        return (hm, L, valid, {k: (v if k == "Pt" else np.stack(v)) for k, v in info.items()}), hq
    return (hm, L, valid), hq


def temporal_reference(total, n, guides, hist, hist_len, hist_guides, cam, prev_cam, raygen, w, h, depth_tol, normal_cos, max_history):
    """rt_film_temporal in numpy.  total: float64 (3, w, h), the sum of n passes of this frame; guides: float32 (8, w, h); hist:
    float64 (3, w, h), the previous frame's mean; hist_len: float32 (w, h); hist_guides: float32 (8, w, h); cam, prev_cam:
    (origin (3,), rotation (3, 3)); raygen = (px, y0, dy, z0, dz).  Returns (out float64 (3, w, h), out_len float32 (w, h));
    temporal_taps_reference gives the intermediate (hm, L, valid).  Per pixel p = (x, y), e = x*h + y, in float64 without fused
    multiply-add, in this order; o, R are the current camera, o', R' the previous one:
        fresh:   out[k][e] = s[k][e] / (double)n   (k = 0..2);   out_len[e] = (float)n
        idp = guides[7][e];     idp < 0 (a miss) or max_history == 0:  fresh
        P = (px, (double)x*dy + y0, (double)y*dz + z0);  d = normalize(R P) exactly as rt_render_guides forms it;  t = (double)guides[3][e]
        Pt_k = o_k + t*d_k;     u_k = Pt_k - o'_k
        q_j = (R'[j]*u_0 + R'[3+j]*u_1) + R'[6+j]*u_2      (j = 0..2: R' transposed times u)
        !(q_0 > 0):  fresh
        r2 = (u_0*u_0 + u_1*u_1) + u_2*u_2;   sc = px / q_0;   fx = (q_1*sc - y0) / dy;   fy = (q_2*sc - z0) / dz
        snap:  rx = floor(fx + 0.5);  |fx - rx| <= 2^-20:  fx = rx        (the same for fy)
        !(fx > -1 && fx < w && fy > -1 && fy < h):  fresh                 (NaN lands here)
        ix = floor(fx); ax = fx - ix;   iy = floor(fy); ay = fy - iy;    W = H_k = Lh = +0.0
        for a = 0, 1 (outer), b = 0, 1 (inner):   q = (ix + a, iy + b);   bw = (a ? ax : 1.0 - ax) * (b ? ay : 1.0 - ay)
            bw == 0, or q outside [0,w) x [0,h):  skip
            hist_guides[7][q] != idp:  skip
            tq = (double)hist_guides[3][q];   !(fabs(tq*tq - r2) <= depth_tol * r2):  skip
            cn = ((nx_p*nx_q) + (ny_p*ny_q)) + (nz_p*nz_q)   (float32 normals widened; p from guides, q from hist_guides);  !(cn >= normal_cos): skip
            lq = (double)hist_len[q];   !(lq > 0):  skip
            W = W + bw;   H_k = H_k + bw * hist[k][q];   Lh = Lh + bw * lq
        !(W > 0):  fresh
        hm_k = H_k / W;   L = Lh / W;   L > max_history:  L = max_history
        out[k][e] = (L * hm_k + s[k][e]) / (L + (double)n);      out_len[e] = (float)(L + (double)n)"""
    depth_tol, normal_cos, max_history, n = check_temporal(depth_tol, normal_cos, max_history, n)
    s = np.asarray(total, dtype=np.float64)
    if s.shape != (3, int(w), int(h)):
        raise ValueError(f"total must have shape {(3, int(w), int(h))}, got {s.shape}")
    hm, L, valid = temporal_taps_reference(guides, hist, hist_len, hist_guides, cam, prev_cam, raygen, w, h, depth_tol, normal_cos,
                                           max_history)
    nn = np.float64(n)
    with np.errstate(all="ignore"):
        out = np.where(valid, (L * hm + s) / (L + nn), s / nn)
        out_len = np.where(valid, L + nn, nn).astype(np.float32)
    return out, out_len


def temporal_moments_reference(total, total_sq, n, guides, hist, hist_sq, hist_len, hist_guides, cam, prev_cam, raygen, w, h, depth_tol,
                               normal_cos, max_history):
    """rt_film_temporal_moments in numpy: temporal_reference with the second moment beside the mean.  total_sq: float64 (3, w, h), the
    sum of squares of the n passes of this frame; hist_sq: float64 (3, w, h), the history's MEAN of squares; everything else as
    temporal_reference.  Returns (out, out_sq, out_len): out and out_len are temporal_reference's bits, out_sq float64 (3, w, h) the
    new mean of squares.  Every line of temporal_reference holds, in the same order, and per pixel, float64, no fused multiply-add:
        fresh:                         out_sq[k][e] = sq[k][e] / (double)n
        in the tap loop, after H_k:    Q_k = Q_k + bw * hist_sq[k][q]
        after hm_k:                    hq_k = Q_k / W
                                       out_sq[k][e] = (L * hq_k + sq[k][e]) / (L + (double)n)"""
    depth_tol, normal_cos, max_history, n = check_temporal(depth_tol, normal_cos, max_history, n)
    s, sq = np.asarray(total, dtype=np.float64), np.asarray(total_sq, dtype=np.float64)
    for name, a in (("total", s), ("total_sq", sq)):
        if a.shape != (3, int(w), int(h)):
            raise ValueError(f"{name} must have shape {(3, int(w), int(h))}, got {a.shape}")
    if hist_sq is None:
        raise ValueError("hist_sq is None: the history of a moments call has a mean of squares")
    (hm, L, valid), hq = _taps(guides, hist, hist_len, hist_guides, cam, prev_cam, raygen, w, h, depth_tol, normal_cos, max_history, False,
                               hist_sq)
    nn = np.float64(n)
    with np.errstate(all="ignore"):
        out = np.where(valid, (L * hm + s) / (L + nn), s / nn)
        out_sq = np.where(valid, (L * hq + sq) / (L + nn), sq / nn)
        out_len = np.where(valid, L + nn, nn).astype(np.float32)
    return out, out_sq, out_len
