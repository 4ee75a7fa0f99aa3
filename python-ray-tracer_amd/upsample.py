"""Guided upsampling — run the film at low resolution, show it at full (rt_render_guides_grid, rt_film_upsample of
include/mi355rt.h).  upsample_reference is the contract's second statement in numpy, as temporal.temporal_reference is the
reprojection's: the header's three stages, vectorised over the output frame with the taps in the header's order.  Upsampler puts
the two calls behind a Film:

    renderer.set_raygen(w // 2, h // 2, *low_raygen)              # the film accumulates and filters a quarter of the pixels
    with Film(renderer, moments=True) as film, Upsampler(film, w, h) as up:
        film.accumulate(params, passes=4)
        film.denoise(variance=True)
        up.upsample(denoised=True)                                # full-resolution guides, then the lift along them
        image, _ = up.resolve(white=400.0, gamma=2, denoised=True)

Nothing in upsample_reference and check_upsample touches the device.
"""
import numpy as np

from . import _lib as L
from .denoise import GUIDE_PLANES
from .film import check_tone

SNAP = 2.0 ** -20

# Upsampler.upsample's default: the choice of the sweep recorded in DESIGN.md (Guided upsampling; tools/upsample_sweep.py) over 0, 0.5,
# 0.8, 0.9, 0.95 and 0.99 on the soft_default_64_d4 scene, 16 passes at 32 x 32 filtered and lifted to 64 x 64 against the 1024-pass
# mean: the largest value whose whole-frame RMSE is within 1 % of the sweep's best.  Up to 0.95 the test changes next to nothing (0.07 %
# of the pixels leave stage 0); at 0.99 curved surfaces fall into stage 1 (1.9 %) and the error rises by a quarter.
NORMAL_COS = 0.95


def _grid(g, what):
    g = tuple(float(v) for v in np.asarray(g, dtype=np.float64).reshape(-1))
    if len(g) != 5:
        raise ValueError(f"{what} must be (px, y0, dy, z0, dz)")
    if not all(np.isfinite(v) for v in g) or g[0] == 0.0 or g[2] == 0.0 or g[4] == 0.0:
        raise ValueError(f"{what} must be finite with px, dy and dz not 0, not {g!r}")
    return g


def check_upsample(lo_grid, hi_grid, normal_cos=NORMAL_COS, demodulate=True, n=1):
    """(lo_grid, hi_grid, normal_cos, demodulate, n) as Python numbers, or ValueError: what rt_film_upsample would refuse of them."""
    if isinstance(n, float) and not n.is_integer():
        raise ValueError(f"n must be an integer >= 1, not {n!r}")
    n = int(n)
    if n < 1:
        raise ValueError(f"n must be >= 1 (the number of passes in the sum), not {n}")
    lo_grid, hi_grid = _grid(lo_grid, "lo_grid"), _grid(hi_grid, "hi_grid")
    normal_cos = float(normal_cos)
    if not -1.0 <= normal_cos <= 1.0:
        raise ValueError(f"normal_cos must lie in [-1, 1], not {normal_cos!r}")
    if demodulate not in (0, 1, False, True):
        raise ValueError(f"demodulate must be 0 or 1, not {demodulate!r}")
    return lo_grid, hi_grid, normal_cos, int(demodulate), n


def hi_raygen(lo_raygen, wl, hl, w, h):
    """The closed-form grid of a w x h frame with the field of view of the wl x hl grid lo_raygen = (px, y0, dy, z0, dz).  The field
    of view is read off the low grid as the extent its pixel centres span at distance px: y0 .. y0 + (wl-1)*dy across and z0 ..
    z0 + (hl-1)*dz down (scene/camera.py puts the first and the last pixel centre on the edges of the field).  The w x h grid spans the
    same extent from the same corner: px, y0 and z0 stay, dy' = dy*(wl-1)/(w-1) and dz' = dz*(hl-1)/(h-1).  A frame of one column
    (or row) spans nothing: its step is the low grid's."""
    px, y0, dy, z0, dz = (float(v) for v in lo_raygen)
    wl, hl, w, h = int(wl), int(hl), int(w), int(h)
    dy2 = dy * (wl - 1) / (w - 1) if w > 1 and wl > 1 else dy
    dz2 = dz * (hl - 1) / (h - 1) if h > 1 and hl > 1 else dz
    return (px, y0, dy2, z0, dz2)


def _snap(f):
    r = np.floor(f + 0.5)
    return np.where(np.abs(f - r) <= SNAP, r, f)


def _clamp(f, last):
    f = np.where(f >= 0.0, f, 0.0)
    return np.where(f > last, np.float64(last), f)


def upsample_reference(lo, n, lo_guides, hi_guides, lo_grid, hi_grid, normal_cos=NORMAL_COS, demodulate=True):
    """rt_film_upsample in numpy.  lo: float64 (3 or more, wl, hl), the sum of n passes of the low frame (planes 0..2 are read);
    lo_guides: float32 (8, wl, hl); hi_guides: float32 (8, w, h); lo_grid, hi_grid: (px, y0, dy, z0, dz).  Returns (out float64
    (3, w, h), kind float32 (w, h)).  Per output pixel p = (X, Y) in float64 without fused multiply-add, in this order:
        m[c][q] = lo[c][q] / (double)n;   a_lo[c][q] = max((double)lo_guides[4+c][q], 1.0);   a_hi[c] = max((double)hi_guides[4+c][p], 1.0)
        sc = lo_px / hi_px;   fx = (((double)X*hi_dy + hi_y0) * sc - lo_y0) / lo_dy;   fy = (((double)Y*hi_dz + hi_z0) * sc - lo_z0) / lo_dz
        snap:  rx = floor(fx + 0.5);  |fx - rx| <= 2^-20:  fx = rx        (the same for fy)
        !(fx >= 0):  fx = 0;   fx > wl-1:  fx = wl-1;     the same for fy with hl              (so NaN becomes 0)
        ix = floor(fx); ax = fx - ix;   iy = floor(fy); ay = fy - iy;    idp = hi_guides[7][p]
        stage 0   W = A_c = +0.0;  for a = 0, 1 (outer), b = 0, 1 (inner):  q = (ix+a, iy+b);  bw = (a ? ax : 1.0 - ax) * (b ? ay : 1.0 - ay)
                    bw == 0, or q outside [0,wl) x [0,hl):  skip;      lo_guides[7][q] != idp:  skip
                    idp >= 0:  cn = ((nx_p*nx_q) + (ny_p*ny_q)) + (nz_p*nz_q)  (float32 normals widened);   !(cn >= normal_cos):  skip
                    v_c = demodulate ? m[c][q] / a_lo[c][q] : m[c][q];     W = W + bw;   A_c = A_c + bw * v_c
                  W > 0:  out[c][p] = demodulate ? (A_c / W) * a_hi[c] : A_c / W;   kind 0
        stage 1   else, for a = -1..2 (outer), b = -1..2 (inner):  q = (ix+a, iy+b) inside the frame with lo_guides[7][q] == idp:
                    ex = (double)(ix+a) - fx;  ey = (double)(iy+b) - fy;   wq = 1.0 / (1.0 + (ex*ex + ey*ey));   W, A_c as above with wq
                  W > 0:  the same output line;   kind 1
        stage 2   else the taps and weights bw of stage 0 (bw == 0 or q outside: skip), no test, no demodulation:  out[c][p] = A_c / W;   kind 2"""
    lo_grid, hi_grid, normal_cos, demodulate, n = check_upsample(lo_grid, hi_grid, normal_cos, demodulate, n)
    s, lg, hg = np.asarray(lo, dtype=np.float64), np.asarray(lo_guides), np.asarray(hi_guides)
    if s.ndim != 3 or s.shape[0] < 3:
        raise ValueError(f"lo must have shape (3 or more, wl, hl), got {s.shape}")
    wl, hl = s.shape[1:]
    if lg.dtype != np.float32 or lg.shape != (GUIDE_PLANES, wl, hl):
        raise ValueError(f"lo_guides must be float32 of shape {(GUIDE_PLANES, wl, hl)}, got {lg.dtype} {lg.shape}")
    if hg.dtype != np.float32 or hg.ndim != 3 or hg.shape[0] != GUIDE_PLANES:
        raise ValueError(f"hi_guides must be float32 of shape (8, w, h), got {hg.dtype} {hg.shape}")
    w, h = hg.shape[1:]
    lpx, ly0, ldy, lz0, ldz = (np.float64(v) for v in lo_grid)
    hpx, hy0, hdy, hz0, hdz = (np.float64(v) for v in hi_grid)
    with np.errstate(all="ignore"):
        m = s[:3] / np.float64(n)
        alb_lo, alb_hi = lg[4:7].astype(np.float64), hg[4:7].astype(np.float64)
        a_lo, a_hi = np.where(alb_lo > 1.0, alb_lo, 1.0), np.where(alb_hi > 1.0, alb_hi, 1.0)
        md = m / a_lo if demodulate else m
        sc = lpx / hpx
        X, Y = np.arange(w, dtype=np.float64)[:, None], np.arange(h, dtype=np.float64)[None, :]
        fx = np.broadcast_to(_clamp(_snap(((X * hdy + hy0) * sc - ly0) / ldy), wl - 1), (w, h))
        fy = np.broadcast_to(_clamp(_snap(((Y * hdz + hz0) * sc - lz0) / ldz), hl - 1), (w, h))
        flx, fly = np.floor(fx), np.floor(fy)
        ax, ay = fx - flx, fy - fly
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        idp = hg[7]
        surface = idp >= 0
        N, LN = hg[0:3].astype(np.float64), lg[0:3].astype(np.float64)

        def bilinear(guided, v):
            W, A = np.zeros((w, h)), np.zeros((3, w, h))
            for a in (0, 1):
                for b in (0, 1):
                    qx, qy = ix + a, iy + b
                    bw = (ax if a else 1.0 - ax) * (ay if b else 1.0 - ay)
                    ok = (bw != 0.0) & (qx >= 0) & (qx < wl) & (qy >= 0) & (qy < hl)
                    cx, cy = np.clip(qx, 0, wl - 1), np.clip(qy, 0, hl - 1)
                    if guided:
                        ok &= lg[7][cx, cy] == idp
                        cn = ((N[0] * LN[0][cx, cy]) + (N[1] * LN[1][cx, cy])) + (N[2] * LN[2][cx, cy])
                        ok &= ~surface | (cn >= normal_cos)
                    W = np.where(ok, W + bw, W)
                    A = np.where(ok, A + bw * v[:, cx, cy], A)
            return W, A

        W0, A0 = bilinear(True, md)
        W1, A1 = np.zeros((w, h)), np.zeros((3, w, h))
        for a in (-1, 0, 1, 2):
            for b in (-1, 0, 1, 2):
                qx, qy = ix + a, iy + b
                ok = (qx >= 0) & (qx < wl) & (qy >= 0) & (qy < hl)
                cx, cy = np.clip(qx, 0, wl - 1), np.clip(qy, 0, hl - 1)
                ok &= lg[7][cx, cy] == idp
                ex, ey = qx.astype(np.float64) - fx, qy.astype(np.float64) - fy
                wq = 1.0 / (1.0 + (ex * ex + ey * ey))
                W1 = np.where(ok, W1 + wq, W1)
                A1 = np.where(ok, A1 + wq * md[:, cx, cy], A1)
        W2, A2 = bilinear(False, m)
        k0 = W0 > 0.0
        k1 = ~k0 & (W1 > 0.0)
        r0, r1, r2 = A0 / W0, A1 / W1, A2 / W2
        if demodulate:
            r0, r1 = r0 * a_hi, r1 * a_hi
        out = np.where(k0, r0, np.where(k1, r1, r2))
        kind = np.where(k0, 0.0, np.where(k1, 1.0, 2.0)).astype(np.float32)
    return out, kind


class Upsampler:
    """The lift of a Film's picture to a w x h frame: it owns the full-resolution guides, the float64 (3, w, h) output and, on
    request, the kind plane.  The film holds the full low-resolution frame of a renderer with a closed-form grid (set_raygen), which
    is read at construction.  raygen: the output frame's closed-form grid; None: hi_raygen(renderer.raygen, ...), the grid of a
    camera of the film's field of view at w x h."""

    def __init__(self, film, w, h, raygen=None):
        r = film.renderer
        film._live()
        if getattr(r, "raygen", None) is None:
            raise ValueError("upsampling needs the closed-form ray grid: call set_raygen before making an Upsampler")
        if film.x0 != 0 or film.x1 != r.w or film.h != r.h:
            raise ValueError(f"upsampling works on the full frame: the film holds columns [{film.x0}, {film.x1}) of height {film.h}, "
                             f"the renderer's frame is {r.w} x {r.h}")
        w, h = int(w), int(h)
        if w < 1 or h < 1 or w * h > L.RT_FILM_MAX_PIXELS:
            raise ValueError(f"the output frame must hold 1..RT_FILM_MAX_PIXELS = 2^27 pixels, not {w} x {h}")
        self.film, self.renderer, self.w, self.h = film, r, w, h
        self.lo_grid = tuple(r.raygen)
        self.hi_grid = hi_raygen(self.lo_grid, film.ws, film.h, w, h) if raygen is None else tuple(float(v) for v in raygen)
        check_upsample(self.lo_grid, self.hi_grid)
        self.d_guides = self.d_out = self.d_kind = None
        self.guides_camera = None                                 # the camera d_guides was last rendered with
        self.lifted = None                                        # ((denoised, temporal, bloom), the serial of the film's write that was lifted)
        self.d_guides = r.malloc(4 * L.RT_GUIDE_PLANES * w * h)
        self.d_out = r.malloc(24 * w * h)

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        held = [self.d_kind, self.d_guides, self.d_out]
        self.d_guides = self.d_out = self.d_kind = None
        self.lifted = None
        for d in held:
            if d and not self.renderer.closed:
                self.renderer.free(d)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if not self.d_out:
            raise ValueError("the upsampler is closed")

    @property
    def buffer(self):
        """The address of the lifted mean, float64 (3, w, h) laid out like a sum: what Renderer.film_bloom, film_meter and
        film_resolve take with n = 1 at full resolution."""
        self._live()
        return self.d_out

    # -- the two calls ----------------------------------------------------------------------
    def guides(self, stream=None, force=False):
        """The full-resolution guides of the renderer's current scene and camera (Renderer.render_guides_grid) into the upsampler's
        own buffer, when the camera is not the one they were last rendered with (the rule Film.temporal uses; force: in any case, a
        scene change being the caller's cue).  The renderer's frame and grid stay the film's.  Asynchronous; returns the address."""
        self._live()
        r = self.renderer
        if getattr(r, "camera", None) is None:
            raise ValueError("the renderer has no camera yet: call set_camera first")
        if force or self.guides_camera is None or any(not np.array_equal(a, b) for a, b in zip(self.guides_camera, r.camera)):
            r.render_guides_grid(self.w, self.h, self.hi_grid, 0, self.w, self.d_guides, self.w * self.h, stream)
            self.guides_camera = r.camera
        return self.d_guides

    def upsample(self, denoised=False, temporal=False, bloom=False, normal_cos=NORMAL_COS, demodulate=True, kinds=False, stream=None):
        """Lift the source that film.resolve(denoised=..., temporal=..., bloom=...) would show (Renderer.film_upsample) into the
        upsampler's buffer, which resolve() shows.  The film's own guides are the low-resolution guides (rendered first if they are
        missing, stale or another camera's), guides() the full-resolution ones.  normal_cos: the least cosine between an output
        pixel's normal and a tap's; demodulate: interpolate colour / albedo and multiply by the full-resolution albedo; kinds: also
        write the plane of stages, which kinds() reads.  Asynchronous."""
        self._live()
        film, r = self.film, self.renderer
        film._has_pass()
        flags = (bool(denoised), bool(temporal), bool(bloom))
        src, n, serial, _ = film.source(*flags)
        _, _, normal_cos, demodulate, _ = check_upsample(self.lo_grid, self.hi_grid, normal_cos, demodulate, n)
        if tuple(r.raygen or ()) != self.lo_grid or r.w != film.x1 or r.h != film.h:
            raise ValueError("the renderer's grid is no longer the one the film and this upsampler were made for")
        cam = getattr(r, "camera", None)
        if not film.d_guides or film.guides_stale or film.guides_camera is None or cam is None or any(
                not np.array_equal(a, b) for a, b in zip(film.guides_camera, cam)):
            film.guides(stream)
        hi = self.guides(stream)
        if kinds and not self.d_kind:
            self.d_kind = r.malloc(4 * self.w * self.h)
        r.film_upsample(src, film.ws, film.h, n, film.d_guides, hi, self.w, self.h, self.lo_grid, self.hi_grid, self.d_out,
                        self.d_kind if kinds else None, normal_cos=normal_cos, demodulate=demodulate, stream=stream)
        self.lifted = (flags, serial)

    def kinds(self, stream=None):
        """The stage that wrote each pixel of the last upsample(kinds=True): float32 (w, h) of 0, 1 and 2.  Waits for the stream."""
        self._live()
        if not self.d_kind:
            raise ValueError("no kind plane yet: call upsample(kinds=True) first")
        out = np.empty((self.w, self.h), np.float32)
        self.renderer.sync(stream)
        self.renderer.d2h(out, self.d_kind)
        return out

    # -- frames -----------------------------------------------------------------------------
    def _request(self, exposure, white, gamma, flags, denoised, temporal, bloom, auto_exposure):
        """What both resolves check before they touch the device: the tone, and that upsample() lifted this source of the film as
        it stands.  Returns the film's meter state for that source, or None."""
        self._live()
        self.film._has_pass()
        check_tone(1, exposure, white, gamma, flags)
        _, _, serial, state = self.film.source(denoised, temporal, bloom, auto_exposure)
        if self.lifted != ((bool(denoised), bool(temporal), bool(bloom)), serial):
            raise ValueError("the upsampler holds no lift of the film's current passes and this source: call upsample() with the same "
                             "denoised, temporal and bloom first")
        return state

    def _resolve_call(self, state, d_u8, d_f32, **tone):
        if state:
            self.renderer.film_resolve_metered(self.d_out, self.w, self.h, 1, state, d_u8, d_f32, **tone)
        else:
            self.renderer.film_resolve(self.d_out, self.w, self.h, 1, d_u8, d_f32, **tone)

    def resolve_device(self, d_u8=None, d_f32=None, exposure=1.0, white=0.0, gamma=1, flags=0, out_stride=None, stream=None,
                       denoised=False, temporal=False, bloom=False, auto_exposure=False):
        """Film.resolve_device of the lifted picture: the w x h frame, tone-mapped, into caller-owned device memory.  denoised,
        temporal and bloom name the source that upsample() lifted; auto_exposure: with the exposure that film.meter() solved for
        that source at low resolution.  ValueError unless upsample() ran for the film as it stands.  Asynchronous."""
        state = self._request(exposure, white, gamma, flags, denoised, temporal, bloom, auto_exposure)
        if not d_u8 and not d_f32:
            raise ValueError("both outputs are None")
        if int(flags) & L.RT_FLAG_U8_HWC and d_f32:
            raise ValueError("RT_FLAG_U8_HWC is a uint8 layout: resolve the float32 frame in a separate call")
        self._resolve_call(state, d_u8, d_f32, exposure=exposure, white=white, gamma=gamma, flags=flags, out_stride=out_stride, stream=stream)

    def resolve(self, exposure=1.0, white=0.0, gamma=1, u8=True, f32=False, flags=0, denoised=False, temporal=False, bloom=False,
                auto_exposure=False):
        """Film.resolve of the lifted picture: (uint8 or None, float32 or None) host arrays (3, w, h), or (h, w, 3) for the uint8
        frame with RT_FLAG_U8_HWC.  Waits for the context's stream."""
        state = self._request(exposure, white, gamma, flags, denoised, temporal, bloom, auto_exposure)
        if not u8 and not f32:
            raise ValueError("neither u8 nor f32 is asked for")
        r, n = self.renderer, self.w * self.h
        hwc = bool(int(flags) & L.RT_FLAG_U8_HWC)
        out8 = np.empty((self.h, self.w, 3) if hwc else (3, self.w, self.h), np.uint8) if u8 else None
        out32 = np.empty((3, self.w, self.h), np.float32) if f32 else None
        d8 = r.malloc(3 * n) if u8 else None
        d32 = r.malloc(12 * n) if f32 else None
        try:
            tone = dict(exposure=exposure, white=white, gamma=gamma, out_stride=None, stream=None)
            if hwc:                                             # (the image layout is uint8 only: two calls)
                self._resolve_call(state, d8, None, flags=flags, **tone)
                if f32:
                    self._resolve_call(state, None, d32, flags=int(flags) & ~L.RT_FLAG_U8_HWC, **tone)
            else:
                self._resolve_call(state, d8, d32, flags=flags, **tone)
            if u8:
                r.d2h(out8, d8)
            if f32:
                r.d2h(out32, d32)
        finally:
            for d in (d8, d32):
                if d:
                    r.free(d)
        return out8, out32
