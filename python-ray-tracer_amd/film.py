"""Film — passes accumulated in device memory and resolved to a frame there (rt_film_accumulate, rt_film_resolve of
include/mi355rt.h), and the numpy restatement of their arithmetic: accumulate_reference, tone_reference and clip_reference are
the contract's second statement, as scene.texel_index, light_terms and sky_color are.

    with Film(renderer) as film:
        film.accumulate(params, passes=64)            # seeds params.seed, params.seed + 1, ...
        image, _ = film.resolve(white=400.0, gamma=2, flags=RT_FLAG_U8_HWC | RT_FLAG_U8_RGB)

Film.guides, Film.denoise and resolve(denoised=True) put the denoiser behind the same object (rt_render_guides, rt_film_denoise;
their arithmetic in numpy is in denoise.py):

        film.accumulate(params, passes=4)
        film.denoise()                                # first-hit guides, then the edge-stopping filter on the mean
        image, _ = film.resolve(white=400.0, denoised=True)
"""
import numpy as np

from . import _lib as L
from .denoise import check_denoise

# Film.denoise's default sigma, in the units the filter sees: colour / albedo with demodulation, so about 0..1 and not 0..255.  The
# best of the sweep 1/32, 1/16, 1/8, 1/4, 1/2 at levels 4, normal_shininess 32 with demodulation on four passes of the
# soft_default_64_d4 scene (one shadow sample) against its 1024-pass mean (Denoiser)
DENOISE_SIGMA = 0.125

_TONE_FLAGS = L.RT_FLAG_U8_RGB | L.RT_FLAG_U8_HWC


def accumulate_reference(total, frames):
    """The sum rule of rt_film_accumulate in numpy.  total: float64 (3, ws, h) or None (reset: start from +0.0); frames: an iterable
    of float32 (3, ws, h) pass frames, in pass order.  Per element, float64, in this order:
        s = reset ? +0.0 : sum[e];   for i in 0..passes-1:  s = s + (double)f_i[e];   sum[e] = s
    Returns a new float64 array."""
    s = None if total is None else np.array(total, dtype=np.float64)
    for f in frames:
        f = np.asarray(f)
        if f.dtype != np.float32:
            raise ValueError(f"pass frames are float32, not {f.dtype}")
        if s is None:
            s = np.zeros(f.shape, np.float64)
        with np.errstate(all="ignore"):
            s = s + f.astype(np.float64)
    if s is None:
        raise ValueError("no sum and no pass frame")
    return s


def tone_reference(total, n, exposure=1.0, white=0.0, gamma=1):
    """The display values v of rt_film_resolve in numpy: float64, the shape of `total`.  Per element, float64, no fused
    multiply-add, in this order, with s the sum:
        v = (s / (double)n) * exposure
        white > 0:   wn = white / 255.0 (once);  x = v / 255.0;
                     x > 0:  y = (x * (1.0 + x / (wn*wn))) / (1.0 + x);  v = y * 255.0      (x <= 0 or NaN: v unchanged)
        gamma == 2:  t = v / 255.0;   t > 0:  v = sqrt(t) * 255.0                           (t <= 0 or NaN: v unchanged)
    The float32 output of a resolve is v.astype(float32), the uint8 output clip_reference(v)."""
    n, exposure, white, gamma = check_tone(n, exposure, white, gamma)
    s = np.asarray(total, dtype=np.float64)
    with np.errstate(all="ignore"):
        v = (s / np.float64(n)) * np.float64(exposure)
        if white > 0.0:
            wn = np.float64(white) / np.float64(255.0)
            wn2 = wn * wn
            x = v / 255.0
            y = (x * (1.0 + x / wn2)) / (1.0 + x)
            v = np.where(x > 0.0, y * 255.0, v)
        if gamma == 2:
            t = v / 255.0
            v = np.where(t > 0.0, np.sqrt(np.where(t > 0.0, t, 0.0)) * 255.0, v)
    return v


def clip_reference(v):
    """clip_color of rt_device.h (common.py:52-57) for float64 values: NaN -> 0, round half to even, clamp to 0..255; uint8."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.rint(np.clip(np.where(np.isnan(v), 0.0, v), -1.0, 256.0))
    return np.clip(r, 0.0, 255.0).astype(np.uint8)


def check_tone(n, exposure, white, gamma, flags=0):
    """(n, exposure, white, gamma) as Python numbers, or ValueError: what rt_film_resolve would refuse."""
    n, exposure, white = int(n), float(exposure), float(white)
    if n < 1:
        raise ValueError(f"n must be >= 1 (the number of passes accumulated), not {n}")
    if not (np.isfinite(exposure) and exposure > 0.0):
        raise ValueError(f"exposure must be finite and > 0, not {exposure!r}")
    if not (white == 0.0 or (np.isfinite(white) and white > 0.0)):
        raise ValueError(f"white must be 0 (no compression), or finite and > 0, not {white!r}")
    if gamma not in (1, 2):
        raise ValueError(f"gamma must be 1 or 2, not {gamma!r}")
    if int(flags) & ~_TONE_FLAGS:
        raise ValueError(f"flags may hold RT_FLAG_U8_RGB and RT_FLAG_U8_HWC only, not {int(flags):#x}")
    return n, exposure, white, int(gamma)


class Film:
    """A float64 (3, x1-x0, h) sum of pass frames in the renderer's device memory, and how many passes it holds.  The frame size is
    the renderer's at construction (set_raygen / set_pixel_loc first)."""

    def __init__(self, renderer, x0=0, x1=None):
        w, h = getattr(renderer, "w", None), getattr(renderer, "h", None)
        if not w or not h:
            raise ValueError("the renderer has no ray grid yet: call set_raygen or set_pixel_loc before making a Film")
        x0 = int(x0)
        x1 = int(w) if x1 is None else int(x1)
        if not 0 <= x0 < x1 <= w:
            raise ValueError(f"column range must satisfy 0 <= x0 < x1 <= w = {w}, not [{x0}, {x1})")
        if (x1 - x0) * h > L.RT_FILM_MAX_PIXELS:
            raise ValueError(f"a film holds at most RT_FILM_MAX_PIXELS = 2^27 pixels, not {(x1 - x0) * h}")
        self.renderer, self.x0, self.x1, self.h = renderer, x0, x1, int(h)
        self.ws = x1 - x0
        self.passes = 0
        self.d_sum = renderer.malloc(24 * self.ws * self.h)
        self.d_guides = self.d_denoised = self.d_work = None      # allocated by guides() and denoise()
        self.denoised_passes = 0                                  # the pass count the filtered mean in d_denoised belongs to (0: none)

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        d, self.d_sum = getattr(self, "d_sum", None), None
        extra = [getattr(self, n, None) for n in ("d_guides", "d_denoised", "d_work")]
        self.d_guides = self.d_denoised = self.d_work = None
        for e in extra + [d]:
            if e and not self.renderer.closed:
                self.renderer.free(e)

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
        if not self.d_sum:
            raise ValueError("the film is closed")

    # -- passes -----------------------------------------------------------------------------
    def accumulate(self, params, passes=1, stream=None):
        """`passes` more passes of `params` (Renderer.params(...)): pass i is rendered with seed params.seed + i.  A caller who
        refines a picture advances params.seed by `passes` between calls.  Asynchronous."""
        self._live()
        passes = int(passes)
        if passes < 1:
            raise ValueError(f"passes must be >= 1, not {passes}")
        if self.renderer.h != self.h or self.x1 > (self.renderer.w or 0):
            raise ValueError(f"the renderer's frame is now {self.renderer.w} x {self.renderer.h}; the film holds columns "
                             f"[{self.x0}, {self.x1}) of height {self.h}")
        self.renderer.film_accumulate(params, self.x0, self.x1, passes, self.passes == 0, self.d_sum, self.ws * self.h, stream)
        self.passes += passes

    def clear(self):
        """Forget every pass: the next accumulate starts from zero.  The guides stay (they do not depend on the passes)."""
        self.passes = 0
        self.denoised_passes = 0

    # -- the denoiser -----------------------------------------------------------------------
    def guides(self, stream=None):
        """Render the first-hit guides of the film's slab (Renderer.render_guides) with the renderer's current scene, camera and
        grid, keep them on the device for denoise(), and return them: float32 (8, ws, h).  clear() does not drop them; a scene,
        camera or grid change is the caller's cue to call this again.  Waits for the stream."""
        self._live()
        if self.renderer.h != self.h or self.x1 > (self.renderer.w or 0):
            raise ValueError(f"the renderer's frame is now {self.renderer.w} x {self.renderer.h}; the film holds columns "
                             f"[{self.x0}, {self.x1}) of height {self.h}")
        r, n = self.renderer, self.ws * self.h
        if not self.d_guides:
            self.d_guides = r.malloc(4 * L.RT_GUIDE_PLANES * n)
        r.render_guides(self.x0, self.x1, self.d_guides, n, stream)
        r.sync(stream)
        out = np.empty((L.RT_GUIDE_PLANES, self.ws, self.h), np.float32)
        r.d2h(out, self.d_guides)
        return out

    def denoise(self, levels=4, normal_shininess=32, sigma=DENOISE_SIGMA, demodulate=True, stream=None):
        """Filter the mean of the passes so far (Renderer.film_denoise: an edge-stopping a-trous filter guided by guides(), which is
        called first if it has not been) into the film's own buffers; resolve(denoised=True) shows the result.  levels 0..6,
        normal_shininess 1, 2, 4, ..., 1024, sigma 0 (no colour weight) or > 0 in colour units, demodulate: filter colour / albedo.
        sigma is measured in what the filter sees: colour units (0..255) without demodulation, colour / albedo (about 0..1) with it.
        The default, DENOISE_SIGMA = 1/8, is the best of the sweep 1/32, 1/16, 1/8, 1/4, 1/2 recorded in DESIGN.md (Denoiser): four
        passes of the soft_default_64_d4 scene with one shadow sample against its 1024-pass mean, RMSE x0.85; the values 4 to 64
        switch the colour weight off under demodulation and make that frame worse (x2.7 to x2.9).  Asynchronous."""
        self._live()
        if self.passes < 1:
            raise ValueError("the film holds no pass yet")
        levels, shin, sigma, demodulate = check_denoise(levels, normal_shininess, sigma, demodulate)
        r, n = self.renderer, self.ws * self.h
        if not self.d_guides:
            self.guides(stream)
        if not self.d_denoised:
            self.d_denoised = r.malloc(24 * n)
        if levels >= 2 and not self.d_work:
            self.d_work = r.malloc(24 * n)
        r.film_denoise(self.d_sum, self.ws, self.h, self.passes, self.d_guides, self.d_denoised, self.d_work, levels=levels,
                       normal_shin=shin, sigma=sigma, demodulate=demodulate, stream=stream)
        self.denoised_passes = self.passes

    def _source(self, denoised):
        """(sum or filtered mean, its n) of a resolve."""
        if not denoised:
            return self.d_sum, self.passes
        if not self.denoised_passes or self.denoised_passes != self.passes:
            raise ValueError("the film has no filtered mean of its current passes: call denoise() first")
        return self.d_denoised, 1

    # -- frames -----------------------------------------------------------------------------
    def resolve_device(self, d_u8=None, d_f32=None, exposure=1.0, white=0.0, gamma=1, flags=0, out_stride=None, stream=None,
                       denoised=False):
        """The mean of the passes so far, tone-mapped, into caller-owned device memory (raw addresses), laid out as
        Renderer.render_device's outputs; denoised: the mean that denoise() filtered instead.  Asynchronous."""
        self._live()
        if self.passes < 1:
            raise ValueError("the film holds no pass yet")
        check_tone(self.passes, exposure, white, gamma, flags)
        if not d_u8 and not d_f32:
            raise ValueError("both outputs are None")
        if int(flags) & L.RT_FLAG_U8_HWC and d_f32:
            raise ValueError("RT_FLAG_U8_HWC is a uint8 layout: resolve the float32 frame in a separate call")
        src, n = self._source(denoised)
        self.renderer.film_resolve(src, self.ws, self.h, n, d_u8, d_f32, exposure=exposure, white=white, gamma=gamma,
                                   flags=flags, out_stride=out_stride, stream=stream)

    def resolve(self, exposure=1.0, white=0.0, gamma=1, u8=True, f32=False, flags=0, denoised=False):
        """(uint8 or None, float32 or None) host arrays shaped like Renderer.render's: (3, ws, h), or (h, ws, 3) for the uint8
        frame with RT_FLAG_U8_HWC; denoised: of the mean that denoise() filtered.  Waits for the context's stream."""
        self._live()
        if self.passes < 1:
            raise ValueError("the film holds no pass yet")
        check_tone(self.passes, exposure, white, gamma, flags)
        if not u8 and not f32:
            raise ValueError("neither u8 nor f32 is asked for")
        self._source(denoised)
        r, n = self.renderer, self.ws * self.h
        hwc = bool(int(flags) & L.RT_FLAG_U8_HWC)
        out8 = np.empty((self.h, self.ws, 3) if hwc else (3, self.ws, self.h), np.uint8) if u8 else None
        out32 = np.empty((3, self.ws, self.h), np.float32) if f32 else None
        d8 = r.malloc(3 * n) if u8 else None
        d32 = r.malloc(12 * n) if f32 else None
        try:
            kw = dict(exposure=exposure, white=white, gamma=gamma, denoised=denoised)
            if hwc:                                             # (the image layout is uint8 only: two calls)
                self.resolve_device(d8, None, flags=flags, **kw)
                if f32:
                    self.resolve_device(None, d32, flags=int(flags) & ~L.RT_FLAG_U8_HWC, **kw)
            else:
                self.resolve_device(d8, d32, flags=flags, **kw)
            if u8:
                r.d2h(out8, d8)
            if f32:
                r.d2h(out32, d32)
        finally:
            for d in (d8, d32):
                if d:
                    r.free(d)
        return out8, out32
