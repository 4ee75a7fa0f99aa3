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

Film.next_frame and Film.temporal carry the film through a camera move (rt_film_temporal; its arithmetic in numpy is in
temporal.py):

        for camera in orbit:
            renderer.set_camera(*camera)
            film.next_frame()                         # the latest mean becomes the history; the passes start again
            film.accumulate(params, passes=4)
            film.temporal()                           # history reprojected through the move, blended with the new passes
            film.denoise(temporal=True)
            image, _ = film.resolve(white=400.0, denoised=True, temporal=True)   # (temporal=True alone: without the filter)

Film(renderer, moments=True) keeps a sum of squares beside the sum (rt_film_accumulate_moments), and denoise(variance=True) takes
every pixel's colour tolerance from the variance of its mean (rt_film_denoise_variance; their arithmetic in numpy is in variance.py):

    with Film(renderer, moments=True) as film:
        film.accumulate(params, passes=8)
        film.denoise(variance=True)                   # no sigma to tune: the filter fades out as the film converges
        image, _ = film.resolve(white=400.0, denoised=True)
        noise = film.variance()                       # float64 (ws, h): the estimated variance of the mean, to stop refining on

On a film with moments, next_frame and temporal carry the second moment through the history beside the mean
(rt_film_temporal_moments), and denoise(variance=True, temporal=True) filters the temporal mean with a tolerance per pixel: tight
where the history survived, wide at a disocclusion (rt_film_denoise_variance_temporal).  One pass per frame is enough:

    with Film(renderer, moments=True) as film:
        for camera in orbit:
            renderer.set_camera(*camera)
            film.next_frame()
            film.accumulate(params, passes=1)
            film.temporal()
            film.denoise(variance=True, temporal=True)
            image, _ = film.resolve(white=400.0, denoised=True, temporal=True)

Film.bloom and resolve(bloom=True) add the glare of what is brighter than white before the tone curve (rt_film_bloom; its arithmetic
in numpy is in bloom.py); bloom(denoised=..., temporal=...) takes the source that resolve would show:

        film.accumulate(params, passes=64)
        film.bloom()                                  # threshold 255, strength 1/4, six scales
        image, _ = film.resolve(white=400.0, gamma=2, bloom=True)

Film.meter and resolve(auto_exposure=True) let the film look at its own picture (rt_film_meter, rt_film_meter_solve,
rt_film_resolve_metered; their arithmetic in numpy is in meter.py): a luminance histogram of the source that resolve would show, an
exposure solved from it on the device, and a resolve that multiplies it in, all on one stream without a copy to the host.  The
exposure survives next_frame() and clear(), so rate < 1 adapts along an orbit:

        film.accumulate(params, passes=16)
        film.meter(key=46.0, rate=0.25)               # the median luminance towards 18 % of 255, a quarter of the way per frame
        image, _ = film.resolve(white=400.0, gamma=2, auto_exposure=True)

A derived picture belongs to what it was made from: the temporal mean to the sum, a filtered mean to the mean it filtered, the glow
and the metering to the source they took.  The film records every write with the writes it read, and a request is refused, before
any device call, unless that chain is intact: redoing an upstream step (more passes, temporal(), denoise()) means redoing what
follows it.  Film.current(product) says whether "temporal", "denoised", "bloom" or "meter" still stands.
"""
import numpy as np

from . import _lib as L
from .bloom import LEVELS as BLOOM_LEVELS, STRENGTH as BLOOM_STRENGTH, THRESHOLD as BLOOM_THRESHOLD, check_bloom
from .denoise import check_denoise
from .meter import KEY as METER_KEY, MAX_EXPOSURE, MIN_EXPOSURE, PERCENTILE as METER_PERCENTILE, RATE as METER_RATE, check_meter
from .temporal import DEPTH_TOL, MAX_HISTORY, NORMAL_COS, check_temporal
from .variance import KAPPA, SPATIAL_BELOW, VAR_PLANES, check_denoise_variance, check_spatial_below

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


# Every device buffer a film may own: name -> (bytes per pixel, fixed bytes), in the order close() frees them (the sum last).  The
# sum, and the sum of squares of a film with moments, come with the film; every other buffer with its first use (Film._buffer)
BUFFERS = {"d_denoised_var": (8 * VAR_PLANES, 0), "d_work_var": (8 * VAR_PLANES, 0), "d_sq": (24, 0), "d_temporal": (24, 0), "d_temporal_len": (4, 0),
           "d_temporal_sq": (24, 0), "d_hist": (24, 0), "d_hist_len": (4, 0), "d_hist_sq": (24, 0), "d_hist_guides": (4 * L.RT_GUIDE_PLANES, 0),
           "d_guides": (4 * L.RT_GUIDE_PLANES, 0), "d_denoised": (24, 0), "d_work": (24, 0), "d_bloom": (24, 0),
           "d_bloom_work": (8 * L.RT_BLOOM_WORK_PLANES, 0), "d_meter_hist": (0, 8 * L.RT_METER_BINS),
           "d_meter_state": (0, 8 * L.RT_METER_STATE_DOUBLES), "d_sum": (24, 0)}

# How a product that is missing, made from something else or older than what it reads is refused: the step to run first
_REFUSALS = {"temporal": "the film has no temporal mean of its current passes: call temporal() first",
             "denoised": "the film has no filtered mean of its current passes: call denoise() first",
             "bloom": "the film has no bloom of its current passes and this source: call bloom() with the same denoised and temporal first",
             "meter": "the film has no metering of its current passes and this source: call meter() with the same denoised, temporal and bloom first"}


def products(denoised=False, temporal=False, bloom=False):
    """The products behind what resolve(denoised=..., temporal=..., bloom=...) shows, upstream first: each is made from the one
    before it, and the last is the one the request reads."""
    return ("sum",) + ("temporal",) * bool(temporal) + ("denoised",) * bool(denoised) + ("bloom",) * bool(bloom)


class Film:
    """A float64 (3, x1-x0, h) sum of pass frames in the renderer's device memory, and how many passes it holds.  The frame size is
    the renderer's at construction (set_raygen / set_pixel_loc first).  moments: the film also owns a float64 sum of the passes'
    squares, which denoise(variance=True) and variance() need."""

    def __init__(self, renderer, x0=0, x1=None, moments=False):
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
        self.moments = bool(moments)
        for name in BUFFERS:
            setattr(self, name, None)
        self._buffer("d_sum")
        if self.moments:
            self._buffer("d_sq")
        self.serial = 0                                           # counts the writes of products
        self.made = {}                                            # product -> (serial of its write, {product it read: that one's serial}, buffer name)
        self.history_camera = None                                # (origin, rotation) the history was rendered with (None: no history)
        self.guides_camera = None                                 # the camera d_guides was last rendered with by this film
        self.guides_stale = False                                 # next_frame() took the guides: d_guides holds an older frame's

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        held = [getattr(self, name, None) for name in BUFFERS]
        for name in BUFFERS:
            setattr(self, name, None)
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
        if not self.d_sum:
            raise ValueError("the film is closed")

    def _has_pass(self):
        if self.passes < 1:
            raise ValueError("the film holds no pass yet")

    def _same_frame(self):
        if self.renderer.h != self.h or self.x1 > (self.renderer.w or 0):
            raise ValueError(f"the renderer's frame is now {self.renderer.w} x {self.renderer.h}; the film holds columns "
                             f"[{self.x0}, {self.x1}) of height {self.h}")

    def _buffer(self, name):
        """The address of the device buffer `name` of BUFFERS, allocated on first use."""
        if not getattr(self, name):
            per_pixel, fixed = BUFFERS[name]
            setattr(self, name, self.renderer.malloc(per_pixel * self.ws * self.h + fixed))
        return getattr(self, name)

    # -- what was made from what ------------------------------------------------------------
    def _wrote(self, product, read=None, buffer=None):
        """Record that `product` has just been written into the buffer named `buffer`, from the product `read` as it stands now."""
        self.serial += 1
        self.made[product] = (self.serial, {read: self.made[read][0]} if read else {}, buffer)

    def _stands(self, product, reads=None):
        """`product` was made from exactly the products `reads` (None: from whatever it was), none of them has been written again
        since, and each of them stands in the same way."""
        serial, read, _ = self.made.get(product, (0, {}, None))
        return serial > 0 and (reads is None or set(read) == set(reads)) and all(
            self.made[p][0] == s and self._stands(p) for p, s in read.items())

    def current(self, product):
        """Whether "temporal", "denoised", "bloom" or "meter" is that of the film as it is: made, and nothing it was made from
        written again since (more passes, or an upstream step redone).  A render loop re-runs the stages that are not."""
        if product not in ("temporal", "denoised", "bloom", "meter"):
            raise ValueError(f"product must be 'temporal', 'denoised', 'bloom' or 'meter', not {product!r}")
        return self._stands(product)

    def _source(self, denoised=False, temporal=False, bloom=False):
        """(address, n) of what a resolve, a filter, bloom() or meter() with these flags reads: the sum of the passes, the temporal
        mean, the filtered mean of either, or one of those plus glow; ValueError, naming the step to run first, where a product on
        the way is missing, was made from something else, or is older than what it was made from."""
        chain = products(denoised, temporal, bloom)
        for read, product in zip(chain, chain[1:]):
            if not self._stands(product, (read,)):
                raise ValueError(self._refusal(product, read))
        return getattr(self, self.made[chain[-1]][2]), self.passes if chain[-1] == "sum" else 1

    def source(self, denoised=False, temporal=False, bloom=False, auto_exposure=False):
        """What resolve() with these flags would read, for a stage outside the film (upsample.Upsampler): (address, n, the serial of
        the write that made it, the meter's state for it or None); ValueError as resolve()'s where the chain is broken.  A later
        write of that source, or of anything it was made from, gives another serial."""
        self._live()
        src, n = self._source(denoised, temporal, bloom)
        return src, n, self.made[products(denoised, temporal, bloom)[-1]][0], self._metered(denoised, temporal, bloom) if auto_exposure else None

    def _refusal(self, product, read):
        """Why `product` is not there to be read as made from `read`, and the step to run first.  A filtered mean that exists says
        which of the two means it is of."""
        made = self.made.get("denoised")
        if product != "denoised" or not made:
            return _REFUSALS[product]
        if read not in made[1]:
            return ("the filtered mean is that of the plain passes: call denoise(temporal=True) first" if read == "temporal" else
                    "the filtered mean is that of the temporal mean, not of the plain passes: call denoise() first")
        return "the film has no filtered mean of its current temporal mean: call denoise(temporal=True) first" if read == "temporal" else _REFUSALS[product]

    # -- passes -----------------------------------------------------------------------------
    def accumulate(self, params, passes=1, stream=None):
        """`passes` more passes of `params` (Renderer.params(...)): pass i is rendered with seed params.seed + i.  A caller who
        refines a picture advances params.seed by `passes` between calls.  Asynchronous."""
        self._live()
        passes = int(passes)
        if passes < 1:
            raise ValueError(f"passes must be >= 1, not {passes}")
        self._same_frame()
        if self.moments:
            self.renderer.film_accumulate_moments(params, self.x0, self.x1, passes, self.passes == 0, self.d_sum, self.d_sq,
                                                  self.ws * self.h, self.ws * self.h, stream)
        else:
            self.renderer.film_accumulate(params, self.x0, self.x1, passes, self.passes == 0, self.d_sum, self.ws * self.h, stream)
        self.passes += passes
        self._wrote("sum", buffer="d_sum")

    def clear(self):
        """Forget every pass, and with them everything made from them: the next accumulate starts from zero.  The guides stay (they
        do not depend on the passes), and so does the meter's exposure (reset_meter() zeroes it)."""
        self.passes = 0
        self.made = {}

    # -- the denoiser -----------------------------------------------------------------------
    def guides(self, stream=None):
        """Render the first-hit guides of the film's slab (Renderer.render_guides) with the renderer's current scene, camera and
        grid, keep them on the device for denoise(), and return them: float32 (8, ws, h).  clear() does not drop them; a scene,
        camera or grid change is the caller's cue to call this again.  Waits for the stream."""
        self._live()
        self._same_frame()
        self._render_guides(stream)
        self.renderer.sync(stream)
        out = np.empty((L.RT_GUIDE_PLANES, self.ws, self.h), np.float32)
        self.renderer.d2h(out, self.d_guides)
        return out

    def _render_guides(self, stream=None):
        """The guides of the current scene, camera and grid into d_guides.  Asynchronous."""
        self.renderer.render_guides(self.x0, self.x1, self._buffer("d_guides"), self.ws * self.h, stream)
        self.guides_camera = getattr(self.renderer, "camera", None)
        self.guides_stale = False

    def denoise(self, levels=4, normal_shininess=32, sigma=DENOISE_SIGMA, demodulate=True, stream=None, temporal=False, variance=False,
                kappa=KAPPA, var_floor=0.0, prefilter=True, spatial_below=SPATIAL_BELOW):
        """Filter the mean of the passes so far (Renderer.film_denoise: an edge-stopping a-trous filter guided by guides(), which is
        called first if it has not been) into the film's own buffers; resolve(denoised=True) shows the result.  levels 0..6,
        normal_shininess 1, 2, 4, ..., 1024, sigma 0 (no colour weight) or > 0 in colour units, demodulate: filter colour / albedo.
        sigma is measured in what the filter sees: colour units (0..255) without demodulation, colour / albedo (about 0..1) with it.
        The default, DENOISE_SIGMA = 1/8, is the best of the sweep 1/32, 1/16, 1/8, 1/4, 1/2 recorded in DESIGN.md (Denoiser): four
        passes of the soft_default_64_d4 scene with one shadow sample against its 1024-pass mean, RMSE x0.85; the values 4 to 64
        switch the colour weight off under demodulation and make that frame worse (x2.7 to x2.9).  temporal: filter the mean that
        temporal() wrote (with n = 1) instead of the mean of the passes.
        variance: the variance-guided filter instead (Renderer.film_denoise_variance), on a film made with moments=True that holds
        at least two passes: sigma is not used; a tap's colour tolerance is kappa standard deviations of the pixel's mean (KAPPA:
        the choice of the sweep in DESIGN.md, Variance-guided denoiser) plus var_floor, with the variance smoothed over 3 x 3 pixels
        of the same object when prefilter is set.  It filters into four-plane buffers of the film's own.  With temporal=True it
        filters the temporal mean with the second moment that temporal() carried through the history
        (Renderer.film_denoise_variance_temporal): it needs temporal() of the current passes, one pass is enough, and a pixel whose
        history is shorter than spatial_below passes takes its variance from its object's neighbours in a 5 x 5 window (SPATIAL_BELOW:
        the choice of the sweep in DESIGN.md, Variance under a history).  Asynchronous."""
        self._live()
        if variance:
            return self._denoise_variance(levels, normal_shininess, kappa, var_floor, demodulate, prefilter, temporal, spatial_below, stream)
        self._has_pass()
        levels, shin, sigma, demodulate = check_denoise(levels, normal_shininess, sigma, demodulate)
        src, n_src = self._source(temporal=temporal)
        if not self.d_guides or self.guides_stale:
            self.guides(stream)
        out, work = self._buffer("d_denoised"), self._buffer("d_work") if levels >= 2 else self.d_work
        self.renderer.film_denoise(src, self.ws, self.h, n_src, self.d_guides, out, work, levels=levels, normal_shin=shin, sigma=sigma,
                                   demodulate=demodulate, stream=stream)
        self._wrote("denoised", products(temporal=temporal)[-1], "d_denoised")

    def _variance_buffers(self, temporal, d_out, d_work, stream):
        """What both variance calls need: a film with moments and, first, their own condition (two passes, or the temporal mean of
        the current passes with its second moment); then current guides, and the four-plane buffers named d_out and d_work (None:
        no work buffer), allocated on first use.  Returns their addresses."""
        if not self.moments:
            raise ValueError("the film keeps no sum of squares: make it with Film(renderer, moments=True)")
        if temporal and not (self._stands("temporal") and self.d_temporal_sq):
            raise ValueError("the film has no temporal mean of its current passes, and so no second moment of one: call temporal() first")
        if not temporal and self.passes < 2:
            raise ValueError(f"a variance needs at least 2 passes, the film holds {self.passes}")
        if not self.d_guides or self.guides_stale:
            self.guides(stream)
        return self._buffer(d_out), self._buffer(d_work) if d_work else None

    def _variance_call(self, d_out, d_work, levels, shin, kappa, var_floor, demodulate, prefilter, stream):
        """rt_film_denoise_variance on the film's sums into d_out (four planes), after what it needs is there."""
        out, work = self._variance_buffers(False, d_out, d_work, stream)
        self.renderer.film_denoise_variance(self.d_sum, self.d_sq, self.ws, self.h, self.passes, self.d_guides, out, work, levels=levels,
                                            normal_shin=shin, kappa=kappa, var_floor=var_floor, demodulate=demodulate, prefilter=prefilter,
                                            stream=stream)

    def _variance_temporal_call(self, d_out, d_work, levels, shin, kappa, var_floor, demodulate, prefilter, spatial_below, stream):
        """rt_film_denoise_variance_temporal on the temporal mean, its mean of squares and its lengths into d_out (four planes)."""
        out, work = self._variance_buffers(True, d_out, d_work, stream)
        self.renderer.film_denoise_variance_temporal(self.d_temporal, self.d_temporal_sq, self.d_temporal_len, self.ws, self.h, self.d_guides,
                                                     out, work, levels=levels, normal_shin=shin, kappa=kappa, var_floor=var_floor,
                                                     demodulate=demodulate, prefilter=prefilter, spatial_below=spatial_below, stream=stream)

    def _denoise_variance(self, levels, normal_shininess, kappa, var_floor, demodulate, prefilter, temporal, spatial_below, stream):
        levels, shin, kappa, var_floor, demodulate, prefilter = check_denoise_variance(levels, normal_shininess, kappa, var_floor, demodulate, prefilter)
        work = "d_work_var" if levels >= 1 else None
        if temporal:
            self._variance_temporal_call("d_denoised_var", work, levels, shin, kappa, var_floor, demodulate, prefilter,
                                         check_spatial_below(spatial_below), stream)
        else:
            self._variance_call("d_denoised_var", work, levels, shin, kappa, var_floor, demodulate, prefilter, stream)
        self._wrote("denoised", products(temporal=temporal)[-1], "d_denoised_var")

    def variance(self, stream=None, temporal=False, spatial_below=SPATIAL_BELOW):
        """The estimated variance of the mean of the passes so far, per pixel, summed over the channels: float64 (ws, h), plane 3 of
        the levels = 0 call of Renderer.film_denoise_variance (into the film's work buffer: a filtered mean stays).  A caller stops
        refining on it.  It needs a film made with moments=True and two passes.  temporal: the variance of the temporal mean instead
        (the levels = 0 call of Renderer.film_denoise_variance_temporal), after temporal() of the current passes; one pass is enough.
        Waits for the stream."""
        self._live()
        if temporal:
            self._variance_temporal_call("d_work_var", None, 0, 1, 0.0, 0.0, 0, 0, check_spatial_below(spatial_below), stream)
        else:
            self._variance_call("d_work_var", None, 0, 1, 0.0, 0.0, 0, 0, stream)
        r = self.renderer
        r.sync(stream)
        out = np.empty((self.ws, self.h), np.float64)
        r.d2h(out, self.d_work_var + 8 * 3 * self.ws * self.h)
        return out

    # -- bloom ------------------------------------------------------------------------------
    def bloom(self, threshold=BLOOM_THRESHOLD, strength=BLOOM_STRENGTH, levels=BLOOM_LEVELS, stream=None, denoised=False, temporal=False):
        """The mean plus the glow of what is brighter than `threshold` (Renderer.film_bloom) into the film's own buffer, which
        resolve(bloom=True) shows: the bright part of every pixel, blurred at `levels` scales (0..8) of the B3 spline, their mean
        times `strength` added in linear colour.  denoised, temporal: the source, exactly what resolve(denoised=..., temporal=...)
        would show.  The result belongs to the current passes and that source.  Asynchronous."""
        self._live()
        self._has_pass()
        threshold, strength, levels, _ = check_bloom(threshold, strength, levels)
        src, n_src = self._source(denoised, temporal)
        self.renderer.film_bloom(src, self.ws, self.h, n_src, self._buffer("d_bloom"), self._buffer("d_bloom_work"), threshold=threshold,
                                 strength=strength, levels=levels, stream=stream)
        self._wrote("bloom", products(denoised, temporal)[-1], "d_bloom")

    # -- metering ---------------------------------------------------------------------------
    def meter(self, key=METER_KEY, percentile=METER_PERCENTILE, min_exposure=MIN_EXPOSURE, max_exposure=MAX_EXPOSURE, rate=METER_RATE,
              stream=None, denoised=False, temporal=False, bloom=False):
        """Meter the source that resolve(denoised=..., temporal=..., bloom=...) would show (Renderer.film_meter: a histogram of its
        luminance, eight bins per octave over 2^-16 .. 2^24) and solve the exposure that maps the `percentile` of it to `key` colour
        units (Renderer.film_meter_solve), clamped to min_exposure .. max_exposure and moved from the exposure before by `rate`
        (1: jump; a film that has not metered yet jumps as well).  Counts and exposure stay in the film's own device buffers;
        resolve(auto_exposure=True) uses them, exposure() and histogram() read them.  The exposure survives next_frame() and clear().
        The defaults are starting points, not measurements: 46 is 18 % of 255.  Asynchronous."""
        self._live()
        self._has_pass()
        key, percentile, min_exposure, max_exposure, rate = check_meter(key, percentile, min_exposure, max_exposure, rate)
        src, n_src = self._source(denoised, temporal, bloom)
        r, new = self.renderer, not self.d_meter_state
        hist, state = self._buffer("d_meter_hist"), self._buffer("d_meter_state")
        if new:                                                   # the state starts as zeros: no history
            r.h2d(state, np.zeros(L.RT_METER_STATE_DOUBLES, np.float64))
        r.film_meter(src, self.ws, self.h, n_src, hist, reset=True, stream=stream)
        r.film_meter_solve(hist, state, key=key, percentile=percentile, min_exposure=min_exposure, max_exposure=max_exposure, rate=rate,
                           stream=stream)
        self._wrote("meter", products(denoised, temporal, bloom)[-1], "d_meter_state")

    def _metered(self, denoised, temporal, bloom):
        """d_meter_state for a resolve with auto_exposure=True, or ValueError where meter() has not run on what that resolve shows."""
        if not self._stands("meter", products(denoised, temporal, bloom)[-1:]):
            raise ValueError(_REFUSALS["meter"])
        return self.d_meter_state

    def exposure(self, stream=None):
        """The meter's state, float64 (4,): the exposure resolve(auto_exposure=True) multiplies in, the metered luminance, the
        number of pixels metered and the bin the percentile fell in; zeros before the first meter().  Waits for the stream."""
        self._live()
        out = np.zeros(L.RT_METER_STATE_DOUBLES, np.float64)
        if self.d_meter_state:
            self.renderer.sync(stream)
            self.renderer.d2h(out, self.d_meter_state)
        return out

    def histogram(self, stream=None):
        """The counts of the last meter(): uint64 (RT_METER_BINS,); meter.bin_edges() has the bins' edges.  Waits for the stream."""
        self._live()
        if not self.d_meter_hist:                                 # (meter() alone allocates it, after its checks)
            raise ValueError("the film has not metered yet: call meter() first")
        out = np.zeros(L.RT_METER_BINS, np.uint64)
        self.renderer.sync(stream)
        self.renderer.d2h(out, self.d_meter_hist)
        return out

    def reset_meter(self):
        """Forget the exposure: the next meter() jumps whatever its rate."""
        self._live()
        self.made.pop("meter", None)
        if self.d_meter_state:
            self.renderer.h2d(self.d_meter_state, np.zeros(L.RT_METER_STATE_DOUBLES, np.float64))

    # -- temporal accumulation ---------------------------------------------------------------
    def _full_frame(self):
        if self.x0 != 0 or self.x1 != self.renderer.w or self.renderer.h != self.h:
            raise ValueError(f"temporal accumulation works on the full frame: the film holds columns [{self.x0}, {self.x1}) of height "
                             f"{self.h}, the renderer's frame is {self.renderer.w} x {self.renderer.h}")

    def _temporal_call(self, hist, hist_sq, hist_len, hist_guides, camera, out, out_sq, out_len, **settings):
        """The film's sums and guides blended with a history (mean, mean of squares, lengths, guides, the camera they were rendered
        with) into out, out_sq and out_len: Renderer.film_temporal_moments on a film with moments, else Renderer.film_temporal,
        which takes neither hist_sq nor out_sq.  settings: depth_tol, normal_cos, max_history, stream."""
        r, (o, R) = self.renderer, camera
        if self.moments:
            r.film_temporal_moments(self.d_sum, self.d_sq, self.passes, self.d_guides, hist, hist_sq, hist_len, hist_guides, o, R,
                                    out, out_sq, out_len, **settings)
        else:
            r.film_temporal(self.d_sum, self.passes, self.d_guides, hist, hist_len, hist_guides, o, R, out, out_len, **settings)

    def next_frame(self, stream=None):
        """The camera has moved (call this after Renderer.set_camera): the film's latest mean becomes the history, with its length
        plane and its guides, and the passes start again (clear()).  The latest mean is what temporal() wrote for the current
        passes, or sum / passes with length passes if it has not run; the history's camera is the one its guides were rendered
        with.  A film without a pass keeps the history it has.  A film with moments keeps the second moment of the frame that ends
        as well (the mean of squares, in d_hist_sq): what temporal() wrote, or sq / passes through Renderer.film_temporal_moments.
        Asynchronous."""
        self._live()
        self._full_frame()
        if self.passes < 1:
            return
        if self._stands("temporal"):                              # the temporal buffers become the history: a swap
            self.d_hist, self.d_temporal = self.d_temporal, self.d_hist
            self.d_hist_len, self.d_temporal_len = self.d_temporal_len, self.d_hist_len
            if self.moments:
                self.d_hist_sq, self.d_temporal_sq = self.d_temporal_sq, self.d_hist_sq
        else:                                                     # the plain mean: a fresh temporal call writes sum / passes and (float)passes
            if self.guides_camera is None:
                raise ValueError("the film has no guides of the frame that ends: call guides() or temporal() before the camera moves")
            hist, hist_len, hist_sq = self._buffer("d_hist"), self._buffer("d_hist_len"), self._buffer("d_hist_sq") if self.moments else None
            # sum / passes, the length passes and with moments sq / passes: max_history 0 makes every pixel fresh, the history a placeholder
            self._temporal_call(self.d_sum, self.d_sq, self.d_guides, self.d_guides, self.guides_camera, hist, hist_sq, hist_len,
                                depth_tol=0.0, normal_cos=1.0, max_history=0.0, stream=stream)
        self.d_hist_guides, self.d_guides = self.d_guides, self.d_hist_guides
        self.history_camera, self.guides_camera = self.guides_camera, None
        self.guides_stale = True
        self.clear()

    def temporal(self, max_history=MAX_HISTORY, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS, stream=None):
        """Blend the passes so far with the history that next_frame() kept (Renderer.film_temporal), into the film's own buffers:
        the guides of the current camera are rendered first, the history is reprojected through them and every pixel whose history
        survives becomes (L * history + sum) / (L + passes) with L its history length, capped at max_history; every other pixel,
        and every pixel of a film without a history, the fresh mean sum / passes.  depth_tol: relative tolerance on the squared
        distance; normal_cos: the least cosine between the pixel's normal and a history tap's.  The defaults are the best of the
        sweep recorded in DESIGN.md (Temporal accumulation).  resolve(temporal=True) and denoise(temporal=True) take the result.
        A film with moments blends the second moment by the same lengths (Renderer.film_temporal_moments) into d_temporal_sq, which
        denoise(variance=True, temporal=True) takes.  Asynchronous."""
        self._live()
        self._has_pass()
        depth_tol, normal_cos, max_history, _ = check_temporal(depth_tol, normal_cos, max_history, self.passes)
        self._full_frame()
        r = self.renderer
        if getattr(r, "camera", None) is None:
            raise ValueError("the renderer has no camera yet: call set_camera first")
        if self.guides_camera is None or any(not np.array_equal(a, b) for a, b in zip(self.guides_camera, r.camera)):
            self._render_guides(stream)
        mean, mean_len = self._buffer("d_temporal"), self._buffer("d_temporal_len")
        out = (mean, self._buffer("d_temporal_sq") if self.moments else None, mean_len)
        kw = dict(depth_tol=depth_tol, normal_cos=normal_cos, stream=stream)
        if self.history_camera is None:                           # no history: every pixel fresh (the inputs are placeholders)
            self._temporal_call(self.d_sum, self.d_sq, self.d_guides, self.d_guides, r.camera, *out, max_history=0.0, **kw)
        else:
            self._temporal_call(self.d_hist, self.d_hist_sq, self.d_hist_len, self.d_hist_guides, self.history_camera, *out,
                                max_history=max_history, **kw)
        self._wrote("temporal", "sum", "d_temporal")

    # -- frames -----------------------------------------------------------------------------
    def _request(self, exposure, white, gamma, flags, denoised, temporal, bloom, auto_exposure):
        """What both resolves check before they touch the device, and what they then read: (source address, its n, the meter's state
        or None)."""
        self._live()
        self._has_pass()
        check_tone(self.passes, exposure, white, gamma, flags)
        return self._source(denoised, temporal, bloom) + (self._metered(denoised, temporal, bloom) if auto_exposure else None,)

    def _resolve_call(self, request, d_u8, d_f32, **tone):
        src, n, state = request
        if state:
            self.renderer.film_resolve_metered(src, self.ws, self.h, n, state, d_u8, d_f32, **tone)
        else:
            self.renderer.film_resolve(src, self.ws, self.h, n, d_u8, d_f32, **tone)

    def resolve_device(self, d_u8=None, d_f32=None, exposure=1.0, white=0.0, gamma=1, flags=0, out_stride=None, stream=None,
                       denoised=False, temporal=False, bloom=False, auto_exposure=False):
        """The mean of the passes so far, tone-mapped, into caller-owned device memory (raw addresses), laid out as
        Renderer.render_device's outputs; denoised: the mean that denoise() filtered instead; temporal: the mean that temporal()
        wrote (with denoised: its filtered version, denoise(temporal=True)); bloom: that source with the glow that bloom() added;
        auto_exposure: `exposure` times the exposure that meter() solved for that source (Renderer.film_resolve_metered).
        ValueError unless each of those was made from the film as it is now (Film.current).  Asynchronous."""
        request = self._request(exposure, white, gamma, flags, denoised, temporal, bloom, auto_exposure)
        if not d_u8 and not d_f32:
            raise ValueError("both outputs are None")
        if int(flags) & L.RT_FLAG_U8_HWC and d_f32:
            raise ValueError("RT_FLAG_U8_HWC is a uint8 layout: resolve the float32 frame in a separate call")
        self._resolve_call(request, d_u8, d_f32, exposure=exposure, white=white, gamma=gamma, flags=flags, out_stride=out_stride, stream=stream)

    def resolve(self, exposure=1.0, white=0.0, gamma=1, u8=True, f32=False, flags=0, denoised=False, temporal=False, bloom=False,
                auto_exposure=False):
        """(uint8 or None, float32 or None) host arrays shaped like Renderer.render's: (3, ws, h), or (h, ws, 3) for the uint8
        frame with RT_FLAG_U8_HWC; denoised: of the mean that denoise() filtered; temporal: of the mean that temporal() wrote; bloom: with
        the glow that bloom() added to that source; auto_exposure: with `exposure` times the exposure that meter() solved for that source
        (ValueError unless meter() ran for the current passes and the same denoised, temporal and bloom).  Waits for the context's
        stream."""
        request = self._request(exposure, white, gamma, flags, denoised, temporal, bloom, auto_exposure)
        if not u8 and not f32:
            raise ValueError("neither u8 nor f32 is asked for")
        r, n = self.renderer, self.ws * self.h
        hwc = bool(int(flags) & L.RT_FLAG_U8_HWC)
        out8 = np.empty((self.h, self.ws, 3) if hwc else (3, self.ws, self.h), np.uint8) if u8 else None
        out32 = np.empty((3, self.ws, self.h), np.float32) if f32 else None
        d8 = r.malloc(3 * n) if u8 else None
        d32 = r.malloc(12 * n) if f32 else None
        try:
            tone = dict(exposure=exposure, white=white, gamma=gamma, out_stride=None, stream=None)
            if hwc:                                             # (the image layout is uint8 only: two calls)
                self._resolve_call(request, d8, None, flags=flags, **tone)
                if f32:
                    self._resolve_call(request, None, d32, flags=int(flags) & ~L.RT_FLAG_U8_HWC, **tone)
            else:
                self._resolve_call(request, d8, d32, flags=flags, **tone)
            if u8:
                r.d2h(out8, d8)
            if f32:
                r.d2h(out32, d32)
        finally:
            for d in (d8, d32):
                if d:
                    r.free(d)
        return out8, out32
