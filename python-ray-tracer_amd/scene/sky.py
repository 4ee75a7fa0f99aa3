"""The sky: the colour of a ray that hits nothing, a gradient with a sun disc and a halo around it
(include/mi355rt.h: rt_set_scene_sky).  sky_color() is the arithmetic of the header, word for word, in numpy float64; the kernel
(rt_device.h: sky_color) must agree with it bit for bit."""
import math
from dataclasses import dataclass

import numpy as np

RT_SKY_DOUBLES = 24
SHARPNESS = (1, 2, 4, 8, 16)
HALO_SHININESS = tuple(1 << i for i in range(11))    # 1, 2, 4, ..., 1024
# offsets in the packed sky
UP, ZENITH, HORIZON, NADIR, SHARP, SUN_DIR, SUN_COS, SUN_RGB, HALO_RGB, HALO_SHIN = 0, 3, 6, 9, 12, 13, 16, 17, 20, 23
COLOURS = (ZENITH, HORIZON, NADIR, SUN_RGB, HALO_RGB)


def _squarings(v, allowed, what):
    f = float(v)
    for i, a in enumerate(allowed):
        if f == float(a):
            return i
    raise ValueError(f"{what} must be one of {', '.join(str(a) for a in allowed)}, got {v}")


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def check_packed(packed):
    """The (24,) float64 array of a packed sky; ValueError for what rt_set_scene_sky refuses in it."""
    k = np.asarray(packed, dtype=np.float64).reshape(-1)
    if k.shape[0] != RT_SKY_DOUBLES:
        raise ValueError(f"a packed sky has {RT_SKY_DOUBLES} doubles, got {k.shape[0]}")
    if not np.isfinite(k).all():
        raise ValueError("every component of a sky must be finite")
    for c in COLOURS:
        if (k[c:c + 3] < 0.0).any():
            raise ValueError("a sky's colours must be >= 0")
    for v, name in ((UP, "up"), (SUN_DIR, "sun_dir")):
        n2 = k[v] * k[v] + k[v + 1] * k[v + 1] + k[v + 2] * k[v + 2]
        if not (1.0 - 1e-6 <= n2 <= 1.0 + 1e-6):
            raise ValueError(f"{name} must be a unit vector, |{name}|^2 = {n2}")
    _squarings(k[SHARP], SHARPNESS, "sharp")
    _squarings(k[HALO_SHIN], HALO_SHININESS, "halo_shin")
    return k


def has_sky(packed):
    """Whether a packed sky is one: some component of its five colours is not zero."""
    k = np.asarray(packed, dtype=np.float64).reshape(-1)
    return any((k[c:c + 3] != 0.0).any() for c in COLOURS)


def sky_color(d, packed):
    """sky(d) for directions d (..., 3) float64 and a packed sky: (..., 3) float64.  float64, no fused multiply-add, in this
    order, per channel c:
        h   = dot(d, up)
        a   = h < 0 ? -h : h;   t = a > 1 ? 1 : a;   far = h < 0 ? nadir : zenith      (h = -0.0 takes zenith with t = 0)
        sharp = 2^j, j > 0:     q = 1 - t;  j times q = q * q;  t = 1 - q               (j = 0: t as it is)
        g_c = horizon_c + (t * (far_c - horizon_c))
        s   = dot(d, sun_dir)
        s > 0:          q = s;  log2(halo_shin) times q = q * q;   g_c = g_c + (halo_c * q)
        s >= sun_cos:   g_c = g_c + sun_c"""
    k = check_packed(packed)
    d = np.asarray(d, dtype=np.float64)
    dv = (d[..., 0], d[..., 1], d[..., 2])
    jsharp = _squarings(k[SHARP], SHARPNESS, "sharp")
    jhalo = _squarings(k[HALO_SHIN], HALO_SHININESS, "halo_shin")
    out = np.empty(d.shape, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        h = _dot(dv, k[UP:UP + 3])
        below = h < 0.0
        a = np.where(below, -h, h)
        t = np.where(a > 1.0, 1.0, a)
        if jsharp > 0:
            q = 1.0 - t
            for _ in range(jsharp):
                q = q * q
            t = 1.0 - q
        s = _dot(dv, k[SUN_DIR:SUN_DIR + 3])
        q = s
        for _ in range(jhalo):
            q = q * q
        for c in range(3):
            far = np.where(below, k[NADIR + c] - k[HORIZON + c], k[ZENITH + c] - k[HORIZON + c])
            g = k[HORIZON + c] + (t * far)
            g = np.where(s > 0.0, g + (k[HALO_RGB + c] * q), g)
            g = np.where(s >= k[SUN_COS], g + k[SUN_RGB + c], g)
            out[..., c] = g
    return out


def _unit(v, name):
    v = np.asarray(v, dtype=np.float64)
    if v.shape != (3,) or not np.isfinite(v).all():
        raise ValueError(f"{name} must have three finite components, got {v!r}")
    n = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if not n > 0.0:
        raise ValueError(f"{name} must not be the zero vector")
    return v / n


def _colour(v, name):
    v = np.asarray(v, dtype=np.float64)
    if v.shape != (3,) or not (np.isfinite(v).all() and (v >= 0.0).all()):
        raise ValueError(f"{name} must have three finite components >= 0, got {v!r}")
    return v


@dataclass(frozen=True)
class Sky:
    """What a ray that hits nothing sees (include/mi355rt.h: rt_set_scene_sky).  zenith, horizon and nadir (default: the
    horizon's colour) are RGB in colour units (the 0..255 scale of the objects' colours): the sky is `horizon` where a direction
    is perpendicular to `up` and goes to `zenith` (above) or `nadir` (below), the faster the larger `sharpness` (1, 2, 4, 8, 16).
    sun_direction (None: no sun) points at the sun, a disc of angular radius sun_angle_deg of colour sun_color added to the
    gradient, inside a glow of colour halo_color that falls off as cos^halo_shininess (1, 2, 4, ..., 1024) of the angle from
    the sun.  The sky gives no light: see sun_light()."""
    zenith: object
    horizon: object
    nadir: object = None
    up: object = (0.0, 0.0, 1.0)
    sharpness: int = 1
    sun_direction: object = None
    sun_angle_deg: float = 2.0
    sun_color: object = (255.0, 255.0, 255.0)
    halo_color: object = (0.0, 0.0, 0.0)
    halo_shininess: int = 64

    def __post_init__(self):
        self.pack()

    def pack(self):
        """float64 (24,): the sky as rt_set_scene_sky takes it; up and sun_direction normalised in float64."""
        k = np.zeros(RT_SKY_DOUBLES, dtype=np.float64)
        k[UP:UP + 3] = _unit(self.up, "up")
        k[ZENITH:ZENITH + 3] = _colour(self.zenith, "zenith")
        k[HORIZON:HORIZON + 3] = _colour(self.horizon, "horizon")
        k[NADIR:NADIR + 3] = _colour(self.horizon if self.nadir is None else self.nadir, "nadir")
        k[SHARP] = float(1 << _squarings(self.sharpness, SHARPNESS, "sharpness"))
        k[HALO_SHIN] = float(1 << _squarings(self.halo_shininess, HALO_SHININESS, "halo_shininess"))
        if self.sun_direction is None:                          # no sun: no disc (sun_cos > 1) and no halo
            k[SUN_DIR:SUN_DIR + 3] = k[UP:UP + 3]
            k[SUN_COS] = 2.0
        else:
            ang = float(self.sun_angle_deg)
            if not (math.isfinite(ang) and 0.0 <= ang <= 180.0):
                raise ValueError(f"sun_angle_deg must be in [0, 180], got {self.sun_angle_deg}")
            k[SUN_DIR:SUN_DIR + 3] = _unit(self.sun_direction, "sun_direction")
            k[SUN_COS] = math.cos(math.radians(ang))
            k[SUN_RGB:SUN_RGB + 3] = _colour(self.sun_color, "sun_color")
            k[HALO_RGB:HALO_RGB + 3] = _colour(self.halo_color, "halo_color")
        return check_packed(k)

    def color(self, d):
        """sky_color(d, self.pack())."""
        return sky_color(d, self.pack())

    def sun_light(self, distance, radius=0.0):
        """A Light of the sun's colour (sun_color / 255 as the light's colour, strength 1) at `distance` along sun_direction
        from the world origin: the sky itself lights nothing."""
        from .scene import Light
        if self.sun_direction is None:
            raise ValueError("this sky has no sun")
        k = self.pack()
        return Light(k[SUN_DIR:SUN_DIR + 3] * float(distance), radius, tuple(k[SUN_RGB:SUN_RGB + 3] / 255.0), 1.0)
