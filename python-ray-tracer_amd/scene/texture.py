"""Textures: a wrapped, nearest-neighbour grid of texels projected along up to three world-space axes
(include/mi355rt.h: rt_set_scene_textures).  A hit object with a texture takes its colour from the texel at the hit
point.  texel_index() is the arithmetic of the header, word for word, in numpy float64 and integers; the kernel
(rt_device.h: texel_of) must agree with it bit for bit."""
import numpy as np

RT_MAX_TEXTURES = 64
RT_MAX_TEXTURE_DIM = 4096
RT_MAX_TEXELS = 1 << 22


def texel_coords(points, origin, axes, dims):
    """The grid coordinates g of texel_index(), a list of three float64 arrays of shape points.shape[:-1]; NaN for an axis
    with dim == 1 (not evaluated)."""
    p = np.asarray(points, dtype=np.float64)
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    ax = np.asarray(axes, dtype=np.float64).reshape(3, 3)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        d = (p[..., 0] - o[0], p[..., 1] - o[1], p[..., 2] - o[2])
        for a in range(3):
            if int(dims[a]) == 1:
                out.append(np.full(p.shape[:-1], np.nan))
            else:
                out.append(((d[0] * ax[a, 0]) + (d[1] * ax[a, 1])) + (d[2] * ax[a, 2]))
    return out


def texel_index(points, origin, axes, dims, first=0):
    """Index into the texel array of the texel that colours each hit point.
    points (..., 3) float64 unbiased hit points Pt; origin (3,); axes (3, 3) rows U, V, W; dims (nx, ny, nz).
    float64, no fused multiply-add, in this order:
      for a = 0..2 with dim[a] > 1:
          d   = (Pt.x - origin.x, Pt.y - origin.y, Pt.z - origin.z)
          g   = ((d.x * axis[a][0]) + (d.y * axis[a][1])) + (d.z * axis[a][2])
          f   = floor(g)
          i_a = -2^30 if f is NaN or f < -2^30;  2^30 - 1 if f > 2^30 - 1;  else (integer) f
          j_a = i_a mod dim[a], Euclidean (0 <= j_a < dim[a])
      for an axis with dim[a] == 1:  j_a = 0, and g is not evaluated
      texel index = first + (j_2 * ny + j_1) * nx + j_0
    Returns int64 of shape points.shape[:-1]."""
    n = [int(v) for v in dims]
    g = texel_coords(points, origin, axes, dims)
    j = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            if n[a] == 1:
                j.append(np.zeros(g[a].shape, dtype=np.int64))
                continue
            f = np.floor(g[a])
            low = np.isnan(f) | (f < -2.0 ** 30)
            high = f > 2.0 ** 30 - 1
            i = np.where(low, -2 ** 30, np.where(high, 2 ** 30 - 1, np.where(low | high, 0.0, f).astype(np.int64)))
            j.append(np.mod(i.astype(np.int64), n[a]))
    return np.int64(first) + (j[2] * n[1] + j[1]) * n[0] + j[0]


def _vec3(v, name):
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError(f"{name} must be three finite numbers, got {v!r}")
    return a


class Texture:
    """A grid of texels in world space.  origin: the world point of grid coordinate (0, 0, 0); axes (3, 3): rows U, V, W, grid
    cells per world unit along each grid axis; texels float32 (nz, ny, nx, 3), true (R, G, B), finite.  The grid repeats
    in every direction; lookups are nearest-neighbour (texel_index)."""

    def __init__(self, origin, axes, texels):
        self.origin = _vec3(origin, "origin")
        ax = np.asarray(axes, dtype=np.float64)
        if ax.shape != (3, 3) or not np.isfinite(ax).all():
            raise ValueError(f"axes must be a finite (3, 3) array, got shape {ax.shape}")
        self.axes = ax.copy()
        t = np.ascontiguousarray(texels, dtype=np.float32)
        if t.ndim != 4 or t.shape[3] != 3:
            raise ValueError(f"texels must have shape (nz, ny, nx, 3), got {t.shape}")
        if min(t.shape[:3]) < 1 or max(t.shape[:3]) > RT_MAX_TEXTURE_DIM:
            raise ValueError(f"texture dimensions must be 1..{RT_MAX_TEXTURE_DIM}, got {t.shape[2]} x {t.shape[1]} x {t.shape[0]}")
        if t.shape[0] * t.shape[1] * t.shape[2] > RT_MAX_TEXELS:
            raise ValueError(f"a texture holds at most {RT_MAX_TEXELS} texels")
        if not np.isfinite(t).all():
            raise ValueError("texels must be finite")
        self.texels = t

    @property
    def dims(self):
        """(nx, ny, nz)"""
        return (self.texels.shape[2], self.texels.shape[1], self.texels.shape[0])

    def key(self):
        return (self.origin.tobytes(), self.axes.tobytes(), self.texels.shape, self.texels.tobytes())

    def __eq__(self, other):
        return isinstance(other, Texture) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def color_at(self, points):
        """float32 (..., 3): the texel colours at world points (the lookup of texel_index)."""
        idx = texel_index(points, self.origin, self.axes, self.dims)
        return self.texels.reshape(-1, 3)[idx]

    @staticmethod
    def _unit_axes(size, axes):
        s = float(size)
        if not (np.isfinite(s) and s > 0.0):
            raise ValueError(f"size must be finite and > 0, got {size!r}")
        ax = np.asarray(axes, dtype=np.float64)
        if ax.shape != (3, 3):
            raise ValueError("axes must have shape (3, 3)")
        return ax / s

    @classmethod
    def checker(cls, color_a, color_b, size, origin=(0.0, 0.0, 0.0), axes=((1, 0, 0), (0, 1, 0), (0, 0, 1)), solid=False):
        """Squares (solid=True: cubes) of edge `size` world units alternating between two colours, along the first two
        (three) of `axes` (unit vectors by default: a floor z = const gets a checkerboard in x and y)."""
        a, b = _vec3(color_a, "color_a"), _vec3(color_b, "color_b")
        nz = 2 if solid else 1
        t = np.empty((nz, 2, 2, 3), dtype=np.float32)
        for z in range(nz):
            for y in range(2):
                for x in range(2):
                    t[z, y, x] = a if (x + y + z) % 2 == 0 else b
        return cls(origin, cls._unit_axes(size, axes), t)

    @classmethod
    def stripes(cls, color_a, color_b, size, origin=(0.0, 0.0, 0.0), axis=(1, 0, 0)):
        """Bands of width `size` world units alternating between two colours along `axis`."""
        a, b = _vec3(color_a, "color_a"), _vec3(color_b, "color_b")
        t = np.stack([a, b]).astype(np.float32).reshape(1, 1, 2, 3)
        ax = np.zeros((3, 3))
        ax[0] = _vec3(axis, "axis")
        return cls(origin, cls._unit_axes(size, ax), t)

    @classmethod
    def image(cls, array_hw3, origin, u_edge, v_edge):
        """An image (H, W, 3), row 0 first, spanning the parallelogram origin, origin + u_edge, origin + v_edge once (columns
        along u_edge, rows along v_edge), then repeating.  Axis U is the vector with U.u_edge = W and U.v_edge = 0 in the
        plane of the two edges (V likewise with H), so that the grid coordinate runs 0..W along u_edge."""
        img = np.asarray(array_hw3, dtype=np.float32)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"image must have shape (H, W, 3), got {img.shape}")
        u, v = _vec3(u_edge, "u_edge"), _vec3(v_edge, "v_edge")
        uu, uv, vv = float(u @ u), float(u @ v), float(v @ v)
        det = uu * vv - uv * uv
        if not det > 0.0:
            raise ValueError("u_edge and v_edge must span a parallelogram")
        ax = np.zeros((3, 3))
        ax[0] = (vv * u - uv * v) / det * img.shape[1]          # the dual basis of (u, v), scaled to cells
        ax[1] = (uu * v - uv * u) / det * img.shape[0]
        return cls(origin, ax, img.reshape(1, img.shape[0], img.shape[1], 3))
