"""Scene description -> the float32 arrays the kernel consumes, reference scene/scene.py:9-115:
spheres (7,S) rows cx,cy,cz,r,R,G,B; lights (3,L); planes (9,P) rows ox,oy,oz,nx,ny,nz,R,G,B with the
normal normalised in float64 before the float32 store (scene.py:50).
Per-object materials (not in the reference, whose README lists them as a to-do) are an optional `material=` of a sphere or
plane; Scene.generate_materials() turns them into the table and ids of Renderer.set_scene(..., materials=...)."""
from dataclasses import dataclass
from typing import ClassVar, List, Optional

import numpy as np

from .colors import RED, BLUE, MAGENTA, YELLOW, GREEN, GREY
from .texture import Texture, RT_MAX_TEXTURES, RT_MAX_TEXELS
from .lighting import squarings


@dataclass(frozen=True)
class Material:
    """Shading coefficients of one object: the reference's ambient_int, lambert_int and reflection_int (trace.py:44, :115),
    per object instead of per frame.  float64; any finite value.
    transparency > 0 makes the object transparent: the ray continues through it (refracted by a sphere with index of
    refraction `ior`, straight through a plane) with weight `transparency` instead of being reflected; such a material must
    have refl == 0.  transparency finite and >= 0, ior finite and > 0 (include/mi355rt.h: rt_set_scene_materials_ex).
    roughness > 0 makes the reflection rough: the reflected ray is scattered around the mirror direction by up to `roughness`
    (a "fuzzy metal"), reproducibly per sample and seed; finite and in [0, 1], and 0 for a transparent material
    (include/mi355rt.h: rt_set_scene_materials_scatter).
    specular > 0 gives the object a Blinn-Phong highlight in the lights' colours: its strength in colour units (the 0..255 scale
    of the objects' colours), finite and >= 0; shininess is the exponent, one of 1, 2, 4, ..., 1024
    (include/mi355rt.h: rt_set_scene_lighting)."""
    amb: float
    lamb: float
    refl: float
    transparency: float = 0.0
    ior: float = 1.0
    roughness: float = 0.0
    specular: float = 0.0
    shininess: int = 1

    def __post_init__(self):
        # (amb, lamb and refl are checked where the table is set, as before: rt_set_scene_materials refuses non-finite ones)
        if not (np.isfinite(float(self.transparency)) and float(self.transparency) >= 0.0):
            raise ValueError(f"transparency must be finite and >= 0, got {self.transparency}")
        if not (np.isfinite(float(self.ior)) and float(self.ior) > 0.0):
            raise ValueError(f"ior must be finite and > 0, got {self.ior}")
        if float(self.transparency) > 0.0 and float(self.refl) != 0.0:
            raise ValueError("a transparent material (transparency > 0) must have refl == 0")
        if not (np.isfinite(float(self.roughness)) and 0.0 <= float(self.roughness) <= 1.0):
            raise ValueError(f"roughness must be finite and in [0, 1], got {self.roughness}")
        if float(self.transparency) > 0.0 and float(self.roughness) > 0.0:
            raise ValueError("a transparent material (transparency > 0) cannot be rough (roughness > 0)")
        if not (np.isfinite(float(self.specular)) and float(self.specular) >= 0.0):
            raise ValueError(f"specular must be finite and >= 0, got {self.specular}")
        squarings(self.shininess)                                 # (ValueError unless one of 1, 2, 4, ..., 1024)

    @property
    def transparent(self):
        return float(self.transparency) > 0.0

    def key(self):
        return (float(self.amb), float(self.lamb), float(self.refl))

    @property
    def rough(self):
        return float(self.roughness) > 0.0

    def key5(self):
        return (float(self.amb), float(self.lamb), float(self.refl), float(self.transparency), float(self.ior))

    def key6(self):
        return self.key5() + (float(self.roughness),)

    @property
    def glossy(self):
        return float(self.specular) > 0.0

    def key8(self):
        return self.key6() + (float(self.specular), float(self.shininess))


@dataclass
class Sphere:
    origin: object
    radius: float
    color: object
    material: Optional[Material] = None
    texture: Optional[Texture] = None
    data_length: ClassVar[int] = 7

    def to_array(self):
        return np.concatenate([np.asarray(self.origin, dtype=np.float64), [self.radius],
                               np.asarray(self.color, dtype=np.float64)]).astype(np.float32)


@dataclass
class Light:
    """A light at `origin`.  radius > 0 makes it an area light, a ball of that radius: shadows from it are soft (penumbrae),
    sampled at Renderer.set_scene's shadow_samples points per light (include/mi355rt.h: rt_set_scene_area_lights).  The radius
    is float32, finite and >= 0; 0 (the default) is the reference's point light.
    color (three components) times intensity is the light's colour and strength e, float32, every component finite and >= 0;
    the default (1, 1, 1) is the reference's white light of unit strength (include/mi355rt.h: rt_set_scene_lighting)."""
    origin: object
    radius: float = 0.0
    color: object = (1.0, 1.0, 1.0)
    intensity: float = 1.0
    data_length: ClassVar[int] = 3

    def __post_init__(self):
        r = float(self.radius)
        if not (np.isfinite(r) and 0.0 <= r <= float(np.finfo(np.float32).max)):
            raise ValueError(f"light radius must be finite and >= 0, got {self.radius}")
        c = np.asarray(self.color, dtype=np.float64)
        if c.shape != (3,):
            raise ValueError(f"light color must have three components, got {self.color!r}")
        with np.errstate(over="ignore", invalid="ignore"):
            e = self.rgb()
        if not (np.isfinite(e).all() and (e >= 0.0).all()):
            raise ValueError(f"light color times intensity must be finite and >= 0, got {self.color!r} x {self.intensity}")

    def rgb(self):
        """e = float32(intensity * color), (3,)."""
        return (float(self.intensity) * np.asarray(self.color, dtype=np.float64)).astype(np.float32)

    def to_array(self):
        return np.asarray(self.origin, dtype=np.float64).astype(np.float32)


@dataclass
class Plane:
    origin: object
    normal: object
    color: object
    material: Optional[Material] = None
    texture: Optional[Texture] = None
    data_length: ClassVar[int] = 9

    def to_array(self):
        n = np.array(self.normal)
        return np.concatenate([np.asarray(self.origin, dtype=np.float64), n / np.linalg.norm(n),
                               np.asarray(self.color, dtype=np.float64)]).astype(np.float32)


def _columns(items, rows):
    out = np.zeros((rows, len(items)), dtype=np.float32)
    for i, it in enumerate(items):
        out[:, i] = it.to_array()
    return out


class Scene:
    def __init__(self, lights: List[Light], spheres: List[Sphere], planes: List[Plane], sky=None):
        self.lights, self.spheres, self.planes = lights, spheres, planes
        self.sky = sky                                  # a scene.sky.Sky, or None: a ray that hits nothing is black

    def get_spheres(self):
        return _columns(self.spheres, Sphere.data_length)

    def get_planes(self):
        return _columns(self.planes, Plane.data_length)

    def get_lights(self):
        return _columns(self.lights, Light.data_length)

    def get_light_radii(self):
        """float32 (L,): the lights' radii, for Renderer.set_scene(..., light_radius=...)."""
        return np.array([float(li.radius) for li in self.lights], dtype=np.float32)

    def get_light_colors(self):
        """float32 (L, 3): the lights' colours times strengths, for Renderer.set_scene(..., light_rgb=...)."""
        return np.array([li.rgb() for li in self.lights], dtype=np.float32).reshape(-1, 3)

    def get_sky(self):
        """float64 (24,), the packed sky for Renderer.set_scene(..., sky=...), or None for a scene without one."""
        return None if self.sky is None else self.sky.pack()

    def generate_scene(self):
        return self.get_spheres(), self.get_lights(), self.get_planes()

    def generate_materials(self, default: Material):
        """(table float64 (M,3) rows amb, lamb, refl; sphere_ids int32 (S,); plane_ids int32 (P,)) for
        Renderer.set_scene(..., materials=...).  Objects without a material get `default`; equal materials share one row,
        in the order of first use (spheres, then planes).  If any material is rough the table is (M,6), rows
        amb, lamb, refl, transparency, ior, roughness; else if any is transparent it is (M,5), the first five of those.  If any
        material has specular > 0 the table is (M,8): those six, then specular and shininess."""
        rows, index = [], {}
        mats = [o.material if o.material is not None else default for o in list(self.spheres) + list(self.planes)]
        ncols = 8 if any(m.glossy for m in mats) else 6 if any(m.rough for m in mats) else (5 if any(m.transparent for m in mats) else 3)

        def ids(objs):
            out = np.zeros(len(objs), dtype=np.int32)
            for i, o in enumerate(objs):
                m = o.material if o.material is not None else default
                k = {3: m.key, 5: m.key5, 6: m.key6, 8: m.key8}[ncols]()
                if k not in index:
                    index[k] = len(rows)
                    rows.append(k)
                out[i] = index[k]
            return out

        sphere_ids, plane_ids = ids(self.spheres), ids(self.planes)
        return np.array(rows, dtype=np.float64).reshape(-1, ncols), sphere_ids, plane_ids

    def generate_textures(self):
        """(records, sphere_ids int32 (S,), plane_ids int32 (P,), texels float32 (N, 3)) for
        Renderer.set_scene(..., textures=...).  records: a list of (origin (3,), axes (3, 3), dims (nx, ny, nz), first), one per
        distinct texture in the order of first use (spheres, then planes): equal textures share one record and its texels.
        Objects without a texture get id -1."""
        records, index, chunks, n = [], {}, [], 0

        def ids(objs):
            nonlocal n
            out = np.full(len(objs), -1, dtype=np.int32)
            for i, o in enumerate(objs):
                t = o.texture
                if t is None:
                    continue
                if not isinstance(t, Texture):
                    raise TypeError(f"texture must be a Texture, got {type(t).__name__}")
                if t not in index:
                    if len(records) >= RT_MAX_TEXTURES:
                        raise ValueError(f"a scene holds at most {RT_MAX_TEXTURES} textures")
                    index[t] = len(records)
                    records.append((t.origin.copy(), t.axes.copy(), t.dims, n))
                    chunks.append(t.texels.reshape(-1, 3))
                    n += chunks[-1].shape[0]
                    if n > RT_MAX_TEXELS:
                        raise ValueError(f"a scene holds at most {RT_MAX_TEXELS} texels")
                out[i] = index[t]
            return out

        sphere_ids, plane_ids = ids(self.spheres), ids(self.planes)
        texels = np.concatenate(chunks).astype(np.float32) if chunks else np.zeros((0, 3), dtype=np.float32)
        return records, sphere_ids, plane_ids, texels

    @staticmethod
    def default_scene():
        """The reference's built-in scene (scene.py:99-115): 3 lights, 6 spheres, 1 ground plane."""
        lights = [Light(p) for p in ([2.5, -2.0, 3.0], [2.5, 2.0, 3.0], [5.0, 0.1, 6.0])]
        spheres = [Sphere(o, r, c) for o, r, c in (([2.2, 0.3, 1.0], 1.0, RED), ([0.6, 0.7, 0.4], 0.4, BLUE),
                                                    ([0.6, -0.8, 0.5], 0.5, YELLOW), ([-1.2, 0.2, 0.5], 0.5, MAGENTA),
                                                    ([-1.7, -0.5, 0.3], 0.3, GREEN), ([-2.0, 1.31, 1.3], 1.3, RED))]
        return Scene(lights, spheres, [Plane([5, 0, 0], [0, 0, 1], GREY)])
