"""Cameras, histories and frames of the temporal-accumulation tests (tests/test_temporal.py on the CPU, tests/test_gpu_temporal.py
on the device): generated from seeds, computed once and read-only.  Not a test module."""
import numpy as np

from conftest import raygen_closed_form
from test_denoise import guide_scene, guides_truth

from python_ray_tracer_amd import denoise as D, temporal as T

# (depth_tol, normal_cos, max_history) of the bit-for-bit cases: loose enough that slanted planes keep their history under the move
SETTINGS = (0.25, 0.5, 16.0)


def rotation(yaw, pitch):
    """A rotation about the camera's z axis (yaw) and then its y axis (pitch), radians."""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Rz = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    return Rz @ Ry


def moved(cam, shift=(0.05, -0.11, 0.07), yaw=0.03, pitch=-0.02):
    """The camera translated (in its own axes) and rotated: (origin (3,), rotation (3, 3))."""
    o, R = np.asarray(cam[0], np.float64).reshape(3), np.asarray(cam[1], np.float64).reshape(3, 3)
    return o + R @ np.asarray(shift, np.float64), R @ rotation(yaw, pitch)


def backward(cam):
    """The camera turned half way round: everything the other one sees lies behind it."""
    o, R = np.asarray(cam[0], np.float64).reshape(3), np.asarray(cam[1], np.float64).reshape(3, 3)
    return o, R @ rotation(np.pi, 0.0)


_FRAMES = {}


def frame(name, prev="moved"):
    """dict(w, h, raygen, cam, prev_cam, guides, hist_guides) of a stored scene seen from its own camera and, before that, from
    `prev`: "moved", "still" or "backward"."""
    key = (name, prev)
    if key not in _FRAMES:
        g, w, h, tex = guide_scene(name)
        assert tex is None
        rg = raygen_closed_form(w, h, float(g["fov"]))
        cam = (np.asarray(g["cam_origin"], np.float64).reshape(3), np.asarray(g["cam_rot"], np.float64).reshape(3, 3))
        prev_cam = {"moved": moved, "still": lambda c: c, "backward": backward}[prev](cam)
        gd = guides_truth(name)
        hg = gd if prev == "still" else D.guides_reference(g["spheres"], g["planes"], prev_cam[0], prev_cam[1], w, h, raygen=rg)
        hg.setflags(write=False)
        _FRAMES[key] = dict(w=w, h=h, raygen=rg, cam=cam, prev_cam=prev_cam, guides=gd, hist_guides=hg, scene=g)
    return _FRAMES[key]


def random_inputs(w, h, n, seed):
    """(sum of n passes, history mean, history lengths) of a w x h frame: finite, the lengths whole numbers 0..40 with a good share
    of zeros."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.0, 300.0, (3, w, h)) * n
    hist = rng.uniform(0.0, 300.0, (3, w, h))
    hl = (rng.integers(0, 41, (w, h)) * (rng.random((w, h)) < 0.85)).astype(np.float32)
    return s, hist, hl


def reference(f, s, n, hist, hl, settings=SETTINGS):
    return T.temporal_reference(s, n, f["guides"], hist, hl, f["hist_guides"], f["cam"], f["prev_cam"], f["raygen"], f["w"], f["h"], *settings)


def taps(f, hist, hl, settings=SETTINGS):
    return T.temporal_taps_reference(f["guides"], hist, hl, f["hist_guides"], f["cam"], f["prev_cam"], f["raygen"], f["w"], f["h"],
                                     *settings, taps=True)


def synthetic_frame(w, h, seed=3):
    """A frame no scene gives, for the grid-stride test: a wall at x = 6 seen from the origin through a plain grid, the previous
    camera a step to the side; ids in 32-pixel blocks so that some taps are refused; random history."""
    rng = np.random.default_rng(seed)
    rg = (1.0, -0.5, 1.0 / (w - 1), 0.4, -0.8 / (h - 1))
    cam = (np.zeros(3), np.eye(3))
    prev_cam = (np.array([0.0, 0.013, -0.007]), np.eye(3))

    def wall(c):
        _, d = D.primary_rays(c[0], c[1], w, h, rg)
        d = d.T.reshape(3, w, h)
        t = (6.0 - c[0][0]) / d[0]
        Pt = c[0][:, None, None] + t * d
        g = np.zeros((8, w, h), np.float32)
        g[0] = -1.0
        g[3] = t.astype(np.float32)
        g[4:7] = 100.0
        g[7] = (np.floor(Pt[1] * 40.0) + 100.0 * np.floor(Pt[2] * 40.0) + 5000.0).astype(np.float32)   # blocks fixed to the wall
        return g

    s = rng.uniform(0.0, 300.0, (3, w, h)) * 3
    hist = rng.uniform(0.0, 300.0, (3, w, h))
    hl = rng.integers(0, 9, (w, h)).astype(np.float32)
    return dict(w=w, h=h, raygen=rg, cam=cam, prev_cam=prev_cam, guides=wall(cam), hist_guides=wall(prev_cam)), s, hist, hl


# ---------------------------------------------------------------------------------------------------------------------
# The orbit of the Film and quality tests (and of tools/temporal_sweep.py): the soft_default_64_d4 scene with a matte floor

ORBIT_STEPS, ORBIT_PASSES, ORBIT_DEGREES = 8, 4, 2.0
ORBIT_MATERIALS = np.array([[0.05, 0.7, 0.0], [0.0, 0.6, 0.3], [0.1, 0.5, 0.1], [0.05, 0.8, 0.0]])      # (ambient, Lambert, reflectivity)


def orbit_scene():
    """The soft_default_64_d4 fixture with its floor made matte (material 3: no reflection), so that matte pixels are most of the
    frame: dict(w, h, raygen, spheres, lights, planes, materials, light_radius, depth, cameras).  cameras: ORBIT_STEPS steps of
    ORBIT_DEGREES about the point 4 units along the fixture camera's axis."""
    import os
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "soft_default_64_d4.npz"))
    w, h = int(g["w"]), int(g["h"])
    start = (np.asarray(g["cam_origin"], np.float64), np.asarray(g["cam_rot"], np.float64))
    pivot = start[0] + 4.0 * start[1][:, 0]
    return dict(w=w, h=h, raygen=raygen_closed_form(w, h, float(g["fov"])), spheres=g["spheres"], lights=g["lights"], planes=g["planes"],
                materials=(ORBIT_MATERIALS, g["sphere_material"], g["plane_material"]), light_radius=g["light_radius"], depth=int(g["depth"]),
                cameras=[T.orbit(start, pivot, ORBIT_DEGREES * k) for k in range(ORBIT_STEPS)])


def matte_mask(sc, guides):
    """Pixels whose first hit is an object without reflection (the table has no transparency and no specular column)."""
    table, sm, pm = sc["materials"]
    refl = np.concatenate([table[np.asarray(sm), 2], table[np.asarray(pm), 2]])
    ids = guides[7].astype(np.int64)
    return (ids >= 0) & (refl[np.clip(ids, 0, refl.size - 1)] == 0.0)
