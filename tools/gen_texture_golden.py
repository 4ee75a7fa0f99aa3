#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — fixtures of textures (rt_set_scene_textures; runs only where the reference checkout is, as
oracle/gen_golden.py does; it changes nothing under oracle/).

Per trace the closest hit is found with the reference's own get_intersection(); if the hit object has a texture, texel_index()
(numpy float64, the arithmetic of include/mi355rt.h; it imports nothing from the reference) picks the texel at the unbiased hit
point of trace.py:60, that texel is written into the hit object's colour columns of a copy of the float32 spheres / planes
array, and the reference's own trace() (trace.py:44-112) runs on the copy — with the continuations of tools/gen_lens_golden.py:
per-object materials, transparent continuations, rough reflections, area lights and the thin lens.

Writes tests/golden/texture_<case>.npz: the keys of the lens_*.npz fixtures (aperture 0 where the case has no lens), the texture
arrays tex_origin (T,3), tex_axes (T,3,3), tex_dims (T,3), tex_first (T,), sphere_texture, plane_texture, texels (N,3), u8_plain
(the same pixels with every texture id -1) and n_integral_g (sampled hits with a grid coordinate g exactly integral).
Before a file is written: at least a quarter of its pixels differ from u8_plain, wrap_33_d2 has at least 8 hits with an
integral g, and the file is no larger than tests/golden/lens_c4_s64_d5_sub32.npz.

Usage:  python tools/gen_texture_golden.py [--only NAME ...] [--jobs 8]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "tools")
for _p in (REPO, TOOLS):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from python_ray_tracer_amd.scene.texture import texel_index, texel_coords  # noqa: E402,F401  (texel_index: the pure lookup)

OUT = os.path.join(REPO, "tests", "golden")
BIAS = 0.0002
SIZE_LIMIT_FILE = os.path.join(OUT, "lens_c4_s64_d5_sub32.npz")
_W = {}


def _init():
    import gen_lens_golden as gl
    gl._init()
    _W["mods"] = gl._W["mods"]
    import gen_soft_shadow_golden as gs
    _W["refract"], _W["scatter"] = gs._W["refract"], gs._W["scatter"]


def _textured(o_, d_, t, idx, typ, spheres, planes, tex, common, events):
    """(spheres, planes) for trace(): copies with the hit object's colour replaced by its texel, or the arrays themselves."""
    if tex is None or typ not in (0, 1):
        return spheres, planes
    origin, axes, dims, first, tsid, tpid, texels = tex
    k = int(tsid[idx]) if typ == 0 else int(tpid[idx])
    if k < 0:
        return spheres, planes
    P = np.array(common.linear_comb(o_, d_, 1.0, t), dtype=np.float64)   # trace.py:60
    g = texel_coords(P, origin[k], axes[k], dims[k])
    if any(np.isfinite(v) and v == np.floor(v) for v in g):
        events.add("integral_g")
    c = texels[int(texel_index(P, origin[k], axes[k], dims[k], int(first[k])))]
    if typ == 0:
        spheres = spheres.copy()
        spheres[4:7, idx] = c
    else:
        planes = planes.copy()
        planes[6:9, idx] = c
    return spheres, planes


def _sample(o, d, spheres, lights, radius, n, planes, table, sid, pid, depth, key, tex, events):
    """gen_soft_shadow_golden._sample with the hit object's colour taken from its texture."""
    from gen_soft_shadow_golden import soft_lights
    trace, common = _W["mods"][1], _W["mods"][2]

    def run(o_, d_, b):
        Qs = soft_lights(lights, radius, n, key, b)
        t, idx, typ = trace.get_intersection(o_, d_, spheres, planes)
        m = table[sid[idx]] if typ == 0 else (table[pid[idx]] if typ == 1 else None)
        amb, lamb = (m[0], m[1]) if m is not None else (np.float64(0.0), np.float64(0.0))
        lamb_n = np.float64(lamb) / np.float64(n)
        sp, pl = _textured(o_, d_, t, idx, typ, spheres, planes, tex, common, events)
        res = trace.trace(o_, d_, sp, Qs, pl, np.float64(amb), lamb_n)
        cont = None
        if m is not None:
            P = common.linear_comb(o_, d_, 1.0, t)
            N = common.get_sphere_normal(P, idx, spheres) if typ == 0 else common.get_plane_normal(idx, planes)
            if m[3] > 0:
                o2, d2, ev = _W["refract"](d_, N, P, m[:5], typ == 0, common)
                cont = (o2, d2, None, True)
            elif m[5] > 0 and b < depth:
                cont = _W["scatter"](res[2], N, common.linear_comb(P, N, 1.0, BIAS), m[5], key, b, common)
        return res, m, cont

    (RGB, POINT, RD), m, cont = run(o, d, 0)
    W = None
    dead = False
    for i in range(depth):
        if dead or (POINT[0] == 404. and POINT[1] == 404. and POINT[2] == 404.) or \
                (RD[0] == 404. and RD[1] == 404. and RD[2] == 404.):
            continue
        c = m[3] if m[3] > 0 else m[2]
        W = c if W is None else W * c
        if cont is not None:
            POINT, RD, fallback, keep = cont
            if fallback is not None and not keep:
                dead = True
                continue
        (RGB_refl, POINT, RD), m, cont = run(POINT, RD, i + 1)
        RGB = common.linear_comb(RGB, RGB_refl, 1.0, W)
    return RGB


def _run(job):
    from oracle.oracle import jitter
    from gen_lens_golden import lens_ray
    (items, cam_o, cam_R, spheres, lights, radius, n, planes, table, sid, pid, depth, mode, spp, seed, dy, dz, aperture, focus,
     tex) = job
    common = _W["mods"][2]
    O = (cam_o[0], cam_o[1], cam_o[2])
    rows = (cam_R[0, :], cam_R[1, :], cam_R[2, :])
    rgb64, u8, evs = [], [], []
    for x, y, P, nb in items:
        events = set()

        def smp(P_, key):
            if aperture > 0.0:
                o, d = lens_ray(key[0], key[1], key[2], key[3], O, cam_R, P_, aperture, focus)
            else:
                o, d = O, common.normalize(common.matmul(rows, P_))
            return _sample(o, d, spheres, lights, radius, n, planes, table, sid, pid, depth, key, tex, events)

        if mode == "stochastic":
            acc = None
            for s_ in range(spp):
                u, v = jitter(x, y, s_, seed)
                c = smp((P[0], P[1] + u * dy, P[2] + v * dz), (2 * x, 2 * y, s_, seed))
                acc = c if acc is None else (acc[0] + c[0], acc[1] + c[1], acc[2] + c[2])
            R, G, B = acc[0] / spp, acc[1] / spp, acc[2] / spp
        else:                                                 # kernels.py:19-65
            R, G, B = smp(P, (2 * x, 2 * y, 0, seed))
            if nb is not None:
                for (ddx, ddy), Pn in nb:
                    R_s, G_s, B_s = smp(Pn, (2 * x + ddx, 2 * y + ddy, 0, seed))
                    R += R_s
                    G += B_s
                    B += G_s
                R, G, B = R / 9, G / 9, B / 9
        rgb64.append((float(R), float(G), float(B)))
        u8.append(common.clip_color_vector((R, G, B)))
        evs.append("integral_g" in events)
    return (np.array(rgb64, dtype=np.float64).reshape(-1, 3), np.array(u8, dtype=np.uint8).reshape(-1, 3),
            np.array(evs, dtype=bool).reshape(-1))


def pack_textures(textures, sphere_tex, plane_tex):
    """textures: a list of (origin, axes (3,3), texels float32 (nz, ny, nx, 3)); ids index it (-1: none)."""
    origin = np.array([t[0] for t in textures], dtype=np.float64).reshape(-1, 3)
    axes = np.array([t[1] for t in textures], dtype=np.float64).reshape(-1, 3, 3)
    tx = [np.asarray(t[2], dtype=np.float32) for t in textures]
    dims = np.array([[t.shape[2], t.shape[1], t.shape[0]] for t in tx], dtype=np.int32).reshape(-1, 3)
    first = np.cumsum([0] + [t.shape[0] * t.shape[1] * t.shape[2] for t in tx])[:-1].astype(np.int64)
    texels = np.concatenate([t.reshape(-1, 3) for t in tx]).astype(np.float32)
    return (origin, axes, dims, first, np.asarray(sphere_tex, dtype=np.int32), np.asarray(plane_tex, dtype=np.int32), texels)


def render_pixels(pool, jobs, mods, w, h, spheres, lights, radius, n, planes, position, euler, table, sid, pid, depth, aperture,
                  focus_point, tex, aa=0, spp=0, seed=1, coords=None, fov=45.0):
    """(dict of the scene's arrays, rgb64, u8, integral-g flags) of the sampled pixels; tex: pack_textures() or None."""
    from oracle import gen_golden as gg
    from gen_soft_shadow_golden import NB, pad6
    from gen_lens_golden import focus_on
    common, scene_mod = mods[2], mods[4]
    cam_o, cam_R, pixel_loc = gg.camera_arrays(scene_mod, w, h, list(position), list(euler), fov)
    focus = focus_on(cam_o, cam_R, focus_point) if aperture > 0.0 else 1.0
    if coords is None:
        coords = gg.all_coords(w, h, w - 1, h - 1) if aa == 1 else gg.all_coords(w, h)
    coords = np.asarray(coords, dtype=np.int32).reshape(-1, 2)
    table = np.asarray(table, dtype=np.float64)
    table = table.reshape(-1, table.shape[-1])
    radius = np.asarray(radius, dtype=np.float32).reshape(-1)
    sid, pid = np.asarray(sid, dtype=np.int32), np.asarray(pid, dtype=np.int32)
    items = []
    for x, y in coords:
        x, y = int(x), int(y)
        P = pixel_loc[0:3, x, y]
        nb = None
        if aa == 1 and 1 <= x and x + 1 <= w and 1 <= y and y + 1 <= h:
            nb = [((dx, dy_), common.linear_comb(P, pixel_loc[0:3, x + dx, y + dy_], 0.5, 0.5)) for dx, dy_ in NB]
        items.append((x, y, P, nb))
    ar = int(w / h)
    dy, dz = (-ar - ar) / float(w - 1), (-1 - 1) / float(h - 1)
    mode = "stochastic" if aa == 2 else "pixels"
    chunks = [items[i::jobs * 8] for i in range(min(len(items), jobs * 8))]
    order = np.concatenate([np.arange(len(items))[i::jobs * 8] for i in range(len(chunks))])

    def render(tx):
        res = pool.map(_run, [(c, cam_o, cam_R, spheres, lights, radius.astype(np.float64), n, planes, pad6(table), sid, pid,
                               depth, mode, spp, seed, dy, dz, float(aperture), focus, tx) for c in chunks])
        rgb64 = np.empty((len(items), 3)); u8 = np.empty((len(items), 3), np.uint8); ev = np.empty(len(items), bool)
        rgb64[order] = np.concatenate([r[0] for r in res]); u8[order] = np.concatenate([r[1] for r in res])
        ev[order] = np.concatenate([r[2] for r in res])
        return rgb64, u8, ev

    d = dict(w=w, h=h, spheres=spheres, lights=lights, planes=planes, cam_origin=cam_o, cam_rot=cam_R,
             position=np.array(position, dtype=np.float64), euler=np.array(euler, dtype=np.float64), fov=fov,
             depth=depth, aa=aa, coords=coords, materials=table, sphere_material=sid, plane_material=pid, seed=seed,
             light_radius=radius, shadow_samples=n, aperture=np.float64(aperture), focus_distance=np.float64(focus))
    if aa == 2:
        d.update(spp=spp)
    return d, render


def case(pool, jobs, mods, name, *args, tex, scalars=(0.0, 0.6, 0.3), **kw):
    t0 = time.time()
    d, render = render_pixels(pool, jobs, mods, *args, tex, **kw)
    rgb64, u8, ev = render(tex)
    _, u8p, _ = render(None)
    amb, lamb, refl = scalars
    depth = int(d["depth"])
    d.update(amb=amb, lamb=lamb, refl=refl,
             refl_pow=np.array([np.float64(refl) ** (i + 1) for i in range(max(depth, 1))], dtype=np.float64),
             rgb64=rgb64, u8=u8, u8_plain=u8p, n_integral_g=int(ev.sum()),
             tex_origin=tex[0], tex_axes=tex[1], tex_dims=tex[2], tex_first=tex[3], sphere_texture=tex[4], plane_texture=tex[5],
             texels=tex[6])
    differ = int((u8 != u8p).any(axis=1).sum())
    if 4 * differ < len(u8):
        raise SystemExit(f"{name}: only {differ} of {len(u8)} pixels differ from the untextured scene (a quarter is required)")
    if name == "wrap_33_d2" and d["n_integral_g"] < 8:
        raise SystemExit(f"{name}: only {d['n_integral_g']} sampled hits with an integral g (8 are required)")
    path = os.path.join(OUT, f"texture_{name}.npz")
    tmp = path + ".tmp.npz"
    np.savez_compressed(tmp, **d)
    size, limit = os.path.getsize(tmp), os.path.getsize(SIZE_LIMIT_FILE)
    if size > limit:
        os.remove(tmp)
        raise SystemExit(f"{name}: {size} bytes, more than {os.path.basename(SIZE_LIMIT_FILE)} ({limit})")
    os.replace(tmp, path)
    print(f"  wrote {path} ({size / 1024:.0f} KiB, {len(u8)} px, differ from plain {differ}, integral g {d['n_integral_g']}, "
          f"{time.time() - t0:.1f} s)", flush=True)


def checker(a, b, size, origin=(0.0, 0.0, 0.0), solid=False):
    from python_ray_tracer_amd.scene import Texture
    t = Texture.checker(a, b, size, origin=origin, solid=solid)
    return (t.origin, t.axes, t.texels)


IMAGE_5x3 = np.array([[[250, 30, 30], [30, 250, 30], [30, 30, 250], [250, 250, 30], [30, 250, 250]],
                      [[250, 30, 250], [240, 240, 240], [20, 20, 20], [250, 140, 20], [140, 20, 250]],
                      [[20, 140, 250], [140, 250, 20], [250, 20, 140], [90, 90, 200], [200, 90, 90]]], dtype=np.float32)


def scenes(gg, workloads):
    """name -> (positional arguments of render_pixels after mods, up to focus_point; tex; keyword arguments)."""
    from gen_scatter_golden import DEFAULT_TABLE, GRID_TABLE, grid_ids
    from python_ray_tracer_amd.scene import Texture
    L3, P1 = gg.lig(gg.DEFAULT_LIGHTS), gg.pla([gg.DEFAULT_PLANE])
    S6, S8 = gg.sph(gg.DEFAULT_SPHERES), gg.sph(gg.DEFAULT_SPHERES + gg.EXTRA_SPHERES)
    CAM = ([-2, 0, 2.0], [0, -30, 0])
    Z3 = [0.0, 0.0, 0.0]
    C0 = gg.DEFAULT_SPHERES[0][0]
    WHITE, BLACK, ORANGE, TEAL = (235, 235, 235), (25, 25, 25), (240, 130, 20), (20, 160, 170)
    MIRRORS = [(0.05, 0.7, 0.0), (0.0, 0.5, 0.5), (0.1, 0.6, 0.1), (0.0, 0.3, 0.8)]
    floor = checker(WHITE, BLACK, 0.5)
    solid = checker(ORANGE, TEAL, 0.3, origin=(0.1, 0.05, 0.02), solid=True)
    img = Texture.image(IMAGE_5x3, (0.0, -0.2, 0.9), (0.0, 1.0, 0.0), (0.0, 0.0, -0.8))   # a slide projected along x
    slide = (img.origin, img.axes, img.texels)
    out = {}
    out["default_64_d4"] = ((64, 64, S6, L3, Z3, 1, P1, *CAM, MIRRORS, [3, 1, 0, 2, 1, 3], [1], 4, 0.0, C0),
                            pack_textures([floor, solid, slide], [-1, -1, 1, 2, -1, -1], [0]), dict(seed=11))
    out["aa_48_d2"] = ((48, 48, S6, L3, Z3, 1, P1, *CAM, MIRRORS, [3, 1, 0, 2, 1, 3], [1], 2, 0.0, C0),
                       pack_textures([floor, solid, slide], [-1, 2, 1, -1, -1, 1], [0]), dict(aa=1, seed=9))
    out["stoch_40x24_spp3_seed7"] = ((40, 24, S8, L3, Z3, 1, P1, *CAM, DEFAULT_TABLE, [0, 1, 2, 3, 4, 5, 3, 5], [6], 2, 0.0, C0),
                                     pack_textures([floor, solid, slide], [1, -1, -1, 2, -1, -1, 1, -1], [0]),
                                     dict(aa=2, spp=3, seed=7))
    # wrap_33_d2: the camera only pitches, so column 16 of the 33 x 33 closed-form grid (y == 0 exactly) has d.y == 0 and
    # Pt.y == cam.y == 0 exactly.  V axes (0, s, 0) with s a power of two and origin.y = cam.y - k/s make g = k there: the floor
    # k = 5 = ny (an exact multiple of ny), the tilted plane k = 0 (g = +-0.0), the sphere's 1 x 1 x 7 grid k = 7 = nz.
    tilted = gg.pla([gg.DEFAULT_PLANE, ([3.0, 0.0, 0.0], [-1.0, 0.3, 0.6], gg.GREY)])
    rng = np.random.default_rng(33)
    t35 = rng.integers(20, 250, size=(1, 5, 3, 3)).astype(np.float32)
    t7 = rng.integers(20, 250, size=(7, 1, 1, 3)).astype(np.float32)
    t35b = rng.integers(20, 250, size=(1, 5, 3, 3)).astype(np.float32)
    wrap = [((-1.75, -2.5, 0.0), [[1.3, 0.0, 0.4], [0.0, 2.0, 0.0], [0.0, 0.0, 1.0]], t35),
            ((0.3, 0.0, -0.4), [[0.9, 0.3, 1.7], [0.0, 4.0, 0.0], [0.0, 0.0, 1.0]], t35b),        # U.V != 0; origin.y = cam.y
            ((0.0, -0.875, 0.0), [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 8.0, 0.0]], t7)]
    out["wrap_33_d2"] = ((33, 33, S6, L3, Z3, 1, tilted, *CAM, MIRRORS, [3, 1, 0, 2, 1, 3], [1, 2], 2, 0.0, C0),
                         pack_textures(wrap, [2, -1, 2, -1, 2, -1], [0, 1]), dict(seed=5))
    # the camera inside a textured glass sphere
    inside = gg.sph(gg.DEFAULT_SPHERES[:5] + [([-2.0, 0.1, 2.0], 0.9, gg.GREY)])
    out["inside_32_d3"] = ((32, 32, inside, L3, Z3, 1, P1, *CAM, DEFAULT_TABLE, [1, 2, 3, 4, 5, 0], [6], 3, 0.0, C0),
                           pack_textures([floor, checker(ORANGE, TEAL, 0.25, solid=True)], [-1, -1, -1, -1, -1, 1], [0]),
                           dict(seed=3))
    # lens + area lights + glass + rough: the glass sphere (row 0) and the rough floor (row 6) textured
    out["everything_48_d4"] = ((48, 48, S6, L3, [0.4, 0.7, 0.5], 2, P1, *CAM, DEFAULT_TABLE, range(6), [6], 4, 0.12,
                                gg.DEFAULT_SPHERES[3][0]),
                               pack_textures([floor, solid], [1, -1, -1, -1, -1, -1], [0]), dict(seed=13))

    def grid(n_side, seed):
        sp = workloads.grid_spheres(n_side, seed)
        return gg.sph([(s.origin, s.radius, s.color) for s in sp])

    def third(n):
        return [(i // 3) % 2 + 1 if i % 3 == 0 else -1 for i in range(n)]

    big = [checker(WHITE, BLACK, 0.4), checker(ORANGE, TEAL, 0.15, solid=True), slide]
    # (c4: a matte floor, row 1 — with the rough mirror floor of row 6 no two of a floor pixel's R, G, B are equal and the
    # float64 colours of 8040 pixels compress to more than the size limit; c5 keeps row 6)
    cs = [(x, y) for x in range(16, 3840, 32) for y in range(16, 2160, 32)]
    out["c4_s64_d5_sub32"] = ((3840, 2160, grid(8, 355), L3, Z3, 1, P1, *CAM, GRID_TABLE, grid_ids(64), [1], 5, 0.0, C0),
                              pack_textures(big, third(64), [0]), dict(coords=cs, seed=21))
    cs = [(x, y) for x in range(48, 7680, 96) for y in range(48, 4320, 96)]
    out["c5_s256_d8_sub96"] = ((7680, 4320, grid(16, 356), L3, Z3, 1, P1, *CAM, GRID_TABLE, grid_ids(256), [6], 8, 0.0, C0),
                               pack_textures(big, third(256), [0]), dict(coords=cs, seed=22))
    return out


def main():
    import multiprocessing as mp
    from oracle import gen_golden as gg
    from python_ray_tracer_amd import workloads
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    mods = gg._import_reference()
    with mp.Pool(a.jobs, initializer=_init) as pool:
        for name, (args, tex, kw) in scenes(gg, workloads).items():
            if a.only is None or name in a.only:
                case(pool, a.jobs, mods, name, *args, tex=tex, **kw)


if __name__ == "__main__":
    main()
