#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — fixtures of lighting (rt_set_scene_lighting; runs only where the reference checkout is, as
oracle/gen_golden.py does; it changes nothing under oracle/).

The reference's trace() cannot weight one light differently from another, so lit_trace() restates the body of trace.py:77-102
with the reference's own get_intersection, get_vector_to_light, dot, linear_comb and normal helpers, and adds each light's two
terms with light_terms() (python_ray_tracer_amd/scene/lighting.py: numpy float64, the arithmetic of include/mi355rt.h; it imports
nothing from the reference).  Everything around a trace is tools/gen_texture_golden.py's: per-object materials, transparent
continuations, rough reflections, area lights, the thin lens and textures.

Writes tests/golden/lighting_<case>.npz: the keys of the texture_*.npz fixtures (no texture: T == 0 and every id -1), materials
with 8 columns (amb, lamb, refl, trans, ior, rough, spec, shin), light_rgb (L,3) float32, u8_plain (the same pixels with white
lights and spec = 0) and events, the counts of EVENTS over the sampled traces.
Before a file is written:
  * the restatement with white lights and spec = 0 is bit-identical to the reference's own trace() on every sampled trace;
  * at least a quarter of the sampled pixels differ from u8_plain;
  * grazing_48_d2 has each of EVENTS at least 8 times;
  * the file is no larger than tests/golden/lens_c4_s64_d5_sub32.npz.

Usage:  python tools/gen_lighting_golden.py [--only NAME ...] [--jobs 8]
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
from python_ray_tracer_amd.scene.lighting import light_terms, light_wants  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
BIAS = 0.0002
SIZE_LIMIT_FILE = os.path.join(OUT, "lens_c4_s64_d5_sub32.npz")
# k <= 0 with a highlight; cN > 0 with s <= 0; occluded with wantS only; a highlight on a transparent hit
EVENTS = ("highlight_without_lambert", "facing_light_no_highlight", "occluded_specular_only", "highlight_on_glass")
_W = {}
MISS = ((0.0, 0.0, 0.0), (404., 404., 404.), (404, 404., 404.))


def _init():
    import gen_texture_golden as gt
    gt._init()
    _W["mods"] = gt._W["mods"]
    _W["refract"], _W["scatter"] = gt._W["refract"], gt._W["scatter"]


def pad8(table):
    """A 3-, 5-, 6- or 8-column table as eight columns (trans 0, ior 1, rough 0, spec 0, shin 1)."""
    t = np.asarray(table, dtype=np.float64)
    t = t.reshape(-1, t.shape[-1]) if t.ndim == 2 else t.reshape(-1, 3)
    out = np.tile(np.array([0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0]), (t.shape[0], 1))
    out[:, :t.shape[1]] = t
    return out


def lit_trace(o, d, spheres, Qs, planes, amb, lamb_n, eQ, spec, spec_n, shin, glass, events):
    """trace.py:44-112 with a colour per light and a highlight: (RGB, P, R) as trace() returns them.  Qs (3, L*n) the lights (or
    their sample points), eQ (L*n, 3) float64 their colours."""
    trace, common = _W["mods"][1], _W["mods"][2]
    t, idx, typ = trace.get_intersection(o, d, spheres, planes)                 # :53
    if typ == 404:
        # (tools/gen_sky_golden.py: under a sky a trace that finds nothing returns the sky's colour with the same sentinels)
        return MISS if _W.get("miss") is None else (_W["miss"](d), MISS[1], MISS[2])
    P = common.linear_comb(o, d, 1.0, t)                                        # :60
    if typ == 0:
        col = common.get_sphere_color(idx, spheres)
        N = common.get_sphere_normal(P, idx, spheres)
    else:
        col = common.get_plane_color(idx, planes)
        N = common.get_plane_normal(idx, planes)
    RGB = common.linear_comb((0.0, 0.0, 0.0), col, 1.0, amb)                     # :77
    P = common.linear_comb(P, N, 1.0, BIAS)                                      # :82-83
    for j in range(Qs.shape[1]):                                                # :86-102
        Ld = common.get_vector_to_light(P, Qs, j)
        cN, k, wantL, wantS = light_wants(np.array(Ld), np.array(N), lamb_n, spec)
        if not (wantL or wantS):
            continue
        _, _, shadow = trace.get_intersection(P, Ld, spheres, planes)
        occluded = shadow != 404
        new = light_terms(np.array(RGB, dtype=np.float64), np.array(d, dtype=np.float64), np.array(N, dtype=np.float64),
                          np.array(Ld, dtype=np.float64), np.array(col, dtype=np.float64), eQ[j], lamb_n, spec, spec_n, shin,
                          occluded)
        if events is not None and wantS:
            if occluded:
                if not wantL:
                    events["occluded_specular_only"] += 1
            else:
                nd = (-d[0], -d[1], -d[2])
                s = common.dot(N, common.normalize((Ld[0] + nd[0], Ld[1] + nd[1], Ld[2] + nd[2])))
                if s > 0:
                    if not wantL:
                        events["highlight_without_lambert"] += 1
                    if glass:
                        events["highlight_on_glass"] += 1
                else:
                    events["facing_light_no_highlight"] += 1
        RGB = (new[0], new[1], new[2])
    R = common.get_reflection(d, N)
    P = common.linear_comb(P, R, 1.0, BIAS)
    return RGB, P, R


def _same(a, b):
    return np.array_equal(np.array(a, dtype=np.float64).view(np.uint64), np.array(b, dtype=np.float64).view(np.uint64))


def _sample(o, d, spheres, lights, radius, n, planes, table, sid, pid, depth, key, tex, e, events):
    """gen_texture_golden._sample with lit_trace() in place of trace(); e (L,3) float64 or None (white lights, spec 0: the plain
    frame, and every trace is compared with the reference's own trace())."""
    from gen_soft_shadow_golden import soft_lights
    from gen_texture_golden import _textured
    trace, common = _W["mods"][1], _W["mods"][2]
    eQ = np.repeat(np.ones((lights.shape[1], 3)) if e is None else np.asarray(e, dtype=np.float64), n, axis=0)

    def run(o_, d_, b):
        Qs = soft_lights(lights, radius, n, key, b)
        t, idx, typ = trace.get_intersection(o_, d_, spheres, planes)
        m = table[sid[idx]] if typ == 0 else (table[pid[idx]] if typ == 1 else None)
        amb, lamb = (m[0], m[1]) if m is not None else (np.float64(0.0), np.float64(0.0))
        spec, shin = (np.float64(m[6]), m[7]) if (m is not None and e is not None) else (np.float64(0.0), 1.0)
        lamb_n = np.float64(lamb) / np.float64(n)
        spec_n = spec / np.float64(n)
        sp, pl = _textured(o_, d_, t, idx, typ, spheres, planes, tex, common, set())
        res = lit_trace(o_, d_, sp, Qs, pl, np.float64(amb), lamb_n, eQ, spec, spec_n, shin,
                        m is not None and m[3] > 0, events if e is not None else None)
        if e is None:
            ref = trace.trace(o_, d_, sp, Qs, pl, np.float64(amb), lamb_n)
            if not all(_same(x, y) for x, y in zip(res, ref)):
                raise RuntimeError(f"the restated trace differs from the reference's trace(): {res} / {ref}")
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

    _W["ray"] = "primary"                           # what the next trace's ray is (read by the miss hook of gen_sky_golden.py)
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
        _W["ray"] = "reflected" if cont is None else ("refracted" if cont[2] is None else "scattered")
        (RGB_refl, POINT, RD), m, cont = run(POINT, RD, i + 1)
        RGB = common.linear_comb(RGB, RGB_refl, 1.0, W)
    return RGB


def _run(job):
    from oracle.oracle import jitter
    from gen_lens_golden import lens_ray
    (items, cam_o, cam_R, spheres, lights, radius, n, planes, table, sid, pid, depth, mode, spp, seed, dy, dz, aperture, focus,
     tex, e) = job
    common = _W["mods"][2]
    O = (cam_o[0], cam_o[1], cam_o[2])
    rows = (cam_R[0, :], cam_R[1, :], cam_R[2, :])
    rgb64, u8 = [], []
    events = {k: 0 for k in EVENTS}
    for x, y, P, nb in items:

        def smp(P_, key):
            if aperture > 0.0:
                o, d = lens_ray(key[0], key[1], key[2], key[3], O, cam_R, P_, aperture, focus)
            else:
                o, d = O, common.normalize(common.matmul(rows, P_))
            return _sample(o, d, spheres, lights, radius, n, planes, table, sid, pid, depth, key, tex, e, events)

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
    return (np.array(rgb64, dtype=np.float64).reshape(-1, 3), np.array(u8, dtype=np.uint8).reshape(-1, 3),
            np.array([events[k] for k in EVENTS], dtype=np.int64))


def render_pixels(pool, jobs, mods, w, h, spheres, lights, radius, n, planes, position, euler, table, sid, pid, depth, aperture,
                  focus_point, tex, light_rgb, aa=0, spp=0, seed=1, coords=None, fov=45.0):
    """(dict of the scene's arrays, render): render(True) gives (rgb64, u8, event counts) of the sampled pixels with the
    lighting, render(False) with white lights and spec = 0 (every trace checked against the reference's trace())."""
    from oracle import gen_golden as gg
    from gen_soft_shadow_golden import NB
    from gen_lens_golden import focus_on
    common, scene_mod = mods[2], mods[4]
    cam_o, cam_R, pixel_loc = gg.camera_arrays(scene_mod, w, h, list(position), list(euler), fov)
    focus = focus_on(cam_o, cam_R, focus_point) if aperture > 0.0 else 1.0
    if coords is None:
        coords = gg.all_coords(w, h, w - 1, h - 1) if aa == 1 else gg.all_coords(w, h)
    coords = np.asarray(coords, dtype=np.int32).reshape(-1, 2)
    table = pad8(table)
    radius = np.asarray(radius, dtype=np.float32).reshape(-1)
    light_rgb = np.asarray(light_rgb, dtype=np.float32).reshape(-1, 3)
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

    def render(lit):
        e = light_rgb.astype(np.float64) if lit else None
        res = pool.map(_run, [(c, cam_o, cam_R, spheres, lights, radius.astype(np.float64), n, planes, table, sid, pid,
                               depth, mode, spp, seed, dy, dz, float(aperture), focus, tex, e) for c in chunks])
        rgb64 = np.empty((len(items), 3)); u8 = np.empty((len(items), 3), np.uint8)
        rgb64[order] = np.concatenate([r[0] for r in res]); u8[order] = np.concatenate([r[1] for r in res])
        return rgb64, u8, np.sum([r[2] for r in res], axis=0)

    d = dict(w=w, h=h, spheres=spheres, lights=lights, planes=planes, cam_origin=cam_o, cam_rot=cam_R,
             position=np.array(position, dtype=np.float64), euler=np.array(euler, dtype=np.float64), fov=fov,
             depth=depth, aa=aa, coords=coords, materials=table, sphere_material=sid, plane_material=pid, seed=seed,
             light_radius=radius, shadow_samples=n, aperture=np.float64(aperture), focus_distance=np.float64(focus),
             light_rgb=light_rgb)
    if aa == 2:
        d.update(spp=spp)
    return d, render


def no_textures(S, P):
    return (np.zeros((0, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3), np.int32), np.zeros(0, np.int64),
            np.full(S, -1, np.int32), np.full(P, -1, np.int32), np.zeros((0, 3), np.float32))


def case(pool, jobs, mods, name, *args, tex, light_rgb, scalars=(0.0, 0.6, 0.3), **kw):
    t0 = time.time()
    if tex is None:
        tex = no_textures(args[2].shape[1], args[6].shape[1])
    d, render = render_pixels(pool, jobs, mods, *args, tex if len(tex[3]) else None, light_rgb, **kw)
    rgb64, u8, ev = render(True)
    _, u8p, _ = render(False)                       # (also: every trace of the restatement equals the reference's trace())
    amb, lamb, refl = scalars
    depth = int(d["depth"])
    d.update(amb=amb, lamb=lamb, refl=refl,
             refl_pow=np.array([np.float64(refl) ** (i + 1) for i in range(max(depth, 1))], dtype=np.float64),
             rgb64=rgb64, u8=u8, u8_plain=u8p, events=np.asarray(ev, dtype=np.int64),
             tex_origin=tex[0], tex_axes=tex[1], tex_dims=tex[2], tex_first=tex[3], sphere_texture=tex[4], plane_texture=tex[5],
             texels=tex[6])
    differ = int((u8 != u8p).any(axis=1).sum())
    if 4 * differ < len(u8):
        raise SystemExit(f"{name}: only {differ} of {len(u8)} pixels differ from the white-light, spec = 0 scene (a quarter is required)")
    if name == "grazing_48_d2" and min(ev) < 8:
        raise SystemExit(f"{name}: events {dict(zip(EVENTS, ev.tolist()))} (8 of each are required)")
    path = os.path.join(OUT, f"lighting_{name}.npz")
    tmp = path + ".tmp.npz"
    np.savez_compressed(tmp, **d)
    size, limit = os.path.getsize(tmp), os.path.getsize(SIZE_LIMIT_FILE)
    if size > limit:
        os.remove(tmp)
        raise SystemExit(f"{name}: {size} bytes, more than {os.path.basename(SIZE_LIMIT_FILE)} ({limit})")
    os.replace(tmp, path)
    print(f"  wrote {path} ({size / 1024:.0f} KiB, {len(u8)} px, differ from plain {differ}, events {ev.tolist()}, "
          f"{time.time() - t0:.1f} s)", flush=True)


def glossy(table, spec, shin):
    """The table with spec and shin columns: spec[i % len], shin[i % len] for row i."""
    t = pad8(table)
    for i in range(len(t)):
        t[i, 6], t[i, 7] = spec[i % len(spec)], shin[i % len(shin)]
    return t


def scenes(gg, workloads):
    """name -> (positional arguments of render_pixels after mods, up to focus_point; tex or None; light_rgb; keyword arguments)."""
    from gen_scatter_golden import DEFAULT_TABLE, GRID_TABLE, grid_ids
    from gen_texture_golden import checker, pack_textures
    L3, P1 = gg.lig(gg.DEFAULT_LIGHTS), gg.pla([gg.DEFAULT_PLANE])
    S6, S8 = gg.sph(gg.DEFAULT_SPHERES), gg.sph(gg.DEFAULT_SPHERES + gg.EXTRA_SPHERES)
    CAM = ([-2, 0, 2.0], [0, -30, 0])
    Z3 = [0.0, 0.0, 0.0]
    C0 = gg.DEFAULT_SPHERES[0][0]
    WHITE, BLACK, ORANGE, TEAL = (235, 235, 235), (25, 25, 25), (240, 130, 20), (20, 160, 170)
    MIRRORS = [(0.05, 0.7, 0.0), (0.0, 0.5, 0.5), (0.1, 0.6, 0.1), (0.0, 0.3, 0.8)]
    WARM_COOL = [(1.0, 0.75, 0.5), (0.25, 0.4, 0.9), (0.3, 0.3, 0.3)]           # a warm key, a cool fill, a dim third
    floor = checker(WHITE, BLACK, 0.5)
    solid = checker(ORANGE, TEAL, 0.3, origin=(0.1, 0.05, 0.02), solid=True)
    out = {}
    out["default_64_d4"] = ((64, 64, S6, L3, Z3, 1, P1, *CAM, glossy(MIRRORS, [120, 0, 60, 200], [64, 1, 8, 256]),
                             [3, 1, 0, 2, 1, 3], [1], 4, 0.0, C0),
                            pack_textures([floor, solid], [-1, -1, 1, -1, -1, -1], [0]), WARM_COOL, dict(seed=11))
    out["aa_48_d2"] = ((48, 48, S6, L3, Z3, 1, P1, *CAM, glossy(MIRRORS, [90, 150, 0, 40], [16, 128, 1, 4]),
                        [3, 1, 0, 2, 1, 3], [1], 2, 0.0, C0), None, [(1.5, 1.5, 1.5), (0.0, 0.6, 1.0), (1.0, 0.2, 0.0)],
                       dict(aa=1, seed=9))
    out["stoch_40x24_spp3_seed7"] = ((40, 24, S8, L3, Z3, 1, P1, *CAM, glossy(DEFAULT_TABLE, [100, 0, 180], [32, 1, 512]),
                                      [0, 1, 2, 3, 4, 5, 3, 5], [6], 2, 0.0, C0), None, WARM_COOL, dict(aa=2, spp=3, seed=7))
    # the camera inside a glossy glass sphere
    inside = gg.sph(gg.DEFAULT_SPHERES[:5] + [([-2.0, 0.1, 2.0], 0.9, gg.GREY)])
    out["inside_32_d3"] = ((32, 32, inside, L3, Z3, 1, P1, *CAM, glossy(DEFAULT_TABLE, [140, 80], [128, 2]),
                            [1, 2, 3, 4, 5, 0], [6], 3, 0.0, C0), None, WARM_COOL, dict(seed=3))
    # lens + area lights + glass + rough + textures + lighting
    out["everything_48_d4"] = ((48, 48, S6, L3, [0.4, 0.7, 0.5], 2, P1, *CAM, glossy(DEFAULT_TABLE, [160, 60, 0], [64, 8, 1]),
                                range(6), [6], 4, 0.12, gg.DEFAULT_SPHERES[3][0]),
                               pack_textures([floor, solid], [1, -1, -1, -1, -1, -1], [0]), WARM_COOL, dict(seed=13))
    # grazing_48_d2: two lights just above the floor's horizon; row 1 has lamb = 0 and spec > 0, row 2 a negative lamb, row 3 is
    # glossy glass (a trace that meets it from inside has d.N > 0: a light with cN > 0 there can have s <= 0)
    GRAZE = np.array([(0.05, 0.7, 0.2, 0.0, 1.0, 0.0, 0.0, 1.0), (0.1, 0.0, 0.0, 0.0, 1.0, 0.0, 150.0, 32.0),
                      (0.3, -0.4, 0.1, 0.0, 1.0, 0.0, 200.0, 16.0), (0.0, 0.1, 0.0, 0.9, 1.5, 0.0, 220.0, 8.0),
                      (0.05, 0.5, 0.3, 0.0, 1.0, 0.0, 80.0, 4.0)])
    graze_l = gg.lig([[1.0, -3.0, 0.02], [-1.5, 0.0, 0.04], [2.5, 2.0, 3.0], [2.5, -2.0, 3.0]])
    out["grazing_48_d2"] = ((48, 48, S6, graze_l, [0.0] * 4, 1, P1, *CAM, GRAZE, [3, 1, 2, 3, 1, 2], [4], 2, 0.0, C0),
                            None, [(1.0, 0.9, 0.8), (0.6, 0.8, 1.0), (1.0, 1.0, 1.0), (0.9, 0.5, 0.2)], dict(seed=17))
    # shin_extremes_32_d1: shin 1 and 1024, rows with spec = 0 mixed in, light components of 0, 0.3 and 4
    EXT = np.array([(0.05, 0.6, 0.2, 0.0, 1.0, 0.0, 90.0, 1.0), (0.05, 0.6, 0.2, 0.0, 1.0, 0.0, 0.0, 1024.0),
                    (0.1, 0.4, 0.0, 0.0, 1.0, 0.0, 250.0, 1024.0), (0.0, 0.5, 0.3, 0.0, 1.0, 0.0, 0.0, 1.0),
                    (0.05, 0.3, 0.1, 0.0, 1.0, 0.0, 60.0, 1.0)])
    out["shin_extremes_32_d1"] = ((32, 32, S6, L3, Z3, 1, P1, *CAM, EXT, [0, 1, 2, 3, 2, 0], [4], 1, 0.0, C0), None,
                                  [(4.0, 0.3, 0.0), (0.0, 4.0, 0.3), (0.3, 0.0, 4.0)], dict(seed=19))

    def grid(n_side, seed):
        sp = workloads.grid_spheres(n_side, seed)
        return gg.sph([(s.origin, s.radius, s.color) for s in sp])

    # (c4: a matte, untextured floor, row 1, under grey lights of three strengths — with coloured lights no two of a floor pixel's
    # R, G, B are equal and the float64 colours of 8040 pixels compress to more than the size limit; c5 has the colours)
    cs = [(x, y) for x in range(16, 3840, 32) for y in range(16, 2160, 32)]
    out["c4_s64_d5_sub32"] = ((3840, 2160, grid(8, 355), L3, Z3, 1, P1, *CAM, glossy(GRID_TABLE, [120, 0, 200], [64, 1, 256]),
                               grid_ids(64), [1], 5, 0.0, C0), None, [(2.0, 2.0, 2.0), (0.5, 0.5, 0.5), (0.25, 0.25, 0.25)],
                              dict(coords=cs, seed=21))
    cs = [(x, y) for x in range(48, 7680, 96) for y in range(48, 4320, 96)]
    out["c5_s256_d8_sub96"] = ((7680, 4320, grid(16, 356), L3, Z3, 1, P1, *CAM, glossy(GRID_TABLE, [100, 160, 0], [32, 512, 1]),
                                grid_ids(256), [6], 8, 0.0, C0), None, WARM_COOL, dict(coords=cs, seed=22))
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
        for name, (args, tex, light_rgb, kw) in scenes(gg, workloads).items():
            if a.only is None or name in a.only:
                case(pool, a.jobs, mods, name, *args, tex=tex, light_rgb=light_rgb, **kw)


if __name__ == "__main__":
    main()
