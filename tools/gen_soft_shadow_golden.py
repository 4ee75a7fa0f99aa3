#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — fixtures of area lights (soft shadows; runs only where the reference checkout is, as
oracle/gen_golden.py does; it changes nothing under oracle/).

Trace b of a sample (X, Y, s) is the reference's own trace() (trace.py:44-112) called with a different lights array: the L*n
shadow sample points Q of rt_set_scene_area_lights (include/mi355rt.h), (m, i) m-major, and lambert_int = lamb_b / n.  Materials,
transparent continuations and rough reflections are tools/gen_scatter_golden.py's (its scatter() and the refraction
continuation of tools/gen_refraction_golden.py).  Every table is padded to six columns (trans 0, ior 1, rough 0).

light_point() is the pure sampler; it uses only the hash (hash32 of tools/gen_scatter_golden.py, oracle/oracle.py's jitter()
restatement) and imports nothing from the reference (tests/test_soft_shadows.py checks it on its own).

Writes tests/golden/soft_<case>.npz: the keys of the scatter_*.npz fixtures, with `light_radius` float32 (L,) and
`shadow_samples` (and, for the rim case, u8_point: the same pixels with every radius 0), plus n_penumbra (sampled pixels where some light's shadow samples were partly occluded: some of its samples
with a positive Lambert term blocked, others not) and n_anchor_miss (sampled pixels where some occluded shadow sample is blocked
only by spheres that the line through its light's CENTRE, with the same direction, misses: a light-anchored cull table would
certify that ray unoccluded).

Usage:  python tools/gen_soft_shadow_golden.py [--only NAME ...] [--jobs 8]
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
from gen_scatter_golden import hash32  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
BIAS = 0.0002
SOFT_SALT = 0x50F7117E
_W = {}


def light_candidate(X, Y, s, b, m, i, j, seed):
    """Candidate j of shadow sample i of light m, trace b, sample (X, Y, s): q_c = (h >> 8) 2^-23 + (2^-24 - 1) (exact)."""
    return tuple(float(hash32(X, Y, ((((s * 32 + b) * 64 + m) * 16 + i) * 8 + j) * 4 + c, seed ^ SOFT_SALT) >> 8) * 2.0 ** -23
                 + (2.0 ** -24 - 1.0) for c in range(3))


def light_point(X, Y, s, b, m, i, seed, centre, radius):
    """Q = c + rho*q (float64, no fused multiply-add) for the first candidate with q.q < 1 (((qx qx + qy qy) + qz qz)), or
    c itself if none of the eight is inside.  centre: three float64 (the float32 centre widened), radius: float64."""
    for j in range(8):
        q = light_candidate(X, Y, s, b, m, i, j, seed)
        if (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2] < 1.0:
            return (centre[0] + radius * q[0], centre[1] + radius * q[1], centre[2] + radius * q[2])
    return (float(centre[0]), float(centre[1]), float(centre[2]))


def soft_lights(lights, radius, n, key, b):
    """float64 (3, L*n): the points Q of trace b of sample key = (X, Y, s, seed), (m, i) m-major."""
    X, Y, s, seed = key
    L = lights.shape[1]
    out = np.empty((3, L * n), dtype=np.float64)
    for m in range(L):
        c = (float(lights[0, m]), float(lights[1, m]), float(lights[2, m]))
        for i in range(n):
            out[:, m * n + i] = light_point(X, Y, s, b, m, i, seed, c, float(radius[m]))
    return out


def _init():
    from oracle import gen_golden as gg
    _W["mods"] = gg._import_reference()
    from gen_refraction_golden import continuation
    from gen_scatter_golden import scatter
    _W["refract"], _W["scatter"] = continuation, scatter


def _line_misses(c, L, spheres):
    """True if the line through c with direction L misses every sphere of `spheres` (float64, with a margin)."""
    cc = spheres[0:3].astype(np.float64)
    r2 = spheres[3].astype(np.float64) ** 2
    A = np.asarray(c, dtype=np.float64)[:, None] - cc
    Lv = np.asarray(L, dtype=np.float64)
    s = Lv @ A
    D = s * s - ((A * A).sum(axis=0) - r2)
    return bool((D < -1e-9).all())


def _shadow_events(Pb, N, Qs, lamb_n, n, lights, spheres, planes, events):
    """Recount trace()'s shadow queries of one hit: partly occluded lights (penumbra) and anchor-certified misses."""
    trace, common = _W["mods"][1], _W["mods"][2]
    L = Qs.shape[1] // n
    for m in range(L):
        blocked = clear = 0
        for i in range(n):
            Ld = common.get_vector_to_light(Pb, Qs, m * n + i)
            if not lamb_n * common.dot(Ld, N) > 0:
                continue
            _, _, typ = trace.get_intersection(Pb, Ld, spheres, planes)
            if typ == 404:
                clear += 1
                continue
            blocked += 1
            if typ == 0 and "anchor_miss" not in events:
                _, _, ptyp = trace.get_intersection(Pb, Ld, spheres[:, :0], planes)
                if ptyp == 404 and _line_misses(lights[0:3, m], Ld, spheres):
                    events.add("anchor_miss")
        if blocked and clear:
            events.add("penumbra")


def _sample(o, d, spheres, lights, radius, n, planes, table, sid, pid, depth, key, events):
    """trace.py:115-133 with per-object materials, transparent continuations, rough reflections and area lights."""
    trace, common = _W["mods"][1], _W["mods"][2]

    def run(o_, d_, b):
        Qs = soft_lights(lights, radius, n, key, b)
        t, idx, typ = trace.get_intersection(o_, d_, spheres, planes)
        m = table[sid[idx]] if typ == 0 else (table[pid[idx]] if typ == 1 else None)
        amb, lamb = (m[0], m[1]) if m is not None else (np.float64(0.0), np.float64(0.0))
        lamb_n = np.float64(lamb) / np.float64(n)
        res = trace.trace(o_, d_, spheres, Qs, planes, np.float64(amb), lamb_n)
        cont = None
        if m is not None:                                       # the same P and N as trace() forms them
            P = common.linear_comb(o_, d_, 1.0, t)
            N = common.get_sphere_normal(P, idx, spheres) if typ == 0 else common.get_plane_normal(idx, planes)
            _shadow_events(common.linear_comb(P, N, 1.0, BIAS), N, Qs, lamb_n, n, lights, spheres, planes, events)
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
        W = c if W is None else W * c                             # ((c_0 * c_1) * ...) * c_{k-1}
        if cont is not None:
            POINT, RD, fallback, keep = cont
            if fallback is not None and not keep:                 # an absorbed rough reflection
                dead = True
                continue
        (RGB_refl, POINT, RD), m, cont = run(POINT, RD, i + 1)
        RGB = common.linear_comb(RGB, RGB_refl, 1.0, W)
    return RGB


def _run(job):
    from oracle.oracle import jitter
    (items, cam_o, cam_R, spheres, lights, radius, n, planes, table, sid, pid, depth, mode, spp, seed, dy, dz) = job
    common = _W["mods"][2]
    o = (cam_o[0], cam_o[1], cam_o[2])
    rows = (cam_R[0, :], cam_R[1, :], cam_R[2, :])
    rgb64, u8, evs = [], [], []
    for x, y, P, nb in items:
        events = set()
        smp = lambda P_, key: _sample(o, common.normalize(common.matmul(rows, P_)), spheres, lights, radius, n, planes,  # noqa: E731
                                      table, sid, pid, depth, key, events)
        if mode == "stochastic":                              # gen_golden._run_stochastic's jitter and mean
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
        evs.append(("penumbra" in events, "anchor_miss" in events))
    return (np.array(rgb64, dtype=np.float64).reshape(-1, 3), np.array(u8, dtype=np.uint8).reshape(-1, 3),
            np.array(evs, dtype=bool).reshape(-1, 2))


NB = ((-1, 0), (1, 0), (0, 1), (0, -1), (-1, 1), (1, 1), (-1, -1), (1, -1))   # kernels.py:53


def pad6(table):
    """A 3-, 5- or 6-column table as six columns (trans 0, ior 1, rough 0): the rows the area-light kernels see."""
    t = np.asarray(table, dtype=np.float64)
    t = t.reshape(-1, t.shape[-1]) if t.ndim == 2 else t.reshape(-1, 3)
    out = np.tile(np.array([0.0, 0.0, 0.0, 0.0, 1.0, 0.0]), (t.shape[0], 1))
    out[:, :t.shape[1]] = t
    return out


def case(pool, jobs, mods, name, w, h, spheres, lights, radius, n, planes, position, euler, table, sid, pid, depth, aa=0, spp=0,
         seed=1, coords=None, scalars=(0.0, 0.6, 0.3), fov=45.0, point=False):
    from oracle import gen_golden as gg
    t0 = time.time()
    common, scene_mod = mods[2], mods[4]
    cam_o, cam_R, pixel_loc = gg.camera_arrays(scene_mod, w, h, list(position), list(euler), fov)
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
        if aa == 1 and 1 <= x and x + 1 <= w and 1 <= y and y + 1 <= h:   # kernels.py:29 (coords exclude the last row / column)
            nb = [((dx, dy_), common.linear_comb(P, pixel_loc[0:3, x + dx, y + dy_], 0.5, 0.5)) for dx, dy_ in NB]
        items.append((x, y, P, nb))
    ar = int(w / h)
    dy, dz = (-ar - ar) / float(w - 1), (-1 - 1) / float(h - 1)
    mode = "stochastic" if aa == 2 else "pixels"
    chunks = [items[i::jobs * 8] for i in range(min(len(items), jobs * 8))]
    res = pool.map(_run, [(c, cam_o, cam_R, spheres, lights, radius.astype(np.float64), n, planes, pad6(table), sid, pid, depth,
                           mode, spp, seed, dy, dz) for c in chunks])
    order = np.concatenate([np.arange(len(items))[i::jobs * 8] for i in range(len(chunks))])
    rgb64 = np.empty((len(items), 3)); u8 = np.empty((len(items), 3), np.uint8); ev = np.empty((len(items), 2), bool)
    rgb64[order] = np.concatenate([r[0] for r in res]); u8[order] = np.concatenate([r[1] for r in res])
    ev[order] = np.concatenate([r[2] for r in res])
    amb, lamb, refl = scalars
    d = dict(w=w, h=h, spheres=spheres, lights=lights, planes=planes, cam_origin=cam_o, cam_rot=cam_R,
             position=np.array(position, dtype=np.float64), euler=np.array(euler, dtype=np.float64), fov=fov,
             amb=amb, lamb=lamb, refl=refl, depth=depth, aa=aa,
             refl_pow=np.array([np.float64(refl) ** (i + 1) for i in range(max(depth, 1))], dtype=np.float64),
             coords=coords, rgb64=rgb64, u8=u8, materials=table, sphere_material=sid, plane_material=pid, seed=seed,
             light_radius=radius, shadow_samples=n, n_penumbra=int(ev[:, 0].sum()), n_anchor_miss=int(ev[:, 1].sum()))
    if aa == 2:
        d.update(spp=spp)
    if point:                 # the same pixels with every radius 0 (n = 1): rt_set_scene_materials_scatter's frame
        res = pool.map(_run, [(c, cam_o, cam_R, spheres, lights, np.zeros(len(radius)), 1, planes, pad6(table), sid, pid, depth,
                               mode, spp, seed, dy, dz) for c in chunks])
        u8p = np.empty((len(items), 3), np.uint8)
        u8p[order] = np.concatenate([r[1] for r in res])
        d.update(u8_point=u8p)
    path = os.path.join(OUT, f"soft_{name}.npz")
    np.savez_compressed(path, **d)
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(coords)} px, penumbra {d['n_penumbra']} anchor-miss "
          f"{d['n_anchor_miss']}, {time.time() - t0:.1f} s)", flush=True)


MATTE_TABLE = [(0.05, 0.7, 0.0), (0.0, 0.6, 0.3), (0.1, 0.5, 0.1), (0.0, 0.4, 0.6)]   # 3 columns: padded by the library


def main():
    import multiprocessing as mp
    from oracle import gen_golden as gg
    from gen_scatter_golden import DEFAULT_TABLE, GRID_TABLE, grid_ids
    from python_ray_tracer_amd import workloads
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    mods = gg._import_reference()
    L3, P1 = gg.lig(gg.DEFAULT_LIGHTS), gg.pla([gg.DEFAULT_PLANE])
    S6, S8 = gg.sph(gg.DEFAULT_SPHERES), gg.sph(gg.DEFAULT_SPHERES + gg.EXTRA_SPHERES)
    CAM = ([-2, 0, 2.0], [0, -30, 0])
    R3 = [0.5, 0.5, 0.5]
    GLASS5 = [(0.05, 0.7, 0.0, 0.0, 1.0), (0.0, 0.1, 0.0, 0.9, 1.5), (0.0, 0.5, 0.4, 0.0, 1.0)]

    def want(nm):
        return a.only is None or nm in a.only

    def grid(n_side, seed):
        sp = workloads.grid_spheres(n_side, seed)
        return gg.sph([(s.origin, s.radius, s.color) for s in sp])

    with mp.Pool(a.jobs, initializer=_init) as pool:
        c = lambda *x, **k: case(pool, a.jobs, mods, *x, **k)  # noqa: E731
        if want("default"):   # the default scene, matte spheres on a matte floor (a 3-column table), three lights of radius 0.5
            c("default_64_d4", 64, 64, S6, L3, R3, 4, P1, *CAM, MATTE_TABLE, [0, 1, 2, 0, 1, 2], [3], 4, seed=11)
        if want("aa"):        # the 9-tap AA mode, a 5-column table with a glass sphere
            c("aa_48_d2", 48, 48, S6, L3, R3, 4, P1, *CAM, GLASS5, [0, 1, 0, 2, 0, 0], [2], 2, aa=1, seed=9)
        if want("stochastic"):
            c("stoch_40x24_spp3_seed7", 40, 24, S8, L3, R3, 2, P1, *CAM, DEFAULT_TABLE, [0, 1, 2, 3, 4, 5, 3, 5], [6], 2, aa=2,
              spp=3, seed=7)
        if want("mixed"):     # n = 16, a point light (radius 0) beside two area lights
            c("mixed_32_n16_d2", 32, 32, S6, L3, [0.6, 0.0, 0.3], 16, P1, *CAM, MATTE_TABLE, [0, 1, 2, 0, 1, 2], [3], 2, seed=4)
        if want("glass_rough"):   # glass and rough rows together with soft lights
            c("glass_rough_48_d4", 48, 48, S6, L3, [0.4, 0.7, 0.5], 4, P1, *CAM, DEFAULT_TABLE, range(6), [6], 4, seed=13)
        if want("rim"):       # a small sphere beside light 0's centre: the lines to the centre miss it, rays to its ball hit it
            sr = gg.sph(gg.DEFAULT_SPHERES[:3] + [([2.5, -1.7, 3.0], 0.12, gg.GREY)])
            c("rim_48_d2", 48, 48, sr, L3, [0.5, 0.0, 0.0], 4, P1, *CAM, MATTE_TABLE, [0, 1, 2, 0], [3], 2, seed=6,
              point=True)
        if want("many_lights"):   # L = 12 (light indices m up to 11), zero and nonzero radii mixed, n = 16
            L12 = gg.lig(gg.DEFAULT_LIGHTS + [[0.0, -3.0, 2.5], [0.0, 3.0, 2.5], [4.0, -1.0, 1.5], [-1.0, 0.0, 4.0], [3.0, 3.0, 0.8],
                                              [1.0, -1.5, 3.5], [6.0, 2.0, 2.0], [-0.5, 2.0, 1.2], [2.0, 0.0, 5.0]])
            R12 = [0.5, 0.0, 0.3, 0.0, 0.6, 0.2, 0.0, 0.4, 0.25, 0.0, 0.35, 0.5]
            c("many_lights_24_n16_d2", 24, 24, S6, L12, R12, 16, P1, *CAM, MATTE_TABLE, [0, 1, 2, 0, 1, 2], [3], 2, seed=15)
        if want("table256"):      # a 256-row table with ids over every row, 324 spheres (clustered, lane-owned traversal)
            rng = np.random.default_rng(256)
            T = np.zeros((256, 6))
            T[:, 0], T[:, 1], T[:, 2], T[:, 4] = rng.uniform(0, 0.15, 256), rng.uniform(0.2, 0.9, 256), rng.uniform(0, 0.9, 256), 1.0
            T[5::7, 2], T[5::7, 3], T[5::7, 4] = 0.0, 0.85, 1.5                       # glass rows
            T[3::7, 5] = 0.3                                                          # rough rows
            G = grid(18, 357)
            c("table256_s324_32x24_d3", 32, 24, G, L3, R3, 2, P1, *CAM, T, [(i * 37) % 256 for i in range(G.shape[1])], [255], 3,
              seed=17)
        if want("deep16"):        # depth 16 between a mirror floor and a mirror ceiling (refl = 1), glass and rough spheres
            DEEP = [(0.0, 0.1, 0.0, 0.9, 1.5, 0.0), (0.02, 0.3, 1.0, 0.0, 1.0, 0.0), (0.0, 0.4, 0.9, 0.0, 1.0, 0.2),
                    (0.1, 0.6, 0.2, 0.0, 1.0, 0.0), (0.0, 0.3, 1.0, 0.0, 1.0, 0.05)]
            P2 = gg.pla([gg.DEFAULT_PLANE, ([0, 0, 3.2], [0, 0.1, -1], gg.GREY)])
            c("deep16_32_d16", 32, 32, S6, L3, [0.4, 0.0, 0.5], 2, P2, *CAM, DEEP, [1, 0, 2, 1, 0, 1], [4, 1], 16, seed=19)
        if want("spp64"):         # 64 stochastic samples (the key's s up to 63) on a small frame
            c("spp64_16x12_d2", 16, 12, S8, L3, R3, 2, P1, *CAM, DEFAULT_TABLE, [0, 1, 2, 3, 4, 5, 3, 5], [6], 2, aa=2, spp=64,
              seed=23)
        if want("c4"):        # 64 spheres (clustered), 3840x2160 on the sub32 lattice
            cs = [(x, y) for x in range(16, 3840, 32) for y in range(16, 2160, 32)]
            c("c4_s64_d5_sub32", 3840, 2160, grid(8, 355), L3, R3, 2, P1, *CAM, GRID_TABLE, grid_ids(64), [6], 5, coords=cs,
              seed=21)
        if want("c5"):        # 256 spheres (clustered, lane-owned traversal), 7680x4320 on the sub96 lattice
            cs = [(x, y) for x in range(48, 7680, 96) for y in range(48, 4320, 96)]
            c("c5_s256_d8_sub96", 7680, 4320, grid(16, 356), L3, R3, 2, P1, *CAM, GRID_TABLE, grid_ids(256), [6], 8, coords=cs,
              seed=22)


if __name__ == "__main__":
    main()
