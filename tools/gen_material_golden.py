#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — fixtures of per-object materials (runs only where the reference checkout is, as
oracle/gen_golden.py does; it changes nothing under oracle/).

The reference has one (ambient_int, lambert_int, reflection_int) per frame.  With a material table, trace k of a sample
(k = 0 the primary ray) that hits an object of material (amb_k, lamb_k, refl_k) is the reference's own trace()
(trace.py:44-112) called with ambient_int = amb_k and lambert_int = lamb_k — the material is learnt from the reference's
own get_intersection() on the same ray — and its colour is added with W_k = ((refl_0 * refl_1) * ...) * refl_{k-1} in
place of reflection_int ** k (trace.py:131).  The sample() loop (trace.py:115-133) and the render() pixel loop
(kernels.py:7-73, incl. the 9-tap AA and its G/B order) are restated below with that one change; the stochastic mode
jitters as oracle/gen_golden.py:_run_stochastic does.

Writes tests/golden/materials_<case>.npz: the keys of the frame_*.npz fixtures plus `materials` (M,3),
`sphere_material` (S,), `plane_material` (P,).  (Not frame_*: tests/conftest.py runs those against the global shading.)

Usage:  python tools/gen_material_golden.py [--only NAME ...] [--jobs 8]
"""
import argparse
import os
import sys
import time
import multiprocessing as mp

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import gen_golden as gg           # noqa: E402  (reference import, scenes, camera helpers)
from oracle.oracle import jitter              # noqa: E402
from python_ray_tracer_amd import workloads   # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
_W = {}


def _init():
    _W["mods"] = gg._import_reference()


def _sample(o, d, spheres, lights, planes, table, sid, pid, depth):
    """trace.py:115-133 with per-object materials."""
    trace, common = _W["mods"][1], _W["mods"][2]

    def material(o_, d_):
        _, idx, typ = trace.get_intersection(o_, d_, spheres, planes)
        if typ == 0:
            return table[sid[idx]]
        if typ == 1:
            return table[pid[idx]]
        return None                                           # a miss: trace() returns black without shading

    def run(o_, d_):
        m = material(o_, d_)
        amb, lamb = (m[0], m[1]) if m is not None else (np.float64(0.0), np.float64(0.0))
        return trace.trace(o_, d_, spheres, lights, planes, np.float64(amb), np.float64(lamb)), m

    (RGB, POINT, RD), m = run(o, d)
    W = None
    for _ in range(depth):
        if (POINT[0] == 404. and POINT[1] == 404. and POINT[2] == 404.) or \
                (RD[0] == 404. and RD[1] == 404. and RD[2] == 404.):
            continue
        W = m[2] if W is None else W * m[2]                   # ((refl_0 * refl_1) * ...) * refl_{k-1}
        (RGB_refl, POINT, RD), m = run(POINT, RD)
        RGB = common.linear_comb(RGB, RGB_refl, 1.0, W)
    return RGB


def _run(job):
    (items, cam_o, cam_R, spheres, lights, planes, table, sid, pid, depth, mode, spp, seed, dy, dz) = job
    common = _W["mods"][2]
    o = (cam_o[0], cam_o[1], cam_o[2])
    rows = (cam_R[0, :], cam_R[1, :], cam_R[2, :])
    smp = lambda P: _sample(o, common.normalize(common.matmul(rows, P)), spheres, lights, planes, table, sid, pid, depth)  # noqa: E731
    rgb64, u8 = [], []
    for x, y, P, nb in items:
        if mode == "stochastic":                              # gen_golden._run_stochastic's jitter and mean
            acc = None
            for s_ in range(spp):
                u, v = jitter(x, y, s_, seed)
                c = smp((P[0], P[1] + u * dy, P[2] + v * dz))
                acc = c if acc is None else (acc[0] + c[0], acc[1] + c[1], acc[2] + c[2])
            R, G, B = acc[0] / spp, acc[1] / spp, acc[2] / spp
        else:                                                 # kernels.py:19-65
            R, G, B = smp(P)
            if nb is not None:
                for Pn in nb:
                    R_s, G_s, B_s = smp(Pn)
                    R += R_s
                    G += B_s
                    B += G_s
                R, G, B = R / 9, G / 9, B / 9
        rgb64.append((float(R), float(G), float(B)))
        u8.append(common.clip_color_vector((R, G, B)))
    return np.array(rgb64, dtype=np.float64).reshape(-1, 3), np.array(u8, dtype=np.uint8).reshape(-1, 3)


def case(pool, jobs, mods, name, w, h, spheres, lights, planes, position, euler, table, sid, pid, depth, aa=0, spp=0, seed=1,
         coords=None, scalars=(0.0, 0.6, 0.3), fov=45.0):
    t0 = time.time()
    common, scene_mod = mods[2], mods[4]
    cam_o, cam_R, pixel_loc = gg.camera_arrays(scene_mod, w, h, list(position), list(euler), fov)
    if coords is None:
        coords = gg.all_coords(w, h, w - 1, h - 1) if aa == 1 else gg.all_coords(w, h)
    coords = np.asarray(coords, dtype=np.int32).reshape(-1, 2)
    table = np.asarray(table, dtype=np.float64).reshape(-1, 3)
    sid, pid = np.asarray(sid, dtype=np.int32), np.asarray(pid, dtype=np.int32)
    items = []
    for x, y in coords:
        x, y = int(x), int(y)
        P = pixel_loc[0:3, x, y]
        nb = None
        if aa == 1 and 1 <= x and x + 1 <= w and 1 <= y and y + 1 <= h:   # kernels.py:29 (coords exclude the last row / column)
            nb = [common.linear_comb(P, pixel_loc[0:3, x + dx, y + dy_], 0.5, 0.5)
                  for dx, dy_ in ((-1, 0), (1, 0), (0, 1), (0, -1), (-1, 1), (1, 1), (-1, -1), (1, -1))]
        items.append((x, y, P, nb))
    ar = int(w / h)
    dy, dz = (-ar - ar) / float(w - 1), (-1 - 1) / float(h - 1)
    mode = "stochastic" if aa == 2 else "pixels"
    chunks = [items[i::jobs * 8] for i in range(min(len(items), jobs * 8))]
    res = pool.map(_run, [(c, cam_o, cam_R, spheres, lights, planes, table, sid, pid, depth, mode, spp, seed, dy, dz) for c in chunks])
    order = np.concatenate([np.arange(len(items))[i::jobs * 8] for i in range(len(chunks))])
    rgb64 = np.empty((len(items), 3)); u8 = np.empty((len(items), 3), np.uint8)
    rgb64[order] = np.concatenate([r[0] for r in res]); u8[order] = np.concatenate([r[1] for r in res])
    amb, lamb, refl = scalars
    d = dict(w=w, h=h, spheres=spheres, lights=lights, planes=planes, cam_origin=cam_o, cam_rot=cam_R,
             position=np.array(position, dtype=np.float64), euler=np.array(euler, dtype=np.float64), fov=fov,
             amb=amb, lamb=lamb, refl=refl, depth=depth, aa=aa,
             refl_pow=np.array([np.float64(refl) ** (i + 1) for i in range(max(depth, 1))], dtype=np.float64),
             coords=coords, rgb64=rgb64, u8=u8, materials=table, sphere_material=sid, plane_material=pid)
    if aa == 2:
        d.update(spp=spp, seed=seed)
    path = os.path.join(OUT, f"materials_{name}.npz")
    np.savez_compressed(path, **d)
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(coords)} px, {time.time() - t0:.1f} s)", flush=True)


# distinct materials per object of the default scene: a matte sphere (refl 0), a near-mirror (0.9), one with a negative
# Lambert coefficient, ambient light on some, a mirror floor
DEFAULT_TABLE = [(0.0, 0.6, 0.3), (0.1, 0.6, 0.0), (0.0, 0.5, 0.9), (0.0, -0.4, 0.3), (0.25, 0.4, 0.5), (0.05, 0.8, 0.25),
                 (0.0, 0.3, 0.9), (0.15, 0.7, 0.125)]
GRID_TABLE = [(0.0, 0.6, 0.3), (0.1, 0.6, 0.0), (0.0, 0.5, 0.9), (0.0, -0.4, 0.3), (0.25, 0.4, 0.5), (0.05, 0.8, 0.25), (0.0, 0.3, 0.75)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    mods = gg._import_reference()
    L3, P1 = gg.lig(gg.DEFAULT_LIGHTS), gg.pla([gg.DEFAULT_PLANE])
    S6, S8 = gg.sph(gg.DEFAULT_SPHERES), gg.sph(gg.DEFAULT_SPHERES + gg.EXTRA_SPHERES)
    CAM = ([-2, 0, 2.0], [0, -30, 0])

    def want(n):
        return a.only is None or n in a.only

    def grid(n_side, seed):
        sp = workloads.grid_spheres(n_side, seed)
        return gg.sph([(s.origin, s.radius, s.color) for s in sp])

    with mp.Pool(a.jobs, initializer=_init) as pool:
        c = lambda *x, **k: case(pool, a.jobs, mods, *x, **k)  # noqa: E731
        if want("default"):   # one material per object (6 spheres, then the floor)
            c("default_64_d3", 64, 64, S6, L3, P1, *CAM, DEFAULT_TABLE[:7], range(6), [6], 3)
        if want("uniform"):   # one power-of-two material for everything: the global path's frame, bit for bit
            c("uniform_48_d4", 48, 48, S6, L3, P1, *CAM, [(0.05, 0.6, 0.5)], [0] * 6, [0], 4, scalars=(0.05, 0.6, 0.5))
        if want("aa"):
            c("aa_48_d2", 48, 48, S6, L3, P1, *CAM, DEFAULT_TABLE[:7], range(6), [6], 2, aa=1)
        if want("stochastic"):
            c("stoch_40x24_spp3_seed7", 40, 24, S8, L3, P1, *CAM, DEFAULT_TABLE, [0, 1, 2, 3, 4, 5, 1, 4], [6], 1, aa=2, spp=3,
              seed=7)
        if want("c4"):        # 64 spheres (clustered), 3840x2160 on the sub32 lattice
            cs = [(x, y) for x in range(16, 3840, 32) for y in range(16, 2160, 32)]
            c("c4_s64_d5_sub32", 3840, 2160, grid(8, 355), L3, P1, *CAM, GRID_TABLE, [i % 7 for i in range(64)], [64 % 7], 5,
              coords=cs)
        if want("c5"):        # 256 spheres (clustered, lane-owned traversal), 7680x4320 on the sub96 lattice
            cs = [(x, y) for x in range(48, 7680, 96) for y in range(48, 4320, 96)]
            c("c5_s256_d8_sub96", 7680, 4320, grid(16, 356), L3, P1, *CAM, GRID_TABLE, [i % 7 for i in range(256)], [256 % 7], 8,
              coords=cs)


if __name__ == "__main__":
    main()
