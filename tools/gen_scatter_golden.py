#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — fixtures of rough materials (scatter; runs only where the reference checkout is, as
oracle/gen_golden.py does; it changes nothing under oracle/).

A material row is (amb, lamb, refl, trans, ior, rough).  Trace b of a sample is the reference's own trace() (trace.py:44-112)
with ambient_int = amb_b and lambert_int = lamb_b, as in tools/gen_material_golden.py; a transparent hit continues as
tools/gen_refraction_golden.py's continuation() says.  What changes is the continuation of a hit on a rough object
(rough > 0) of trace b < depth: instead of trace()'s own mirror ray it is the scattered ray of the rule documented at
rt_set_scene_materials_scatter (include/mi355rt.h) and restated in scatter() below, from the reflection R that trace()
returns, the outward normal N and the biased point Pt that the reference's own get_intersection(), linear_comb(),
get_sphere_normal() and get_plane_normal() give.  A path that is absorbed ends there, like a miss.

ball_point() is the pure candidate search; it uses only the hash (hash32: oracle/oracle.py's jitter() restatement, whose
(u, v) carry the 32 hash bits exactly) and imports nothing from the reference (tests/test_scatter.py checks it on its own).

Writes tests/golden/scatter_<case>.npz: the keys of the refraction_*.npz fixtures, with `materials` (M,6) and `seed`, plus
n_scatter, n_absorbed and n_fallback: the number of sampled pixels whose paths took at least one scatter, were absorbed at
least once and fell back to R at least once (none of the eight candidates inside the ball).

Usage:  python tools/gen_scatter_golden.py [--only NAME ...] [--jobs 8]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from oracle.oracle import jitter  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
BIAS = 0.0002
SEED_SALT = 0x5CA77E12
_W = {}
_C = 2.0 ** -17 - 0.5


def hash32(x, y, s, seed):
    """jitter_hash(x, y, s, seed) (rt_device.h): the 32 bits that oracle.jitter() turns into (u, v), recovered exactly."""
    u, v = jitter(x, y, s, seed)
    return (int((v - _C) * 65536.0) << 16) | int((u - _C) * 65536.0)


def candidate(X, Y, s, b, j, seed):
    """Candidate j of trace b of sample (X, Y, s): q_c = (h >> 8) 2^-23 + (2^-24 - 1), c = 0..2 (exact)."""
    return tuple(float(hash32(X, Y, ((s * 16 + b) * 8 + j) * 4 + c, seed ^ SEED_SALT) >> 8) * 2.0 ** -23 + (2.0 ** -24 - 1.0)
                 for c in range(3))


def ball_point(X, Y, s, b, seed):
    """The first of the eight candidates with q.q < 1 (((qx qx + qy qy) + qz qz), exact), or None."""
    for j in range(8):
        q = candidate(X, Y, s, b, j, seed)
        if (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2] < 1.0:
            return q
    return None


def scatter(R, N, Pt, rough, key, b, common):
    """The scattered continuation (origin, direction, fallback, keep) of a rough hit of trace b with reflection R."""
    X, Y, s, seed = key
    q = ball_point(X, Y, s, b, seed)
    D = R if q is None else common.normalize(common.linear_comb(R, q, 1.0, rough))
    sR, sD = common.dot(R, N), common.dot(D, N)
    keep = (sR > 0 and sD > 0) or (sR < 0 and sD < 0)
    return common.linear_comb(Pt, D, 1.0, BIAS), D, q is None, keep


def _init():
    from oracle import gen_golden as gg
    _W["mods"] = gg._import_reference()
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from gen_refraction_golden import continuation
    _W["refract"] = continuation


def _sample(o, d, spheres, lights, planes, table, sid, pid, depth, key, events):
    """trace.py:115-133 with per-object materials, transparent continuations and scattered rough reflections."""
    trace, common = _W["mods"][1], _W["mods"][2]

    def run(o_, d_, b):
        t, idx, typ = trace.get_intersection(o_, d_, spheres, planes)
        m = table[sid[idx]] if typ == 0 else (table[pid[idx]] if typ == 1 else None)
        amb, lamb = (m[0], m[1]) if m is not None else (np.float64(0.0), np.float64(0.0))
        res = trace.trace(o_, d_, spheres, lights, planes, np.float64(amb), np.float64(lamb))
        cont = None
        if m is not None and (m[3] > 0 or (m[5] > 0 and b < depth)):   # the same P and N as trace() forms them
            P = common.linear_comb(o_, d_, 1.0, t)
            N = common.get_sphere_normal(P, idx, spheres) if typ == 0 else common.get_plane_normal(idx, planes)
            if m[3] > 0:
                o2, d2, ev = _W["refract"](d_, N, P, m[:5], typ == 0, common)
                cont = (o2, d2, None, True)
            else:
                cont = scatter(res[2], N, common.linear_comb(P, N, 1.0, BIAS), m[5], key, b, common)
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
            if fallback is not None:                              # a rough hit
                events.add("scatter")
                if fallback:
                    events.add("fallback")
                if not keep:
                    events.add("absorbed")
                    dead = True
                    continue
        (RGB_refl, POINT, RD), m, cont = run(POINT, RD, i + 1)
        RGB = common.linear_comb(RGB, RGB_refl, 1.0, W)
    return RGB


def _run(job):
    (items, cam_o, cam_R, spheres, lights, planes, table, sid, pid, depth, mode, spp, seed, dy, dz) = job
    common = _W["mods"][2]
    o = (cam_o[0], cam_o[1], cam_o[2])
    rows = (cam_R[0, :], cam_R[1, :], cam_R[2, :])
    rgb64, u8, evs = [], [], []
    for x, y, P, nb in items:
        events = set()
        smp = lambda P_, key: _sample(o, common.normalize(common.matmul(rows, P_)), spheres, lights, planes, table, sid, pid,  # noqa: E731
                                      depth, key, events)
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
        evs.append(("scatter" in events, "absorbed" in events, "fallback" in events))
    return (np.array(rgb64, dtype=np.float64).reshape(-1, 3), np.array(u8, dtype=np.uint8).reshape(-1, 3),
            np.array(evs, dtype=bool).reshape(-1, 3))


NB = ((-1, 0), (1, 0), (0, 1), (0, -1), (-1, 1), (1, 1), (-1, -1), (1, -1))   # kernels.py:53


def case(pool, jobs, mods, name, w, h, spheres, lights, planes, position, euler, table, sid, pid, depth, aa=0, spp=0, seed=1,
         coords=None, scalars=(0.0, 0.6, 0.3), fov=45.0):
    from oracle import gen_golden as gg
    t0 = time.time()
    common, scene_mod = mods[2], mods[4]
    cam_o, cam_R, pixel_loc = gg.camera_arrays(scene_mod, w, h, list(position), list(euler), fov)
    if coords is None:
        coords = gg.all_coords(w, h, w - 1, h - 1) if aa == 1 else gg.all_coords(w, h)
    coords = np.asarray(coords, dtype=np.int32).reshape(-1, 2)
    table = np.asarray(table, dtype=np.float64).reshape(-1, 6)
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
    res = pool.map(_run, [(c, cam_o, cam_R, spheres, lights, planes, table, sid, pid, depth, mode, spp, seed, dy, dz) for c in chunks])
    order = np.concatenate([np.arange(len(items))[i::jobs * 8] for i in range(len(chunks))])
    rgb64 = np.empty((len(items), 3)); u8 = np.empty((len(items), 3), np.uint8); ev = np.empty((len(items), 3), bool)
    rgb64[order] = np.concatenate([r[0] for r in res]); u8[order] = np.concatenate([r[1] for r in res])
    ev[order] = np.concatenate([r[2] for r in res])
    amb, lamb, refl = scalars
    d = dict(w=w, h=h, spheres=spheres, lights=lights, planes=planes, cam_origin=cam_o, cam_rot=cam_R,
             position=np.array(position, dtype=np.float64), euler=np.array(euler, dtype=np.float64), fov=fov,
             amb=amb, lamb=lamb, refl=refl, depth=depth, aa=aa,
             refl_pow=np.array([np.float64(refl) ** (i + 1) for i in range(max(depth, 1))], dtype=np.float64),
             coords=coords, rgb64=rgb64, u8=u8, materials=table, sphere_material=sid, plane_material=pid, seed=seed,
             n_scatter=int(ev[:, 0].sum()), n_absorbed=int(ev[:, 1].sum()), n_fallback=int(ev[:, 2].sum()))
    if aa == 2:
        d.update(spp=spp)
    path = os.path.join(OUT, f"scatter_{name}.npz")
    np.savez_compressed(path, **d)
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(coords)} px, scatter {d['n_scatter']} absorbed "
          f"{d['n_absorbed']} fallback {d['n_fallback']}, {time.time() - t0:.1f} s)", flush=True)


GLASS = (0.0, 0.0, 0.0, 0.9, 1.5, 0.0)
# the default scene's spheres: a glass one (0), a matte one, a mirror, brushed metal (3, 5), a satin sphere; a satin floor
DEFAULT_TABLE = [GLASS, (0.1, 0.6, 0.0, 0.0, 1.0, 0.0), (0.0, 0.5, 0.9, 0.0, 1.0, 0.0), (0.05, 0.3, 0.8, 0.0, 1.0, 0.15),
                 (0.05, 0.8, 0.25, 0.0, 1.0, 0.6), (0.0, 0.2, 0.9, 0.0, 1.0, 0.05), (0.0, 0.3, 0.7, 0.0, 1.0, 0.3)]
GRID_TABLE = [(0.0, 0.6, 0.3, 0.0, 1.0, 0.0), (0.1, 0.6, 0.0, 0.0, 1.0, 0.0), (0.0, 0.5, 0.9, 0.0, 1.0, 0.3),
              (0.0, 0.5, 0.9, 0.0, 1.0, 0.0), (0.25, 0.4, 0.5, 0.0, 1.0, 0.1), (0.02, 0.1, 0.0, 0.85, 2.4, 0.0),
              (0.0, 0.3, 0.75, 0.0, 1.0, 0.2)]


def grid_ids(n):
    """every third sphere rough (rows 2 and 4 alternately), every fifth of the others glass, the rest opaque rows"""
    opaque = [0, 1, 3]
    return [(2 if (i // 3) % 2 == 0 else 4) if i % 3 == 0 else (5 if i % 5 == 0 else opaque[i % 3]) for i in range(n)]


def main():
    sys.path.insert(0, REPO)
    import multiprocessing as mp
    from oracle import gen_golden as gg
    from python_ray_tracer_amd import workloads
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
        if want("default"):   # the default scene: brushed and satin spheres among glass, matte and mirror ones, a satin floor
            c("default_64_d4", 64, 64, S6, L3, P1, *CAM, DEFAULT_TABLE, range(6), [6], 4, seed=11)
        if want("grazing"):   # a rough-1.0 floor and sphere seen low and at grazing angles: absorption and the 8-candidate fallback
            tab = [(0.05, 0.6, 0.8, 0.0, 1.0, 1.0), (0.0, 0.4, 0.9, 0.0, 1.0, 1.0), (0.1, 0.6, 0.0, 0.0, 1.0, 0.0)]
            sg = gg.sph(gg.DEFAULT_SPHERES[:3])
            c("grazing_48_d3", 48, 48, sg, L3, P1, [-3.0, 0.0, 0.35], [0, -4, 0], tab, [1, 2, 1], [0], 3, seed=3)
        if want("inside"):    # the camera inside an opaque rough sphere: rays hit its inside, where R.N < 0
            si = gg.sph(gg.DEFAULT_SPHERES + [([-2.0, 0.1, 1.9], 0.45, gg.GREY)])
            c("inside_32_d4", 32, 32, si, L3, P1, *CAM, DEFAULT_TABLE, [4, 1, 2, 1, 4, 2, 3], [6], 4, seed=5)
        if want("aa"):
            c("aa_48_d2", 48, 48, S6, L3, P1, *CAM, DEFAULT_TABLE, range(6), [6], 2, aa=1, seed=9)
        if want("stochastic"):
            c("stoch_40x24_spp3_seed7", 40, 24, S8, L3, P1, *CAM, DEFAULT_TABLE, [0, 1, 2, 3, 4, 5, 3, 5], [6], 2, aa=2, spp=3,
              seed=7)
        if want("c4"):        # 64 spheres (clustered), 3840x2160 on the sub32 lattice
            cs = [(x, y) for x in range(16, 3840, 32) for y in range(16, 2160, 32)]
            c("c4_s64_d5_sub32", 3840, 2160, grid(8, 355), L3, P1, *CAM, GRID_TABLE, grid_ids(64), [6], 5, coords=cs, seed=21)
        if want("c5"):        # 256 spheres (clustered, lane-owned traversal), 7680x4320 on the sub96 lattice
            cs = [(x, y) for x in range(48, 7680, 96) for y in range(48, 4320, 96)]
            c("c5_s256_d8_sub96", 7680, 4320, grid(16, 356), L3, P1, *CAM, GRID_TABLE, grid_ids(256), [6], 8, coords=cs, seed=22)


if __name__ == "__main__":
    main()
