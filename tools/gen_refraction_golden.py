#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — fixtures of transparent materials (refraction; runs only where the reference checkout is, as
oracle/gen_golden.py does; it changes nothing under oracle/).

A material row is (amb, lamb, refl, trans, ior).  Trace k of a sample is the reference's own trace() (trace.py:44-112) with
ambient_int = amb_k and lambert_int = lamb_k, as in tools/gen_material_golden.py — transparent objects are shaded, and cast
shadows, like opaque ones.  What changes is the continuation: for a hit on a transparent object (trans > 0) the next ray is
the refracted one (a sphere), the totally internally reflected one (a sphere, where Snell's law has no solution) or the
incoming ray carried through (a plane, a thin sheet), from the hit point P = o + t*d and the outward normal N that the
reference's own get_intersection(), linear_comb(), get_sphere_normal() and get_plane_normal() give; the rules are those
documented at rt_set_scene_materials_ex (include/mi355rt.h) and restated in continuation() below.  Bounce k+1 is weighted
with W_{k+1} = W_k * c_k, c_k = trans_k for a transparent hit and refl_k otherwise.

refract() is the pure Snell step; it imports nothing from the reference (tests/test_refraction.py checks it on its own) and
is run here with the reference's linear_comb(), normalize() and dot().

Writes tests/golden/refraction_<case>.npz: the keys of the materials_*.npz fixtures, with `materials` (M,5), plus
n_refract, n_tir and n_pass: the number of sampled pixels whose path took at least one refraction, total internal
reflection and plane pass-through.  (Not materials_*: those are required to have 3 columns.)

Usage:  python tools/gen_refraction_golden.py [--only NAME ...] [--jobs 8]
"""
import argparse
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
BIAS = 0.0002
_W = {}


def _lc(a, b, c1, c2):
    return (c1 * a[0] + c2 * b[0], c1 * a[1] + c2 * b[1], c1 * a[2] + c2 * b[2])


def _normalize(v):
    x, y, z = v
    n = math.sqrt(x * x + y * y + z * z)
    return (x / n, y / n, z / n)


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def refract(d, N, ior, linear_comb=_lc, normalize=_normalize, dot=_dot):
    """The Snell step at a sphere: unit incoming direction d, outward unit normal N, index of refraction ior (> 0).
    Returns (T, n, enter): T the refracted unit direction, or None for total internal reflection; n the normal on the side
    the ray comes from (N entering, -N leaving); enter whether the ray enters (d.N < 0).  float64, in this order:
    c = d.N; entering eta = 1/ior, ci = -c; leaving eta = ior, ci = c; k = 1 - eta^2 (1 - ci^2);
    T = normalize(eta d + (eta ci - sqrt(k)) n) where k >= 0."""
    c = dot(d, N)
    enter = c < 0
    if enter:
        eta, ci, n = 1.0 / ior, -c, N
    else:
        eta, ci, n = ior, c, (-N[0], -N[1], -N[2])
    k = 1.0 - (eta * eta) * (1.0 - ci * ci)
    if k < 0:
        return None, n, enter
    return normalize(linear_comb(d, n, eta, eta * ci - math.sqrt(k))), n, enter


def continuation(d, N, P, row, sphere, common):
    """The next ray (origin, direction) after a hit on a transparent object, and the event ('refract', 'tir' or 'pass')."""
    lc = common.linear_comb
    if sphere:
        T, n, _ = refract(d, N, row[4], lc, common.normalize, common.dot)
        if T is None:
            R = common.get_reflection(d, N)
            return lc(lc(P, n, 1.0, BIAS), R, 1.0, BIAS), R, "tir"
        return lc(lc(P, n, 1.0, -BIAS), T, 1.0, BIAS), T, "refract"
    n = N if common.dot(d, N) < 0 else (-N[0], -N[1], -N[2])   # a thin sheet: ior is ignored
    return lc(lc(P, n, 1.0, -BIAS), d, 1.0, BIAS), d, "pass"


def _init():
    from oracle import gen_golden as gg
    _W["mods"] = gg._import_reference()


def _sample(o, d, spheres, lights, planes, table, sid, pid, depth, events):
    """trace.py:115-133 with per-object materials and transparent continuations."""
    trace, common = _W["mods"][1], _W["mods"][2]

    def run(o_, d_):
        t, idx, typ = trace.get_intersection(o_, d_, spheres, planes)
        m = table[sid[idx]] if typ == 0 else (table[pid[idx]] if typ == 1 else None)
        amb, lamb = (m[0], m[1]) if m is not None else (np.float64(0.0), np.float64(0.0))
        res = trace.trace(o_, d_, spheres, lights, planes, np.float64(amb), np.float64(lamb))
        cont = None
        if m is not None and m[3] > 0:                           # transparent: the same P and N as trace() forms them
            P = common.linear_comb(o_, d_, 1.0, t)
            N = common.get_sphere_normal(P, idx, spheres) if typ == 0 else common.get_plane_normal(idx, planes)
            cont = continuation(d_, N, P, m, typ == 0, common)
        return res, m, cont

    (RGB, POINT, RD), m, cont = run(o, d)
    W = None
    for _ in range(depth):
        if (POINT[0] == 404. and POINT[1] == 404. and POINT[2] == 404.) or \
                (RD[0] == 404. and RD[1] == 404. and RD[2] == 404.):
            continue
        c = m[3] if m[3] > 0 else m[2]
        W = c if W is None else W * c                             # ((c_0 * c_1) * ...) * c_{k-1}
        if cont is not None:
            POINT, RD, ev = cont
            events.add(ev)
        (RGB_refl, POINT, RD), m, cont = run(POINT, RD)
        RGB = common.linear_comb(RGB, RGB_refl, 1.0, W)
    return RGB


def _run(job):
    from oracle.oracle import jitter
    (items, cam_o, cam_R, spheres, lights, planes, table, sid, pid, depth, mode, spp, seed, dy, dz) = job
    common = _W["mods"][2]
    o = (cam_o[0], cam_o[1], cam_o[2])
    rows = (cam_R[0, :], cam_R[1, :], cam_R[2, :])
    rgb64, u8, evs = [], [], []
    for x, y, P, nb in items:
        events = set()
        smp = lambda P_: _sample(o, common.normalize(common.matmul(rows, P_)), spheres, lights, planes, table, sid, pid, depth,  # noqa: E731
                                 events)
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
        evs.append(("refract" in events, "tir" in events, "pass" in events))
    return (np.array(rgb64, dtype=np.float64).reshape(-1, 3), np.array(u8, dtype=np.uint8).reshape(-1, 3),
            np.array(evs, dtype=bool).reshape(-1, 3))


def case(pool, jobs, mods, name, w, h, spheres, lights, planes, position, euler, table, sid, pid, depth, aa=0, spp=0, seed=1,
         coords=None, scalars=(0.0, 0.6, 0.3), fov=45.0):
    from oracle import gen_golden as gg
    t0 = time.time()
    common, scene_mod = mods[2], mods[4]
    cam_o, cam_R, pixel_loc = gg.camera_arrays(scene_mod, w, h, list(position), list(euler), fov)
    if coords is None:
        coords = gg.all_coords(w, h, w - 1, h - 1) if aa == 1 else gg.all_coords(w, h)
    coords = np.asarray(coords, dtype=np.int32).reshape(-1, 2)
    table = np.asarray(table, dtype=np.float64).reshape(-1, 5)
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
    rgb64 = np.empty((len(items), 3)); u8 = np.empty((len(items), 3), np.uint8); ev = np.empty((len(items), 3), bool)
    rgb64[order] = np.concatenate([r[0] for r in res]); u8[order] = np.concatenate([r[1] for r in res])
    ev[order] = np.concatenate([r[2] for r in res])
    amb, lamb, refl = scalars
    d = dict(w=w, h=h, spheres=spheres, lights=lights, planes=planes, cam_origin=cam_o, cam_rot=cam_R,
             position=np.array(position, dtype=np.float64), euler=np.array(euler, dtype=np.float64), fov=fov,
             amb=amb, lamb=lamb, refl=refl, depth=depth, aa=aa,
             refl_pow=np.array([np.float64(refl) ** (i + 1) for i in range(max(depth, 1))], dtype=np.float64),
             coords=coords, rgb64=rgb64, u8=u8, materials=table, sphere_material=sid, plane_material=pid,
             n_refract=int(ev[:, 0].sum()), n_tir=int(ev[:, 1].sum()), n_pass=int(ev[:, 2].sum()))
    if aa == 2:
        d.update(spp=spp, seed=seed)
    path = os.path.join(OUT, f"refraction_{name}.npz")
    np.savez_compressed(path, **d)
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(coords)} px, refract {d['n_refract']} tir {d['n_tir']} "
          f"pass {d['n_pass']}, {time.time() - t0:.1f} s)", flush=True)


GLASS, DIAMOND = (0.0, 0.0, 0.0, 0.9, 1.5), (0.0, 0.0, 0.0, 0.9, 2.4)
# the default scene's spheres: two glass ones (0 clear glass, 5 diamond), matte and mirror ones, a tinted glass (3), a mirror floor
DEFAULT_TABLE = [GLASS, (0.1, 0.6, 0.0, 0.0, 1.0), (0.0, 0.5, 0.9, 0.0, 1.0), (0.05, 0.3, 0.0, 0.7, 1.33),
                 (0.05, 0.8, 0.25, 0.0, 1.0), DIAMOND, (0.0, 0.3, 0.8, 0.0, 1.0)]
GRID_TABLE = [(0.0, 0.6, 0.3, 0.0, 1.0), (0.1, 0.6, 0.0, 0.0, 1.0), GLASS, (0.0, 0.5, 0.9, 0.0, 1.0), (0.25, 0.4, 0.5, 0.0, 1.0),
              (0.02, 0.1, 0.0, 0.85, 2.4), (0.0, 0.3, 0.75, 0.0, 1.0)]


def grid_ids(n):
    """every third sphere glass (rows 2 and 5 alternately), the others opaque rows"""
    opaque = [0, 1, 3, 4]
    return [(2 if (i // 3) % 2 == 0 else 5) if i % 3 == 0 else opaque[i % 4] for i in range(n)]


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
        if want("default"):   # the default scene: glass, diamond and tinted-glass spheres among matte and mirror ones
            c("default_64_d4", 64, 64, S6, L3, P1, *CAM, DEFAULT_TABLE, range(6), [6], 4)
        if want("tir"):       # overlapping diamond spheres seen at grazing angles low over the floor: rays inside one leave
                              # through the other's surface at angles Snell's law cannot bend (a lone sphere never does that)
            st = gg.sph([([1.0, 0.0, 0.6], 0.6, gg.RED), ([1.5, 0.35, 0.7], 0.55, gg.BLUE), ([0.7, -0.55, 0.45], 0.45, gg.GREEN),
                         ([2.6, -0.4, 0.9], 0.9, gg.YELLOW), ([2.2, 1.2, 0.5], 0.5, gg.MAGENTA)])
            tab = [DIAMOND, (0.0, 0.0, 0.0, 0.95, 2.4), (0.05, 0.6, 0.0, 0.0, 1.0), (0.0, 0.3, 0.8, 0.0, 1.0)]
            c("tir_48_d6", 48, 48, st, L3, P1, [-1.5, 0.1, 0.5], [0, -5, 0], tab, [0, 1, 0, 2, 1], [3], 6)
        if want("window"):    # a tilted window (transparent plane) between the camera and the spheres
            pw = gg.pla([gg.DEFAULT_PLANE, ([-0.6, 0.0, 0.0], [1.0, 0.15, 0.05], [200, 220, 255])])
            tab = [(0.0, 0.6, 0.3, 0.0, 1.0), (0.1, 0.6, 0.0, 0.0, 1.0), (0.0, 0.5, 0.9, 0.0, 1.0), (0.02, 0.1, 0.0, 0.8, 1.5), GLASS,
                   (0.0, 0.3, 0.8, 0.0, 1.0)]
            sw = gg.sph(gg.DEFAULT_SPHERES[:3])
            c("window_48_d3", 48, 48, sw, L3, pw, *CAM, tab, [4, 1, 2], [5, 3], 3)
        if want("inside"):    # the camera inside a glass sphere
            si = gg.sph(gg.DEFAULT_SPHERES + [([-2.0, 0.1, 1.9], 0.45, gg.GREY)])
            c("inside_32_d4", 32, 32, si, L3, P1, *CAM, DEFAULT_TABLE, [4, 1, 2, 1, 4, 2, 0], [6], 4)
        if want("overlap"):   # glass spheres overlapping opaque ones: rays inside glass hit opaque spheres from within
            so = gg.sph([([1.0, 0.0, 0.8], 0.8, gg.RED), ([1.0, 0.45, 0.8], 0.35, gg.BLUE), ([0.6, -0.5, 0.5], 0.3, gg.YELLOW),
                         ([2.0, 0.8, 0.7], 0.7, gg.GREEN), ([1.6, 0.5, 0.9], 0.4, gg.MAGENTA)])
            tab = [GLASS, (0.1, 0.6, 0.0, 0.0, 1.0), (0.0, 0.5, 0.9, 0.0, 1.0), DIAMOND, (0.0, 0.3, 0.8, 0.0, 1.0)]
            c("overlap_48_d5", 48, 48, so, L3, P1, *CAM, tab, [0, 1, 2, 3, 1], [4], 5)
        if want("aa"):
            c("aa_48_d2", 48, 48, S6, L3, P1, *CAM, DEFAULT_TABLE, range(6), [6], 2, aa=1)
        if want("stochastic"):
            c("stoch_40x24_spp3_seed7", 40, 24, S8, L3, P1, *CAM, DEFAULT_TABLE, [0, 1, 2, 3, 4, 5, 0, 3], [6], 2, aa=2, spp=3,
              seed=7)
        if want("c4"):        # 64 spheres (clustered), 3840x2160 on the sub32 lattice
            cs = [(x, y) for x in range(16, 3840, 32) for y in range(16, 2160, 32)]
            c("c4_s64_d5_sub32", 3840, 2160, grid(8, 355), L3, P1, *CAM, GRID_TABLE, grid_ids(64), [6], 5, coords=cs)
        if want("c5"):        # 256 spheres (clustered, lane-owned traversal), 7680x4320 on the sub96 lattice
            cs = [(x, y) for x in range(48, 7680, 96) for y in range(48, 4320, 96)]
            c("c5_s256_d8_sub96", 7680, 4320, grid(16, 356), L3, P1, *CAM, GRID_TABLE, grid_ids(256), [6], 8, coords=cs)


if __name__ == "__main__":
    main()
