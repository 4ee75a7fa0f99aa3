#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — fixtures of depth of field (the thin-lens camera of rt_set_lens; runs only where the reference
checkout is, as oracle/gen_golden.py does; it changes nothing under oracle/).

The primary ray of a sample (X, Y, s) is lens_ray()'s (L, D) in place of (cam_o, normalize(R P)); it goes into the reference's
own trace() (trace.py:44-112) with the continuations of tools/gen_soft_shadow_golden.py: per-object materials, transparent
continuations, rough reflections and area lights.  Every table is padded to six columns (trans 0, ior 1, rough 0).

lens_ray() is the pure sampler; it uses only the hash (hash32 of tools/gen_scatter_golden.py, oracle/oracle.py's jitter()
restatement) and imports nothing from the reference (tests/test_lens.py checks it on its own).

Writes tests/golden/lens_<case>.npz: the keys of the soft_*.npz fixtures, with `aperture`, `focus_distance` and u8_pinhole
(the same pixels with aperture 0: the pinhole camera), plus n_anchor_miss (sampled pixels where some lens ray's closest hit
is a sphere that the line through cam_o, with the same direction, misses: a camera-anchored cull table would certify that
ray a miss).

Usage:  python tools/gen_lens_golden.py [--only NAME ...] [--jobs 8]
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
LENS_SALT = 0x1E45D0F5
_W = {}


def lens_candidate(X, Y, s, j, seed):
    """Candidate j of sample (X, Y, s): u_c = (h >> 8) 2^-23 + (2^-24 - 1), c = 0..1 (exact)."""
    return tuple(float(hash32(X, Y, (s * 8 + j) * 2 + c, seed ^ LENS_SALT) >> 8) * 2.0 ** -23 + (2.0 ** -24 - 1.0)
                 for c in range(2))


def disk_point(X, Y, s, seed):
    """The first of the eight candidates with u.u < 1 (u0 u0 + u1 u1, exact), or (0, 0) if none is inside."""
    for j in range(8):
        u = lens_candidate(X, Y, s, j, seed)
        if u[0] * u[0] + u[1] * u[1] < 1.0:
            return u
    return (0.0, 0.0)


def lens_ray(X, Y, s, seed, O, R, P, aperture, focus):
    """(L, D) of sample (X, Y, s), float64, no fused multiply-add (include/mi355rt.h, rt_set_lens):
    v = R P (kernels.py:22 before the normalisation), F = O + (f / P.x) v (linear_comb(O, v, 1.0, f / P.x)),
    L = (O + (a u0) ey) + (a u1) ez with ey, ez columns 1 and 2 of R, D = normalize(F - L)."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    P = tuple(float(c) for c in P)
    O = tuple(float(c) for c in O)
    v = tuple(float(R[i, 0]) * P[0] + float(R[i, 1]) * P[1] + float(R[i, 2]) * P[2] for i in range(3))
    t = float(focus) / P[0]
    F = tuple(1.0 * O[i] + t * v[i] for i in range(3))
    u0, u1 = disk_point(X, Y, s, seed)
    a = float(aperture)
    a0, a1 = a * u0, a * u1
    L = tuple(np.float64((O[i] + a0 * float(R[i, 1])) + a1 * float(R[i, 2])) for i in range(3))
    d = (F[0] - L[0], F[1] - L[1], F[2] - L[2])
    n = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    # (numpy float64 scalars, as the reference's camera origin and directions are: with NumPy >= 2 a plain Python float
    # meeting the float32 scene would be evaluated in float32)
    return L, (d[0] / n, d[1] / n, d[2] / n)


def _init():
    import gen_soft_shadow_golden as gs
    gs._init()
    _W["mods"] = gs._W["mods"]
    _W["sample"] = gs._sample


def _anchor_miss(L, D, cam_o, spheres, planes):
    """True if the closest hit of (L, D) is a sphere that the line through cam_o with direction D misses."""
    from gen_soft_shadow_golden import _line_misses
    trace = _W["mods"][1]
    _, idx, typ = trace.get_intersection(L, D, spheres, planes)
    return typ == 0 and _line_misses(cam_o, D, spheres[:, idx:idx + 1])


def _run(job):
    from oracle.oracle import jitter
    (items, cam_o, cam_R, spheres, lights, radius, n, planes, table, sid, pid, depth, mode, spp, seed, dy, dz, aperture, focus,
     lens) = job
    common = _W["mods"][2]
    O = (cam_o[0], cam_o[1], cam_o[2])
    rows = (cam_R[0, :], cam_R[1, :], cam_R[2, :])
    rgb64, u8, evs = [], [], []
    for x, y, P, nb in items:
        events = set()

        def smp(P_, key):
            if lens:
                o, d = lens_ray(key[0], key[1], key[2], key[3], O, cam_R, P_, aperture, focus)
                if _anchor_miss(o, d, O, spheres, planes):
                    events.add("anchor_miss")
            else:
                o, d = O, common.normalize(common.matmul(rows, P_))
            return _W["sample"](o, d, spheres, lights, radius, n, planes, table, sid, pid, depth, key, set())

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
        evs.append("anchor_miss" in events)
    return (np.array(rgb64, dtype=np.float64).reshape(-1, 3), np.array(u8, dtype=np.uint8).reshape(-1, 3),
            np.array(evs, dtype=bool).reshape(-1))


def focus_on(cam_o, cam_R, point):
    """The forward-axis distance of `point` from the camera: dot(point - O, R e_x) (Camera.focus_on)."""
    d = np.asarray(point, dtype=np.float64) - np.asarray(cam_o, dtype=np.float64)
    return float(np.dot(d, np.asarray(cam_R, dtype=np.float64)[:, 0]))


def case(pool, jobs, mods, name, w, h, spheres, lights, radius, n, planes, position, euler, table, sid, pid, depth, aperture,
         focus_point, aa=0, spp=0, seed=1, coords=None, scalars=(0.0, 0.6, 0.3), fov=45.0):
    from oracle import gen_golden as gg
    from gen_soft_shadow_golden import NB, pad6
    t0 = time.time()
    common, scene_mod = mods[2], mods[4]
    cam_o, cam_R, pixel_loc = gg.camera_arrays(scene_mod, w, h, list(position), list(euler), fov)
    focus = focus_on(cam_o, cam_R, focus_point)
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
    order = np.concatenate([np.arange(len(items))[i::jobs * 8] for i in range(len(chunks))])

    def render(lens):
        res = pool.map(_run, [(c, cam_o, cam_R, spheres, lights, radius.astype(np.float64), n, planes, pad6(table), sid, pid,
                               depth, mode, spp, seed, dy, dz, aperture, focus, lens) for c in chunks])
        rgb64 = np.empty((len(items), 3)); u8 = np.empty((len(items), 3), np.uint8); ev = np.empty(len(items), bool)
        rgb64[order] = np.concatenate([r[0] for r in res]); u8[order] = np.concatenate([r[1] for r in res])
        ev[order] = np.concatenate([r[2] for r in res])
        return rgb64, u8, ev

    rgb64, u8, ev = render(True)
    _, u8p, _ = render(False)
    amb, lamb, refl = scalars
    d = dict(w=w, h=h, spheres=spheres, lights=lights, planes=planes, cam_origin=cam_o, cam_rot=cam_R,
             position=np.array(position, dtype=np.float64), euler=np.array(euler, dtype=np.float64), fov=fov,
             amb=amb, lamb=lamb, refl=refl, depth=depth, aa=aa,
             refl_pow=np.array([np.float64(refl) ** (i + 1) for i in range(max(depth, 1))], dtype=np.float64),
             coords=coords, rgb64=rgb64, u8=u8, materials=table, sphere_material=sid, plane_material=pid, seed=seed,
             light_radius=radius, shadow_samples=n, aperture=np.float64(aperture), focus_distance=np.float64(focus),
             u8_pinhole=u8p, n_anchor_miss=int(ev.sum()))
    if aa == 2:
        d.update(spp=spp)
    path = os.path.join(OUT, f"lens_{name}.npz")
    np.savez_compressed(path, **d)
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(coords)} px, differ from pinhole "
          f"{int((u8 != u8p).any(axis=1).sum())}, anchor-miss {d['n_anchor_miss']}, {time.time() - t0:.1f} s)", flush=True)


def main():
    import multiprocessing as mp
    from oracle import gen_golden as gg
    from gen_scatter_golden import DEFAULT_TABLE, GRID_TABLE, grid_ids
    from gen_soft_shadow_golden import MATTE_TABLE
    from python_ray_tracer_amd import workloads
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    mods = gg._import_reference()
    L3, P1 = gg.lig(gg.DEFAULT_LIGHTS), gg.pla([gg.DEFAULT_PLANE])
    S6, S8 = gg.sph(gg.DEFAULT_SPHERES), gg.sph(gg.DEFAULT_SPHERES + gg.EXTRA_SPHERES)
    CAM = ([-2, 0, 2.0], [0, -30, 0])
    Z3 = [0.0, 0.0, 0.0]
    GLASS5 = [(0.05, 0.7, 0.0, 0.0, 1.0), (0.0, 0.1, 0.0, 0.9, 1.5), (0.0, 0.5, 0.4, 0.0, 1.0)]
    C0 = gg.DEFAULT_SPHERES[0][0]                      # the large red sphere: the usual plane of focus

    def want(nm):
        return a.only is None or nm in a.only

    def grid(n_side, seed):
        sp = workloads.grid_spheres(n_side, seed)
        return gg.sph([(s.origin, s.radius, s.color) for s in sp])

    with mp.Pool(a.jobs, initializer=_init) as pool:
        c = lambda *x, **k: case(pool, a.jobs, mods, *x, **k)  # noqa: E731
        if want("default"):   # the default scene, matte spheres on a matte floor (a 3-column table), focused on sphere 0
            c("default_64_d4", 64, 64, S6, L3, Z3, 1, P1, *CAM, MATTE_TABLE, [0, 1, 2, 0, 1, 2], [3], 4, 0.15, C0, seed=11)
        if want("aa"):        # the 9-tap AA mode, a 5-column table with a glass sphere
            c("aa_48_d2", 48, 48, S6, L3, Z3, 1, P1, *CAM, GLASS5, [0, 1, 0, 2, 0, 0], [2], 2, 0.1, gg.DEFAULT_SPHERES[1][0],
              aa=1, seed=9)
        if want("stochastic"):
            c("stoch_40x24_spp3_seed7", 40, 24, S8, L3, Z3, 1, P1, *CAM, DEFAULT_TABLE, [0, 1, 2, 3, 4, 5, 3, 5], [6], 2, 0.2,
              C0, aa=2, spp=3, seed=7)
        if want("soft_glass_rough"):   # lens, area lights, glass and rough rows together
            c("soft_glass_rough_48_d4", 48, 48, S6, L3, [0.4, 0.7, 0.5], 2, P1, *CAM, DEFAULT_TABLE, range(6), [6], 4, 0.12,
              gg.DEFAULT_SPHERES[3][0], seed=13)
        if want("rim"):       # small spheres and a wide lens: lens rays graze rims that the lines through cam_o miss
            sr = gg.sph(gg.DEFAULT_SPHERES[:3] + [([0.5, 0.0, 1.6], 0.12, gg.GREY), ([-0.4, -0.5, 1.2], 0.08, gg.GREY)])
            c("rim_48_d2", 48, 48, sr, L3, Z3, 1, P1, *CAM, MATTE_TABLE, [0, 1, 2, 0, 1], [3], 2, 0.4, C0, seed=6)
        if want("straddle"):  # a sphere 0.05 beside the camera and a lens of radius 0.15: some lens points are inside it
            ss = gg.sph(gg.DEFAULT_SPHERES[:5] + [([-2.0, 0.55, 2.0], 0.5, gg.GREY)])
            c("straddle_32_d3", 32, 32, ss, L3, Z3, 1, P1, *CAM, DEFAULT_TABLE, [1, 2, 3, 4, 5, 0], [6], 3, 0.15, C0, seed=3)
        if want("c4"):        # 64 spheres (clustered), 3840x2160 on the sub32 lattice
            cs = [(x, y) for x in range(16, 3840, 32) for y in range(16, 2160, 32)]
            c("c4_s64_d5_sub32", 3840, 2160, grid(8, 355), L3, Z3, 1, P1, *CAM, GRID_TABLE, grid_ids(64), [6], 5, 0.1,
              [0.0, 0.0, 0.5], coords=cs, seed=21)
        if want("c5"):        # 256 spheres (clustered, lane-owned traversal), 7680x4320 on the sub96 lattice
            cs = [(x, y) for x in range(48, 7680, 96) for y in range(48, 4320, 96)]
            c("c5_s256_d8_sub96", 7680, 4320, grid(16, 356), L3, Z3, 1, P1, *CAM, GRID_TABLE, grid_ids(256), [6], 8, 0.1,
              [0.0, 0.0, 0.5], coords=cs, seed=22)


if __name__ == "__main__":
    main()
