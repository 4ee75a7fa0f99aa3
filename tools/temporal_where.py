#!/usr/bin/env python3
"""Where the error of temporal accumulation sits: the orbit of tools/temporal_sweep.py beside a still camera with the same passes.

    python tools/temporal_where.py > profiles/temporal_where.txt

The scene, the orbit, the seeds and the truth are the sweep's (tests/temporal_cases.py: orbit_scene; one shadow sample; the mean of
1024 passes at the last camera).  For max_history 8 and 32, at Film.temporal's other defaults, the film is carried through the 8
camera steps and, for comparison, through 8 frames of the last camera alone.  Printed per run, over matte pixels without an object
edge within one pixel: the RMSE; the RMSE of pixels whose history has its full length and of the others, with their counts; the
mean signed error per channel; the RMSE by object id (6 is the floor).  The first line is the RMSE between two 1024-pass means of
different seeds: how far the truth itself is from its limit.
"""
import os, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
import python_ray_tracer_amd as pkg
from python_ray_tracer_amd import denoise as D
import temporal_cases as tc
sc = tc.orbit_scene(); w, h = sc["w"], sc["h"]; last = sc["cameras"][-1]
gd = D.guides_reference(sc["spheres"], sc["planes"], last[0], last[1], w, h, raygen=sc["raygen"])
matte = tc.matte_mask(sc, gd); ids = gd[7]
edge = np.zeros((w, h), bool)
edge[1:, :] |= ids[1:, :] != ids[:-1, :]; edge[:-1, :] |= ids[1:, :] != ids[:-1, :]
edge[:, 1:] |= ids[:, 1:] != ids[:, :-1]; edge[:, :-1] |= ids[:, 1:] != ids[:, :-1]
inner = matte & ~edge
with pkg.Renderer(0) as r:
    r.set_scene(sc["spheres"], sc["lights"], sc["planes"], materials=sc["materials"], light_radius=sc["light_radius"], shadow_samples=1)
    r.set_raygen(w, h, *sc["raygen"])
    P = lambda seed: r.params(0.0, 0.0, 0.0, sc["depth"], 0, seed=seed)
    def read(d, shape, dt=np.float64):
        a = np.empty(shape, dt); r.d2h(a, d); return a
    r.set_camera(*last)
    with pkg.Film(r) as f:
        f.accumulate(P(5000), 1024); r.sync(); truth = read(f.d_sum, (3, w, h)) / 1024.0
    with pkg.Film(r) as f:
        f.accumulate(P(9000), 1024); r.sync(); truth2 = read(f.d_sum, (3, w, h)) / 1024.0
    rm = lambda x, m: float(np.sqrt(np.mean((x - truth)[:, m] ** 2))) if m.any() else float("nan")
    print("two 1024-pass means differ by (rmse, inner)", rm(truth2, inner))
    for cams, tag in ((sc["cameras"], "orbit"), ([last] * 8, "still")):
        for mh in (8.0, 32.0):
            with pkg.Film(r) as f:
                for k, cam in enumerate(cams):
                    r.set_camera(*cam); f.next_frame(); f.accumulate(P(1 + 4 * k), 4); f.temporal(max_history=mh)
                r.sync()
                t, ln = read(f.d_temporal, (3, w, h)), read(f.d_temporal_len, (w, h), np.float32)
            full = ln >= (mh + 4 if mh < 30 else 31.5)
            print(tag, "max_history", mh, "inner rmse", round(rm(t, inner), 4), "| full-length inner", int((inner & full).sum()), round(rm(t, inner & full), 4),
                  "| short inner", int((inner & ~full).sum()), round(rm(t, inner & ~full), 4), "| bias per channel (inner, full)", np.round((t - truth)[:, inner & full].mean(axis=1), 3),
                  "| by id:", {int(i): round(rm(t, inner & (ids == i)), 3) for i in np.unique(ids[inner])})
