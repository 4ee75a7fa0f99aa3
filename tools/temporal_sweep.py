#!/usr/bin/env python3
"""The sweep behind Film.temporal's defaults: depth_tol, normal_cos and max_history on a camera orbit.

    python tools/temporal_sweep.py [--out profiles/temporal_sweep.json]

The orbit is the one of the tests (tests/temporal_cases.py: orbit_scene): the soft_default_64_d4 scene with a matte floor, area
lights with ONE shadow sample, 8 camera steps of 2 degrees about the point 4 units along the view axis, 4 passes per frame with
seeds that never repeat.  Truth is the mean of 1024 passes at the last camera.  For every setting the film is carried through the
orbit (Film.next_frame, accumulate, temporal) and the last frame's temporal mean, and that mean filtered at Film.denoise's defaults,
are compared with the truth: RMSE in linear colour over the whole frame, over matte pixels (first hit without reflection) and over
the rest; matte pixels are also split into those with an object edge within one pixel and the others.  The raw figure is the last
frame's 4-pass mean, and `denoise` that mean filtered without a history.  Prints a table and one JSON line, and writes the line to
--out.
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import python_ray_tracer_amd as pkg                       # noqa: E402
from python_ray_tracer_amd import denoise as D            # noqa: E402
import temporal_cases as tc                               # noqa: E402

DEPTH_TOL = (0.003, 0.01, 0.03, 0.1, 0.3, 1.0)
NORMAL_COS = (-1.0, 0.5, 0.9, 0.99, 0.999)
MAX_HISTORY = (4.0, 8.0, 16.0, 32.0, 1024.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "temporal_sweep.json"))
    a = ap.parse_args()
    sc = tc.orbit_scene()
    w, h = sc["w"], sc["h"]
    last = sc["cameras"][-1]
    gd = D.guides_reference(sc["spheres"], sc["planes"], last[0], last[1], w, h, raygen=sc["raygen"])
    matte = tc.matte_mask(sc, gd)
    ids = gd[7]
    edge = np.zeros((w, h), bool)                                 # an id edge within one pixel (4-neighbourhood)
    edge[1:, :] |= ids[1:, :] != ids[:-1, :]; edge[:-1, :] |= ids[1:, :] != ids[:-1, :]
    edge[:, 1:] |= ids[:, 1:] != ids[:, :-1]; edge[:, :-1] |= ids[:, 1:] != ids[:, :-1]
    masks = {"all": np.ones((w, h), bool), "matte": matte, "rest": ~matte, "matte_edge": matte & edge, "matte_inner": matte & ~edge}
    with pkg.Renderer(0) as r:
        r.set_scene(sc["spheres"], sc["lights"], sc["planes"], materials=sc["materials"], light_radius=sc["light_radius"], shadow_samples=1)
        r.set_raygen(w, h, *sc["raygen"])
        params_of = lambda seed: r.params(0.0, 0.0, 0.0, sc["depth"], 0, seed=seed)

        def read(d, shape, dtype=np.float64):
            out = np.empty(shape, dtype)
            r.d2h(out, d)
            return out

        r.set_camera(*last)
        with pkg.Film(r) as film:
            film.accumulate(params_of(5000), 1024)
            r.sync()
            truth = read(film.d_sum, (3, w, h)) / 1024.0
        rmse = lambda x: {k: round(float(np.sqrt(np.mean((x - truth)[:, m] ** 2))), 4) for k, m in masks.items()}

        def orbit(depth_tol, normal_cos, max_history):
            with pkg.Film(r) as film:
                for k, cam in enumerate(sc["cameras"]):
                    r.set_camera(*cam)
                    film.next_frame()
                    film.accumulate(params_of(1 + tc.ORBIT_PASSES * k), tc.ORBIT_PASSES)
                    film.temporal(max_history=max_history, depth_tol=depth_tol, normal_cos=normal_cos)
                film.denoise(temporal=True)
                r.sync()
                res = dict(temporal=rmse(read(film.d_temporal, (3, w, h))), temporal_denoise=rmse(read(film.d_denoised, (3, w, h))))
                ln = read(film.d_temporal_len, (w, h), np.float32)
                res.update(mean_length=round(float(ln.mean()), 2), fresh=int((ln == tc.ORBIT_PASSES).sum()))
                raw = rmse(read(film.d_sum, (3, w, h)) / float(tc.ORBIT_PASSES))
                film.denoise()
                r.sync()
                return res, raw, rmse(read(film.d_denoised, (3, w, h)))

        rows = []
        for dt, nc, mh in itertools.product(DEPTH_TOL, NORMAL_COS, MAX_HISTORY):
            res, raw, den = orbit(dt, nc, mh)
            rows.append(dict(depth_tol=dt, normal_cos=nc, max_history=mh, **res))
    out = dict(metric="temporal_sweep", steps=tc.ORBIT_STEPS, passes=tc.ORBIT_PASSES, degrees=tc.ORBIT_DEGREES, pixels={k: int(m.sum()) for k, m in masks.items()},
               raw=raw, denoise=den, rows=rows)
    print(f"raw {raw}  denoise alone {den}  ({int(matte.sum())} of {w * h} pixels matte)")
    print("depth_tol normal_cos max_history | temporal all matte rest | +denoise all matte rest | mean length, fresh pixels")
    for row in rows:
        t, d = row["temporal"], row["temporal_denoise"]
        print(f"{row['depth_tol']:9g} {row['normal_cos']:10g} {row['max_history']:11g} | {t['all']:7.4f} {t['matte']:7.4f} {t['rest']:7.4f} | "
              f"{d['all']:7.4f} {d['matte']:7.4f} {d['rest']:7.4f} | {row['mean_length']:6.2f} {row['fresh']:5d}")
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
