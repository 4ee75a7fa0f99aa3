#!/usr/bin/env python3
"""The sweep behind Film.denoise(variance=True, temporal=True)'s default spatial_below (python-ray-tracer_amd/variance.py:
SPATIAL_BELOW).  The arithmetic is the numpy restatements (temporal.temporal_moments_reference,
variance.denoise_variance_temporal_reference), which the kernels match bit for bit; only the pass frames come from a renderer: the
CPU oracle's by default, the device's with --device.

    python tools/temporal_variance_sweep.py [--device] [--out profiles/temporal_variance_sweep.json]

The orbit is the one of the tests (tests/temporal_cases.py: orbit_scene): the soft_default_64_d4 scene with a matte floor, area lights
with ONE shadow sample, 8 camera steps of 2 degrees, seeds that never repeat; truth the mean of 1024 passes at the last camera.  For 1,
2 and 4 passes per frame the film's moments are carried through the orbit at Film.temporal's defaults, and the last frame is compared
with the truth, RMSE in linear colour over the whole frame, matte pixels (first hit without reflection) and mirror pixels (the rest):
  raw                 the last frame's mean of its own passes
  temporal            the temporal mean
  temporal_sigma      the temporal mean through rt_film_denoise at Film.denoise's defaults (sigma 1/8)
  temporal_variance   the temporal mean through rt_film_denoise_variance_temporal, for kappa 0.5 .. 4 and spatial_below 0, 2, 4, 8
  variance            rt_film_denoise_variance on the last frame's own passes at KAPPA (2 and 4 passes per frame: one pass has no variance)
all at levels 4, normal shininess 32, demodulation and the variance prefilter, var_floor 0.  The choice: among the spatial_below values
whose filtered temporal mean does not lose to the unfiltered one over matte pixels at 1, 2 and 4 passes per frame, at kappa = KAPPA, the
one with the lowest matte RMSE at 4 passes per frame (ties: the smallest).  `best_kappa` is the same rule over every kappa: if it is not
KAPPA, a history wants a tolerance of its own.  Prints the tables and one JSON line, and writes the line to --out.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from python_ray_tracer_amd import denoise as D            # noqa: E402
from python_ray_tracer_amd import film as F               # noqa: E402
from python_ray_tracer_amd import temporal as T           # noqa: E402
from python_ray_tracer_amd import variance as V           # noqa: E402
import temporal_cases as tc                               # noqa: E402

PASSES = (1, 2, 4)
KAPPAS = (0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0)
SPATIAL_BELOW = (0.0, 2.0, 4.0, 8.0)
LEVELS, NORMAL_SHIN, TRUTH_SEED, TRUTH_PASSES = 4, 32, 5000, 1024


def oracle_frames(sc):
    """frame(cam, seed) -> float32 (3, w, h) from the CPU oracle."""
    from oracle import oracle as orc
    orc.build()

    def frame(cam, seed):
        return orc.render(sc["w"], sc["h"], cam[0], cam[1], sc["spheres"], sc["lights"], sc["planes"], 0.0, 0.0, 0.0, sc["depth"], False,
                          raygen=sc["raygen"], want=("f32",), seed=seed, materials=sc["materials"], light_radius=sc["light_radius"],
                          shadow_samples=1)["f32"]
    return frame, lambda: None


def device_frames(sc):
    """frame(cam, seed) -> float32 (3, w, h) from rt_render_device."""
    import python_ray_tracer_amd as pkg
    r = pkg.Renderer(0)
    w, h = sc["w"], sc["h"]
    r.set_scene(sc["spheres"], sc["lights"], sc["planes"], materials=sc["materials"], light_radius=sc["light_radius"], shadow_samples=1)
    r.set_raygen(w, h, *sc["raygen"])
    d32 = r.malloc(12 * w * h)

    def frame(cam, seed):
        r.set_camera(*cam)
        r.render_device(r.params(0.0, 0.0, 0.0, sc["depth"], 0, seed=seed), 0, w, None, d32)
        r.sync()
        out = np.empty((3, w, h), np.float32)
        r.d2h(out, d32)
        return out

    def close():
        r.free(d32)
        r.close()
    return frame, close


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true", help="render the pass frames on the GPU instead of with the CPU oracle")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "temporal_variance_sweep.json"))
    a = ap.parse_args()
    sc = tc.orbit_scene()
    w, h, rg, cams = sc["w"], sc["h"], sc["raygen"], sc["cameras"]
    guides = [D.guides_reference(sc["spheres"], sc["planes"], c[0], c[1], w, h, raygen=rg) for c in cams]
    matte = tc.matte_mask(sc, guides[-1])
    masks = {"all": np.ones((w, h), bool), "matte": matte, "mirror": ~matte}
    frame, close = (device_frames if a.device else oracle_frames)(sc)
    try:
        truth = np.zeros((3, w, h))
        for i in range(TRUTH_PASSES):
            truth += frame(cams[-1], TRUTH_SEED + i)
        truth /= TRUTH_PASSES
        rmse = lambda x: {k: round(float(np.sqrt(np.mean((np.asarray(x)[:3] - truth)[:, m] ** 2))), 4) for k, m in masks.items()}
        settings = (T.DEPTH_TOL, T.NORMAL_COS, T.MAX_HISTORY)
        per = {}
        for n in PASSES:
            mean = msq = ln = None
            for k, cam in enumerate(cams):
                s, q = V.accumulate_moments_reference(None, None, [frame(cam, 1 + n * k + i) for i in range(n)])
                if k == 0:
                    mean, msq, ln = s / np.float64(n), q / np.float64(n), np.full((w, h), n, np.float32)
                else:
                    mean, msq, ln = T.temporal_moments_reference(s, q, n, guides[k], mean, msq, ln, guides[k - 1], cam, cams[k - 1], rg, w, h, *settings)
            gd = guides[-1]
            res = dict(raw=rmse(s / np.float64(n)), temporal=rmse(mean),
                       temporal_sigma=rmse(D.denoise_reference(mean, 1, gd, LEVELS, NORMAL_SHIN, F.DENOISE_SIGMA, 1)),
                       variance=rmse(V.denoise_variance_reference(s, q, n, gd, LEVELS, NORMAL_SHIN, V.KAPPA, 0.0, 1, 1)) if n >= 2 else None,
                       mean_length=round(float(ln.mean()), 2), fresh=int((ln == n).sum()), rows=[])
            for kappa in KAPPAS:
                for sb in SPATIAL_BELOW:
                    out, pooled = V.denoise_variance_temporal_reference(mean, msq, ln, gd, LEVELS, NORMAL_SHIN, kappa, 0.0, 1, 1, sb, pooled=True)
                    res["rows"].append(dict(kappa=kappa, spatial_below=sb, pooled=int(pooled.sum()), **rmse(out)))
            per[n] = res
    finally:
        close()

    def matte_of(n, kappa, sb):
        return next(r["matte"] for r in per[n]["rows"] if r["kappa"] == kappa and r["spatial_below"] == sb)

    def choose(kappas):
        ok = [(matte_of(4, k, sb), sb, k) for k in kappas for sb in SPATIAL_BELOW if all(matte_of(n, k, sb) <= per[n]["temporal"]["matte"] for n in PASSES)]
        return min(ok) if ok else None

    at_kappa, over_all = choose((V.KAPPA,)), choose(KAPPAS)
    out = dict(metric="temporal_variance_sweep", frames="device" if a.device else "oracle", steps=tc.ORBIT_STEPS, degrees=tc.ORBIT_DEGREES,
               truth_passes=TRUTH_PASSES, levels=LEVELS, normal_shin=NORMAL_SHIN, var_floor=0.0, kappa=V.KAPPA, temporal=dict(zip(("depth_tol", "normal_cos", "max_history"), settings)),
               pixels={k: int(m.sum()) for k, m in masks.items()}, passes={str(n): per[n] for n in PASSES},
               choice=None if at_kappa is None else dict(spatial_below=at_kappa[1], matte_rmse_at_4=at_kappa[0]),
               best_kappa=None if over_all is None else dict(kappa=over_all[2], spatial_below=over_all[1], matte_rmse_at_4=over_all[0]))
    for n in PASSES:
        p = per[n]
        print(f"\n{n} passes per frame (mean length {p['mean_length']}, {p['fresh']} fresh pixels): all / matte / mirror")
        for k in ("raw", "temporal", "temporal_sigma", "variance"):
            if p[k]:
                print(f"  {k:18s} {p[k]['all']:8.4f} {p[k]['matte']:8.4f} {p[k]['mirror']:8.4f}")
        print("  temporal_variance: kappa spatial_below | all matte mirror | pooled pixels")
        for r in p["rows"]:
            print(f"  {r['kappa']:24g} {r['spatial_below']:13g} | {r['all']:8.4f} {r['matte']:8.4f} {r['mirror']:8.4f} | {r['pooled']:5d}")
    print(f"\nchoice at kappa {V.KAPPA}: {out['choice']};  over every kappa: {out['best_kappa']}")
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
