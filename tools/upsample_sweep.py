#!/usr/bin/env python3
"""The sweep behind Upsampler.upsample's default normal_cos, and what a film at half resolution loses at an equal ray budget.  It runs
on the CPU: the frames are the oracle's, the filter and the lift are the numpy restatements (python-ray-tracer_amd/variance.py:
denoise_variance_reference; upsample.py: upsample_reference), which the kernels match bit for bit.

    python tools/upsample_sweep.py [--out profiles/upsample_sweep.json]

The scene and the truth are those of the variance sweep (tests/variance_cases.py): soft_default_64_d4 with area lights and ONE shadow
sample, truth the mean of 1024 passes at 64 x 64.  RMSE in linear colour against it, over the whole frame and over matte pixels (first
hit without reflection), of:
  full4_raw, full4_denoised     4 passes at 64 x 64, the raw mean and the variance-guided filter at Film's defaults
  nearest, bilinear             16 passes at 32 x 32 (the same ray count), filtered the same way, then replicated / interpolated plainly
  cos<c>_dem<d>                 that filtered mean through upsample_reference with normal_cos c in 0, 0.5, 0.8, 0.9, 0.95, 0.99, with
                                (d = 1) and without demodulation; the shares of pixels of kind 1 and 2 stand beside every row
NORMAL_COS is the largest normal_cos whose whole-frame RMSE with demodulation is within 1 % of the best of the six.  Prints the table and
one JSON line, and writes the line to --out.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import raygen_closed_form                   # noqa: E402
from oracle import oracle as orc                          # noqa: E402
from python_ray_tracer_amd import denoise as D            # noqa: E402
from python_ray_tracer_amd import upsample as U           # noqa: E402
from python_ray_tracer_amd import variance as V           # noqa: E402
import temporal_cases as tc                               # noqa: E402
import variance_cases as vc                               # noqa: E402

COSINES = (0.0, 0.5, 0.8, 0.9, 0.95, 0.99)
FULL_PASSES, LOW_PASSES, RATIO = 4, 16, 2


def low_frames(g, wl, hl, rg, n):
    seed = int(g["seed"])
    return [orc.render(wl, hl, g["cam_origin"], g["cam_rot"], g["spheres"], g["lights"], g["planes"], 0.0, 0.0, 0.0, int(g["depth"]), False,
                       raygen=rg, want=("f32",), seed=seed + i, materials=(g["materials"], g["sphere_material"], g["plane_material"]),
                       light_radius=g["light_radius"], shadow_samples=1)["f32"] for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "upsample_sweep.json"))
    a = ap.parse_args()
    orc.build()
    g = vc.fixture()
    w, h = vc.size()
    wl, hl = w // RATIO, h // RATIO
    truth, hg = vc.oracle_truth(orc), vc.guides()
    hi_grid, lo_grid = raygen_closed_form(w, h, float(g["fov"])), raygen_closed_form(wl, hl, float(g["fov"]))
    lg = D.guides_reference(g["spheres"], g["planes"], g["cam_origin"], g["cam_rot"], wl, hl, raygen=lo_grid)
    matte = tc.matte_mask(dict(materials=(g["materials"], g["sphere_material"], g["plane_material"])), hg)
    filt = lambda s, q, n, gd: V.denoise_variance_reference(s, q, n, gd, vc.LEVELS, vc.NORMAL_SHIN, V.KAPPA, 0.0, 1, 1)[:3]

    def errors(pic, kind=None):
        d2 = ((pic - truth) ** 2).mean(axis=0)
        row = dict(all=round(float(np.sqrt(d2.mean())), 4), matte=round(float(np.sqrt(d2[matte].mean())), 4))
        if kind is not None:
            row.update(kind1=round(float((kind == 1.0).mean()), 4), kind2=round(float((kind == 2.0).mean()), 4))
        return row

    s4, q4 = V.accumulate_moments_reference(None, None, vc.oracle_frames(orc, FULL_PASSES))
    s16, q16 = V.accumulate_moments_reference(None, None, low_frames(g, wl, hl, lo_grid, LOW_PASSES))
    low = filt(s16, q16, LOW_PASSES, lg)
    rows = {"full4_raw": errors(s4 / FULL_PASSES), "full4_denoised": errors(filt(s4, q4, FULL_PASSES, hg)), "low16_raw_bilinear": None}
    nowhere = np.array(hg)
    nowhere[7] = -5.0                                       # an id the low frame does not have: every pixel the plain bilinear mean
    rows["low16_raw_bilinear"] = errors(U.upsample_reference(s16, LOW_PASSES, lg, nowhere, lo_grid, hi_grid, 0.0, 0)[0])
    rows["bilinear"] = errors(U.upsample_reference(low, 1, lg, nowhere, lo_grid, hi_grid, 0.0, 0)[0])
    ix = np.clip(np.floor(np.arange(w) * (wl - 1) / (w - 1) + 0.5).astype(int), 0, wl - 1)
    iy = np.clip(np.floor(np.arange(h) * (hl - 1) / (h - 1) + 0.5).astype(int), 0, hl - 1)
    rows["nearest"] = errors(low[:, ix][:, :, iy])
    for cos in COSINES:
        for dem in (1, 0):
            pic, kind = U.upsample_reference(low, 1, lg, hg, lo_grid, hi_grid, cos, dem)
            rows[f"cos{cos:g}_dem{dem}"] = errors(pic, kind)
    best = min(rows[f"cos{c:g}_dem1"]["all"] for c in COSINES)
    choice = max(c for c in COSINES if rows[f"cos{c:g}_dem1"]["all"] <= 1.01 * best)
    chosen = rows[f"cos{choice:g}_dem1"]
    out = dict(metric="upsample_sweep", scene="soft_default_64_d4", shadow_samples=1, truth_passes=vc.TRUTH_PASSES, full=[w, h], low=[wl, hl],
               full_passes=FULL_PASSES, low_passes=LOW_PASSES, levels=vc.LEVELS, normal_shin=vc.NORMAL_SHIN, kappa=V.KAPPA,
               matte_pixels=int(matte.sum()), rows=rows, choice=choice, default=U.NORMAL_COS,
               upsampled_vs_full_denoised=dict(all=round(chosen["all"] / rows["full4_denoised"]["all"], 4),
                                               matte=round(chosen["matte"] / rows["full4_denoised"]["matte"], 4)))
    print(f"{'row':22s} {'all':>8s} {'matte':>8s}  kind1  kind2     ({int(matte.sum())} of {w * h} pixels matte)")
    for name, r in rows.items():
        print(f"{name:22s} {r['all']:8.4f} {r['matte']:8.4f}  " + (f"{r['kind1']:.4f} {r['kind2']:.4f}" if "kind1" in r else ""))
    print(f"choice: normal_cos = {choice} (the module's NORMAL_COS is {U.NORMAL_COS}); upsampled / full-resolution denoised at equal rays: "
          f"{out['upsampled_vs_full_denoised']}")
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
