#!/usr/bin/env python3
"""The sweep behind Film.denoise(variance=True)'s default kappa.  It runs on the CPU: the frames are the oracle's, the filter is the
numpy restatement (python-ray-tracer_amd/variance.py: denoise_variance_reference), which the kernels match bit for bit.

    python tools/variance_sweep.py [--out profiles/variance_sweep.json]

The scene and the truth are those of the tests (tests/variance_cases.py): soft_default_64_d4 with area lights and ONE shadow sample,
truth the mean of 1024 passes.  For n = 2, 4, 8, 16 passes, prefilter 0 and 1, demodulate 0 and 1 and kappa 0.5 .. 4 the filtered mean
at levels 4, normal shininess 32, var_floor 0 is compared with the truth: RMSE in linear colour over all pixels, as a ratio to the raw
mean's.  `parent` is rt_film_denoise at its defaults (sigma 1/8, demodulation) on the same frames.  The default is chosen among the
rows with prefilter and demodulation (Film's defaults): the kappa with the lowest RMSE at n = 4 among those whose ratio to raw is below
1 at every n.  Prints the tables and one JSON line, and writes the line to --out.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from oracle import oracle as orc                          # noqa: E402
from python_ray_tracer_amd import denoise as D            # noqa: E402
from python_ray_tracer_amd import film as F               # noqa: E402
from python_ray_tracer_amd import variance as V           # noqa: E402
import variance_cases as vc                               # noqa: E402

KAPPAS = (0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "variance_sweep.json"))
    a = ap.parse_args()
    orc.build()
    truth, gd = vc.oracle_truth(orc), vc.guides()
    sums, raw, parent = {}, {}, {}
    for n in vc.QUALITY_N:
        sums[n] = V.accumulate_moments_reference(None, None, vc.oracle_frames(orc, n))
        raw[n] = vc.rmse(sums[n][0] / n, truth)
        parent[n] = vc.rmse(D.denoise_reference(sums[n][0], n, gd, vc.LEVELS, vc.NORMAL_SHIN, F.DENOISE_SIGMA, 1), truth) / raw[n]
    rows = []
    for dem in (0, 1):
        for pre in (0, 1):
            for kappa in KAPPAS:
                ratio = {n: vc.rmse(V.denoise_variance_reference(*sums[n], n, gd, vc.LEVELS, vc.NORMAL_SHIN, kappa, 0.0, dem, pre), truth) / raw[n]
                         for n in vc.QUALITY_N}
                rows.append(dict(demodulate=dem, prefilter=pre, kappa=kappa, ratio={str(n): round(r, 4) for n, r in ratio.items()}))
    eligible = [r for r in rows if r["demodulate"] == 1 and r["prefilter"] == 1 and all(v < 1.0 for v in r["ratio"].values())]
    choice = min(eligible, key=lambda r: r["ratio"]["4"])["kappa"] if eligible else None
    out = dict(metric="variance_sweep", scene="soft_default_64_d4", shadow_samples=1, truth_passes=vc.TRUTH_PASSES, levels=vc.LEVELS,
               normal_shin=vc.NORMAL_SHIN, var_floor=0.0, raw_rmse={str(n): round(v, 4) for n, v in raw.items()},
               parent_ratio={str(n): round(v, 4) for n, v in parent.items()}, rows=rows, choice=choice)
    print("raw RMSE      " + "  ".join(f"n={n}: {raw[n]:.3f}" for n in vc.QUALITY_N))
    print("parent ratio  " + "  ".join(f"n={n}: {parent[n]:.3f}" for n in vc.QUALITY_N))
    print("demodulate prefilter kappa | " + " ".join(f"n={n:<5d}" for n in vc.QUALITY_N))
    for r in rows:
        print(f"{r['demodulate']:10d} {r['prefilter']:9d} {r['kappa']:5g} | " + " ".join(f"{r['ratio'][str(n)]:7.4f}" for n in vc.QUALITY_N))
    print(f"choice: kappa = {choice}")
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
