#!/usr/bin/env python3
"""Cost of the denoiser: rt_render_guides per frame against rt_render_device, and rt_film_denoise per level against its compulsory
bytes, on the three standing workloads, interleaved, timed with device events.

    python tools/denoise_bench.py [--rounds 5] [--reps 8] [--cases c2,c4,c5] [--out profiles/denoise_bench.json]

  render   rt_render_device with a float32 output, per frame: the parent's single pass on the same scene
  guides   rt_render_guides into eight float32 planes, per frame
  den1     rt_film_denoise with levels = 1 (sigma 1/8, normal_shin 32, demodulate 1), per call: the level that folds in / n, the
           division by the albedo and the multiplication back
  den4     the same with levels = 4, per call; level_ms is a quarter of it
  flat4    levels = 4 with sigma 0 and demodulate 0, per call: the same taps and loads with 3 divisions per pixel and level (and 3 per
           tap on the first level, for / n) instead of 103: what the loads alone cost
One context per workload; the sum is four film passes of the workload.  A round times `reps` calls (--reps for the headline
workload, fewer for the larger ones) of each way in turn; one more round is run first and dropped (the first round of an
interleaved run is slow for every way); the median over the rounds that count is reported with the spread (max - min) / median.
Derived figures:
  guides_vs_render  guides / render
  den*_fraction     the compulsory bytes per second of the call, as a fraction of the 6.29 TB/s of a float4 copy.  Per pixel and
                    level: 24 B of colour read, 24 B written and 16 B of guides (normal and id), plus 12 B of albedo on the first
                    and on the last level (once where they are the same level)
  den*_div_per_s    float64 divisions per second: per pixel and level 4 per tap that passes the id and normal tests (counted as
                    all 25: an upper bound) and 3 for A / W, plus on the first level 6 per tap for / n and / albedo
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import python_ray_tracer_amd as pkg                       # noqa: E402
from python_ray_tracer_amd import workloads               # noqa: E402

CASES = {"c2": ("c2_1920x1080_s8_d3", 1.0), "c4": ("c4_3840x2160_s64_d5", 0.5), "c5": ("c5_7680x4320_s256_d8", 0.25)}
WAYS = ("render", "guides", "den1", "den4", "flat4")
COPY_RATE = 6.29e12                                       # bytes per second of a float4 copy on this chip
SETTINGS = dict(normal_shin=32, sigma=0.125, demodulate=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "denoise_bench.json"))
    a = ap.parse_args()
    out = {"metric": "denoise_cost", "rounds": a.rounds, "reps": a.reps, "copy_rate_TBps": COPY_RATE / 1e12, "settings": SETTINGS}
    for case in a.cases.split(","):
        name, rel = CASES[case]
        reps = max(2, int(round(a.reps * rel)))
        wl = workloads.build(name)
        w, h = wl["w"], wl["h"]
        npx = w * h
        r = pkg.Renderer(0)
        try:
            r.set_scene(wl["spheres"], wl["lights"], wl["planes"])
            r.set_camera(wl["camera"].position, wl["camera"].rotation)
            r.set_raygen(w, h, *wl["camera"].raygen())
            p = r.params(wl["amb"], wl["lamb"], wl["refl"], wl["depth"], wl["aa"], spp=wl["spp"], seed=wl["seed"])
            d32, dg = r.malloc(12 * npx), r.malloc(32 * npx)
            dsum, dout, dwork = r.malloc(24 * npx), r.malloc(24 * npx), r.malloc(24 * npx)
            r.film_accumulate(p, 0, w, 4, True, dsum)

            def run(way):
                for _ in range(reps):
                    if way == "render":
                        r.render_device(p, 0, w, None, d32, npx)
                    elif way == "guides":
                        r.render_guides(0, w, dg, npx)
                    elif way == "flat4":
                        r.film_denoise(dsum, w, h, 4, dg, dout, dwork, levels=4, normal_shin=32, sigma=0.0, demodulate=0)
                    else:
                        r.film_denoise(dsum, w, h, 4, dg, dout, dwork, levels=int(way[3:]), **SETTINGS)

            for way in WAYS:                                  # code objects, cull tables, a settled dispatch order
                run(way)
            r.sync()
            times = {k: [] for k in WAYS}
            for rnd in range(a.rounds + 1):
                for way in WAYS:
                    r.timer_begin()
                    run(way)
                    ms = r.timer_end() / reps
                    if rnd > 0:                                # (round 0: dropped)
                        times[way].append(ms)
            res = {}
            for k, t in times.items():
                t = np.array(t)
                res[k] = dict(ms=round(float(np.median(t)), 5), spread=round(float((t.max() - t.min()) / np.median(t)), 4),
                              rounds_ms=[round(float(v), 5) for v in t])
            res["guides"].update(vs_render=round(res["guides"]["ms"] / res["render"]["ms"], 4), bytes=32 * npx)
            for levels in (1, 4):
                k = f"den{levels}"
                nbytes = npx * (64 * levels + (12 if levels == 1 else 24))
                divs = npx * (levels * (25 * 4 + 3) + 25 * 6)
                sec = res[k]["ms"] * 1e-3
                res[k].update(level_ms=round(res[k]["ms"] / levels, 5), bytes=int(nbytes), fraction=round(nbytes / sec / COPY_RATE, 4),
                              div_per_s=round(divs / sec, 0))
            res["flat4"].update(level_ms=round(res["flat4"]["ms"] / 4, 5), bytes=int(npx * 64 * 4),
                                fraction=round(npx * 256 / (res["flat4"]["ms"] * 1e-3) / COPY_RATE, 4), vs_den4=round(res["flat4"]["ms"] / res["den4"]["ms"], 4))
            for d in (d32, dg, dsum, dout, dwork):
                r.free(d)
            out[case] = dict(workload=name, reps_per_round=reps, pixels=npx, **res)
        finally:
            r.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
