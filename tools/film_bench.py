#!/usr/bin/env python3
"""Cost of the film: rt_film_accumulate per pass and rt_film_resolve per frame against rt_render_device, on the three standing
workloads, interleaved, timed with device events.

    python tools/film_bench.py [--rounds 5] [--passes 48] [--cases c2,c4,c5] [--out profiles/film_bench.json]

  render       rt_render_device with a float32 output, per frame: what one pass costs without a film
  acc1         rt_film_accumulate with passes = 1, per pass: one render into the scratch and one add kernel per pass
  acc4, acc16  the same with passes = 4 and 16, per pass: four renders per add kernel (one where the scratch of four passes
               would exceed 256 MB: the json says which)
  resolve      rt_film_resolve of the sum to uint8 (white = 400, gamma 2), per frame
One context per workload; its dispatch order is settled by the warm-up.  A round times the same number of passes (a multiple of 16:
--passes for the headline workload, fewer for the larger ones) for each way in turn; one more round is run first and dropped
(the first round of an interleaved run is slow for every way); the median over the rounds that count is reported with the spread
(max - min) / median.  Derived figures:
  acc*_vs_render   (b) / (a): what a pass into the film costs against a frame
  add_us           acc* - render per pass: the add kernel's share (the render into the scratch is the render into any buffer)
  add_fraction     the add kernel's compulsory bytes (4 B per element and pass of float32 read, 16 B per element and add kernel of
                   float64 read and written) per second of add_us, as a fraction of the 6.29 TB/s of a float4 copy
  resolve_fraction the same for the resolve's 24 B read and 3 B written per pixel
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

CASES = {"c2": ("c2_1920x1080_s8_d3", 1.0), "c4": ("c4_3840x2160_s64_d5", 0.34), "c5": ("c5_7680x4320_s256_d8", 0.34)}
WAYS = ("render", "acc1", "acc4", "acc16", "resolve")
COPY_RATE = 6.29e12                                       # bytes per second of a float4 copy on this chip
SCRATCH_MAX = 256 << 20                                   # rt_film.h FILM_SCRATCH_MAX


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--passes", type=int, default=48)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "film_bench.json"))
    a = ap.parse_args()
    out = {"metric": "film_cost", "rounds": a.rounds, "passes": a.passes, "copy_rate_TBps": COPY_RATE / 1e12}
    for case in a.cases.split(","):
        name, rel = CASES[case]
        total = max(16, int(round(a.passes * rel / 16.0)) * 16)
        wl = workloads.build(name)
        w, h = wl["w"], wl["h"]
        npx = w * h
        r = pkg.Renderer(0)
        try:
            r.set_scene(wl["spheres"], wl["lights"], wl["planes"])
            r.set_camera(wl["camera"].position, wl["camera"].rotation)
            r.set_raygen(w, h, *wl["camera"].raygen())
            p = r.params(wl["amb"], wl["lamb"], wl["refl"], wl["depth"], wl["aa"], spp=wl["spp"], seed=wl["seed"])
            d32, d8, dsum = r.malloc(12 * npx), r.malloc(3 * npx), r.malloc(24 * npx)

            def run(way):
                if way == "render":
                    for _ in range(total):
                        r.render_device(p, 0, w, None, d32, npx)
                elif way == "resolve":
                    for _ in range(total):
                        r.film_resolve(dsum, w, h, total, d8, None, white=400.0, gamma=2)
                else:
                    n = int(way[3:])
                    for i in range(total // n):
                        r.film_accumulate(p, 0, w, n, i == 0, dsum)

            for way in WAYS:                                  # code objects, cull tables, the scratch, a settled dispatch order
                run(way)
            r.sync()
            times = {k: [] for k in WAYS}
            for rnd in range(a.rounds + 1):
                for way in WAYS:
                    r.timer_begin()
                    run(way)
                    ms = r.timer_end() / total
                    if rnd > 0:                                # (round 0: dropped)
                        times[way].append(ms)
            res = {}
            for k, t in times.items():
                t = np.array(t)
                res[k] = dict(ms=round(float(np.median(t)), 5), spread=round(float((t.max() - t.min()) / np.median(t)), 4),
                              rounds_ms=[round(float(v), 5) for v in t])
            batch4 = 4 * 12 * ((npx + 3) & ~3) <= SCRATCH_MAX
            for n in (1, 4, 16):
                k = f"acc{n}"
                b = 4 if (n >= 4 and batch4) else 1
                add_ms = res[k]["ms"] - res["render"]["ms"]
                nbytes = 3 * npx * (4 + 16.0 / b)
                res[k].update(passes_per_add_kernel=b, vs_render=round(res[k]["ms"] / res["render"]["ms"], 4),
                              add_us=round(1e3 * add_ms, 2), add_bytes_per_pass=int(nbytes),
                              add_fraction=round(nbytes / (add_ms * 1e-3) / COPY_RATE, 4) if add_ms > 0 else None)
            res["resolve"].update(bytes=27 * npx, resolve_fraction=round(27 * npx / (res["resolve"]["ms"] * 1e-3) / COPY_RATE, 4))
            r.free(d32), r.free(d8), r.free(dsum)
            out[case] = dict(workload=name, passes_per_round=total, pixels=npx, **res)
        finally:
            r.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
