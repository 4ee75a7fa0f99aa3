#!/usr/bin/env python3
"""Cost of guided upsampling: the film chain at full resolution against the same chain at half resolution in each axis plus the lift,
and the two new calls alone against their compulsory bytes, on the three standing workloads with area lights and one shadow sample,
interleaved, timed with device events.

    python tools/upsample_bench.py [--rounds 5] [--reps 8] [--cases c2,c4,c5] [--out profiles/upsample_bench.json]

  full       at w x h: rt_film_accumulate_moments of 1 pass, rt_render_guides, rt_film_denoise_variance with four levels at Film's defaults,
             rt_film_resolve to uint8; per frame
  half       at w/2 x h/2: the same accumulate, guides and filter; then rt_render_guides_grid at w x h, rt_film_upsample of the filtered
             mean (demodulation, the kind plane off) and rt_film_resolve at w x h; per frame
  guides     rt_render_guides_grid at w x h alone, from the context whose own grid is w/2 x h/2
  up2, up3   rt_film_upsample alone from w/2 x h/2 and from w/3 x h/3 (that low mean is a stretch of the half-resolution buffer: the
             bytes moved are the same, the picture is not one)
One context per resolution and workload (the table of tools/soft_shadow_bench.py, every light of radius 0.5); the sums the filters read
hold four passes, the timed accumulate writes sums of its own.  A round times `reps` calls (--reps for the headline workload, fewer for
the larger ones) of each way in turn; one more round is run first and dropped; the median over the rounds that count is reported with the
spread (max - min) / median.
Derived figures:
  half.vs_full   half / full
  up*.fraction   the compulsory bytes per second of the call as a fraction of the 6.29 TB/s of a float4 copy: per output pixel 28 B of its
                 own guides read and 24 B written, per low pixel 52 B read (24 B of mean, 28 B of guides): (52 + 52 / r^2) bytes per pixel
  up*.expected_ms   those bytes at the copy rate: the floor written down before the first measurement
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import python_ray_tracer_amd as pkg                       # noqa: E402
from python_ray_tracer_amd import upsample as U           # noqa: E402
from python_ray_tracer_amd import variance as V           # noqa: E402
from python_ray_tracer_amd import workloads               # noqa: E402
from soft_shadow_bench import table                       # noqa: E402

CASES = {"c2": ("c2_1920x1080_s8_d3", 1.0), "c4": ("c4_3840x2160_s64_d5", 0.5), "c5": ("c5_7680x4320_s256_d8", 0.25)}
COPY_RATE = 6.29e12                                       # bytes per second of a float4 copy on this chip
VAR = dict(levels=4, normal_shin=32, kappa=V.KAPPA, var_floor=0.0, demodulate=1, prefilter=1)
WAYS = ("full", "half", "guides", "up2", "up3")
PASSES = 4


def stats(t):
    t = np.array(t)
    med = float(np.median(t))
    return dict(ms=round(med, 5), spread=round(float((t.max() - t.min()) / abs(med)), 4) if med else None, rounds_ms=[round(float(v), 5) for v in t])


class Chain:
    """A context at fw x fh with the workload's area-light scene, and the buffers of its film chain."""

    def __init__(self, wl, fw, fh, raygen):
        S, P = wl["spheres"].shape[1], wl["planes"].shape[1]
        self.r, self.w, self.h, self.npx, self.raygen = pkg.Renderer(0), fw, fh, fw * fh, raygen
        r = self.r
        r.set_scene(wl["spheres"], wl["lights"], wl["planes"], materials=table(S, P),
                    light_radius=np.full(wl["lights"].shape[1], 0.5, np.float32), shadow_samples=1)
        r.set_camera(wl["camera"].position, wl["camera"].rotation)
        r.set_raygen(fw, fh, *raygen)
        self.p = r.params(wl["amb"], wl["lamb"], wl["refl"], wl["depth"], wl["aa"], spp=wl["spp"], seed=wl["seed"])
        n = self.npx
        self.dsum, self.dsq, self.ssum, self.ssq = (r.malloc(24 * n) for _ in range(4))
        self.dg, self.dout, self.dwork = r.malloc(32 * n), r.malloc(32 * n), r.malloc(32 * n)
        r.film_accumulate_moments(self.p, 0, fw, PASSES, True, self.dsum, self.dsq)

    def filtered(self):
        r = self.r
        r.film_accumulate_moments(self.p, 0, self.w, 1, True, self.ssum, self.ssq)
        r.render_guides(0, self.w, self.dg, self.npx)
        r.film_denoise_variance(self.dsum, self.dsq, self.w, self.h, PASSES, self.dg, self.dout, self.dwork, **VAR)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "upsample_bench.json"))
    a = ap.parse_args()
    out = {"metric": "upsample_cost", "rounds": a.rounds, "reps": a.reps, "copy_rate_TBps": COPY_RATE / 1e12, "denoise_variance": VAR,
           "normal_cos": U.NORMAL_COS, "passes": PASSES}
    for case in a.cases.split(","):
        name, rel = CASES[case]
        reps = max(2, int(round(a.reps * rel)))
        wl = workloads.build(name)
        w, h = wl["w"], wl["h"]
        npx = w * h
        hi_grid = tuple(wl["camera"].raygen())
        sizes = {2: (w // 2, h // 2), 3: (w // 3, h // 3)}
        grids = {k: U.hi_raygen(hi_grid, w, h, *s) for k, s in sizes.items()}
        full, half = Chain(wl, w, h, hi_grid), Chain(wl, *sizes[2], grids[2])
        try:
            r = half.r
            d_hg, d_up, d_u8 = r.malloc(32 * npx), r.malloc(24 * npx), r.malloc(3 * npx)
            d_lg3 = r.malloc(32 * sizes[3][0] * sizes[3][1])
            f_u8 = full.r.malloc(3 * npx)
            r.render_guides_grid(*sizes[3], grids[3], 0, sizes[3][0], d_lg3)

            def lift(k, d_lg):
                r.film_upsample(half.dout, *sizes[k], 1, d_lg, d_hg, w, h, grids[k], hi_grid, d_up, None, normal_cos=U.NORMAL_COS, demodulate=1)

            def run(way, n=reps):
                for _ in range(n):
                    if way == "full":
                        full.filtered()
                        full.r.film_resolve(full.dout, w, h, 1, f_u8, None, white=400.0, gamma=2)
                    elif way == "half":
                        half.filtered()
                        r.render_guides_grid(w, h, hi_grid, 0, w, d_hg)
                        lift(2, half.dg)
                        r.film_resolve(d_up, w, h, 1, d_u8, None, white=400.0, gamma=2)
                    elif way == "guides":
                        r.render_guides_grid(w, h, hi_grid, 0, w, d_hg)
                    else:
                        lift(int(way[2:]), half.dg if way == "up2" else d_lg3)

            for way in WAYS:                                  # code objects, cull tables, the film scratch, a settled dispatch order
                run(way, 2)
            full.r.sync()
            r.sync()
            times = {k: [] for k in WAYS}
            for rnd in range(a.rounds + 1):
                for way in WAYS:
                    timer = full.r if way == "full" else r
                    timer.timer_begin()
                    run(way)
                    ms = timer.timer_end() / reps
                    if rnd > 0:                                # (round 0: dropped)
                        times[way].append(ms)
            res = {k: stats(t) for k, t in times.items()}
            res["half"]["vs_full"] = round(res["half"]["ms"] / res["full"]["ms"], 4)
            for k in (2, 3):
                nbytes = 52 * npx + 52 * sizes[k][0] * sizes[k][1]
                res[f"up{k}"].update(low=list(sizes[k]), bytes=int(nbytes), expected_ms=round(nbytes / COPY_RATE * 1e3, 5),
                                     fraction=round(nbytes / (res[f"up{k}"]["ms"] * 1e-3) / COPY_RATE, 4))
            out[case] = dict(workload=name, reps_per_round=reps, pixels=npx, **res)
        finally:
            full.r.close()
            half.r.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
