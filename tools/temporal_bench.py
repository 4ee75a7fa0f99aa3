#!/usr/bin/env python3
"""Cost of temporal accumulation: rt_film_temporal per call under a small camera move and under a still camera, beside the render
and the guides it needs, on the three standing workloads, interleaved, timed with device events.

    python tools/temporal_bench.py [--rounds 5] [--reps 8] [--cases c2,c4,c5] [--out profiles/temporal_bench.json]

  render   rt_render_device with a float32 output, per frame: a single pass on the same scene
  guides   rt_render_guides into eight float32 planes, per frame
  move     rt_film_temporal, per call, with a history rendered from a camera a quarter of a degree back on an orbit about the point
           4 units along the view axis: four taps per pixel, neighbouring pixels reading neighbouring taps
  still    rt_film_temporal, per call, with the history of the same camera: the snap leaves one tap per pixel
Settings are Film.temporal's defaults.  One context per workload; the sum is four film passes of the workload; the history is the
previous camera's four-pass mean with length 4 and its guides.  A round times `reps` calls (--reps for the headline workload, fewer
for the larger ones) of each way in turn; one more round is run first and dropped (the first round of an interleaved run is slow
for every way); the median over the rounds that count is reported with the spread (max - min) / median.
Derived figures:
  guides_vs_render   guides / render
  *_vs_render        the call / render
  fraction           the call's compulsory bytes per second as a fraction of the 6.29 TB/s of a float4 copy.  Compulsory: every byte
                     the call needs, once: per pixel 44 B of this frame read (24 B of sum, 4 B of id, 4 B of distance, 12 B of
                     normal), 48 B of history (24 B of mean, 4 B of length, and of its guides 4 B of id, 4 B of distance and 12 B
                     of normal: under a small move each history pixel is a tap of about four pixels and is counted once) and 28 B
                     written: 120 B
  fraction_requested (move only) the same with what the lanes ask for under a move: 44 B + 4 x 48 B + 28 B = 264 B per pixel (an upper bound:
                     a refused tap stops at its id)
  fresh              the share of pixels whose history did not survive
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
from python_ray_tracer_amd import temporal as T, workloads   # noqa: E402

CASES = {"c2": ("c2_1920x1080_s8_d3", 1.0), "c4": ("c4_3840x2160_s64_d5", 0.5), "c5": ("c5_7680x4320_s256_d8", 0.25)}
WAYS = ("render", "guides", "move", "still")
COPY_RATE = 6.29e12                                       # bytes per second of a float4 copy on this chip
SETTINGS = dict(depth_tol=T.DEPTH_TOL, normal_cos=T.NORMAL_COS, max_history=T.MAX_HISTORY)
BYTES_COMPULSORY, BYTES_REQUESTED = 44 + 48 + 28, 44 + 4 * 48 + 28
MOVE_DEGREES = 0.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "temporal_bench.json"))
    a = ap.parse_args()
    out = {"metric": "temporal_cost", "rounds": a.rounds, "reps": a.reps, "copy_rate_TBps": COPY_RATE / 1e12, "settings": SETTINGS,
           "move_degrees": MOVE_DEGREES, "bytes_per_pixel": {"compulsory": BYTES_COMPULSORY, "requested": BYTES_REQUESTED}}
    for case in a.cases.split(","):
        name, rel = CASES[case]
        reps = max(2, int(round(a.reps * rel)))
        wl = workloads.build(name)
        w, h = wl["w"], wl["h"]
        npx = w * h
        now = (np.asarray(wl["camera"].position, np.float64), np.asarray(wl["camera"].rotation, np.float64))
        before = T.orbit(now, now[0] + 4.0 * now[1][:, 0], -MOVE_DEGREES)
        r = pkg.Renderer(0)
        try:
            r.set_scene(wl["spheres"], wl["lights"], wl["planes"])
            r.set_raygen(w, h, *wl["camera"].raygen())
            p = r.params(wl["amb"], wl["lamb"], wl["refl"], wl["depth"], wl["aa"], spp=wl["spp"], seed=wl["seed"])
            d32, dsum, dout, dlen = r.malloc(12 * npx), r.malloc(24 * npx), r.malloc(24 * npx), r.malloc(4 * npx)
            dg = r.malloc(32 * npx)
            hist = {}
            for key, cam in (("move", before), ("still", now)):   # a history per way: the camera's four-pass mean, length 4, its guides
                r.set_camera(*cam)
                hg, hm, hl = r.malloc(32 * npx), r.malloc(24 * npx), r.malloc(4 * npx)
                r.film_accumulate(p, 0, w, 4, True, dsum)
                r.render_guides(0, w, hg, npx)
                r.film_temporal(dsum, 4, hg, dsum, hg, hg, cam[0], cam[1], hm, hl, depth_tol=0.0, normal_cos=1.0, max_history=0.0)
                hist[key] = (hm, hl, hg, cam)
            r.render_guides(0, w, dg, npx)                        # (the camera is `now`: the sum and the guides of this frame)
            r.sync()

            def run(way):
                for _ in range(reps):
                    if way == "render":
                        r.render_device(p, 0, w, None, d32, npx)
                    elif way == "guides":
                        r.render_guides(0, w, dg, npx)
                    else:
                        hm, hl, hg, cam = hist[way]
                        r.film_temporal(dsum, 4, dg, hm, hl, hg, cam[0], cam[1], dout, dlen, **SETTINGS)

            for way in WAYS:                                      # code objects, cull tables, a settled dispatch order
                run(way)
            r.sync()
            fresh = {}
            for way in ("move", "still"):
                run(way)
                r.sync()
                ln = np.empty(npx, np.float32)
                r.d2h(ln, dlen)
                fresh[way] = round(float((ln == 4.0).mean()), 4)
            times = {k: [] for k in WAYS}
            for rnd in range(a.rounds + 1):
                for way in WAYS:
                    r.timer_begin()
                    run(way)
                    ms = r.timer_end() / reps
                    if rnd > 0:                                    # (round 0: dropped)
                        times[way].append(ms)
            res = {}
            for k, t in times.items():
                t = np.array(t)
                res[k] = dict(ms=round(float(np.median(t)), 5), spread=round(float((t.max() - t.min()) / np.median(t)), 4),
                              rounds_ms=[round(float(v), 5) for v in t])
            res["guides"].update(vs_render=round(res["guides"]["ms"] / res["render"]["ms"], 4))
            for way in ("move", "still"):
                sec = res[way]["ms"] * 1e-3
                res[way].update(vs_render=round(res[way]["ms"] / res["render"]["ms"], 4), fresh=fresh[way],
                                fraction=round(npx * BYTES_COMPULSORY / sec / COPY_RATE, 4))
            res["move"].update(fraction_requested=round(npx * BYTES_REQUESTED / (res["move"]["ms"] * 1e-3) / COPY_RATE, 4))
            for d in [d32, dsum, dout, dlen, dg] + [b for v in hist.values() for b in v[:3]]:
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
