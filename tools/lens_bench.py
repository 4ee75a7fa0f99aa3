#!/usr/bin/env python3
"""Cost of depth of field: workloads.build configs through a thin lens (rt_set_lens) of radius 0.1, against the same scene
with the pinhole camera, interleaved, timed with device events.

    python tools/lens_bench.py [--rounds 5] [--frames 50] [--cases c2,c4,c5]

  pinhole  aperture 0: the 6-column table below has no rough or transparent row, so it is repacked to 3 columns and runs the
           material kernels (MAT)
  lens     the same table, aperture 0.1 focused 3.0 ahead: the lens kernels (LENS, scatter twins; the table padded to 6
           columns), whose primary rays take the origin-form cull instead of the camera-anchored table
  soft1    aperture 0 with every light of radius 0.5, n = 1: the area-light kernels (SOFT)
  lens_soft1  the same lights through the lens: the lens twins of the area-light kernels
All four have the same geometry and reflectivities; only the primary rays (lens) or the shadow rays (soft) differ.  Each way has its own context (its scene set once,
its dispatch order settled by the warm-up).  A round times `--frames` launches (fewer for the larger configs, about the
same time) into device memory for each way in turn; the median over rounds is reported, with the spread
(max - min) / median.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import python_ray_tracer_amd as pkg                       # noqa: E402
from python_ray_tracer_amd import workloads               # noqa: E402

# rows 0-2: spheres; 3 the floor (a mirror)
TABLE = [(0.0, 0.6, 0.3, 0.0, 1.0, 0.0), (0.0, 0.4, 0.8, 0.0, 1.0, 0.0), (0.1, 0.6, 0.0, 0.0, 1.0, 0.0),
         (0.0, 0.3, 0.75, 0.0, 1.0, 0.0)]
WAYS = {"pinhole": (0.0, 0.0), "lens": (0.0, 0.1), "soft1": (0.5, 0.0), "lens_soft1": (0.5, 0.1)}   # (light radius, aperture)
FOCUS = 3.0
# case -> (workload, frames per round relative to --frames)
CASES = {"c2": ("c2_1920x1080_s8_d3", 1.0), "c4": ("c4_3840x2160_s64_d5", 0.2), "c5": ("c5_7680x4320_s256_d8", 0.04)}


def table(S, P):
    sid = np.array([1 if i % 3 == 0 else (0 if i % 2 else 2) for i in range(S)], np.int32)
    return np.array(TABLE, dtype=np.float64), sid, np.full(P, 3, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    out = {"metric": "lens_cost", "rounds": a.rounds, "frames": a.frames}
    for case in a.cases.split(","):
        name, rel = CASES[case]
        frames = max(2, int(round(a.frames * rel)))
        wl = workloads.build(name)
        w, h, S, P = wl["w"], wl["h"], wl["spheres"].shape[1], wl["planes"].shape[1]
        mats = table(S, P)
        ways = WAYS
        ctx = {}
        try:
            for k, (rad, ap) in ways.items():
                r = pkg.Renderer(0)
                r.set_scene(wl["spheres"], wl["lights"], wl["planes"], materials=mats,
                            light_radius=np.full(wl["lights"].shape[1], rad, np.float32), shadow_samples=1)
                r.set_camera(wl["camera"].position, wl["camera"].rotation)
                r.set_lens(ap, FOCUS)
                r.set_raygen(w, h, *wl["camera"].raygen())
                p = r.params(wl["amb"], wl["lamb"], wl["refl"], wl["depth"], wl["aa"], spp=wl["spp"], seed=wl["seed"])
                d8 = r.malloc(3 * w * h)
                for _ in range(max(6, frames)):                # code objects, cull tables, a settled dispatch order
                    r.render_device(p, 0, w, d8, None, w * h)
                r.sync()
                ctx[k] = (r, p, d8)
            times = {k: [] for k in ways}
            for _ in range(a.rounds):
                for k, (r, p, d8) in ctx.items():
                    r.timer_begin()
                    for _ in range(frames):
                        r.render_device(p, 0, w, d8, None, w * h)
                    times[k].append(r.timer_end() / frames)
            res = {}
            for k, t in times.items():
                t = np.array(t)
                res[k] = dict(ms=round(float(np.median(t)), 5), spread=round(float((t.max() - t.min()) / np.median(t)), 4))
            res["lens"]["vs_pinhole"] = round(res["lens"]["ms"] / res["pinhole"]["ms"], 4)
            res["soft1"]["vs_pinhole"] = round(res["soft1"]["ms"] / res["pinhole"]["ms"], 4)
            res["lens_soft1"]["vs_soft1"] = round(res["lens_soft1"]["ms"] / res["soft1"]["ms"], 4)
            out[case] = dict(workload=name, frames=frames, **res)
        finally:
            for r, _, d8 in ctx.values():
                r.free(d8)
                r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
