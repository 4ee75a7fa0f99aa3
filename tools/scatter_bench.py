#!/usr/bin/env python3
"""Cost of rough materials: workloads.build configs with every third sphere rough (0.3), against the same table with
rough = 0 (the material kernels), interleaved, timed with device events.

    python tools/scatter_bench.py [--rounds 5] [--frames 50] [--cases c2,c4,c5]

  smooth  rt_set_scene_materials_scatter with the 6-column table below and every rough set to 0 (no transparent row either:
          repacked to 3 columns, the material kernels, MAT)
  rough   the same table (every third sphere brushed metal, rough 0.3): the scatter kernels (SCAT)
Both tables have the same reflectivities, so they weight paths alike; only the rough spheres' continuations differ
(scattered instead of mirrored, and ended where they would leave through the surface).  Each way has its own context (its scene set once,
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

# rows 0, 2: smooth; 1: rough; 3 the floor (a mirror)
TABLE = [(0.0, 0.6, 0.3, 0.0, 1.0, 0.0), (0.0, 0.4, 0.8, 0.0, 1.0, 0.3), (0.1, 0.6, 0.0, 0.0, 1.0, 0.0),
         (0.0, 0.3, 0.75, 0.0, 1.0, 0.0)]
# case -> (workload, frames per round relative to --frames)
CASES = {"c2": ("c2_1920x1080_s8_d3", 1.0), "c4": ("c4_3840x2160_s64_d5", 0.2), "c5": ("c5_7680x4320_s256_d8", 0.04)}


def tables(S, P):
    sid = np.array([1 if i % 3 == 0 else (0 if i % 2 else 2) for i in range(S)], np.int32)
    pid = np.full(P, 3, np.int32)
    rough = np.array(TABLE, dtype=np.float64)
    smooth = rough.copy()
    smooth[:, 5] = 0.0
    return {"smooth": (smooth, sid, pid), "rough": (rough, sid, pid)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    out = {"metric": "scatter_cost", "rounds": a.rounds, "frames": a.frames}
    for case in a.cases.split(","):
        name, rel = CASES[case]
        frames = max(2, int(round(a.frames * rel)))
        wl = workloads.build(name)
        w, h, S, P = wl["w"], wl["h"], wl["spheres"].shape[1], wl["planes"].shape[1]
        ways = tables(S, P)
        ctx = {}
        try:
            for k, mats in ways.items():
                r = pkg.Renderer(0)
                r.set_scene(wl["spheres"], wl["lights"], wl["planes"], materials=mats)
                r.set_camera(wl["camera"].position, wl["camera"].rotation)
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
            res["rough"]["vs_smooth"] = round(res["rough"]["ms"] / res["smooth"]["ms"], 4)
            out[case] = dict(workload=name, frames=frames, **res)
        finally:
            for r, _, d8 in ctx.values():
                r.free(d8)
                r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
