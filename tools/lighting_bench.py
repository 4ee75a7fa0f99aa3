#!/usr/bin/env python3
"""Cost of lighting: workloads.build configs with coloured lights and highlights (rt_set_scene_lighting) against the same scene
without, interleaved, timed with device events.

    python tools/lighting_bench.py [--rounds 5] [--frames 50] [--cases c2,c4,c5]

  twin    white lights and no spec row: the table below has a rough row, so the scene runs the scatter kernels (SCAT)
  unused  the same scene with one more table row that no object uses and that has spec > 0: the lighting kernels (LIT_SCAT,
          every texture id -1), and the frame is the twin's, byte for byte — the price of the kernels themselves
  lit     a warm, a cool and a dim light, and spec = 120, shin = 64 on every object
All three have the same geometry and materials.  Each way has its own context (its scene set once, its dispatch order settled
by the warm-up).  A round times `--frames` launches (fewer for the larger configs, about the same time) into device memory
for each way in turn; the median over rounds is reported, with the spread (max - min) / median.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import python_ray_tracer_amd as pkg                       # noqa: E402
from python_ray_tracer_amd import workloads               # noqa: E402

# rows 0-2: spheres (row 1 a brushed mirror); 3 the floor (a mirror)
TABLE = [(0.0, 0.6, 0.3, 0.0, 1.0, 0.0), (0.0, 0.4, 0.8, 0.0, 1.0, 0.1), (0.1, 0.6, 0.0, 0.0, 1.0, 0.0),
         (0.0, 0.3, 0.75, 0.0, 1.0, 0.0)]
WAYS = ("twin", "unused", "lit")
LIGHTS = [(1.3, 1.04, 0.7), (0.35, 0.5, 0.7), (0.25, 0.25, 0.25)]
# case -> (workload, frames per round relative to --frames)
CASES = {"c2": ("c2_1920x1080_s8_d3", 1.0), "c4": ("c4_3840x2160_s64_d5", 0.2), "c5": ("c5_7680x4320_s256_d8", 0.04)}


def scene_args(way, S, P, NL):
    """(materials, light_rgb) of Renderer.set_scene."""
    sid = np.array([1 if i % 3 == 0 else (0 if i % 2 else 2) for i in range(S)], np.int32)
    pid = np.full(P, 3, np.int32)
    t6 = np.array(TABLE, dtype=np.float64)
    if way == "twin":
        return (t6, sid, pid), None
    t8 = np.concatenate([t6, np.tile([0.0, 64.0], (len(t6), 1))], axis=1)
    if way == "unused":
        return (np.concatenate([t8, [[0.0, 0.6, 0.3, 0.0, 1.0, 0.0, 120.0, 64.0]]]), sid, pid), None
    t8[:, 6] = 120.0
    return (t8, sid, pid), np.array([LIGHTS[i % len(LIGHTS)] for i in range(NL)], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    out = {"metric": "lighting_cost", "rounds": a.rounds, "frames": a.frames}
    for case in a.cases.split(","):
        name, rel = CASES[case]
        frames = max(2, int(round(a.frames * rel)))
        wl = workloads.build(name)
        w, h, S, P, NL = wl["w"], wl["h"], wl["spheres"].shape[1], wl["planes"].shape[1], wl["lights"].shape[1]
        ctx = {}
        try:
            for k in WAYS:
                mats, rgb = scene_args(k, S, P, NL)
                r = pkg.Renderer(0)
                r.set_scene(wl["spheres"], wl["lights"], wl["planes"], materials=mats, light_rgb=rgb)
                r.set_camera(wl["camera"].position, wl["camera"].rotation)
                r.set_raygen(w, h, *wl["camera"].raygen())
                p = r.params(wl["amb"], wl["lamb"], wl["refl"], wl["depth"], wl["aa"], spp=wl["spp"], seed=wl["seed"])
                d8 = r.malloc(3 * w * h)
                for _ in range(max(6, frames)):                # code objects, cull tables, a settled dispatch order
                    r.render_device(p, 0, w, d8, None, w * h)
                r.sync()
                ctx[k] = (r, p, d8)
            times = {k: [] for k in WAYS}
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
            frames8 = {}
            for k, (r, p, d8) in ctx.items():
                r.sync()
                buf = np.empty(3 * w * h, np.uint8)
                r.d2h(buf, d8)
                frames8[k] = buf
            res["unused"]["same_frame_as_twin"] = bool(np.array_equal(frames8["unused"], frames8["twin"]))
            res["lit"]["differs_from_twin"] = bool(not np.array_equal(frames8["lit"], frames8["twin"]))
            res["unused"]["vs_twin"] = round(res["unused"]["ms"] / res["twin"]["ms"], 4)
            res["lit"]["vs_twin"] = round(res["lit"]["ms"] / res["twin"]["ms"], 4)
            out[case] = dict(workload=name, frames=frames, **res)
        finally:
            for r, _, d8 in ctx.values():
                r.free(d8)
                r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
