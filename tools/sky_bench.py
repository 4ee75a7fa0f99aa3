#!/usr/bin/env python3
"""Cost of the sky: workloads.build configs under a sky (rt_set_scene_sky) against the same scene without, interleaved, timed
with device events.

    python tools/sky_bench.py [--rounds 5] [--frames 50] [--cases c2,c4,c5] [--out profiles/sky_bench.json]

  scat         white lights, no spec row, no sky: the table below has a rough row, so the scene runs the scatter kernels (SCAT)
  lit          the same scene with one more table row that no object uses and that has spec > 0: the lighting kernels (LIT_SCAT),
               and the scatter frame, byte for byte
  unreachable  the scatter scene under a black gradient whose sun no ray can see (sun_rgb > 0, sun_cos = 2): the sky kernels
               (SKY_SCAT), and the scatter frame, byte for byte — the price of the kernels themselves
  sky          the scatter scene under a full sky: gradient, halo and disc (tools/feature_scenes.py: bench_sky)
All four have the same geometry and materials.  Each way has its own context (its scene set once, its dispatch order settled
by the warm-up).  A round times `--frames` launches (fewer for the larger configs, about the same time) into device memory
for each way in turn; one more round is run first and dropped (the first round of an interleaved run is slow for every way,
whatever the warm-up of each context alone was); the median over the rounds that count is reported, with the spread
(max - min) / median.  Prints one JSON line and writes it to --out.
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
from python_ray_tracer_amd import workloads               # noqa: E402
from feature_scenes import bench_sky                      # noqa: E402
from lighting_bench import CASES, scene_args              # noqa: E402

WAYS = ("scat", "lit", "unreachable", "sky")


def way_args(way, S, P, NL):
    """(materials, sky) of Renderer.set_scene."""
    if way == "lit":
        return scene_args("unused", S, P, NL)[0], None
    mats = scene_args("twin", S, P, NL)[0]
    return mats, (None if way == "scat" else bench_sky("unreachable" if way == "unreachable" else "full"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sky_bench.json"))
    a = ap.parse_args()
    out = {"metric": "sky_cost", "rounds": a.rounds, "frames": a.frames}
    for case in a.cases.split(","):
        name, rel = CASES[case]
        frames = max(2, int(round(a.frames * rel)))
        wl = workloads.build(name)
        w, h, S, P, NL = wl["w"], wl["h"], wl["spheres"].shape[1], wl["planes"].shape[1], wl["lights"].shape[1]
        ctx = {}
        try:
            for k in WAYS:
                mats, sky = way_args(k, S, P, NL)
                r = pkg.Renderer(0)
                r.set_scene(wl["spheres"], wl["lights"], wl["planes"], materials=mats, sky=sky)
                r.set_camera(wl["camera"].position, wl["camera"].rotation)
                r.set_raygen(w, h, *wl["camera"].raygen())
                p = r.params(wl["amb"], wl["lamb"], wl["refl"], wl["depth"], wl["aa"], spp=wl["spp"], seed=wl["seed"])
                d8 = r.malloc(3 * w * h)
                for _ in range(max(6, frames)):                # code objects, cull tables, a settled dispatch order
                    r.render_device(p, 0, w, d8, None, w * h)
                r.sync()
                ctx[k] = (r, p, d8)
            times = {k: [] for k in WAYS}
            for rnd in range(a.rounds + 1):
                for k, (r, p, d8) in ctx.items():
                    r.timer_begin()
                    for _ in range(frames):
                        r.render_device(p, 0, w, d8, None, w * h)
                    ms = r.timer_end() / frames
                    if rnd > 0:                                # (round 0: dropped)
                        times[k].append(ms)
            res = {}
            for k, t in times.items():
                t = np.array(t)
                res[k] = dict(ms=round(float(np.median(t)), 5), spread=round(float((t.max() - t.min()) / np.median(t)), 4),
                              rounds_ms=[round(float(v), 5) for v in t])
            frames8 = {}
            for k, (r, p, d8) in ctx.items():
                r.sync()
                buf = np.empty(3 * w * h, np.uint8)
                r.d2h(buf, d8)
                frames8[k] = buf
            for k in ("lit", "unreachable"):
                res[k]["same_frame_as_scat"] = bool(np.array_equal(frames8[k], frames8["scat"]))
            res["sky"]["differs_from_scat"] = bool(not np.array_equal(frames8["sky"], frames8["scat"]))
            res["sky"]["pixels_changed"] = round(float((frames8["sky"].reshape(3, -1) != frames8["scat"].reshape(3, -1)).any(axis=0).mean()), 4)
            for k in WAYS[1:]:
                res[k]["vs_scat"] = round(res[k]["ms"] / res["scat"]["ms"], 4)
            res["unreachable"]["vs_lit"] = round(res["unreachable"]["ms"] / res["lit"]["ms"], 4)
            res["sky"]["vs_lit"] = round(res["sky"]["ms"] / res["lit"]["ms"], 4)
            out[case] = dict(workload=name, frames=frames, **res)
        finally:
            for r, _, d8 in ctx.values():
                r.free(d8)
                r.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
