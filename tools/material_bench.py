#!/usr/bin/env python3
"""Cost of per-object materials: workloads.build configs rendered three ways, interleaved, timed with device events.

    python tools/material_bench.py [--rounds 7] [--frames 50] [--cases c2,c4,...]

Cases: c2 and c4 (the default kernels' headline configs), and the paths whose material kernels spill more than their default
twins: c2 with stochastic AA at 4 spp and with the reference's 9 taps per pixel (the parked per-pixel AA kernels),
c5 (lane-owned traversal) and c5 at 4 spp (the lane-owned AA kernel).

  global   rt_set_scene, the launch's amb / lamb / refl (the default kernels)
  uniform  rt_set_scene_materials with one material (amb, lamb, refl) for every object (the material kernels)
  objects  rt_set_scene_materials with material i % 7 for sphere i (and the plane) — the table of tools/gen_material_golden.py
Each way has its own context (its scene set once, its dispatch order settled by the warm-up).  A round times `--frames`
launches (fewer for the larger configs, about the same time) into device memory for each way in turn; the median over rounds
is reported, with the spread (max - min) / median.
Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import python_ray_tracer_amd as pkg                       # noqa: E402
from python_ray_tracer_amd import workloads               # noqa: E402

TABLE = [(0.0, 0.6, 0.3), (0.1, 0.6, 0.0), (0.0, 0.5, 0.9), (0.0, -0.4, 0.3), (0.25, 0.4, 0.5), (0.05, 0.8, 0.25), (0.0, 0.3, 0.75)]
FLAG_AA_PER_PIXEL = 32
# case -> (workload, aa, spp, flags, frames per round relative to --frames)
CASES = {"c2": ("c2_1920x1080_s8_d3", None, None, 0, 1.0), "c4": ("c4_3840x2160_s64_d5", None, None, 0, 0.2),
         "c2_spp4": ("c2_1920x1080_s8_d3", 2, 4, 0, 0.3), "c2_aa9": ("c2_1920x1080_s8_d3", 1, 0, FLAG_AA_PER_PIXEL, 0.2),
         "c5": ("c5_7680x4320_s256_d8", None, None, 0, 0.04), "c5_spp4": ("c5_7680x4320_s256_d8_spp4", None, None, 0, 0.02)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    out = {"metric": "material_cost", "rounds": a.rounds, "frames": a.frames}
    for case in a.cases.split(","):
        name, aa, spp, flags, rel = CASES[case]
        frames = max(2, int(round(a.frames * rel)))
        wl = workloads.build(name)
        if aa is not None:
            wl["aa"], wl["spp"] = aa, spp
        w, h, S, P = wl["w"], wl["h"], wl["spheres"].shape[1], wl["planes"].shape[1]
        ways = {"global": None,
                "uniform": (np.array([[wl["amb"], wl["lamb"], wl["refl"]]]), np.zeros(S, np.int32), np.zeros(P, np.int32)),
                "objects": (np.array(TABLE), (np.arange(S) % len(TABLE)).astype(np.int32), ((S + np.arange(P)) % len(TABLE)).astype(np.int32))}
        ctx = {}
        try:
            for k, mats in ways.items():
                r = pkg.Renderer(0)
                r.set_scene(wl["spheres"], wl["lights"], wl["planes"], materials=mats)
                r.set_camera(wl["camera"].position, wl["camera"].rotation)
                r.set_raygen(w, h, *wl["camera"].raygen())
                p = r.params(wl["amb"], wl["lamb"], wl["refl"], wl["depth"], wl["aa"], flags=flags, spp=wl["spp"], seed=wl["seed"])
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
            for k in ("uniform", "objects"):
                res[k]["vs_global"] = round(res[k]["ms"] / res["global"]["ms"], 4)
            out[case] = dict(workload=name, frames=frames, **res)
        finally:
            for r, _, d8 in ctx.values():
                r.free(d8)
                r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
