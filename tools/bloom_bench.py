#!/usr/bin/env python3
"""Cost of the bloom: rt_film_bloom against rt_render_device and against its compulsory bytes, with tiles and with
RT_BLOOM_NO_TILES, on the three standing workloads, interleaved, timed with device events.

    python tools/bloom_bench.py [--per-level] [--rounds 5] [--reps 8] [--cases c2,c4,c5] [--out profiles/bloom_bench.json]

  render     rt_render_device with a float32 output, per frame: the single pass on the same scene
  tilesL     rt_film_bloom with levels = L (1, 4, 6, 8), threshold 255, strength 0.25, per call: the levels whose step is at most
             BLOOM_TILE_MAX_STEP (rt_bloom.h) run as one LDS-tile kernel each, the others as two gather kernels
  gatherL    the same with RT_BLOOM_NO_TILES: two gather kernels at every level
--per-level times levels = 0, 1, 2, 3 in both forms instead.  The cost of the level with step 2^k is the call with levels = k + 1 minus
the call with levels = k, taken round by round: what adding that level costs (the level before it now also stores its b, in both
forms alike).  The library must have been built with the tile kernel switched on for every step measured
(-DRT_BLOOM_TILE_MAX_STEP=4, the largest the kernel is built for); the JSON records what the two forms' outputs say: equal bytes.
One context per workload; the sum is four film passes of the workload.  A round times `reps` calls (--reps for the headline workload,
fewer for the larger ones) of each way in turn; one more round is run first and dropped; the median over the rounds that count is
reported with the spread (max - min) / median.
Derived figures:
  vs_render   the call / render
  fraction    the compulsory bytes per second of the call, as a fraction of the 6.29 TB/s of a float4 copy.  Per pixel: 24 B of sum
              read, 24 B of out and 24 B of b_0 written by the bright pass; per level 24 B of b read, 24 B of b written (not on the last
              level) and 48 B of out read and written: 48 + 96 L bytes for L >= 1 levels
  tile_vs_gather (per level)  the tile form's cost of the level / the gather form's, and `wins`: the tile form is cheaper by more
              than both spreads
Prints one JSON line and writes it to --out (per level: under the key "per_level" of the file that is there).
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import python_ray_tracer_amd as pkg                       # noqa: E402
from python_ray_tracer_amd import workloads               # noqa: E402
from python_ray_tracer_amd import _lib as L               # noqa: E402

CASES = {"c2": ("c2_1920x1080_s8_d3", 1.0), "c4": ("c4_3840x2160_s64_d5", 0.5), "c5": ("c5_7680x4320_s256_d8", 0.25)}
COPY_RATE = 6.29e12                                       # bytes per second of a float4 copy on this chip
SETTINGS = dict(threshold=255.0, strength=0.25)
PASSES = 4


def stats(t):
    t = np.array(t)
    med = float(np.median(t))
    return dict(ms=round(med, 5), spread=round(float((t.max() - t.min()) / abs(med)), 4) if med else None, rounds_ms=[round(float(v), 5) for v in t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-level", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bloom_bench.json"))
    a = ap.parse_args()
    levels = (0, 1, 2, 3) if a.per_level else (1, 4, 6, 8)
    ways = ([] if a.per_level else ["render"]) + [f"{form}{k}" for k in levels for form in ("tiles", "gather")]
    out = {"metric": "bloom_per_level" if a.per_level else "bloom_cost", "rounds": a.rounds, "reps": a.reps, "copy_rate_TBps": COPY_RATE / 1e12,
           "settings": SETTINGS, "passes": PASSES}
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
            d32, dsum, dout = r.malloc(12 * npx), r.malloc(24 * npx), r.malloc(24 * npx)
            dwork = r.malloc(8 * L.RT_BLOOM_WORK_PLANES * npx)
            r.film_accumulate(p, 0, w, PASSES, True, dsum)

            def run(way, n=reps):
                for _ in range(n):
                    if way == "render":
                        r.render_device(p, 0, w, None, d32, npx)
                    else:
                        tiles = way.startswith("tiles")
                        r.film_bloom(dsum, w, h, PASSES, dout, dwork, levels=int(way[5 if tiles else 6:]), flags=0 if tiles else L.RT_BLOOM_NO_TILES,
                                     **SETTINGS)

            sha = {}
            host = np.empty((3, npx), np.float64)
            for way in ways:                                  # code objects, a settled dispatch order; and what each way computes
                run(way, 1)
                if way != "render":
                    r.sync()
                    r.d2h(host, dout)
                    sha[way] = hashlib.sha256(host.tobytes()).hexdigest()[:16]
            same = all(sha[f"tiles{k}"] == sha[f"gather{k}"] for k in levels)
            times = {k: [] for k in ways}
            for rnd in range(a.rounds + 1):
                for way in ways:
                    r.timer_begin()
                    run(way)
                    ms = r.timer_end() / reps
                    if rnd > 0:                                # (round 0: dropped)
                        times[way].append(ms)
            res = {k: stats(t) for k, t in times.items()}
            if a.per_level:
                for k in levels[:-1]:
                    step = 1 << k
                    lvl = {}
                    for form in ("tiles", "gather"):
                        lvl[form] = stats(np.array(times[f"{form}{k + 1}"]) - np.array(times[f"{form}{k}"]))
                    ratio = lvl["tiles"]["ms"] / lvl["gather"]["ms"]
                    margin = lvl["tiles"]["spread"] * lvl["tiles"]["ms"] + lvl["gather"]["spread"] * lvl["gather"]["ms"]
                    res[f"step{step}"] = dict(tiles=lvl["tiles"], gather=lvl["gather"], tile_vs_gather=round(ratio, 4),
                                              wins=bool(lvl["gather"]["ms"] - lvl["tiles"]["ms"] > margin))
            else:
                for way in ways[1:]:
                    k = int(way[5 if way.startswith("tiles") else 6:])
                    nbytes = npx * (48 + 96 * k)
                    res[way].update(vs_render=round(res[way]["ms"] / res["render"]["ms"], 4), bytes=int(nbytes),
                                    fraction=round(nbytes / (res[way]["ms"] * 1e-3) / COPY_RATE, 4))
            for d in (d32, dsum, dout, dwork):
                r.free(d)
            out[case] = dict(workload=name, reps_per_round=reps, pixels=npx, tiles_and_gather_same_bytes=same, **res)
        finally:
            r.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        doc = out
        if a.per_level:                                       # beside the cost table, if the file has one
            try:
                with open(a.out) as f:
                    doc = json.loads(f.read())
            except (OSError, ValueError):
                doc = {}
            doc["per_level"] = out
        with open(a.out, "w") as f:
            f.write(json.dumps(doc) + "\n")


if __name__ == "__main__":
    main()
