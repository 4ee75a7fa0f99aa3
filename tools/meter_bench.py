#!/usr/bin/env python3
"""Cost of metering: rt_film_meter, rt_film_meter_solve and rt_film_resolve_metered against rt_film_resolve and against the
histogram's compulsory bytes, on the three standing workloads, interleaved, timed with device events.

    python tools/meter_bench.py [--rounds 5] [--reps 8] [--cases c2,c4,c5] [--lib BUILD.so --label copies4] [--out profiles/meter_bench.json]

  render          rt_render_device with a float32 output, per frame: the single pass on the same scene
  meter           rt_film_meter with reset on the rendered film (four passes of the workload), per call
  meter_const     the same on a constant frame: every lane of a wave hits one counter, the worst contention in LDS
  meter_solve     rt_film_meter and rt_film_meter_solve, per pair
  solve           rt_film_meter_solve alone: one workgroup; its cost is the launch
  resolve         rt_film_resolve into a uint8 image (RT_FLAG_U8_HWC | RT_FLAG_U8_RGB, white 400, gamma 2)
  resolve_metered rt_film_resolve_metered with the solved state, the same outputs
One context per workload.  A round times `reps` calls (--reps for the headline workload, fewer for the larger ones) of each way in turn;
one more round is run first and dropped; the median over the rounds that count is reported with the spread (max - min) / median.
Derived figures:
  fraction        the compulsory bytes per second of the histogram (24 B per pixel: three float64 read, the counts are nothing beside
                  them), as a fraction of the 6.29 TB/s of a float4 copy
  const_vs_film   meter_const / meter, and `slower`: the constant frame is slower by more than both spreads
  metered_vs_plain  resolve_metered / resolve
The library's number of LDS copies per workgroup is a build setting (-DRT_METER_COPIES=1, 4, 8; rt_meter.h): --lib takes another
build of the library, --label names the build that is measured, and the result goes under that key of --out beside what is there,
so that the three builds stand in one file.
Prints one JSON line.
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
from python_ray_tracer_amd import _lib as L               # noqa: E402

CASES = {"c2": ("c2_1920x1080_s8_d3", 1.0), "c4": ("c4_3840x2160_s64_d5", 0.5), "c5": ("c5_7680x4320_s256_d8", 0.25)}
COPY_RATE = 6.29e12                                       # bytes per second of a float4 copy on this chip
PASSES = 4
TONE = dict(exposure=1.0, white=400.0, gamma=2, flags=L.RT_FLAG_U8_HWC | L.RT_FLAG_U8_RGB)
WAYS = ("render", "meter", "meter_const", "meter_solve", "solve", "resolve", "resolve_metered")


def stats(t):
    t = np.array(t)
    med = float(np.median(t))
    return dict(ms=round(med, 5), spread=round(float((t.max() - t.min()) / abs(med)), 4) if med else None, rounds_ms=[round(float(v), 5) for v in t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--lib", default=None, help="another build of libmi355rt.so (default: the tree's)")
    ap.add_argument("--label", default="copies4")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "meter_bench.json"))
    a = ap.parse_args()
    out = {"metric": "meter_cost", "rounds": a.rounds, "reps": a.reps, "copy_rate_TBps": COPY_RATE / 1e12, "passes": PASSES, "label": a.label}
    for case in a.cases.split(","):
        name, rel = CASES[case]
        reps = max(2, int(round(a.reps * rel)))
        wl = workloads.build(name)
        w, h = wl["w"], wl["h"]
        npx = w * h
        r = pkg.Renderer(0, lib=L.bind(os.path.abspath(a.lib))) if a.lib else pkg.Renderer(0)
        try:
            r.set_scene(wl["spheres"], wl["lights"], wl["planes"])
            r.set_camera(wl["camera"].position, wl["camera"].rotation)
            r.set_raygen(w, h, *wl["camera"].raygen())
            p = r.params(wl["amb"], wl["lamb"], wl["refl"], wl["depth"], wl["aa"], spp=wl["spp"], seed=wl["seed"])
            d32, dsum, dconst, d8 = r.malloc(12 * npx), r.malloc(24 * npx), r.malloc(24 * npx), r.malloc(3 * npx)
            dhist, dstate = r.malloc(8 * L.RT_METER_BINS), r.malloc(8 * L.RT_METER_STATE_DOUBLES)
            r.film_accumulate(p, 0, w, PASSES, True, dsum)
            plane = np.full(npx, 100.0 * PASSES)
            for c in range(3):
                r.h2d(dconst + 8 * c * npx, plane)
            r.h2d(dstate, np.zeros(L.RT_METER_STATE_DOUBLES))

            def run(way, n=reps):
                for _ in range(n):
                    if way == "render":
                        r.render_device(p, 0, w, None, d32, npx)
                    elif way == "meter":
                        r.film_meter(dsum, w, h, PASSES, dhist)
                    elif way == "meter_const":
                        r.film_meter(dconst, w, h, PASSES, dhist)
                    elif way == "meter_solve":
                        r.film_meter(dsum, w, h, PASSES, dhist)
                        r.film_meter_solve(dhist, dstate)
                    elif way == "solve":
                        r.film_meter_solve(dhist, dstate)
                    elif way == "resolve":
                        r.film_resolve(dsum, w, h, PASSES, d8, None, **TONE)
                    else:
                        r.film_resolve_metered(dsum, w, h, PASSES, dstate, d8, None, **TONE)

            for way in WAYS:                                  # code objects, a settled dispatch order
                run(way, 1)
            # what the histogram says, and that the constant frame lands in one bin
            run("meter_const", 1)
            r.sync()
            hist = np.zeros(L.RT_METER_BINS, np.uint64)
            r.d2h(hist, dhist)
            const_one_bin = bool(int(hist.max()) == npx)
            run("meter_solve", 1)
            r.sync()
            r.d2h(hist, dhist)
            state = np.zeros(L.RT_METER_STATE_DOUBLES)
            r.d2h(state, dstate)
            times = {k: [] for k in WAYS}
            for rnd in range(a.rounds + 1):
                for way in WAYS:
                    r.timer_begin()
                    run(way)
                    ms = r.timer_end() / reps
                    if rnd > 0:                                # (round 0: dropped)
                        times[way].append(ms)
            res = {k: stats(t) for k, t in times.items()}
            nbytes = 24 * npx
            for way in ("meter", "meter_const"):
                res[way].update(bytes=int(nbytes), fraction=round(nbytes / (res[way]["ms"] * 1e-3) / COPY_RATE, 4),
                                vs_render=round(res[way]["ms"] / res["render"]["ms"], 4))
            margin = res["meter"]["spread"] * res["meter"]["ms"] + res["meter_const"]["spread"] * res["meter_const"]["ms"]
            res["const_vs_film"] = round(res["meter_const"]["ms"] / res["meter"]["ms"], 4)
            res["slower"] = bool(res["meter_const"]["ms"] - res["meter"]["ms"] > margin)
            res["metered_vs_plain"] = round(res["resolve_metered"]["ms"] / res["resolve"]["ms"], 4)
            for d in (d32, dsum, dconst, d8, dhist, dstate):
                r.free(d)
            out[case] = dict(workload=name, reps_per_round=reps, pixels=npx, constant_frame_in_one_bin=const_one_bin,
                             counts_add_up=bool(int(hist.sum()) == npx), bins_filled=int((hist > 0).sum()),
                             state=[float(v) for v in state], **res)
        finally:
            r.close()
    print(json.dumps(out))
    if a.out:
        try:
            with open(a.out) as f:
                doc = json.loads(f.read())
        except (OSError, ValueError):
            doc = {}
        doc[a.label] = out
        with open(a.out, "w") as f:
            f.write(json.dumps(doc) + "\n")


if __name__ == "__main__":
    main()
