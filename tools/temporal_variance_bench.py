#!/usr/bin/env python3
"""Cost of the second moment under a history against its parents: rt_film_temporal_moments against rt_film_temporal, and
rt_film_denoise_variance_temporal against rt_film_denoise_variance, on the three standing workloads, interleaved in one run, timed
with device events.

    python tools/temporal_variance_bench.py [--rounds 5] [--reps 8] [--cases c2,c4,c5] [--out profiles/temporal_variance_bench.json]

  tmove, tstill       rt_film_temporal per call under a quarter-degree camera move (four taps per pixel) and under a still camera (one)
  mmove, mstill       rt_film_temporal_moments on the same inputs with the second moment beside them
  var1, var4          rt_film_denoise_variance at Film.denoise(variance=True)'s defaults with levels 1 and 4, on the frame's own sums
  own1, own4          rt_film_denoise_variance_temporal on what mmove wrote with spatial_below 0: no pixel pools
  dflt1, dflt4        the same at SPATIAL_BELOW: the pixels the move uncovered pool (`pooled` is their share)
  pool1, pool4        the same with a spatial_below above every length: every pixel walks the 25 taps
Settings, workloads, rounds and the history are tools/temporal_bench.py's and tools/variance_bench.py's: one context per workload, the
sums four film passes, the history the previous camera's four-pass moments with length 4.  A round times `reps` calls of each way in
turn; one more round is run first and dropped; the median over the rounds that count is reported with the spread (max - min) / median.

The expectation, stated before measuring, from bytes per pixel.  rt_film_temporal asks for 44 B of this frame, 48 B per tap of history
and writes 28 B: 264 B per pixel under a move (four taps), 120 B under a still camera.  The moments call reads 24 B more of this frame,
24 B more per tap and writes 24 B more: 408 B under a move, 192 B still.  Both kernels stream, so the expected ratios are 408 / 264 =
1.545 (move) and 192 / 120 = 1.6 (still).  The filter's prepare pass reads 4 B of length more than its parent's and the levels are the
parent's launches, so own* is expected at the parent's time; pool* adds up to 25 x 56 B of cached reads per pixel to one launch.
`expected` and `vs_parent` are printed side by side; nothing here is a pass or fail.
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
from python_ray_tracer_amd import temporal as T           # noqa: E402
from python_ray_tracer_amd import variance as V           # noqa: E402
from python_ray_tracer_amd import workloads               # noqa: E402

CASES = {"c2": ("c2_1920x1080_s8_d3", 1.0), "c4": ("c4_3840x2160_s64_d5", 0.5), "c5": ("c5_7680x4320_s256_d8", 0.25)}
FILTERS = {"own": 0.0, "dflt": V.SPATIAL_BELOW, "pool": 1e6}
WAYS = ("tmove", "mmove", "tstill", "mstill") + tuple(f"{k}{lv}" for lv in (1, 4) for k in ("var", "own", "dflt", "pool"))
SETTINGS = dict(depth_tol=T.DEPTH_TOL, normal_cos=T.NORMAL_COS, max_history=T.MAX_HISTORY)
VAR = dict(normal_shin=32, kappa=V.KAPPA, var_floor=0.0, demodulate=1, prefilter=1)
BYTES = {"tmove": 44 + 4 * 48 + 28, "mmove": 68 + 4 * 72 + 52, "tstill": 44 + 48 + 28, "mstill": 68 + 72 + 52}
EXPECTED = {"mmove": round(BYTES["mmove"] / BYTES["tmove"], 4), "mstill": round(BYTES["mstill"] / BYTES["tstill"], 4)}
MOVE_DEGREES = 0.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "temporal_variance_bench.json"))
    a = ap.parse_args()
    out = {"metric": "temporal_variance_cost", "rounds": a.rounds, "reps": a.reps, "settings": SETTINGS, "denoise_variance": VAR,
           "spatial_below": FILTERS, "move_degrees": MOVE_DEGREES, "requested_bytes_per_pixel": BYTES, "expected_vs_parent": EXPECTED}
    for case in a.cases.split(","):
        name, rel = CASES[case]
        reps = max(2, int(round(a.reps * rel)))
        wl = workloads.build(name)
        w, h = wl["w"], wl["h"]
        npx = w * h
        now = (np.asarray(wl["camera"].position, np.float64), np.asarray(wl["camera"].rotation, np.float64))
        before = T.orbit(now, now[0] + 4.0 * now[1][:, 0], -MOVE_DEGREES)
        r = pkg.Renderer(0)
        held = []

        def malloc(n):
            held.append(r.malloc(n))
            return held[-1]

        try:
            r.set_scene(wl["spheres"], wl["lights"], wl["planes"])
            r.set_raygen(w, h, *wl["camera"].raygen())
            p = r.params(wl["amb"], wl["lamb"], wl["refl"], wl["depth"], wl["aa"], spp=wl["spp"], seed=wl["seed"])
            dsum, dsq, dg = malloc(24 * npx), malloc(24 * npx), malloc(32 * npx)
            dout, dosq, dlen = malloc(24 * npx), malloc(24 * npx), malloc(4 * npx)
            tout, tlen = malloc(24 * npx), malloc(4 * npx)
            dout4, dwork4 = malloc(32 * npx), malloc(32 * npx)
            hist = {}
            for key, cam in (("move", before), ("still", now)):   # a history per way: the camera's four-pass moments, length 4, its guides
                r.set_camera(*cam)
                hg, hm, hq, hl = malloc(32 * npx), malloc(24 * npx), malloc(24 * npx), malloc(4 * npx)
                r.film_accumulate_moments(p, 0, w, 4, True, dsum, dsq)
                r.render_guides(0, w, hg, npx)
                r.film_temporal_moments(dsum, dsq, 4, hg, dsum, dsq, hg, hg, cam[0], cam[1], hm, hq, hl, depth_tol=0.0, normal_cos=1.0, max_history=0.0)
                hist[key] = (hm, hq, hl, hg, cam)
            r.render_guides(0, w, dg, npx)                        # (the camera is `now`: the sums and the guides of this frame)
            r.sync()

            def run(way):
                for _ in range(reps):
                    if way[0] in "tm" and way[1:] in hist:
                        hm, hq, hl, hg, cam = hist[way[1:]]
                        if way[0] == "t":
                            r.film_temporal(dsum, 4, dg, hm, hl, hg, cam[0], cam[1], tout, tlen, **SETTINGS)
                        else:
                            r.film_temporal_moments(dsum, dsq, 4, dg, hm, hq, hl, hg, cam[0], cam[1], dout, dosq, dlen, **SETTINGS)
                    elif way.startswith("var"):
                        r.film_denoise_variance(dsum, dsq, w, h, 4, dg, dout4, dwork4, levels=int(way[3:]), **VAR)
                    else:
                        r.film_denoise_variance_temporal(dout, dosq, dlen, w, h, dg, dout4, dwork4, levels=int(way[-1]), spatial_below=FILTERS[way[:-1]], **VAR)

            run("mstill")
            run("mmove")                                          # the filters' input: the moved camera's temporal moments, left in place below
            r.sync()
            ln = np.empty(npx, np.float32)
            r.d2h(ln, dlen)
            fresh = round(float((ln == 4.0).mean()), 4)
            pooled = {k: round(float((ln < np.float32(sb)).mean()), 4) for k, sb in FILTERS.items()}
            order = tuple(k for k in WAYS if k != "mstill") + ("mstill", "mmove")   # (mmove last in a round: dout holds the move's result for the filters)
            for way in order:                                     # code objects, a settled dispatch order
                run(way)
            r.sync()
            times = {k: [] for k in WAYS}
            for rnd in range(a.rounds + 1):
                for way in order:
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
            for k in ("move", "still"):
                res["m" + k].update(vs_parent=round(res["m" + k]["ms"] / res["t" + k]["ms"], 4), expected=EXPECTED["m" + k])
            for lv in (1, 4):
                for k in FILTERS:
                    res[f"{k}{lv}"].update(vs_parent=round(res[f"{k}{lv}"]["ms"] / res[f"var{lv}"]["ms"], 4), pooled=pooled[k])
            out[case] = dict(workload=name, reps_per_round=reps, pixels=npx, fresh=fresh, **res)
        finally:
            for d in held:
                r.free(d)
            r.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
