#!/usr/bin/env python3
"""Cost of the variance-guided denoiser against its parents: rt_film_accumulate_moments against rt_film_accumulate, and
rt_film_denoise_variance against rt_film_denoise, on the three standing workloads, interleaved, timed with device events.

    python tools/variance_bench.py [--rounds 5] [--reps 8] [--cases c2,c4,c5] [--out profiles/variance_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/variance_bench.py --add-only --cases c5

  acc1, acc4, acc16   rt_film_accumulate with 1, 4 and 16 passes (reset), per call: the passes' renders and their add kernels
  mom1, mom4, mom16   rt_film_accumulate_moments with the same passes, per call: the same renders, add2 kernels in place of add
  den1, den4          rt_film_denoise at Film.denoise's defaults (sigma 1/8, normal_shin 32, demodulate 1) with levels 1 and 4, per call
  var1, var4          rt_film_denoise_variance at Film.denoise(variance=True)'s defaults (kappa, var_floor 0, normal_shin 32, demodulate 1,
                      prefilter 1) with levels 1 and 4, per call: a prepare launch and one launch per level over four planes
One context per workload; the sums are four film passes of the workload.  A round times `reps` calls (--reps for the headline
workload, fewer for the larger ones) of each way in turn; one more round is run first and dropped (the first round of an interleaved
run is slow for every way); the median over the rounds that count is reported with the spread (max - min) / median.
Derived figures:
  mom*.vs_parent, var*.vs_parent   the call against its parent's
  mom*.add_ms, acc*.add_ms         the call less `passes` renders (the `render` way: rt_render_device with a float32 output): what the
                                   add kernels cost, and mom*.add_vs_parent their ratio
  mom*.add_fraction, acc*          the add kernels' compulsory bytes per second as a fraction of the 6.29 TB/s of a float4 copy: 4 B per
                                   element and pass read, and per element and add kernel 16 B (add) or 32 B (add2) read and written (a
                                   reset call's first kernel only writes: half of that).  A kernel folds four passes, or one where four
                                   pass frames exceed the library's 256 MiB of scratch (2160p and 4320p)
The add_ms figures are differences of event times and carry the difference between a render alone and a render inside the call;
the add kernels' own times come from a kernel trace: --add-only runs four 16-pass calls of each entry point per workload and nothing
else, for rocprofv3 --kernel-trace --stats (profiles/variance_add_trace.txt).
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
from python_ray_tracer_amd import film as F               # noqa: E402
from python_ray_tracer_amd import variance as V           # noqa: E402
from python_ray_tracer_amd import workloads               # noqa: E402

CASES = {"c2": ("c2_1920x1080_s8_d3", 1.0), "c4": ("c4_3840x2160_s64_d5", 0.5), "c5": ("c5_7680x4320_s256_d8", 0.25)}
PASSES = (1, 4, 16)
WAYS = ("render",) + tuple(f"{k}{n}" for n in PASSES for k in ("acc", "mom")) + ("den1", "var1", "den4", "var4")
COPY_RATE = 6.29e12                                       # bytes per second of a float4 copy on this chip
DEN = dict(normal_shin=32, sigma=F.DENOISE_SIGMA, demodulate=1)
VAR = dict(normal_shin=32, kappa=V.KAPPA, var_floor=0.0, demodulate=1, prefilter=1)
BATCH, SCRATCH_MAX = 4, 256 << 20                         # passes one add kernel folds, unless their frames exceed the scratch cap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "variance_bench.json"))
    ap.add_argument("--add-only", action="store_true", help="four 16-pass calls of each accumulate entry per workload, for a kernel trace")
    a = ap.parse_args()
    out = {"metric": "variance_cost", "rounds": a.rounds, "reps": a.reps, "copy_rate_TBps": COPY_RATE / 1e12, "denoise": DEN, "denoise_variance": VAR}
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
            d32, dg = r.malloc(12 * npx), r.malloc(32 * npx)
            dsum, dsq, dscratch_s, dscratch_q = (r.malloc(24 * npx) for _ in range(4))
            dout, dwork, dout4, dwork4 = r.malloc(24 * npx), r.malloc(24 * npx), r.malloc(32 * npx), r.malloc(32 * npx)
            if a.add_only:
                for _ in range(4):
                    r.film_accumulate(p, 0, w, 16, True, dscratch_s)
                    r.film_accumulate_moments(p, 0, w, 16, True, dscratch_s, dscratch_q)
                r.sync()
                continue
            r.render_guides(0, w, dg, npx)
            r.film_accumulate_moments(p, 0, w, 4, True, dsum, dsq)

            def run(way):
                n = reps if way[:3] in ("ren", "den", "var") else max(1, reps // 2)
                for _ in range(n):
                    if way == "render":
                        r.render_device(p, 0, w, None, d32, npx)
                    elif way.startswith("acc"):
                        r.film_accumulate(p, 0, w, int(way[3:]), True, dscratch_s)
                    elif way.startswith("mom"):
                        r.film_accumulate_moments(p, 0, w, int(way[3:]), True, dscratch_s, dscratch_q)
                    elif way.startswith("den"):
                        r.film_denoise(dsum, w, h, 4, dg, dout, dwork, levels=int(way[3:]), **DEN)
                    else:
                        r.film_denoise_variance(dsum, dsq, w, h, 4, dg, dout4, dwork4, levels=int(way[3:]), **VAR)
                return n

            for way in WAYS:                                  # code objects, cull tables, the film scratch, a settled dispatch order
                run(way)
            r.sync()
            times = {k: [] for k in WAYS}
            for rnd in range(a.rounds + 1):
                for way in WAYS:
                    r.timer_begin()
                    n = run(way)
                    ms = r.timer_end() / n
                    if rnd > 0:                                # (round 0: dropped)
                        times[way].append(ms)
            res = {}
            for k, t in times.items():
                t = np.array(t)
                res[k] = dict(ms=round(float(np.median(t)), 5), spread=round(float((t.max() - t.min()) / np.median(t)), 4),
                              rounds_ms=[round(float(v), 5) for v in t])
            elems = 3 * npx
            for n in PASSES:
                batch = BATCH if BATCH * 12 * ((npx + 3) & ~3) <= SCRATCH_MAX else 1
                kernels = (n + batch - 1) // batch
                for k, per in (("acc", 16), ("mom", 32)):
                    e = res[f"{k}{n}"]
                    nbytes = elems * (4 * n + per * kernels - per // 2)          # (the first kernel of a reset call does not read the sums)
                    e["add_ms"] = round(e["ms"] - n * res["render"]["ms"], 5)
                    e["add_bytes"] = int(nbytes)
                    e["add_fraction"] = round(nbytes / (e["add_ms"] * 1e-3) / COPY_RATE, 4) if e["add_ms"] > 0 else None
                m, p_ = res[f"mom{n}"], res[f"acc{n}"]
                m["vs_parent"] = round(m["ms"] / p_["ms"], 4)
                m["add_vs_parent"] = round(m["add_ms"] / p_["add_ms"], 4) if p_["add_ms"] > 0 else None
            for levels in (1, 4):
                res[f"var{levels}"]["vs_parent"] = round(res[f"var{levels}"]["ms"] / res[f"den{levels}"]["ms"], 4)
            for d in (d32, dg, dsum, dsq, dscratch_s, dscratch_q, dout, dwork, dout4, dwork4):
                r.free(d)
            out[case] = dict(workload=name, reps_per_round=reps, pixels=npx, **res)
        finally:
            r.close()
    if a.add_only:
        return
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
