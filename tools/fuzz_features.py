#!/usr/bin/env python3
"""Soak test of the feature kernels: random scenes of tools/feature_scenes.py (per-object materials, glass, rough surfaces, area
lights and a thin lens together), HIP kernel vs the CPU oracle's orc_render_ex, bit-exact uint8 and float32.
    python tools/fuzz_features.py [--seconds 240] [--seed 1] [--lit]
Scene i of a run is feature_scenes.draw(seed * 1000003 + i), so a mismatch is replayed from its printed number alone; with --lit it
is feature_scenes.draw_lit of that number: the same scene with non-uniform textures, coloured lights, highlights and a sky, which
runs the texture, lighting and sky kernels with their features live.  Every fourth scene is also checked for liveness (five more
oracle frames, eight with --lit): the summary reports how many of those were vacuous (no feature changes the oracle's frame; with
--lit: none of textures, lighting and sky does).  Vacuous scenes are compared like the others and counted in the scene total."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402

import feature_scenes as fs  # noqa: E402


def main():
    import python_ray_tracer_amd as pkg
    from oracle import oracle as orc
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--lit", action="store_true", help="feature_scenes.draw_lit: textures, coloured lights, highlights and a sky as well")
    a = ap.parse_args()
    r = pkg.Renderer(0)
    t0, n, bad, vacuous = time.time(), 0, 0, 0
    kinds = {}
    try:
        while time.time() - t0 < a.seconds:
            sid = a.seed * 1000003 + n
            sc = fs.draw_lit(sid) if a.lit else fs.draw(sid)
            r8, r32 = fs.oracle_frame(orc, sc)
            if n % 4 == 0:                                    # liveness on a quarter of the scenes (it costs five oracle frames)
                lv = fs.live(orc, sc, r8)
                if max(lv[k] for k in (fs.LIT if a.lit else lv)) == 0:
                    vacuous += 1
            u8, f32 = fs.gpu_frame(r, sc)
            n += 1
            kinds[sc["kind"]] = kinds.get(sc["kind"], 0) + 1
            if not (np.array_equal(u8, r8) and np.array_equal(f32.view(np.uint32), r32.view(np.uint32))):
                bad += 1
                d = (u8 != r8).any(axis=0) | (f32.view(np.uint32) != r32.view(np.uint32)).any(axis=0)
                print(f"MISMATCH scene {sid}: kind={sc['kind']} S={sc['spheres'].shape[1]} P={sc['planes'].shape[1]} "
                      f"L={sc['lights'].shape[1]} {sc['w']}x{sc['h']} depth={sc['depth']} aa={sc['aa']}: {int(d.sum())} px", flush=True)
            if n % 200 == 0:
                print(f"{n} scenes, {bad} mismatches, {time.time() - t0:.0f}s", flush=True)
    finally:
        r.close()
    print(f"DONE seed {a.seed}{' --lit' if a.lit else ''}: {n} scenes, {bad} mismatches, {vacuous} vacuous of {(n + 3) // 4} checked; kinds {kinds}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
