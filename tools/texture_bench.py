#!/usr/bin/env python3
"""Cost of textures: workloads.build configs with textures (rt_set_scene_textures) against the same scene without, interleaved,
timed with device events.

    python tools/texture_bench.py [--rounds 5] [--frames 50] [--cases c2,c4,c5]

  plain    no texture: the table below has a rough row, so the scene runs the scatter kernels (SCAT) — the twins of the texture
           kernels, so that the next column is the price of the texture kernels themselves
  uniform  the same scene with a 1 x 1 x 1 texture of its own colour on every object (one record per distinct colour): the
           texture kernels (TEX_SCAT), every hit looks its texel up, and the frame is the plain one, byte for byte
  textured a checkered floor (cells of 0.5) and a 256 x 256 image projected on every third sphere: the lookups scatter over
           65 540 texels (1 MB)
All three have the same geometry and materials.  Each way has its own context (its scene set once, its dispatch order settled
by the warm-up).  A round times `--frames` launches (fewer for the larger configs, about the same time) into device memory
for each way in turn; the median over rounds is reported, with the spread (max - min) / median.  set_scene_ms is the host time
of one rt_set_scene_textures call of the textured scene and of one with RT_MAX_TEXELS texels (every call uploads its texels).
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import python_ray_tracer_amd as pkg                       # noqa: E402
from python_ray_tracer_amd import workloads               # noqa: E402
from python_ray_tracer_amd.scene import Texture           # noqa: E402

# rows 0-2: spheres (row 1 a brushed mirror); 3 the floor (a mirror)
TABLE = [(0.0, 0.6, 0.3, 0.0, 1.0, 0.0), (0.0, 0.4, 0.8, 0.0, 1.0, 0.1), (0.1, 0.6, 0.0, 0.0, 1.0, 0.0),
         (0.0, 0.3, 0.75, 0.0, 1.0, 0.0)]
WAYS = ("plain", "uniform", "textured")
# case -> (workload, frames per round relative to --frames)
CASES = {"c2": ("c2_1920x1080_s8_d3", 1.0), "c4": ("c4_3840x2160_s64_d5", 0.2), "c5": ("c5_7680x4320_s256_d8", 0.04)}


def table(S, P):
    sid = np.array([1 if i % 3 == 0 else (0 if i % 2 else 2) for i in range(S)], np.int32)
    return np.array(TABLE, dtype=np.float64), sid, np.full(P, 3, np.int32)


def textures(way, S, P, wl=None):
    if way == "plain":
        return None
    if way == "uniform":
        cols = np.concatenate([wl["spheres"][4:7].T, wl["planes"][6:9].T]).astype(np.float32)
        uniq, ids = np.unique(cols, axis=0, return_inverse=True)
        assert len(uniq) <= 64, "more distinct colours than texture records"
        recs = [((0.0, 0.0, 0.0), np.eye(3), (1, 1, 1), k) for k in range(len(uniq))]
        ids = ids.reshape(-1).astype(np.int32)
        return recs, ids[:S], ids[S:], uniq
    rng = np.random.default_rng(256)
    floor = Texture.checker((235, 235, 235), (25, 25, 25), 0.5)
    image = Texture.image(rng.integers(0, 256, (256, 256, 3)), (0.0, -0.5, 1.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0))
    recs = [(floor.origin, floor.axes, floor.dims, 0), (image.origin, image.axes, image.dims, 4)]
    st = np.array([1 if i % 3 == 0 else -1 for i in range(S)], np.int32)
    return recs, st, np.zeros(P, np.int32), np.concatenate([floor.texels.reshape(-1, 3), image.texels.reshape(-1, 3)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    out = {"metric": "texture_cost", "rounds": a.rounds, "frames": a.frames}
    for case in a.cases.split(","):
        name, rel = CASES[case]
        frames = max(2, int(round(a.frames * rel)))
        wl = workloads.build(name)
        w, h, S, P = wl["w"], wl["h"], wl["spheres"].shape[1], wl["planes"].shape[1]
        mats = table(S, P)
        ctx = {}
        try:
            for k in WAYS:
                r = pkg.Renderer(0)
                r.set_scene(wl["spheres"], wl["lights"], wl["planes"], materials=mats, textures=textures(k, S, P, wl))
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
            res["uniform"]["same_frame_as_plain"] = bool(np.array_equal(frames8["uniform"], frames8["plain"]))
            res["uniform"]["vs_plain"] = round(res["uniform"]["ms"] / res["plain"]["ms"], 4)
            res["textured"]["vs_plain"] = round(res["textured"]["ms"] / res["plain"]["ms"], 4)
            # the host side of a scene change: the textured scene, and the largest texel array
            r = ctx["textured"][0]
            tx = textures("textured", S, P)
            big = (tx[0], tx[1], tx[2], np.zeros((pkg._lib.RT_MAX_TEXELS, 3), np.float32))
            big[3][:len(tx[3])] = tx[3]
            ms = {}
            for label, t_ in (("textured", tx), ("max_texels", big)):
                r.set_scene(wl["spheres"], wl["lights"], wl["planes"], materials=mats, textures=t_)    # (allocates)
                t0 = time.perf_counter()
                for _ in range(3):
                    r.set_scene(wl["spheres"], wl["lights"], wl["planes"], materials=mats, textures=t_)
                ms[label] = round((time.perf_counter() - t0) / 3 * 1e3, 3)
            out[case] = dict(workload=name, frames=frames, set_scene_ms=ms, **res)
        finally:
            for r, _, d8 in ctx.values():
                r.free(d8)
                r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
