"""The call sequence whose cull-table builds tests/golden/stream_state_trace.npz records, for tests/test_gpu_stream_state.py: one
stream that uses every per-stream buffer the context keeps for it (python-ray-tracer_amd/csrc/rt_streams.h).

The scene is tests/golden/frame_default_128_d3.npz's at 128 x 128.  A round is STEPS on one library-made stream, the stream
synchronised after every step:
    "render"   a depth-3 rt_render_device: the stream's first table set
    "lattice"  the same launch with RT_AA_REFERENCE: the lattice buffer, the same tables
    "guides"   rt_render_guides: a depth-0 table set, the stream's second
    "film"     rt_film_accumulate of one pass, twice (the first resets the sum): the film scratch, the first set again
ROUNDS is three rounds that each end in rt_stream_forget, then the steps twice with no forget between them: the second time every
step finds its tables.

    python stream_state_cases.py record OUT.npz    runs ROUNDS on the GPU with the library the package loads (MI355RT_SO selects
                                                   another build) on a context of its own, twice, and writes the per-step
                                                   table_builds deltas if the two recordings are equal
"""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(TESTS, "golden")
FIXTURE = "default_128_d3"
W = H = 128
RT_AA_REFERENCE, RT_GUIDE_PLANES = 1, 8
STEPS = ("render", "lattice", "guides", "film", "film")
ROUNDS = [STEPS + ("forget",)] * 3 + [STEPS, STEPS]
OUTPUTS = {"render": ((3, W, H), np.uint8), "lattice": ((3, W, H), np.uint8), "guides": ((RT_GUIDE_PLANES, W, H), np.float32),
           "film": ((3, W, H), np.float64)}


def setup(r):
    """The fixture's scene, camera and grid on renderer r; returns the fixture."""
    for d in (TESTS, os.path.dirname(TESTS)):            # (as a script: the suite's helpers and the package)
        if d not in sys.path:
            sys.path.insert(0, d)
    from conftest import raygen_closed_form
    g = np.load(os.path.join(GOLDEN, f"frame_{FIXTURE}.npz"))
    r.set_scene(g["spheres"], g["lights"], g["planes"])
    r.set_camera(g["cam_origin"], g["cam_rot"])
    r.set_raygen(W, H, *raygen_closed_form(W, H, float(g["fov"])))
    return g


def run(r, g, stream, rounds=ROUNDS):
    """`rounds` on `stream` of renderer r (setup(r) has run): (the table_builds delta of every step, int64; per round a dict of what
    its steps left in device memory, by step name)."""
    params = {aa: r.params(float(g["amb"]), float(g["lamb"]), float(g["refl"]), int(g["depth"]), aa, refl_pow=g["refl_pow"])
              for aa in (0, RT_AA_REFERENCE)}
    bufs = {n: r.malloc(int(np.prod(shape)) * np.dtype(dt).itemsize) for n, (shape, dt) in OUTPUTS.items()}
    deltas, left = [], []
    try:
        for steps in rounds:
            film_passes = 0
            for s in steps:
                before = r.stats()["table_builds"]
                if s == "render":
                    r.render_device(params[0], 0, W, bufs[s], None, stream=stream)
                elif s == "lattice":
                    r.render_device(params[RT_AA_REFERENCE], 0, W, bufs[s], None, stream=stream)
                elif s == "guides":
                    r.render_guides(0, W, bufs[s], stream=stream)
                elif s == "film":
                    r.film_accumulate(params[0], 0, W, 1, film_passes == 0, bufs[s], stream=stream)
                    film_passes += 1
                elif s == "forget":
                    r.stream_forget(stream)
                else:
                    raise ValueError(s)
                r.sync(stream)
                deltas.append(r.stats()["table_builds"] - before)
            out = {}
            for n, (shape, dt) in OUTPUTS.items():
                out[n] = np.empty(shape, dt)
                r.d2h(out[n], bufs[n])
            left.append(out)
    finally:
        r.sync(stream)
        for b in bufs.values():
            r.free(b)
    return np.asarray(deltas, np.int64), left


def record_once():
    for d in (TESTS, os.path.dirname(TESTS)):
        if d not in sys.path:
            sys.path.insert(0, d)
    from python_ray_tracer_amd import Renderer
    r = Renderer(0)
    try:
        g = setup(r)
        stream = r.stream_create()
        deltas, _ = run(r, g, stream)
        r.stream_destroy(stream)
    finally:
        r.close()
    return deltas


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "record":
        sys.exit(__doc__)
    first, second = record_once(), record_once()
    if not np.array_equal(first, second):
        sys.exit(f"the two recordings differ: {first.tolist()} {second.tolist()}")
    np.savez_compressed(sys.argv[2], steps=np.array([s for rd in ROUNDS for s in rd]), table_builds=first.astype(np.int32))
    print("recorded", first.tolist())
