"""The call sequences whose dispatch-order feedback decisions tests/golden/feedback_trace.npz records, for the CPU replay of
tests/algo/feedback_check.cpp (tests/test_algorithms.py) and the GPU replay of tests/test_gpu_feedback_trace.py.

The scene is tests/golden/frame_default_128_d3.npz's at 128 x 128; the launch geometries are the full frame and eleven column
ranges (8i, 8i + 40); three streams (0: the context's own) and four cameras (0: the fixture's); one context per
MI355RT_REMEASURE of REMEASURES.  A step is a tuple:
    ("scene",)  ("camera", i)  ("grid", w, h)  ("forget", stream)  ("launch", stream, geometry, variant)
    ("sequence", stream, geometry, frames, frames_per_launch)      (static rt_render_sequence; Script B only)
SCRIPT_A is replayed on the CPU and on the GPU, SCRIPT_B (its beginning, then sequences on a fresh and on a settled geometry:
the unsettled-sequence path of dispatch()) on the GPU only.  After every step the launching stream is synchronised, so every
order kernel is complete by the next call and the decisions do not depend on timing.

    python feedback_trace_cases.py record OUT.npz    replays both scripts on the GPU with the library the package loads
                                                     (MI355RT_SO selects another build), twice, and writes the per-step deltas
                                                     of FIELDS if the two recordings are equal
"""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(TESTS, "golden")
FIXTURE = "default_128_d3"
REMEASURES = (24, 2, 0)
FIELDS = ("launches", "frames", "launches_measuring", "launches_settled", "table_builds")
W = H = 128
GEOMETRIES = [(0, W)] + [(8 * i, 8 * i + 40) for i in range(11)]
SMALL = 12                                              # geometry index of the 8 x 8 frame's only range
RT_AA_REFERENCE, RT_AA_STOCHASTIC, RT_FLAG_NO_FEEDBACK = 1, 2, 4
VARIANTS = {"d3": dict(depth=3), "d1": dict(depth=1), "spp2": dict(depth=3, aa=RT_AA_STOCHASTIC, spp=2),
            "ref": dict(depth=3, aa=RT_AA_REFERENCE), "nofb": dict(depth=3, flags=RT_FLAG_NO_FEEDBACK)}
CAMERA_SHIFTS = [(0.0, 0.0, 0.0), (0.25, 0.0, 0.0), (0.0, 0.5, 0.25), (-0.5, 0.25, 0.0)]     # added to the fixture's position


def _launches(stream_geometry_variant):
    return [("launch", s, g, v) for s, g, v in stream_geometry_variant]


def _script_a():
    st = [("scene",), ("camera", 0), ("grid", W, H)]
    # settle in three launches, on three streams; the same camera again keeps the settled state
    st += _launches([(0, 0, "d3"), (1, 0, "d3"), (2, 0, "d3"), (0, 0, "d3")])
    st += [("camera", 0)] + _launches([(1, 0, "d3")])
    # every variant is a geometry of its own; a launch without feedback takes no slot
    for v, s in (("d1", 0), ("spp2", 1), ("ref", 2)):
        st += _launches([(s, 0, v)] * 3)
    st += _launches([(0, 0, "nofb"), (1, 0, "nofb"), (0, 0, "d3")])
    # a camera change loses the settled state; the order is kept for MI355RT_REMEASURE launches, then measured again
    st += [("camera", 1)] + _launches([(s % 3, 0, "d3") for s in range(6)])
    st += [("camera", 2)] + _launches([(0, 0, "d3"), (1, 0, "d1"), (2, 0, "d3"), (2, 0, "ref")])
    # the same scene again is a new epoch too
    st += [("scene",)] + _launches([(1, 0, "d3"), (1, 0, "d3"), (2, 0, "d3"), (0, 0, "spp2")])
    # forgotten streams come back
    st += [("forget", 1)] + _launches([(1, 0, "d3"), (2, 0, "d3")]) + [("forget", 2), ("forget", 1)] + _launches([(2, 0, "d3")])
    # twelve geometries share eight slots: the ninth evicts a live one, and an evicted geometry starts again
    for rep in range(3):
        st += _launches([((g + rep) % 3, g, "d3") for g in range(1, 12)])
    st += _launches([(0, 0, "d3"), (1, 0, "d3"), (0, 0, "d3"), (2, 3, "d3"), (0, 0, "d1")])
    # an 8 x 8 frame is one block: no feedback
    st += [("grid", 8, 8)] + _launches([(0, SMALL, "d3"), (1, SMALL, "d3"), (0, SMALL, "nofb")]) + [("grid", W, H)]
    st += _launches([(0, 0, "d3"), (1, 0, "d3"), (2, 0, "d3")])
    # a camera that moves with every launch, then rests at the fixture's
    for i in range(9):
        st += [("camera", 1 + i % 3)] + _launches([(i % 3, 0, "d3")])
    st += [("camera", 0)] + _launches([(0, 0, "d3"), (1, 0, "d3"), (2, 0, "d3"), (0, 0, "d3")])
    return st


SCRIPT_A = _script_a()
SCRIPT_B = SCRIPT_A[:7] + [("sequence", 0, 1, 5, 4), ("sequence", 1, 0, 5, 4), ("sequence", 2, 1, 5, 4), ("camera", 1),
                           ("sequence", 0, 0, 5, 4), ("camera", 0), ("sequence", 1, 2, 5, 4)] + _launches([(0, 0, "d3")] * 3)
SCRIPTS = {"A": SCRIPT_A, "B": SCRIPT_B}


def _range(g):
    return (0, 8) if g == SMALL else GEOMETRIES[g]


def write_script(path):
    """SCRIPT_A, once per MI355RT_REMEASURE, in the text form feedback_check reads: the scene, the cameras' origins, then `ctx R` and the
    steps."""
    g = np.load(os.path.join(GOLDEN, f"frame_{FIXTURE}.npz"))
    with open(path, "w") as f:
        f.write(f"scene {g['spheres'].shape[1]} {g['lights'].shape[1]} {g['planes'].shape[1]}\n")
        for a in (g["spheres"], g["lights"], g["planes"]):
            f.write(" ".join(repr(float(v)) for v in np.ascontiguousarray(a, np.float32).ravel()) + "\n")
        f.write(f"cameras {len(CAMERA_SHIFTS)}\n")              # rt_set_camera's origins, as replay() passes them
        for shift in CAMERA_SHIFTS:
            f.write(" ".join(repr(float(v)) for v in np.asarray(g["cam_origin"], np.float64) + np.asarray(shift)) + "\n")
        for rm in REMEASURES:
            f.write(f"ctx {rm}\n")
            for s in SCRIPT_A:
                if s[0] == "launch":
                    v = VARIANTS[s[3]]
                    f.write("launch %d %d %d %d %d %d %d\n" % ((s[1],) + _range(s[2]) + (v["depth"], v.get("aa", 0), v.get("spp", 0), v.get("flags", 0))))
                else:
                    f.write(" ".join(str(x) for x in s) + "\n")


def replay(script, remeasure):
    """The script on a context of its own on the GPU, created under MI355RT_REMEASURE = remeasure: (the deltas of FIELDS per
    step, int64 (steps, 5); the uint8 frame of the last launch)."""
    for d in (TESTS, os.path.dirname(TESTS)):            # (as a script: the suite's helpers and the package)
        if d not in sys.path:
            sys.path.insert(0, d)
    from conftest import raygen_closed_form
    from python_ray_tracer_amd import Renderer
    g = np.load(os.path.join(GOLDEN, f"frame_{FIXTURE}.npz"))
    was = os.environ.get("MI355RT_REMEASURE")
    os.environ["MI355RT_REMEASURE"] = str(remeasure)
    try:
        r = Renderer(0)
    finally:
        if was is None:
            del os.environ["MI355RT_REMEASURE"]
        else:
            os.environ["MI355RT_REMEASURE"] = was
    rows, last = [], None
    frame_bytes = 3 * W * H
    try:
        streams = [None, r.stream_create(), r.stream_create()]
        bufs = [r.malloc(5 * frame_bytes) for _ in streams]
        params = {n: r.params(float(g["amb"]), float(g["lamb"]), float(g["refl"]), v["depth"], v.get("aa", 0), v.get("flags", 0),
                              refl_pow=g["refl_pow"][:v["depth"]], spp=v.get("spp", 0)) for n, v in VARIANTS.items()}
        before = r.stats()
        for s in script:
            if s[0] == "scene":
                r.set_scene(g["spheres"], g["lights"], g["planes"])
            elif s[0] == "camera":
                r.set_camera(np.asarray(g["cam_origin"], np.float64) + np.asarray(CAMERA_SHIFTS[s[1]]), g["cam_rot"])
            elif s[0] == "grid":
                r.set_raygen(s[1], s[2], *raygen_closed_form(s[1], s[2], float(g["fov"])))
            elif s[0] == "forget":
                r.stream_forget(streams[s[1]])
            elif s[0] == "launch":
                x0, x1 = _range(s[2])
                r.render_device(params[s[3]], x0, x1, bufs[s[1]], None, stream=streams[s[1]])
                r.sync(streams[s[1]])
                last = (s, bufs[s[1]])
            elif s[0] == "sequence":
                x0, x1 = _range(s[2])
                r.render_sequence(params["d3"], x0, x1, s[3], bufs[s[1]], None, streams=[streams[s[1]]] if streams[s[1]] else None,
                                  frames_per_launch=s[4])
                r.sync(streams[s[1]])
            else:
                raise ValueError(s)
            now = r.stats()
            rows.append([now[k] - before[k] for k in FIELDS])
            before = now
        (_, _, geo, _), buf = last
        x0, x1 = _range(geo)
        frame = np.empty((3, x1 - x0, r.h), np.uint8)
        r.d2h(frame, buf)
        for b in bufs:
            r.free(b)
        for st in streams[1:]:
            r.stream_destroy(st)
    finally:
        r.close()
    return np.asarray(rows, np.int64), frame


def replay_all():
    """{"A/24": deltas, ...} of every script and MI355RT_REMEASURE, and {"A/24": last frame, ...}."""
    rows, frames = {}, {}
    for name, script in SCRIPTS.items():
        for rm in REMEASURES:
            rows[f"{name}/{rm}"], frames[f"{name}/{rm}"] = replay(script, rm)
    return rows, frames


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "record":
        sys.exit(__doc__)
    first, _ = replay_all()
    second, _ = replay_all()
    for k in first:
        if not np.array_equal(first[k], second[k]):
            bad = np.flatnonzero((first[k] != second[k]).any(axis=1))
            sys.exit(f"{k}: the two recordings differ at steps {bad.tolist()}: {[SCRIPTS[k[0]][i] for i in bad[:5]]}")
    np.savez_compressed(sys.argv[2], fields=np.array(FIELDS), **{k: v.astype(np.int32) for k, v in first.items()})
    print("recorded", {k: v.sum(axis=0).tolist() for k, v in first.items()})
