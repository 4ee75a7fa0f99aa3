"""Scene queries that form their float64 direction only when their cull leaves a sphere (rt_device.h: closest_hit, any_hit_masks;
rt_cull.h has the guard and the bound).  Six small frames at depth 3 built for the cases of that change, each through the default
variant and the counting instantiation, every byte against the CPU oracle: uint8 and float32, and the ray counters."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEPTH = 3
GREY, RED, BLUE, GREEN = (128, 128, 128), (255, 0, 0), (0, 0, 255), (0, 255, 0)


def _spheres(rows):
    return np.array([[*c, r, *col] for c, r, col in rows], np.float32).reshape(-1, 7).T.copy()


def _planes(rows):
    return np.array([[*p0, *n, *col] for p0, n, col in rows], np.float32).reshape(-1, 9).T.copy()


def _frames():
    from python_ray_tracer_amd import workloads
    from python_ray_tracer_amd.scene import Camera
    wl = workloads.build(workloads.HEADLINE)
    big = workloads.build("c4_3840x2160_s64_d5")
    lights = np.asarray(wl["lights"], np.float32)
    cam = np.asarray(workloads.CAMERA["position"], np.float64)
    ground = _planes([((0, 0, 0), (0, 0, 1), GREY)])
    out = {
        # a: the headline scene: tiles whose lanes' queries mix empty and non-empty cull masks
        "headline": (64, 40, wl["spheres"], lights, wl["planes"]),
        # b: a tilted plane whose stored normal is not unit length in float64: the directions reflected off it leave the unit
        #    window, and tiles mix plane and sphere hits
        "tilted_plane": (64, 40, _spheres([((2.5, -0.6, 0.9), 0.7, RED), ((3.5, 0.9, 0.8), 0.6, BLUE)]), lights,
                         _planes([((0, 0, 0), (0.3, 0.2, 1.0), GREY)])),
        # c: the camera inside a sphere and a light inside a sphere: anchors that certify nothing
        "anchors_inside": (48, 32, _spheres([(tuple(cam), 3.0, GREEN), (tuple(lights[:, 0]), 0.5, RED), ((0.5, 0.4, 0.5), 0.5, BLUE),
                                             ((-0.5, -1.0, 0.4), 0.4, RED)]), lights, ground),
        # d: no planes
        "spheres_only": (48, 32, wl["spheres"], lights, np.zeros((9, 0), np.float32)),
        # e: no spheres
        "planes_only": (48, 32, np.zeros((7, 0), np.float32), lights,
                        _planes([((0, 0, 0), (0, 0, 1), GREY), ((6, 0, 0), (-1, 0.1, 0.2), BLUE)])),
        # f: 65 spheres, two cull chunks: the 64 of config 4 and one on its own, high above them
        "two_chunks": (64, 40, np.concatenate([big["spheres"], _spheres([((2.0, 2.5, 4.0), 0.7, RED)])], axis=1), lights, ground),
    }
    cams = {k: Camera(resolution=(v[0], v[1]), **workloads.CAMERA) for k, v in out.items()}
    return out, cams, wl


_REF = {}


def _reference(oracle, name):
    """The oracle's frame and counters of frame `name`, computed once."""
    if name not in _REF:
        frames, cams, wl = _frames()
        w, h, sp, li, pl = frames[name]
        cam = cams[name]
        rg = cam.raygen()
        ref = oracle.render(w, h, cam.position, cam.rotation, sp, li, pl, wl["amb"], wl["lamb"], wl["refl"], DEPTH, wl["aa"],
                            raygen=rg, want=("u8", "f32"))
        _REF[name] = (frames[name], cam, rg, wl, ref)
    return _REF[name]


@pytest.mark.parametrize("name", ["headline", "tilted_plane", "anchors_inside", "spheres_only", "planes_only", "two_chunks"])
def test_frame_bit_identical_to_oracle(renderer, oracle, name):
    from python_ray_tracer_amd import _lib as L
    (w, h, sp, li, pl), cam, rg, wl, ref = _reference(oracle, name)
    assert w <= 64 and h <= 40
    renderer.set_scene(sp, li, pl)
    renderer.set_camera(cam.position, cam.rotation)
    renderer.set_raygen(w, h, *rg)
    for flags in (0, L.RT_FLAG_COUNT_RAYS):
        renderer.reset_stats()
        u8, f32 = renderer.render(wl["amb"], wl["lamb"], wl["refl"], DEPTH, wl["aa"], u8=True, f32=True, flags=flags)
        assert np.array_equal(u8, ref["u8"]), f"flags {flags}: {(u8 != ref['u8']).any(axis=0).sum()} pixels differ (uint8)"
        assert np.array_equal(f32, ref["f32"]), f"flags {flags}: float32 colours differ from the oracle"
        assert u8.any(), "empty frame"
    st, cnt = renderer.stats(), ref["counters"]
    assert st["closest_queries"] == cnt["closest"] and st["hits"] == cnt["hits"]
    assert st["shadow_traced"] + st["shadow_skipped"] == cnt["shadow"]
    assert cnt["closest"] > w * h                                  # reflected rays were traced
    renderer.reset_stats()
