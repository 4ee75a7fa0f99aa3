"""TEST INFRASTRUCTURE ONLY — seeded random scenes with every feature of include/mi355rt.h (per-object materials, glass,
rough surfaces, area lights, a thin lens), for tests/test_gpu_features_vs_oracle.py and the soak tools/fuzz_features.py.

draw(seed) returns one scene as a dict; every key of it is plain data (numpy arrays and numbers).  Scenes are biased toward
what the feature paths get wrong: cameras, lights and lens points inside glass spheres, touching and nested spheres, total
internal reflection and grazing absorption, glass windows (transparent planes), negative ambient, refl = 1 at depth 16 and
scales from 1e-3 to 1e3.

oracle_kwargs(sc) / oracle_frame(orc, sc) give the CPU oracle's arguments and frame; strip(sc, what) the same scene with one
feature turned off ("materials", "glass", "rough", "soft", "lens"), for the tests' liveness checks."""
import numpy as np

KINDS = ("plain", "touching", "camera_in_glass", "lens_in_glass", "light_in_glass", "tir", "grazing", "window", "mirror16",
         "negative_ambient")


def _rot(euler):
    from python_ray_tracer_amd.scene.rotation import euler_rotation
    return np.asarray(euler_rotation(*euler), dtype=np.float64)


def _raygen(w, h, fov):
    ar = int(w / h)
    px = float(1 / np.tan(np.radians(fov) / 2))
    return (px, float(ar), (-ar - ar) / float(w - 1), 1.0, (-1 - 1) / float(h - 1))


def _row(rng, kind):
    """(amb, lamb, refl, trans, ior, rough) of one material of the given kind."""
    amb = float(rng.uniform(0.0, 0.15))
    lamb = float(rng.uniform(0.1, 0.9))
    if kind == "glass":
        return [amb * 0.3, lamb * 0.3, 0.0, float(rng.uniform(0.3, 1.0)), float(rng.choice([1.0, 1.33, 1.5, 1.5, 2.4, 0.7])), 0.0]
    if kind == "rough":
        return [amb, lamb, float(rng.uniform(0.2, 1.0)), 0.0, 1.0, float(rng.choice([1.0, rng.uniform(0.01, 1.0)]))]
    if kind == "mirror":
        return [amb, lamb, float(rng.choice([1.0, rng.uniform(0.3, 1.0)])), 0.0, 1.0, 0.0]
    return [amb, lamb, float(rng.uniform(0.0, 0.5)), 0.0, 1.0, 0.0]


def draw(seed, w=None, h=None, kind=None):
    """One random scene with every feature (a material table of 6 columns with glass and rough rows, area lights, a lens)."""
    rng = np.random.default_rng(seed)
    kind = KINDS[int(rng.integers(0, len(KINDS)))] if kind is None else kind
    scale = float(rng.choice([1e-3, 0.05, 1.0, 1.0, 1.0, 30.0, 1e3]))
    S = int(rng.choice([1, 3, 5, 8, 17, 40, 97, 170]))
    sp = np.zeros((7, S), np.float32)
    sp[0:3] = rng.uniform(-3, 5, (3, S)) * scale
    sp[0] = np.abs(sp[0]) + 1.0 * scale                            # mostly in front of the camera (forward is +x)
    sp[3] = rng.uniform(0.2, 1.2, S) * scale
    sp[4:7] = rng.integers(0, 256, (3, S))
    P = int(rng.integers(0, 3))
    pl = np.zeros((9, P), np.float32)
    if P:
        pl[0:3] = rng.uniform(-2, 2, (3, P)) * scale
        nrm = rng.normal(size=(3, P))
        nrm[2] += 2.0                                              # mostly floors
        pl[3:6] = nrm / np.linalg.norm(nrm, axis=0, keepdims=True)
        pl[6:9] = rng.integers(0, 256, (3, P))
    NL = int(rng.choice([1, 2, 3, 5, 9]))
    li = (rng.uniform(-4, 6, (3, NL)) * scale).astype(np.float32)
    li[2] = np.abs(li[2]) + 2.0 * scale
    radius = (rng.uniform(0.05, 1.0, NL) * scale * (rng.uniform(size=NL) < 0.7)).astype(np.float32)
    radius[0] = np.float32(0.3 * scale)
    n = int(rng.choice([1, 2, 3, 4, 16]))
    # the table: matte, mirror, rough and glass rows
    kinds = ["matte", "mirror", "rough", "glass"] + [str(k) for k in rng.choice(["matte", "mirror", "rough", "glass"], int(rng.integers(0, 5)))]
    table = np.array([_row(rng, k) for k in kinds], np.float64)
    sid = rng.integers(0, len(table), S).astype(np.int32)
    pid = rng.integers(0, len(table), P).astype(np.int32)
    pos = np.array([0.0, 0.0, 0.5 * scale])
    euler = [float(rng.uniform(-20, 20)), float(rng.uniform(-25, 10)), float(rng.uniform(-30, 30))]
    depth = int(rng.choice([1, 2, 3, 4, 6, 9, 16]))
    glass = 3
    if kind == "touching" and S >= 3:                              # touching and nested spheres, one of them glass
        sp[0:3, 1] = sp[0:3, 0] + np.array([0.0, sp[3, 0] + sp[3, 1], 0.0], np.float32)
        sp[0:3, 2] = sp[0:3, 0]
        sp[3, 2] = sp[3, 0] * 0.5
        sid[0] = glass
    elif kind in ("camera_in_glass", "lens_in_glass", "tir"):     # the camera (and its lens) inside a glass sphere
        sp[0:3, 0] = pos
        sp[3, 0] = np.float32(rng.uniform(0.5, 2.0) * scale)
        sid[0] = glass
        if kind == "tir":
            table[glass, 4] = 2.4
        if kind == "lens_in_glass":                                # the lens rim straddles the glass surface
            sp[0:3, 0] = pos + np.array([0.0, 1.0, 0.0]) * scale
            sp[3, 0] = np.float32(1.0 * scale)
    elif kind == "light_in_glass":
        sp[0:3, 0] = li[:, 0]
        sp[3, 0] = np.float32(0.8 * scale)
        sid[0] = glass
    elif kind == "grazing":                                        # a rough floor seen at a grazing angle
        P = 1
        pl = np.array([[0], [0], [0], [0], [0], [1], [200], [180], [160]], np.float32) * np.array([scale] * 3 + [1] * 6, np.float32)[:, None]
        pid = np.array([2], np.int32)
        table[2, 5] = 1.0
        pos = np.array([-3.0, 0.0, 0.05]) * scale
        euler = [0.0, float(rng.uniform(-6, -1)), float(rng.uniform(-10, 10))]
    elif kind == "window":                                         # a glass sheet between the camera and the spheres
        P = 2
        pl = np.zeros((9, 2), np.float32)
        pl[:, 0] = [0.6 * scale, 0, 0, 1, 0.05, 0.02, 120, 140, 200]
        pl[:, 1] = [0, 0, -1.0 * scale, 0, 0, 1, 200, 200, 200]
        pid = np.array([glass, 0], np.int32)
    elif kind == "mirror16":                                       # refl = 1 at depth 16
        table[1, 2] = 1.0
        sid[: max(1, S // 2)] = 1
        depth = 16
    elif kind == "negative_ambient":
        table[:, 0] = -np.abs(table[:, 0]) - 0.05
    if w is None:
        w, h = int(rng.integers(20, 56)), int(rng.integers(14, 40))
    fov = float(rng.uniform(35, 80))
    aperture = float(rng.uniform(0.02, 0.3) * scale)
    focus = float(rng.uniform(0.5, 6.0) * scale)
    aa = int(rng.choice([0, 0, 1, 1, 2]))
    flags_aa = 32 if (aa == 1 and rng.uniform() < 0.5) else 0     # RT_FLAG_AA_PER_PIXEL
    typed = int(rng.uniform() < 0.3)                               # RT_FLAG_TYPED_BIAS (a scene flag)
    return dict(kind=kind, seed=int(seed), w=int(w), h=int(h), spheres=sp, lights=li, planes=pl, table=table, sid=sid, pid=pid,
                radius=radius, n=n, lens=(aperture, focus), cam_origin=pos.astype(np.float64), cam_rot=_rot(euler), fov=fov,
                raygen=_raygen(w, h, fov), depth=depth, aa=aa, flags_aa=flags_aa, spp=int(rng.integers(1, 5)),
                hseed=int(rng.integers(0, 2 ** 32)), typed=typed)


def strip(sc, what):
    """The same scene with one feature off: 'glass' (trans 0), 'rough' (rough 0), 'soft' (radii 0), 'lens' (aperture 0),
    'materials' (one table row for every object)."""
    sc = dict(sc)
    t = np.array(sc["table"])
    if what == "glass":
        t[:, 3], t[:, 4] = 0.0, 1.0
    elif what == "rough":
        t[:, 5] = 0.0
    elif what == "soft":
        sc["radius"] = np.zeros_like(sc["radius"])
    elif what == "lens":
        sc["lens"] = (0.0, sc["lens"][1])
    elif what == "materials":
        sc["sid"] = np.zeros_like(sc["sid"])
        sc["pid"] = np.zeros_like(sc["pid"])
    sc["table"] = t
    return sc


def oracle_kwargs(sc):
    return dict(raygen=sc["raygen"], flags=int(sc["typed"]), spp=sc["spp"], seed=sc["hseed"],
                materials=(sc["table"], sc["sid"], sc["pid"]), light_radius=sc["radius"], shadow_samples=sc["n"], lens=sc["lens"])


def oracle_frame(orc, sc, **kw):
    """The oracle's uint8 and float32 frames (columns [x0, x1) of kw, the rest zero)."""
    ref = orc.render(sc["w"], sc["h"], sc["cam_origin"], sc["cam_rot"], sc["spheres"], sc["lights"], sc["planes"], 0.0, 0.0, 0.0,
                     sc["depth"], sc["aa"], want=("u8", "f32"), **{**oracle_kwargs(sc), **kw})
    return ref["u8"], ref["f32"]


def gpu_frame(r, sc, **kw):
    """The library's frames for the scene on Renderer r (scene, camera, lens and grid set here)."""
    r.set_scene(sc["spheres"], sc["lights"], sc["planes"], flags=int(sc["typed"]), materials=(sc["table"], sc["sid"], sc["pid"]),
                light_radius=sc["radius"], shadow_samples=sc["n"])
    r.set_camera(sc["cam_origin"], sc["cam_rot"])
    r.set_lens(*sc["lens"])
    r.set_raygen(sc["w"], sc["h"], *sc["raygen"])
    return r.render(7.0, -3.0, 2.0, sc["depth"], sc["aa"], u8=True, f32=True, flags=sc["flags_aa"], spp=sc["spp"], seed=sc["hseed"],
                    **kw)


def live(orc, sc, u8=None):
    """{feature: pixels of the uint8 frame that change when it is turned off} for the oracle's frame of the scene."""
    if u8 is None:
        u8 = oracle_frame(orc, sc)[0]
    out = {}
    for what in ("materials", "glass", "rough", "soft", "lens"):
        o8 = oracle_frame(orc, strip(sc, what))[0]
        out[what] = int((o8 != u8).any(axis=0).sum())
    return out


def bench_sky(way="full"):
    """The packed sky (rt_set_scene_sky, 24 float64) of tools/sky_bench.py: "full", a blue gradient with a low sun and its halo
    in front of the camera, or "unreachable", a black gradient and halo whose sun no ray can see (sun_cos = 2), which makes a scene
    run the sky kernels and leaves its bytes alone."""
    from python_ray_tracer_amd.scene import Sky
    k = Sky(zenith=(25, 70, 190), horizon=(190, 215, 240), nadir=(70, 65, 60), sharpness=2, sun_direction=(1.0, 0.25, 0.12),
            sun_angle_deg=2.5, sun_color=(255, 240, 200), halo_color=(130, 100, 50), halo_shininess=64).pack()
    if way == "unreachable":
        k[3:12] = 0.0
        k[20:23] = 0.0
        k[16] = 2.0
    return k
