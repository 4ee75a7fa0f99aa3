"""TEST INFRASTRUCTURE ONLY — seeded random scenes with every feature of include/mi355rt.h (per-object materials, glass,
rough surfaces, area lights, a thin lens; with draw_lit also textures, coloured lights, highlights and a sky), for
tests/test_gpu_features_vs_oracle.py, tests/test_gpu_lit_vs_oracle.py and the soak tools/fuzz_features.py.

draw(seed) returns one scene as a dict; every key of it is plain data (numpy arrays and numbers).  Scenes are biased toward
what the feature paths get wrong: cameras, lights and lens points inside glass spheres, touching and nested spheres, total
internal reflection and grazing absorption, glass windows (transparent planes), negative ambient, refl = 1 at depth 16 and
scales from 1e-3 to 1e3.

draw_lit(seed) is draw(seed) with non-uniform textures, coloured lights, spec / shin columns and a sky added from a random
stream of its own (draw(seed) itself never changes: the seed lists of the tests depend on it).

oracle_kwargs(sc) / oracle_frame(orc, sc) give the CPU oracle's arguments and frame; strip(sc, what) the same scene with one
feature turned off ("materials", "glass", "rough", "soft", "lens", "textures", "lighting", "sky"), for the tests' liveness checks."""
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


SHININESS = tuple(float(1 << i) for i in range(11))
SHARPNESS = (1.0, 2.0, 4.0, 8.0, 16.0)
LIT = ("textures", "lighting", "sky")


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def draw_lit(seed, w=None, h=None, kind=None):
    """draw(seed, w, h, kind) plus, from a random stream of its own:
      textures   1 to 4 records of random dimensions along up to three axes (non-uniform texels), skewed axes, texel ranges
                 that overlap, most objects textured and some left at -1;
      light_rgb  a colour times strength per light, zeros and values above 1 among them;
      table      8 columns: spec 0 on some rows, shin through all eleven exponents over the seeds, and now and then lamb <= 0
                 on the matte row with spec > 0;
      sky        random unit up and sun_dir, every sharp over the seeds, the sun near the camera's forward axis so that some ray
                 sees its disc."""
    sc = draw(seed, w, h, kind)
    rng = np.random.default_rng([int(seed), 0x11D])
    S, P, NL = sc["spheres"].shape[1], sc["planes"].shape[1], sc["lights"].shape[1]
    scale = float(sc["spheres"][3].mean()) / 0.7
    # textures
    T = int(rng.integers(1, 5))
    recs, need = [], 0
    for k in range(T):
        dims = [int(rng.choice([2, 3, 5, 8])) if a < int(rng.integers(1, 4)) else 1 for a in range(3)]
        rng.shuffle(dims)
        recs.append([rng.uniform(-2, 2, 3) * scale, rng.normal(size=(3, 3)) * float(rng.choice([0.3, 2.0, 40.0])) / scale, tuple(dims), 0])
        need = max(need, dims[0] * dims[1] * dims[2])
    N = need + int(rng.integers(0, 24))
    for r in recs:                                                 # shared texels: every range somewhere inside one short array
        r[3] = int(rng.integers(0, N - r[2][0] * r[2][1] * r[2][2] + 1))
    texels = rng.integers(0, 256, (N, 3)).astype(np.float32)
    st = np.where(rng.uniform(size=S) < 0.7, rng.integers(0, T, S), -1).astype(np.int32)
    pt = np.where(rng.uniform(size=P) < 0.85, rng.integers(0, T, P), -1).astype(np.int32)
    st[0] = int(rng.integers(0, T))
    if S > 1:
        st[1] = -1
    # lighting
    rgb = (rng.uniform(0.0, 2.5, (NL, 3)) * (rng.uniform(size=(NL, 3)) < 0.8)).astype(np.float32)
    rgb[0] = np.maximum(rgb[0], np.float32(0.4))                   # (the first light, the one with a radius, stays on)
    if NL > 2 and rng.uniform() < 0.5:
        rgb[NL - 1] = 0.0                                          # a black light among the coloured ones
    t6 = np.asarray(sc["table"], np.float64)
    table = np.zeros((len(t6), 8))
    table[:, :6] = t6
    table[:, 6] = rng.uniform(20.0, 300.0, len(t6)) * (rng.uniform(size=len(t6)) < 0.75)
    table[:, 7] = [SHININESS[(int(seed) + 3 * i) % 11] for i in range(len(t6))]
    table[0, 6] = float(rng.uniform(40.0, 200.0))
    if rng.uniform() < 0.3:
        table[0, 1] = float(rng.choice([0.0, -0.2]))               # lamb <= 0 with spec > 0
    # the sky: the sun close to where the camera looks
    fwd = np.asarray(sc["cam_rot"], np.float64)[:, 0]
    sun = _unit(_unit(fwd) + rng.normal(size=3) * 0.25)
    sky = np.zeros(24)
    sky[0:3] = _unit(rng.normal(size=3) + np.array([0.0, 0.0, 1.5]))
    sky[3:12] = rng.uniform(0.0, 255.0, 9)
    sky[12] = SHARPNESS[int(seed) % 5]
    sky[13:16] = sun
    sky[16] = float(np.cos(np.radians(rng.uniform(3.0, 25.0))))
    sky[17:20] = rng.uniform(50.0, 300.0, 3)
    sky[20:23] = rng.uniform(0.0, 150.0, 3)
    sky[23] = SHININESS[int(rng.integers(0, 11))]
    sc.update(table=table, textures=([tuple(r) for r in recs], st, pt, texels), light_rgb=rgb, sky=sky)
    return sc


def strip(sc, what):
    """The same scene with one feature off: 'glass' (trans 0), 'rough' (rough 0), 'soft' (radii 0), 'lens' (aperture 0),
    'materials' (one table row for every object), 'textures' (none), 'lighting' (white lights and spec 0), 'sky' (none)."""
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
    elif what == "textures":
        sc["textures"] = None
    elif what == "lighting":
        sc["light_rgb"] = None
        if t.shape[1] == 8:
            t[:, 6] = 0.0
    elif what == "sky":
        sc["sky"] = None
    sc["table"] = t
    return sc


def _lit_kwargs(sc):
    """The textures=, light_rgb= and sky= keywords of a draw_lit scene; none for a scene of draw(), whose calls stay as they were."""
    return {k: sc[k] for k in ("textures", "light_rgb", "sky") if sc.get(k) is not None}


def oracle_kwargs(sc):
    return dict(raygen=sc["raygen"], flags=int(sc["typed"]), spp=sc["spp"], seed=sc["hseed"],
                materials=(sc["table"], sc["sid"], sc["pid"]), light_radius=sc["radius"], shadow_samples=sc["n"], lens=sc["lens"],
                **_lit_kwargs(sc))


def oracle_frame(orc, sc, **kw):
    """The oracle's uint8 and float32 frames (columns [x0, x1) of kw, the rest zero)."""
    ref = orc.render(sc["w"], sc["h"], sc["cam_origin"], sc["cam_rot"], sc["spheres"], sc["lights"], sc["planes"], 0.0, 0.0, 0.0,
                     sc["depth"], sc["aa"], want=("u8", "f32"), **{**oracle_kwargs(sc), **kw})
    return ref["u8"], ref["f32"]


def oracle_pixels(orc, sc, coords, **kw):
    """The oracle's (u8 (n,3) in stored order, f64 (n,3)) at the sampled pixels coords (n,2) of the scene's frame."""
    return orc.render_pixels(sc["w"], sc["h"], coords, sc["cam_origin"], sc["cam_rot"], sc["spheres"], sc["lights"], sc["planes"],
                             0.0, 0.0, 0.0, sc["depth"], sc["aa"], **{**oracle_kwargs(sc), **kw})


def gpu_frame(r, sc, **kw):
    """The library's frames for the scene on Renderer r (scene, camera, lens and grid set here)."""
    r.set_scene(sc["spheres"], sc["lights"], sc["planes"], flags=int(sc["typed"]), materials=(sc["table"], sc["sid"], sc["pid"]),
                light_radius=sc["radius"], shadow_samples=sc["n"], **_lit_kwargs(sc))
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
    for what in ("materials", "glass", "rough", "soft", "lens") + tuple(k for k in LIT if sc.get("textures" if k == "textures" else
                                                                                                 ("light_rgb" if k == "lighting" else "sky")) is not None):
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
