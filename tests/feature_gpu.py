"""What the GPU feature tests share (test_gpu_materials, _refraction, _scatter, _soft_shadows, _lens, _textures, _lighting, _sky
and the oracle modules beside them): the fixture comparison, the walk through every entry point, the environment tables that
reach every kernel of a family with the loop over them, the bodies of the traversal and column-slab tests, the example runner and
the scenes and comparisons that more than one module uses.  A plain helper module like film_stub.py: nothing here is collected.
tests/test_feature_gpu_harness.py checks on the CPU that check() and walk_entry_points() still bite."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_frame, raygen_closed_form

sys.path.insert(0, os.path.join(REPO, "tools"))
import feature_scenes as fs  # noqa: E402

IGNORED = dict(amb=7.0, lamb=-3.0, refl=2.0)   # rt_params shading scalars: a material scene must not read them
BIG = ("c4_s64_d5_sub32", "c5_s256_d8_sub96")
AA_PER_PIXEL = 32                              # RT_FLAG_AA_PER_PIXEL
MODES = ((0, 0, 0), (1, 0, 0), (1, AA_PER_PIXEL, 0), (2, 0, 2))     # (aa, flags, spp): plain, the lattice, per-pixel AA, stochastic
KERNEL_LINE = re.compile(r"mi355rt: render_kernel<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), \(rt::Family\)(\d+)>")
TEX_FAMILIES = {"scatter": 7, "area_lights": 8, "lens": 9, "both": 10}      # rt::Family numbers of the texture kernels
LIT_FAMILIES = {"scatter": 11, "area_lights": 12, "lens": 13, "both": 14}   # and of their lighting twins


@pytest.fixture
def rend(renderer):
    """The session's renderer, with the pinhole camera restored afterwards (later tests share it)."""
    yield renderer
    renderer.set_lens(0.0, 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# A fixture (tests/golden/<feature>_<case>.npz: the scene, sampled coordinates and the reference's pixels there) and a frame

def grid(w, h, rg):
    """The closed-form pixel grid as an explicit array (3, w, h)."""
    px, y0, dy, z0, dz = rg
    out = np.empty((3, w, h))
    out[0] = px
    out[1] = (np.arange(w) * dy + y0)[:, None]
    out[2] = (np.arange(h) * dz + z0)[None, :]
    return out


def kw(g):
    return dict(spp=int(g["spp"]) if "spp" in g else 0, seed=int(g["seed"]) if "seed" in g else 1)


def pick(g, a, x0=0):
    """The fixture's sampled pixels (n, 3) of a frame (3, w, h) whose first column is x0."""
    co = g["coords"]
    return a[:, co[:, 0] - x0, co[:, 1]].T


def check(g, u8, f32=None, what="", x0=0, key="u8"):
    """uint8 equal to g[key] and float32 bit for bit (the sign of zero included) equal to g["rgb64"], at the fixture's coordinates."""
    got = pick(g, u8, x0)
    bad = (got != g[key]).any(axis=1)
    assert not bad.any(), (f"{what}: uint8 differs at {bad.sum()} of {len(bad)} pixels, e.g. {g['coords'][bad][:4].tolist()}: "
                           f"{got[bad][:4].tolist()} != {g[key][bad][:4].tolist()}")
    if f32 is not None:
        a, e = pick(g, f32, x0), g["rgb64"].astype(np.float32)
        bad = (a.view(np.uint32) != e.view(np.uint32)).any(axis=1)
        assert not bad.any(), (f"{what}: float32 differs at {bad.sum()} of {len(bad)} pixels, e.g. {g['coords'][bad][:4].tolist()}: "
                               f"{a[bad][:4].tolist()} != {e[bad][:4].tolist()}")


def render_host(r, g, flags=0, aa=None, **over):
    return r.render(*IGNORED.values(), int(g["depth"]), int(g["aa"]) if aa is None else aa, u8=True, f32=True, flags=flags,
                    **{**kw(g), **over})


def set_view(r, g, scene, lens=None, explicit=False):
    """scene(r, g) sets the module's scene; then the fixture's camera, the lens where one is given and the closed-form grid, or
    the same grid as an explicit array."""
    w, h = int(g["w"]), int(g["h"])
    scene(r, g)
    r.set_camera(g["cam_origin"], g["cam_rot"])
    if lens is not None:
        r.set_lens(*lens)
    rg = raygen_closed_form(w, h, float(g["fov"]))
    if explicit:
        r.set_pixel_loc(grid(w, h, rg))
    else:
        r.set_raygen(w, h, *rg)
    return w, h


def fixture_lens(g):
    return float(g["aperture"]), float(g["focus_distance"])


def _d2h(r, shape, d8, d32):
    got = np.empty(shape, np.uint8)
    r.d2h(got, d8)
    g32 = None
    if d32 is not None:
        g32 = np.empty(shape, np.float32)
        r.d2h(g32, d32)
    return got, g32


def walk_entry_points(r, g, setup, big, *, cameras, begin_end, explicit):
    """The fixture g through rt_render, rt_render_device and rt_render_sequence (3 frames in launches of 2; with a camera per
    frame too where `cameras`), rt_render_begin / rt_render_end (where `begin_end`, small fixtures), an explicit pixel grid
    (where `explicit`; stochastic needs the closed-form grid) and RT_FLAG_AA_PER_PIXEL (aa 1).  setup(r, g, explicit=False)
    sets the scene and the view and returns (w, h).  Large fixtures (`big`) get no float32 device buffer."""
    w, h = setup(r, g)
    u8, f32 = render_host(r, g)
    check(g, u8, f32, "rt_render")
    aa = int(g["aa"])
    p = r.params(*IGNORED.values(), int(g["depth"]), aa, **kw(g))
    n, npx = 3, w * h
    d8 = r.malloc(n * 3 * npx)
    d32 = None if big else r.malloc(n * 12 * npx)
    try:
        r.render_device(p, 0, w, d8, d32, npx)
        r.sync()
        check(g, *_d2h(r, (3, w, h), d8, d32), "rt_render_device")
        every = np.tile(np.concatenate([g["cam_origin"], g["cam_rot"].reshape(9)]), (n, 1))
        for cams in (None, every) if cameras else (None,):
            r.h2d(d8, np.zeros(n * 3 * npx, np.uint8))
            r.render_sequence(p, 0, w, n, d8, d32, npx, 3 * npx, cams, None, 2)   # (cameras=None: launches of 2 frames)
            r.sync()
            seq, s32 = _d2h(r, (n, 3, w, h), d8, d32)
            for i in range(n):
                check(g, seq[i], None if s32 is None else s32[i], f"rt_render_sequence cameras={cams is not None} frame {i}")
    finally:
        r.free(d8)
        if d32 is not None:
            r.free(d32)
    if begin_end and not big:
        o8, o32 = np.empty((3, w, h), np.uint8), np.empty((3, w, h), np.float32)
        r.render_begin(0, *IGNORED.values(), int(g["depth"]), aa, o8, o32, **kw(g))
        r.render_end(0)
        check(g, o8, o32, "rt_render_begin/end")
    if explicit and aa != 2:
        setup(r, g, explicit=True)
        u8, f32 = render_host(r, g)
        check(g, u8, f32, "explicit pixel_loc")
    if aa == 1:                                                 # the per-pixel 9-tap kernel on the closed-form grid
        setup(r, g)
        u8, f32 = render_host(r, g, flags=AA_PER_PIXEL)
        check(g, u8, f32, "RT_FLAG_AA_PER_PIXEL")


def large_fixtures_on_a_traversal(monkeypatch, lanes_mins, records, load, setup):
    """The 64- and 256-sphere fixtures (clustered scenes) on the lane-owned (MI355RT_LANES_MINS=30) and the wave-uniform
    (=100000) kernels, with and without float64 sphere records in LDS (MI355RT_F32_RECORDS)."""
    import python_ray_tracer_amd as pkg
    monkeypatch.setenv("MI355RT_LANES_MINS", lanes_mins)
    monkeypatch.setenv("MI355RT_F32_RECORDS", records)
    r = pkg.Renderer(0)
    try:
        for case in BIG:
            g = load(case)
            setup(r, g)
            u8, f32 = render_host(r, g)
            check(g, u8, f32, f"{case} LANES_MINS={lanes_mins} F32_RECORDS={records}")
    finally:
        r.close()


def column_slabs_are_the_full_frame(r, g, setup, aa, spp, slabs):
    """X is the absolute column: a slab [x0, x1) is the same columns of the whole frame."""
    setup(r, g)
    full8, full32 = render_host(r, g, aa=aa, spp=spp)
    for x0, x1 in slabs:
        u8, f32 = render_host(r, g, aa=aa, spp=spp, x0=x0, x1=x1)
        assert np.array_equal(u8, full8[:, x0:x1]) and np.array_equal(f32, full32[:, x0:x1]), (x0, x1)


def run_example(out, size, depth, frames, *flags):
    """examples/render_png.py in a process of its own: what it printed and the picture it wrote."""
    from PIL import Image
    log = subprocess.check_output([sys.executable, os.path.join(REPO, "examples", "render_png.py"), "--size", size, "--depth", str(depth),
                                   "--frames", str(frames), "--out", out, *flags], text=True)
    assert "wrote" in log
    return log, np.asarray(Image.open(out))


# ---------------------------------------------------------------------------------------------------------------------
# Every kernel of a family.  The dispatcher's choice follows the scene (flat or clustered, sphere count, LDS image) and the
# overrides read at rt_create; between them these (scene, environment) pairs launch every instantiation it can pick (rt_device.h:
# all 22 MAT kernels, 14 of each later family; the parked wave-uniform variants of those need 13 to 19 per-thread slots, over the
# parking budget for any scene).  ENVS lists the pairs one by one, VARIANTS the same pairs by scene; a same-bytes test renders
# one scene of VARIANTS in the four MODES under each of its environments and wants the same bytes every time.
ENVS = [
    ("c5_s256_d8_sub96", {}),                                                 # lane-owned, parked (MODE 2 / 3)
    ("c5_s256_d8_sub96", {"MI355RT_LANES_PARK": "0"}),                        # lane-owned, registers
    ("c4_s64_d5_sub32", {"MI355RT_LANES_MINS": "100000"}),                    # wave-uniform clusters, 4 waves, parked (MODE 1)
    ("c4_s64_d5_sub32", {"MI355RT_LANES_MINS": "100000", "MI355RT_F32_RECORDS": "0"}),   # ... MODE 0
    ("c5_s256_d8_sub96", {"MI355RT_LANES_MINS": "100000"}),                   # 4 waves, registers (MODE 1)
    ("c5_s256_d8_sub96", {"MI355RT_LANES_MINS": "100000", "MI355RT_F32_RECORDS": "0"}),  # ... MODE 0
    ("aa_48_d2", {}),                                                         # flat, 2 waves, parked (AA: registers)
    ("tiny", {}),                                                             # one sphere, one light: 2 waves, parked AA too
    ("aa_48_d2", {"MI355RT_WPW2_MAX_IMAGE": "0"}),                            # flat, 4 waves, parked (MODE 0)
    ("c4_s64_d5_sub32", {"MI355RT_LANES_MINS": "30"}),                        # lane-owned on a small image: parked (MODE 2 / 3)
    ("c4_s64_d5_sub32", {"MI355RT_LANES_MINS": "100000", "MI355RT_CLUSTER_MINS": "100000",
                         "MI355RT_WPW2_MAX_IMAGE": "0"}),                     # flat 64 spheres, 4 waves (MODE 1 where it saves LDS)
    ("c5_s256_d8_sub96", {"MI355RT_LANES_MINS": "100000", "MI355RT_CLUSTER_MINS": "100000",
                          "MI355RT_WPW2_MAX_IMAGE": "10000000"}),             # flat 256 spheres, 2 waves, registers
]
ENVS_KEYS = sorted({k for _, e in ENVS for k in e})
ENVS_IDS = [f"{c}-{'-'.join(f'{k[8:]}={v}' for k, v in e.items()) or 'default'}" for c, e in ENVS]
VARIANTS = {
    "c5_s256_d8_sub96": [{}, {"MI355RT_LANES_PARK": "0"}, {"MI355RT_LANES_MINS": "100000"},
                         {"MI355RT_LANES_MINS": "100000", "MI355RT_F32_RECORDS": "0"},
                         {"MI355RT_LANES_MINS": "100000", "MI355RT_CLUSTER_MINS": "100000", "MI355RT_WPW2_MAX_IMAGE": "10000000"}],
    "c4_s64_d5_sub32": [{"MI355RT_LANES_MINS": "100000"}, {"MI355RT_LANES_MINS": "100000", "MI355RT_F32_RECORDS": "0"},
                        {"MI355RT_LANES_MINS": "30"},
                        {"MI355RT_LANES_MINS": "100000", "MI355RT_CLUSTER_MINS": "100000", "MI355RT_WPW2_MAX_IMAGE": "0"}],
    "aa_48_d2": [{}, {"MI355RT_WPW2_MAX_IMAGE": "0"}],
    "tiny": [{}],
}
ENV_KEYS = sorted({k for vs in VARIANTS.values() for v in vs for k in v})


def variant_source(case, load):
    """The scene of a row of ENVS or VARIANTS: "tiny" (one sphere and one light of aa_48_d2, no plane), a frame_aa_* fixture, or
    the module's own large fixture load(case)."""
    if case == "tiny":
        g = load_frame("aa_48_d2")
        return dict(spheres=g["spheres"][:, :1], lights=g["lights"][:, :1], planes=g["planes"][:, :0], fov=g["fov"],
                    cam_origin=g["cam_origin"], cam_rot=g["cam_rot"])
    return load_frame(case) if case.startswith("aa_") else load(case)


def variant_renderers(monkeypatch, case, extra_env=None):
    """(env, renderer) for each environment of VARIANTS[case]: the table's variables cleared, env (and extra_env) set, a fresh
    Renderer(0) that is closed before the next one opens."""
    import python_ray_tracer_amd as pkg
    for env in VARIANTS[case]:
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in {**env, **(extra_env or {})}.items():
            monkeypatch.setenv(k, v)
        r = pkg.Renderer(0)
        try:
            yield env, r
        finally:
            r.close()


def aim(r, src, w, h):
    r.set_camera(src["cam_origin"], src["cam_rot"])
    r.set_raygen(w, h, *raygen_closed_form(w, h, float(src["fov"])))


def render_modes(r, depth=3, seed=3):
    return [r.render(*IGNORED.values(), depth, aa, u8=True, f32=True, flags=flags, spp=spp, seed=seed) for aa, flags, spp in MODES]


def same_as_first(first, outs, what):
    """The frames of render_modes() are the bytes of the first variant's; returns those (the first time: outs, none of them black)."""
    if first is None:
        assert all(u8.any() for u8, _ in outs), what
        return outs
    for (aa, flags, _), (u8, f32), (r8, r32) in zip(MODES, outs, first):
        assert u8.tobytes() == r8.tobytes(), (what, aa, flags)
        assert f32.tobytes() == r32.tobytes(), (what, aa, flags)
    return first


def logged_kernels(capfd):
    """The kernels that the launches since the last call named on stderr (MI355RT_LOG_KERNELS=1): tuples of seven strings."""
    return KERNEL_LINE.findall(capfd.readouterr().err)


# ---------------------------------------------------------------------------------------------------------------------
# Scenes that more than one module renders on those tables

def lens_materials(S, P):
    """matte, mirror-ish, rough and glass spheres; a satin floor"""
    table = np.array([[0.05, 0.6, 0.5, 0.0, 1.0, 0.0], [0.0, 0.4, 0.8, 0.0, 1.0, 0.3], [0.02, 0.6, 0.2, 0.0, 1.0, 0.0],
                      [0.0, 0.5, 0.4, 0.0, 1.0, 0.1], [0.0, 0.1, 0.0, 0.9, 1.5, 0.0]])
    sid = np.array([(1 + (i // 3) % 2) if i % 3 == 0 else (4 if i % 5 == 0 else 0) for i in range(S)], np.int32)
    return table, sid, np.full(P, 3, np.int32)


def glossy(table):
    """The 6-column table with spec and shin columns: every row glossy, the exponents 1 .. 1024 in turn."""
    t = np.zeros((len(table), 8))
    t[:, :6] = table
    t[:, 6] = [40.0 + 30.0 * (i % 4) for i in range(len(table))]
    t[:, 7] = [float(1 << ((3 * i + 1) % 11)) for i in range(len(table))]
    return t


def scene_textures(src):
    """A checkered floor on every plane, a solid checker on every third sphere and a projected image on the ones after them."""
    from python_ray_tracer_amd.scene import Texture
    S, P = src["spheres"].shape[1], src["planes"].shape[1]
    rng = np.random.default_rng(S)
    img = Texture.image(rng.integers(0, 256, (7, 5, 3)), (0.0, -0.3, 0.8), (0.0, 0.9, 0.1), (0.1, 0.0, -0.7))
    tex = [Texture.checker((240, 240, 240), (20, 20, 20), 0.35), Texture.checker((250, 120, 10), (10, 150, 160), 0.12, solid=True), img]
    recs, first = [], 0
    for t in tex:
        recs.append((t.origin, t.axes, t.dims, first))
        first += t.texels.shape[0] * t.texels.shape[1] * t.texels.shape[2]
    st = np.array([1 if i % 3 == 0 else (2 if i % 3 == 1 and i % 2 else -1) for i in range(S)], np.int32)
    return recs, st, np.zeros(P, np.int32), np.concatenate([t.texels.reshape(-1, 3) for t in tex])


def lit_scene(src, case):
    """The lighting and sky tables' scene: (lens_materials, the same with glossy rows, scene_textures but for "tiny", a colour
    per light)."""
    table, sid, pid = lens_materials(src["spheres"].shape[1], src["planes"].shape[1])
    rgb = np.array([[1.0, 0.7, 0.4], [0.3, 0.5, 1.5], [0.0, 0.3, 0.2]][:src["lights"].shape[1]], np.float32)
    return (table, sid, pid), (glossy(table), sid, pid), scene_textures(src) if case != "tiny" else None, rgb


def frames(r, g):
    return [render_host(r, g, aa=aa, spp=spp) for aa, spp in ((0, 0), (1, 0), (2, 2))]


def same_frames(a, b, what):
    for i, ((u8, f32), (r8, r32)) in enumerate(zip(a, b)):
        assert u8.tobytes() == r8.tobytes() and f32.tobytes() == r32.tobytes(), (what, i)


# ---------------------------------------------------------------------------------------------------------------------
# Frames against the CPU oracle (oracle/rt_oracle.c): uint8 and float32, bit for bit

def same(what, u8, f32, r8, r32):
    bad8 = (u8 != r8).any(axis=0)
    assert not bad8.any(), f"{what}: {int(bad8.sum())} of {bad8.size} pixels differ (uint8), e.g. {np.argwhere(bad8)[:4].tolist()}"
    bad = (f32.view(np.uint32) != r32.view(np.uint32)).any(axis=0)
    assert not bad.any(), f"{what}: float32 differs at {int(bad.sum())} pixels, e.g. {np.argwhere(bad)[:4].tolist()}"


def same_pixels(what, co, u8, f32, r8, r64, x0=0):
    """Sampled pixels co (n,2) of frames (3,w,h) against orc.render_pixels' (n,3) outputs."""
    g8 = u8[:, co[:, 0] - x0, co[:, 1]].T
    g32 = f32[:, co[:, 0] - x0, co[:, 1]].T
    e32 = r64.astype(np.float32)
    bad = (g8 != r8).any(axis=1) | (g32.view(np.uint32) != e32.view(np.uint32)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(co)} pixels differ, e.g. {co[bad][:4].tolist()}"


def kernel_table_refs(oracle, src, w, h, modes, feature, *, materials, radius, lens, depth=3, seed=3, textures=None, light_rgb=None,
                      sky=None):
    """[(uint8, float32)] per (aa, flags, spp) of `modes`: the oracle's frames of the scene the kernel tables render, after
    asserting that `feature` ("textures", "lighting" or "sky") changes at least 20 pixels of the first."""
    sc = dict(kind="table", w=w, h=h, spheres=src["spheres"], lights=src["lights"], planes=src["planes"], table=materials[0],
              sid=materials[1], pid=materials[2], radius=radius, n=2, lens=lens, cam_origin=np.asarray(src["cam_origin"], np.float64),
              cam_rot=np.asarray(src["cam_rot"], np.float64), raygen=raygen_closed_form(w, h, float(src["fov"])), depth=depth, aa=0,
              flags_aa=0, spp=1, hseed=seed, typed=0, textures=textures, light_rgb=light_rgb, sky=sky)
    refs = [fs.oracle_frame(oracle, {**sc, "aa": aa, "spp": max(spp, 1)}) for aa, _, spp in modes]
    off = fs.oracle_frame(oracle, fs.strip(sc, feature))[0]
    n_live = int((off != refs[0][0]).any(axis=0).sum())
    assert n_live >= 20, f"{feature} changes only {n_live} pixels of the oracle's frame"
    return refs


def family_kernels_same_bytes(monkeypatch, capfd, oracle, kind, families, load, size, feature, scenes, twins=None):
    """The body of test_every_{texture,lighting,sky}_kernel_same_bytes.  VARIANTS x MODES reaches all 14 shapes of the family
    families[kind] ("scatter", "area_lights", "lens" or "both"); MI355RT_LOG_KERNELS makes every launch name its
    kernel on stderr, which is how this knows.  scenes(src, case) gives the set_scene keywords (materials, textures, light_rgb,
    sky) of the scene without `feature` and with it.  Every variant renders the oracle's frames and the first variant's bytes,
    with a kernel of the family; the scene without the feature renders other bytes (with a kernel of twins[kind], where given)."""
    radii, lens = kind in ("area_lights", "both"), (0.08 if kind in ("lens", "both") else 0.0, 3.0)
    w, h = size
    seen = set()
    for case in VARIANTS:
        src = variant_source(case, load)
        NL = src["lights"].shape[1]
        radius = np.array([0.5, 0.0, 0.3][:NL], np.float32) if radii else np.zeros(NL, np.float32)
        without, full = scenes(src, case)
        refs = kernel_table_refs(oracle, src, w, h, MODES, feature, materials=full["materials"], radius=radius, lens=lens,
                                 textures=full.get("textures"), light_rgb=full.get("light_rgb"), sky=full.get("sky"))
        first = None
        for env, r in variant_renderers(monkeypatch, case, {"MI355RT_LOG_KERNELS": "1"}):
            aim(r, src, w, h)
            r.set_lens(*lens)
            if first is None:
                r.set_scene(src["spheres"], src["lights"], src["planes"], light_radius=radius, shadow_samples=2, **without)
                plain = r.render(*IGNORED.values(), 3, 0, u8=True, seed=3)[0]
                names = logged_kernels(capfd)
                assert twins is None or (names and all(int(n[6]) == twins[kind] for n in names)), (case, env, names)
            r.set_scene(src["spheres"], src["lights"], src["planes"], light_radius=radius, shadow_samples=2, **full)
            outs = render_modes(r)
            names = logged_kernels(capfd)
            assert names and all(int(n[6]) == families[kind] for n in names), (case, env, names)
            seen.update(names)
            for (aa, flags, _), (u8, f32), (r8, r32) in zip(MODES, outs, refs):     # every kernel against the CPU oracle
                same(f"{kind} {case} {env} aa={aa} flags={flags}", u8, f32, r8, r32)
            assert first is not None or not np.array_equal(outs[0][0], plain), case      # (the feature shows)
            first = same_as_first(first, outs, (case, env))
    print(f"{kind}: {len(seen)} kernels: {sorted(seen)}")
    assert len(seen) == 14, f"{kind}: {len(seen)} of the family's 14 kernels ran: {sorted(seen)}"


# The scenes of ENVS with a seeded random table per family, and the oracle's frames of them in the four MODES
FAMILIES = ("mat", "refr", "scat", "soft", "lens_scat", "lens_soft")
_W, _H, _DEPTH, _SEED = 160, 96, 3, 5
_FEATURE_OF = dict(mat="materials", refr="glass", scat="rough", soft="soft", lens_scat="lens", lens_soft="lens")
_ORACLE = {}


def family_scene(family, case):
    """The scene of `case` with a random table for `family` (seeded by both): ids over every row, ids above 7 included.  For
    scatter, "tiny" gets the floor of aa_48_d2: a lone convex sphere never sees its own reflections, so a rough one renders
    the bytes of a mirror."""
    src = dict(variant_source(case, lambda c: np.load(os.path.join(GOLDEN, f"lens_{c}.npz"))))
    if case == "tiny" and family == "scat":
        src["planes"] = load_frame("aa_48_d2")["planes"][:, :1]
    S, P, NL = src["spheres"].shape[1], src["planes"].shape[1], src["lights"].shape[1]
    rng = np.random.default_rng(FAMILIES.index(family) * 101 + len(case))
    M = 12 if family == "mat" else 5               # (5 rows of 5 or 6 columns leave the LDS room for the parked variants)
    table = np.zeros((M, 6))
    table[:, 0] = rng.uniform(-0.05, 0.12, M)
    table[:, 1] = rng.uniform(0.2, 0.9, M)
    table[:, 2] = rng.uniform(0.0, 0.9, M)
    table[:, 4] = 1.0
    if family != "mat":                            # glass rows 1 and 4 (ior 1.5 and 0.8), rough rows 2 and 3
        table[1::3, 2], table[1::3, 3], table[1::3, 4] = 0.0, rng.uniform(0.5, 1.0, 2), (1.5, 0.8)
    if family not in ("mat", "refr"):
        table[2:4, 5] = (0.3, 1.0)
    ncols = 3 if family == "mat" else (5 if family == "refr" else 6)
    table = table[:, :ncols]
    sid = rng.integers(0, M, S).astype(np.int32)
    first = [1, 2, 9, 11] if family == "mat" else ([2, 1, 3, 4] if family == "scat" else [1, 2, 3, 4])
    sid[: min(S, 4)] = first[: min(S, 4)]          # (the one sphere of "tiny")
    pid = rng.integers(0, M, P).astype(np.int32)
    radius = np.zeros(NL, np.float32)
    if family in ("soft", "lens_soft"):
        radius[:] = np.array([0.5, 0.0, 0.3] * NL, np.float32)[:NL]
        radius[0] = 0.5
    lens = (0.08, 3.0) if family.startswith("lens") else (0.0, 1.0)
    return dict(kind=family, w=_W, h=_H, spheres=src["spheres"], lights=src["lights"], planes=src["planes"], table=table, sid=sid,
                pid=pid, radius=radius, n=2, lens=lens, cam_origin=np.asarray(src["cam_origin"], np.float64),
                cam_rot=np.asarray(src["cam_rot"], np.float64), fov=float(src["fov"]),
                raygen=raygen_closed_form(_W, _H, float(src["fov"])), depth=_DEPTH, aa=0, flags_aa=0, spp=1, hseed=_SEED, typed=0)


def oracle_modes(oracle, family, case):
    """(the oracle's frames of family_scene in the four MODES, the pixels its feature changes in the first), computed once."""
    key = (family, case)
    if key not in _ORACLE:
        sc = family_scene(family, case)
        outs = [fs.oracle_frame(oracle, {**sc, "aa": aa, "spp": max(spp, 1)}) for aa, _, spp in MODES]
        off = fs.oracle_frame(oracle, fs.strip(sc, _FEATURE_OF[family]))[0]
        _ORACLE[key] = (outs, int((off != outs[0][0]).any(axis=0).sum()))
    return _ORACLE[key]
