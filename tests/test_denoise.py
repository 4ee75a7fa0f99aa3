"""The denoiser on the CPU (rt_render_guides, rt_film_denoise): the header, the binding and the exported symbols; properties of the
numpy restatement denoise_reference on constructed inputs; guides_reference against the CPU oracle's leaf functions, pixel by pixel
and bit for bit, on stored scenes; the arithmetic of python-ray-tracer_amd/csrc/rt_denoise.h, the text the denoise kernel compiles,
run by tests/algo/denoise_check.cpp under AddressSanitizer and UBSan and compared bit for bit with denoise_reference; the wrappers'
ValueErrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_frame, raygen_closed_form
from film_stub import NoDevice
from test_film import same_bits

from python_ray_tracer_amd import Film, denoise as D, film as F
from python_ray_tracer_amd import _lib as L

ALGO = os.path.join(REPO, "tests", "algo")


# ---------------------------------------------------------------------------------------------------------------------
# The scenes whose guides are checked (here against the oracle's leaves, in test_gpu_denoise.py against the kernel): 8 spheres, 64
# clustered and 256 spheres reach every table layout of the guides kernel; a frame without spheres, one without planes (misses),
# one from inside a sphere, one with textures

def _records(g):
    return [(g["tex_origin"][k], g["tex_axes"][k], g["tex_dims"][k], int(g["tex_first"][k])) for k in range(len(g["tex_first"]))]


def guide_scene(name):
    """(fixture, w, h, textures or None) of a guides case: the big scenes on a 32 x 32 grid of their own."""
    if name in ("c4_s64_d5_sub32", "c5_s256_d8_sub96"):
        return load_frame(name), 32, 32, None
    if name == "texture_default_64_d4":
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        return g, 40, 24, (_records(g), g["sphere_texture"], g["plane_texture"], g["texels"])
    g = load_frame(name)
    return g, int(g["w"]), int(g["h"]), None


GUIDE_SCENES = ("odd_37x29", "planes_only_32", "spheres_only_32", "inside_sphere_32", "c4_s64_d5_sub32", "c5_s256_d8_sub96",
                "texture_default_64_d4")
_GUIDES = {}


def guides_truth(name):
    """guides_reference of a guides case, computed once and read-only."""
    if name not in _GUIDES:
        g, w, h, tex = guide_scene(name)
        a = D.guides_reference(g["spheres"], g["planes"], g["cam_origin"], g["cam_rot"], w, h,
                               raygen=raygen_closed_form(w, h, float(g["fov"])), textures=tex)
        a.setflags(write=False)
        _GUIDES[name] = a
    return _GUIDES[name]


# ---------------------------------------------------------------------------------------------------------------------
# Header, binding, exported symbols

def test_header_binding_and_exported_symbols(tmp_path):
    hdr = open(os.path.join(REPO, "include", "mi355rt.h")).read()
    assert "int rt_render_guides(rt_ctx *ctx, int x0, int x1, void *d_guides, int64_t plane_stride, void *stream);" in hdr
    assert "int rt_film_denoise(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n," in hdr
    assert "#define RT_GUIDE_PLANES 8" in hdr and "#define RT_ABI_VERSION 7" in hdr
    assert L.RT_GUIDE_PLANES == 8 == D.GUIDE_PLANES and L.RT_ABI_VERSION == 7
    gd, dn = L.PROTOTYPES["rt_render_guides"], L.PROTOTYPES["rt_film_denoise"]
    assert gd[0] is C.c_int and len(gd[1]) == 6 and gd[1][4] is C.c_int64
    assert dn[0] is C.c_int and len(dn[1]) == 14 and all(dn[1][i] is C.c_int64 for i in (2, 5, 7, 10, 12))
    assert C.sizeof(L.rt_denoise) == 24
    src = tmp_path / "size.c"
    src.write_text('#include "mi355rt.h"\n#include <stddef.h>\n_Static_assert(sizeof(rt_denoise) == 24, "rt_denoise is 24 bytes");\n'
                   '_Static_assert(offsetof(rt_denoise, sigma) == 8 && offsetof(rt_denoise, demodulate) == 16, "layout");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)])
    lib = L.load()                                               # the cross-compiled library
    assert lib.rt_abi_version() == 7 and hasattr(lib, "rt_render_guides") and hasattr(lib, "rt_film_denoise")
    # header and numpy restatement state the same arithmetic, line for line
    doc = D.denoise_reference.__doc__
    for line in ("m_0[c][p] = s[c][p] / (double)n",
                 "demodulate:  a[c][p] = max((double)albedo_c[p], 1.0);   m_0[c][p] = m_0[c][p] / a[c][p]",
                 "levels == 0 (with or without demodulate):  out[c][p] = s[c][p] / (double)n, and nothing else is evaluated",
                 "for i = 0 .. levels-1:      step = 1 << i;   q_i = sigma / 2^i  (exact)",
                 "id[p] >= 0:  cn = ((nx_p*nx_q) + (ny_p*ny_q)) + (nz_p*nz_q)   (float32 normals widened to double)",
                 "sigma > 0:   e_c = (m_i[c][q] - m_i[c][p]) / q_i;  d2 = (e_0*e_0 + e_1*e_1) + e_2*e_2;  wc = 1.0 / (1.0 + d2)",
                 "w = ((k[dx] * k[dy]) * cn) * wc          k = (1/16, 1/4, 3/8, 1/4, 1/16)  (the B3 spline)",
                 "W = W + w;   A_c = A_c + w * m_i[c][q]",
                 "out[c][p] = demodulate ? m_levels[c][p] * a[c][p] : m_levels[c][p]"):
        assert line in hdr, line
        assert line in doc, line
    for name in ("README.md", "DESIGN.md"):
        text = open(os.path.join(REPO, name)).read()
        assert "rt_render_guides" in text and "rt_film_denoise" in text and "wc = 1.0 / (1.0 + d2)" in text, name


# ---------------------------------------------------------------------------------------------------------------------
# denoise_reference on constructed inputs

def _flat_guides(ws, h, ident=0.0, normal=(0.0, 0.0, 1.0), albedo=(200.0, 100.0, 50.0)):
    g = np.zeros((8, ws, h), np.float32)
    for c in range(3):
        g[c] = normal[c]
        g[4 + c] = albedo[c]
    g[7] = ident
    return g


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5, 6])
def test_no_colour_crosses_an_id_edge(levels):
    """Two regions of ids 0 and 1 with colours 0 and 100, identical normals, sigma 0: the weights are dyadic, so A = 100 W exactly and
    every output is exactly 0.0 or 100.0."""
    ws, h = 23, 19
    g = _flat_guides(ws, h)
    region = (np.add.outer(np.arange(ws) * 2, np.arange(h)) > 30) | (np.arange(ws)[:, None] == 3)
    g[7] = region.astype(np.float32)
    s = np.where(region, 100.0, 0.0)[None].repeat(3, 0) * 5.0
    out = D.denoise_reference(s, 5, g, levels, 32, 0.0, 0)
    assert same_bits(out, np.where(region, 100.0, 0.0)[None].repeat(3, 0))
    # with sky pixels (id -1) as one of the regions
    g[7] = np.where(region, 2.0, -1.0).astype(np.float32)
    g[0:3] = np.where(region, g[0:3], 0.0)
    assert same_bits(D.denoise_reference(s, 5, g, levels, 32, 0.0, 0), np.where(region, 100.0, 0.0)[None].repeat(3, 0))


def test_levels_0_is_the_mean():
    rng = np.random.default_rng(5)
    s = rng.uniform(0.0, 900.0, (3, 7, 5))
    g = _flat_guides(7, 5)
    for dem in (0, 1):
        for sigma in (0.0, 3.0):
            assert same_bits(D.denoise_reference(s, 7, g, 0, 1, sigma, dem), s / np.float64(7))


def test_opposed_normals_do_not_mix():
    ws, h = 9, 11
    g = _flat_guides(ws, h)
    g[2, :, 6:] = -1.0                                           # same id, normals (0,0,1) and (0,0,-1): cn = -1
    s = np.zeros((3, ws, h))
    s[:, :, 6:] = 60.0
    for shin in (1, 32):
        assert same_bits(D.denoise_reference(s, 1, g, 3, shin, 0.0, 0), s)
    g[2, :, 6:] = 0.0
    g[0, :, 6:] = 1.0                                            # perpendicular: cn = 0, !(cn > 0)
    assert same_bits(D.denoise_reference(s, 1, g, 3, 1, 0.0, 0), s)


def test_normal_shininess_narrows_the_filter_on_a_curved_surface():
    """Normals turning along y by 4 degrees per pixel, a colour step half way: shininess 1 blurs the step widely, 1024 keeps it."""
    ws, h = 5, 32
    ang = np.radians(4.0) * np.arange(h)
    g = _flat_guides(ws, h)
    g[0], g[1], g[2] = 0.0, np.sin(ang)[None, :], np.cos(ang)[None, :]
    s = np.zeros((3, ws, h))
    s[:, :, h // 2:] = 100.0
    soft = D.denoise_reference(s, 1, g, 3, 1, 0.0, 0)
    hard = D.denoise_reference(s, 1, g, 3, 1024, 0.0, 0)
    err = lambda a: float(np.abs(a - s).max())
    assert err(soft) > 25.0 and err(hard) < err(soft) / 3 and np.abs(hard - s).sum() < np.abs(soft - s).sum() / 3
    assert (soft >= 0.0).all() and (soft <= 100.0 * (1 + 1e-12)).all()      # (a weighted mean, to rounding)


@pytest.mark.parametrize("ws, h", [(1, 1), (1, 7), (5, 1), (3, 3)])
def test_steps_beyond_the_frame(ws, h):
    """levels 6: from some level on every tap but the centre falls outside; the mean of a constant stays the constant."""
    rng = np.random.default_rng(ws * 10 + h)
    g = _flat_guides(ws, h)
    s = rng.uniform(1.0, 500.0, (3, ws, h))
    out = D.denoise_reference(s, 3, g, 6, 32, 8.0, 1)
    assert out.shape == s.shape and np.isfinite(out).all()
    assert out.min() >= (s / 3).min() * (1 - 1e-12) and out.max() <= (s / 3).max() * (1 + 1e-12)
    if ws * h == 1:                                              # one pixel: (s / n / a) * a, the centre tap alone
        a = np.array([200.0, 100.0, 50.0]).reshape(3, 1, 1)
        w = 0.375 * 0.375
        m = s / np.float64(3) / a
        for _ in range(6):
            m = (0.0 + w * m) / (0.0 + w)
        assert same_bits(out, m * a)
    const = np.full((3, ws, h), 640.0)
    assert np.allclose(D.denoise_reference(const, 4, g, 6, 32, 0.0, 0), 160.0, rtol=1e-15)


# ---------------------------------------------------------------------------------------------------------------------
# guides_reference against the oracle's leaf functions

@pytest.mark.parametrize("name", GUIDE_SCENES)
def test_guides_reference_matches_the_oracle_leaves(oracle, name):
    g, w, h, tex = guide_scene(name)
    got = guides_truth(name)
    assert got.shape == (8, w, h) and got.dtype == np.float32
    px, y0, dy, z0, dz = raygen_closed_form(w, h, float(g["fov"]))
    o, R = [float(v) for v in g["cam_origin"]], np.asarray(g["cam_rot"], np.float64).reshape(3, 3).tolist()
    sp, pl = g["spheres"], g["planes"]
    S = sp.shape[1]
    want = np.zeros((8, w, h), np.float32)
    n_miss = 0
    for x in range(w):
        for y in range(h):
            P = (px, float(x) * dy + y0, float(y) * dz + z0)
            d = oracle.normalize([R[i][0] * P[0] + R[i][1] * P[1] + R[i][2] * P[2] for i in range(3)])
            t, idx, typ = oracle.get_intersection(o, d, sp, pl)
            if typ == 404:
                want[7, x, y] = -1.0
                n_miss += 1
                continue
            Pt = np.array([1.0 * o[i] + t * d[i] for i in range(3)])
            if typ == 0:
                N = oracle.normalize(Pt - sp[0:3, idx].astype(np.float64))
                col, tid, ident = sp[4:7, idx], (int(tex[1][idx]) if tex else -1), idx
            else:
                N = oracle.plane_normal_f32(pl[3:6, idx])
                col, tid, ident = pl[6:9, idx], (int(tex[2][idx]) if tex else -1), S + idx
            if tid >= 0:
                col = np.asarray(tex[3], np.float32).reshape(-1, 3)[int(oracle.texel_index(Pt, *tex[0][tid]))]
            want[0:3, x, y] = np.asarray(N, np.float64).astype(np.float32)
            want[3, x, y] = np.float32(t)
            want[4:7, x, y] = col
            want[7, x, y] = ident
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (name, bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    hit = want[7] >= 0
    assert hit.any() and (n_miss > 0) == (name == "spheres_only_32"), (name, n_miss)
    if tex:                                                      # some texel differs from its object's own colour
        ids = want[7].astype(int)
        own = np.where(ids[None] < S, sp[4:7][:, np.clip(ids, 0, S - 1)], pl[6:9][:, np.clip(ids - S, 0, pl.shape[1] - 1)])
        assert (want[4:7] != own)[:, hit].any()


def test_guides_reference_slab_and_explicit_grid():
    g, w, h, _ = guide_scene("odd_37x29")
    rg = raygen_closed_form(w, h, float(g["fov"]))
    full = guides_truth("odd_37x29")
    slab = D.guides_reference(g["spheres"], g["planes"], g["cam_origin"], g["cam_rot"], w, h, raygen=rg, x0=5, x1=22)
    assert same_bits(slab, np.ascontiguousarray(full[:, 5:22]))
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64), indexing="ij")
    loc = np.stack([np.full((w, h), rg[0]), xs * rg[2] + rg[1], ys * rg[4] + rg[3]])
    assert same_bits(D.guides_reference(g["spheres"], g["planes"], g["cam_origin"], g["cam_rot"], w, h, pixel_loc=loc), full)


# ---------------------------------------------------------------------------------------------------------------------
# rt_denoise.h's arithmetic under the sanitizers against denoise_reference

def denoise_cases():
    """[(sum (3, ws, h), n, guides, levels, normal_shin, sigma, demodulate, pad)]: random finite sums on real guides and on random
    id maps with sky, the tiny frames, every levels value, both parities of the ping-pong."""
    rng = np.random.default_rng(20261018)
    real = guides_truth("odd_37x29")
    cases = []

    def sums(ws, h, n):
        return rng.uniform(0.0, 300.0, (3, ws, h)) * n * (rng.random((3, ws, h)) < 0.9) - rng.uniform(0.0, 5.0, (3, ws, h))

    for levels, shin, sigma, dem, n, pad in ((0, 1, 0.0, 0, 7, 0), (0, 32, 4.0, 1, 1, 3), (1, 32, 0.0, 0, 1, 1), (1, 4, 16.0, 1, 7, 0),
                                             (2, 32, 0.125, 1, 7, 3), (3, 1024, 8.0, 0, 4, 0), (4, 32, 0.125, 1, 4, 5), (5, 2, 0.0, 1, 1, 0),
                                             (6, 1, 64.0, 0, 3, 2)):
        cases.append((sums(37, 29, n), n, real, levels, shin, sigma, dem, pad))
    for ws, h in ((1, 1), (1, 7), (5, 1), (3, 3)):
        gd = np.ascontiguousarray(real[:, 10:10 + ws, 12:12 + h])
        cases.append((sums(ws, h, 2), 2, gd, 6, 32, 8.0, 1, 1))
        cases.append((sums(ws, h, 2), 2, gd, 1, 1, 0.0, 0, 0))
    gd = np.zeros((8, 16, 12), np.float32)                       # random ids with sky, random (unnormalised) normals, dark albedo
    gd[7] = rng.integers(-1, 3, (16, 12))
    gd[0:3] = rng.normal(size=(3, 16, 12))
    gd[4:7] = rng.uniform(0.0, 3.0, (3, 16, 12))
    gd[:, gd[7] < 0] = 0.0
    gd[7][gd[7] == 0] = -1.0
    cases.append((sums(16, 12, 5), 5, gd, 3, 8, 2.0, 1, 0))
    cases.append((sums(16, 12, 5), 5, gd, 2, 1, 0.0, 0, 4))
    return cases


def test_denoise_arithmetic_under_sanitizers_matches_numpy(tmp_path):
    exe, table, got = str(tmp_path / "denoise_check"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ALGO, "denoise_check.cpp")])
    cases = denoise_cases()
    with open(table, "wb") as f:
        f.write(np.array([len(cases)], "<i8").tobytes())
        for s, n, gd, levels, shin, sigma, dem, pad in cases:
            ws, h = s.shape[1:]
            f.write(np.array([ws, h, n, levels, shin, dem, pad], "<i8").tobytes() + np.array([sigma], "<f8").tobytes())
            ps = np.full((3, ws * h + pad), 1e300)
            ps[:, :ws * h] = s.reshape(3, -1)
            pg = np.full((8, ws * h + pad), np.nan, np.float32)
            pg[:, :ws * h] = gd.reshape(8, -1)
            f.write(ps.astype("<f8").tobytes() + pg.astype("<f4").tobytes())
    res = subprocess.run([exe, table, got], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stdout + res.stderr
    assert res.stdout.strip() == f"cases={len(cases)} ok", res.stdout
    raw = np.frombuffer(open(got, "rb").read(), "<f8")
    at = 0
    for i, (s, n, gd, levels, shin, sigma, dem, pad) in enumerate(cases):
        want = D.denoise_reference(s, n, gd, levels, shin, sigma, dem)
        out = raw[at:at + want.size].reshape(want.shape)
        at += want.size
        bad = np.argwhere(out.view(np.uint64) != want.view(np.uint64))
        assert bad.size == 0, (i, levels, shin, sigma, dem, bad[:4], out[tuple(bad[0])], want[tuple(bad[0])])
        if levels and want[0].size > 1:
            assert np.isfinite(want).all() and not np.array_equal(want, s / n)
    assert at == raw.size and len(cases) >= 19


# ---------------------------------------------------------------------------------------------------------------------
# The wrappers' argument checks, before the library sees anything

def test_check_denoise():
    assert D.check_denoise(4, 32, 0.125, True) == (4, 32, 0.125, 1) and D.check_denoise(0, 1, 0, 0) == (0, 1, 0.0, 0)
    nan, inf = float("nan"), float("inf")
    for bad, match in (((-1, 32, 1.0, 1), "levels"), ((7, 32, 1.0, 1), "levels"), ((1.5, 32, 1.0, 1), "levels"), ((4, 0, 1.0, 1), "normal_shin"),
                       ((4, 3, 1.0, 1), "normal_shin"), ((4, 2048, 1.0, 1), "normal_shin"), ((4, 32, -1.0, 1), "sigma"), ((4, 32, nan, 1), "sigma"),
                       ((4, 32, inf, 1), "sigma"), ((4, 32, 1.0, 2), "demodulate"), ((4, 32, 1.0, -1), "demodulate")):
        with pytest.raises(ValueError, match=match):
            D.check_denoise(*bad)
    s, g = np.zeros((3, 4, 4)), np.zeros((8, 4, 4), np.float32)
    for args in ((s, 0, g, 1, 1, 0.0, 0), (s[:2], 1, g, 1, 1, 0.0, 0), (s, 1, g.astype(np.float64), 1, 1, 0.0, 0), (s, 1, g[:, :3], 1, 1, 0.0, 0)):
        with pytest.raises(ValueError):
            D.denoise_reference(*args)


def test_film_denoise_value_errors_and_buffers():
    r = NoDevice()
    with Film(r, 2, 6) as film:
        assert [c[0] for c in r.calls] == ["malloc"]              # the guides and filter buffers come with their first use
        with pytest.raises(ValueError, match="no pass"):
            film.denoise()
        film.accumulate(L.rt_params(), 4)
        with pytest.raises(ValueError, match="denoise\\(\\) first"):
            film.resolve(denoised=True)
        n = len(r.calls)
        for kw, match in ((dict(levels=7), "levels"), (dict(normal_shininess=3), "normal_shin"), (dict(sigma=-1.0), "sigma"),
                          (dict(sigma=float("nan")), "sigma"), (dict(demodulate=2), "demodulate")):
            with pytest.raises(ValueError, match=match):
                film.denoise(**kw)
        assert len(r.calls) == n                                  # nothing reached the library
        film.denoise(levels=1)
        kinds = [c[0] for c in r.calls[n:]]
        assert kinds == ["malloc", "guides", "sync", "malloc", "denoise"]     # guides first; no work buffer for one level
        assert r.calls[n] == ("malloc", 4 * 8 * 16) and r.calls[n + 1][1:] == (2, 6, film.d_guides, 16, None)
        call = r.calls[-1]
        assert call[1:8] == (film.d_sum, 4, 4, 4, film.d_guides, film.d_denoised, None)
        assert call[8] == dict(levels=1, normal_shin=32, sigma=F.DENOISE_SIGMA, demodulate=1, stream=None)
        film.denoise()                                            # defaults: four levels, a work buffer, the guides are cached
        assert [c[0] for c in r.calls[n + 5:]] == ["malloc", "denoise"] and r.calls[-1][7] == film.d_work
        assert r.calls[-1][8]["levels"] == 4 and r.calls[-1][8]["sigma"] == 0.125
        film.resolve(denoised=True)
        res = [c for c in r.calls if c[0] == "resolve"][-1]
        assert res[1:5] == (film.d_denoised, 4, 4, 1)             # the filtered mean resolves with n = 1
        film.resolve()
        assert [c for c in r.calls if c[0] == "resolve"][-1][1:5] == (film.d_sum, 4, 4, 4)
        film.accumulate(L.rt_params(), 1)                         # more passes: the filtered mean is stale
        with pytest.raises(ValueError, match="denoise\\(\\) first"):
            film.resolve_device(d_u8=1, denoised=True)
        film.clear()
        assert film.d_guides and not film.current("denoised")        # clear() keeps the guides
        r.h = 5
        with pytest.raises(ValueError, match="frame is now"):
            film.guides()
        r.h = 4
        held = [film.d_guides, film.d_denoised, film.d_work, film.d_sum]
    assert [c[1] for c in r.calls[-4:]] == held and all(c[0] == "free" for c in r.calls[-4:])
