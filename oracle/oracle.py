"""TEST INFRASTRUCTURE ONLY — ctypes binding of oracle/librt_oracle.so (the CPU restatement).

Importers: tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg.  The product
package never imports this module (tests/test_boundary.py checks that).
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "librt_oracle.so")

FLAG_TYPED_BIAS = 1

# Deliberately wrong restatements of the feature path (rt_oracle.c ORC_WRONG_*): test-only, for showing that the fixtures
# catch each of them (tests/test_oracle_features.py).
WRONG = dict(key_pixel=1, pow_weight=2, soft_i_major=4, lamb_whole=8, tir_far=16, no_bounce=32, focus_f=64, no_absorb=128,
             tex_biased=256, tex_trunc=512, spec_texel=1024, spec_whole=2048, sun_first=4096, sky_flat=8192, lamb_order=16384)
SKY_DOUBLES = 24

_lib = None


def build(force=False):
    src = os.path.join(HERE, "rt_oracle.c")
    if force or not os.path.exists(SO) or os.path.getmtime(SO) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", HERE, "-B", "librt_oracle.so"], stdout=subprocess.DEVNULL)
    return SO


class _RayGen(C.Structure):
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("pixel_loc", C.c_void_p),
                ("px", C.c_double), ("y0", C.c_double), ("dy", C.c_double), ("z0", C.c_double), ("dz", C.c_double)]


class _Features(C.Structure):
    _fields_ = [("M", C.c_int), ("ncols", C.c_int), ("materials", C.c_void_p), ("sphere_material", C.c_void_p),
                ("plane_material", C.c_void_p), ("light_radius", C.c_void_p), ("shadow_samples", C.c_int),
                ("aperture", C.c_double), ("focus", C.c_double), ("wrong", C.c_int),
                ("T", C.c_int), ("textures", C.c_void_p), ("sphere_texture", C.c_void_p), ("plane_texture", C.c_void_p),
                ("texels", C.c_void_p), ("n_texels", C.c_int64), ("light_rgb", C.c_void_p), ("sky", C.c_void_p)]


class _Texture(C.Structure):
    """rt_oracle.c orc_texture: the layout of include/mi355rt.h's rt_texture."""
    _fields_ = [("origin", C.c_double * 3), ("axis", (C.c_double * 3) * 3), ("dim", C.c_int32 * 3), ("reserved", C.c_int32),
                ("first", C.c_int64)]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO):
            build()
        L = C.CDLL(SO)
        dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
        L.orc_normalize.argtypes = [dp, dp]
        L.orc_intersect_ray_sphere.argtypes = [dp, dp, fp, C.c_float]
        L.orc_intersect_ray_sphere.restype = C.c_double
        L.orc_intersect_ray_plane.argtypes = [dp, dp, fp, fp]
        L.orc_intersect_ray_plane.restype = C.c_double
        L.orc_get_intersection.argtypes = [dp, dp, fp, C.c_int, fp, C.c_int, dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.orc_get_reflection.argtypes = [dp, dp, dp]
        L.orc_plane_normal_f32.argtypes = [fp, fp]
        L.orc_clip_color.argtypes = [C.c_double]
        L.orc_clip_color.restype = C.c_int
        L.orc_sample.argtypes = [fp, C.c_int, fp, C.c_int, fp, C.c_int, dp, dp, C.c_double, C.c_double, dp, C.c_int, C.c_int, dp]
        L.orc_render.argtypes = [C.POINTER(_RayGen), dp, dp, fp, C.c_int, fp, C.c_int, fp, C.c_int,
                                 C.c_double, C.c_double, dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong), C.c_int, C.c_uint32]
        L.orc_render.restype = C.c_int
        L.orc_render_pixels.argtypes = [C.POINTER(_RayGen), dp, dp, fp, C.c_int, fp, C.c_int, fp, C.c_int,
                                        C.c_double, C.c_double, dp, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32]
        L.orc_render_pixels.restype = C.c_int
        L.orc_render_ex.argtypes = list(L.orc_render.argtypes) + [C.POINTER(_Features)]
        L.orc_render_ex.restype = C.c_int
        L.orc_render_pixels_ex.argtypes = list(L.orc_render_pixels.argtypes) + [C.POINTER(_Features)]
        L.orc_render_pixels_ex.restype = C.c_int
        L.orc_max_threads.restype = C.c_int
        L.orc_texel_index.argtypes = [dp, C.POINTER(_Texture), C.c_int]
        L.orc_texel_index.restype = C.c_int64
        L.orc_light_terms.argtypes = [dp, dp, dp, dp, dp, dp, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int]
        L.orc_light_terms.restype = None
        L.orc_sky_color.argtypes = [dp, dp, dp]
        L.orc_sky_color.restype = None
        _lib = L
    return _lib


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def normalize(v):
    v = _d(v); out = np.empty(3)
    lib().orc_normalize(_dp(v), _dp(out))
    return out


def intersect_ray_sphere(o, d, c, r):
    o, d, c = _d(o), _d(d), _f(c)
    return lib().orc_intersect_ray_sphere(_dp(o), _dp(d), _fp(c), C.c_float(float(np.float32(r))))


def intersect_ray_plane(o, d, po, pn):
    o, d, po, pn = _d(o), _d(d), _f(po), _f(pn)
    return lib().orc_intersect_ray_plane(_dp(o), _dp(d), _fp(po), _fp(pn))


def get_intersection(o, d, spheres, planes):
    o, d, spheres, planes = _d(o), _d(d), _f(spheres), _f(planes)
    t = C.c_double(); i = C.c_int(); ty = C.c_int()
    lib().orc_get_intersection(_dp(o), _dp(d), _fp(spheres), spheres.shape[1], _fp(planes), planes.shape[1],
                               C.byref(t), C.byref(i), C.byref(ty))
    return t.value, i.value, ty.value


def get_reflection(d, n):
    d, n = _d(d), _d(n); out = np.empty(3)
    lib().orc_get_reflection(_dp(d), _dp(n), _dp(out))
    return out


def plane_normal_f32(n):
    n = _f(n); out = np.empty(3, np.float32)
    lib().orc_plane_normal_f32(_fp(n), _fp(out))
    return out


def clip_color(c):
    return lib().orc_clip_color(float(c))


def _aa_code(aa, spp):
    """0 none, 1 the reference's 9-tap mode, 0x100|spp stochastic supersampling (aa == 2)."""
    if int(aa) == 2:
        assert 1 <= int(spp) <= 64
        return 0x100 | int(spp)
    return int(bool(aa))


def jitter(x, y, s, seed):
    """(u, v) in [-1/2, 1/2)^2 of sample s of pixel (x, y): the counter hash of rt_oracle.c:jitter_hash."""
    M = 0xFFFFFFFF
    h = (seed ^ 0x9E3779B9) & M
    h = ((h ^ x) * 0x85EBCA6B) & M; h ^= h >> 13
    h = ((h ^ y) * 0xC2B2AE35) & M; h ^= h >> 16
    h = ((h ^ s) * 0x27D4EB2F) & M; h ^= h >> 15
    h = (h * 0x165667B1) & M; h ^= h >> 13
    return (h & 0xFFFF) * 2.0 ** -16 + (2.0 ** -17 - 0.5), (h >> 16) * 2.0 ** -16 + (2.0 ** -17 - 0.5)


def refl_powers(refl, depth):
    """refl ** (i+1) as the reference evaluates it (trace.py:131)."""
    return np.array([float(refl) ** (i + 1) for i in range(max(int(depth), 1))], dtype=np.float64)


def sample(spheres, lights, planes, o, d, amb, lamb, refl, depth, flags=0):
    spheres, lights, planes, o, d = _f(spheres), _f(lights), _f(planes), _d(o), _d(d)
    rp = refl_powers(refl, depth); out = np.empty(3)
    lib().orc_sample(_fp(spheres), spheres.shape[1], _fp(lights), lights.shape[1], _fp(planes), planes.shape[1],
                     _dp(o), _dp(d), float(amb), float(lamb), _dp(rp), int(depth), int(flags), _dp(out))
    return out


def _texture_records(records):
    """A ctypes array of orc_texture from records (origin (3,), axes (3,3), (nx, ny, nz), first)."""
    recs = (_Texture * max(len(records), 1))()
    for k, (o, ax, dims, first) in enumerate(records):
        o, ax = _d(o).reshape(3), _d(ax).reshape(3, 3)
        for a in range(3):
            recs[k].origin[a] = o[a]
            recs[k].dim[a] = int(dims[a])
            for i in range(3):
                recs[k].axis[a][i] = ax[a, i]
        recs[k].first = int(first)
    return recs


def texel_index(points, origin, axes, dims, first=0, wrong=0):
    """rt_oracle.c orc_texel_index for points (..., 3): int64 of shape points.shape[:-1] (scene.texel_index's arguments)."""
    p = _d(points)
    recs = _texture_records([(origin, axes, dims, first)])
    flat = p.reshape(-1, 3)
    out = np.empty(len(flat), np.int64)
    fn = lib().orc_texel_index
    for i in range(len(flat)):
        out[i] = fn(_dp(flat[i]), recs, int(wrong))
    return out.reshape(p.shape[:-1])


def light_terms(rgb, d, N, Ld, col, e, lamb_n, spec, spec_n, shin, occluded, wrong=0):
    """rt_oracle.c orc_light_terms for arrays (..., 3) (scene.lighting.light_terms' arguments): (..., 3) float64."""
    rgb = np.array(_d(rgb))
    shape = rgb.shape[:-1]
    b3 = lambda a: np.ascontiguousarray(np.broadcast_to(_d(a), rgb.shape)).reshape(-1, 3)
    b1 = lambda a, dt=np.float64: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=dt), shape)).reshape(-1)
    d, N, Ld, col = b3(d), b3(N), b3(Ld), b3(col)
    e = _d(e).reshape(3)
    lamb_n, spec, spec_n, shin, occ = b1(lamb_n), b1(spec), b1(spec_n), b1(shin), b1(occluded, bool)
    flat = rgb.reshape(-1, 3)
    fn = lib().orc_light_terms
    for i in range(len(flat)):
        nsq = int(shin[i]).bit_length() - 1
        assert float(1 << nsq) == shin[i] and 0 <= nsq <= 10
        fn(_dp(flat[i]), _dp(d[i]), _dp(N[i]), _dp(Ld[i]), _dp(col[i]), _dp(e), float(lamb_n[i]), float(spec[i]), float(spec_n[i]),
           nsq, int(occ[i]), int(wrong))
    return flat.reshape(rgb.shape)


def sky_color(d, packed):
    """rt_oracle.c orc_sky_color for directions (..., 3) and a packed sky (24 float64; not checked here): (..., 3) float64."""
    d = _d(d)
    k = _d(packed).reshape(-1)
    assert k.shape == (SKY_DOUBLES,)
    flat = d.reshape(-1, 3)
    out = np.empty_like(flat)
    fn = lib().orc_sky_color
    for i in range(len(flat)):
        fn(_dp(flat[i]), _dp(k), _dp(out[i]))
    return out.reshape(d.shape)


def _features(S, L, P, materials, light_radius, shadow_samples, lens, wrong, textures=None, light_rgb=None, sky=None):
    """(struct, arrays it points into) for the keyword arguments of render / render_pixels, or (None, None) when none is given:
    then the plain entry points run."""
    if materials is None and light_radius is None and lens is None and not wrong and textures is None and light_rgb is None \
            and sky is None:
        return None, None
    fe = _Features()
    keep = []
    if materials is not None:
        table, sid, pid = materials
        table = _d(table)
        table = table.reshape(-1, table.shape[-1]) if table.ndim == 2 else table.reshape(-1, 3)
        sid = np.ascontiguousarray(sid, dtype=np.int32).reshape(-1)
        pid = np.ascontiguousarray(pid, dtype=np.int32).reshape(-1)
        assert sid.shape == (S,) and pid.shape == (P,)
        keep += [table, sid, pid]
        fe.M, fe.ncols = table.shape
        fe.materials, fe.sphere_material, fe.plane_material = table.ctypes.data, sid.ctypes.data, pid.ctypes.data
    if light_radius is not None:
        rad = _f(light_radius).reshape(-1)
        assert rad.shape == (L,)
        keep.append(rad)
        fe.light_radius = rad.ctypes.data if L else None
    fe.shadow_samples = int(shadow_samples)
    fe.aperture, fe.focus = (0.0, 1.0) if lens is None else (float(lens[0]), float(lens[1]))
    fe.wrong = int(wrong)
    if textures is not None:
        records, tsid, tpid, texels = textures
        recs = _texture_records(records)
        tsid = np.ascontiguousarray(tsid, dtype=np.int32).reshape(-1)
        tpid = np.ascontiguousarray(tpid, dtype=np.int32).reshape(-1)
        tx = _f(texels).reshape(-1, 3)
        assert tsid.shape == (S,) and tpid.shape == (P,)
        keep += [recs, tsid, tpid, tx]
        fe.T, fe.textures = len(records), C.addressof(recs)
        fe.sphere_texture, fe.plane_texture = tsid.ctypes.data, tpid.ctypes.data
        fe.texels, fe.n_texels = tx.ctypes.data, tx.shape[0]
    if light_rgb is not None:
        rgb = _f(light_rgb).reshape(-1, 3)
        assert rgb.shape == (L, 3)
        keep.append(rgb)
        fe.light_rgb = rgb.ctypes.data if L else None
    if sky is not None:
        k = _d(sky.pack() if hasattr(sky, "pack") else sky).reshape(-1)
        if k.shape != (SKY_DOUBLES,):
            raise ValueError(f"sky: {k.shape[0]} doubles, a packed sky has {SKY_DOUBLES}")
        keep.append(k)
        fe.sky = k.ctypes.data
    return fe, keep


def render(w, h, cam_origin, cam_rot, spheres, lights, planes, amb, lamb, refl, depth, aa=False, *,
           pixel_loc=None, raygen=None, x0=0, x1=None, flags=0, want=("u8", "f64"), nthreads=0, refl_pow=None,
           spp=0, seed=1, materials=None, light_radius=None, shadow_samples=1, lens=None, wrong=0, textures=None,
           light_rgb=None, sky=None):
    """Run the restated `render` (kernels.py:6-73) for columns [x0,x1).

    raygen = (px, y0, dy, z0, dz) closed form, or pixel_loc = explicit float64 (3,w,h) array.
    Returns dict with any of 'u8' (3,w,h) uint8 [R,B,G], 'f64' (3,w,h), 'f32' (3,w,h) and 'counters'.
    Columns outside [x0,x1) are left zero.

    The features of include/mi355rt.h (rt_oracle.c orc_render_ex): materials = (table (M,3|5|6|8) float64, sphere ids (S,),
    plane ids (P,)) as rt_set_scene_lighting takes them (amb, lamb and refl are then ignored); light_radius (L,)
    and shadow_samples as rt_set_scene_area_lights; lens = (aperture, focus_distance) as rt_set_lens; textures = (records,
    sphere ids (S,), plane ids (P,), texels (N,3)), light_rgb (L,3) float32 and sky (a scene.Sky or its 24 packed float64)
    with the shapes Renderer.set_scene takes (rt_set_scene_textures, _lighting, _sky).  wrong: WRONG bits (test-only).
    Input the header refuses raises ValueError.
    """
    L = lib()
    x1 = w if x1 is None else x1
    rg = _RayGen()
    rg.w, rg.h = int(w), int(h)
    keep = None
    if pixel_loc is not None:
        keep = _d(pixel_loc)
        assert keep.shape == (3, w, h)
        rg.pixel_loc = keep.ctypes.data
    else:
        rg.pixel_loc = None
        rg.px, rg.y0, rg.dy, rg.z0, rg.dz = [float(v) for v in raygen]
    spheres, lights, planes = _f(spheres), _f(lights), _f(planes)
    o, R = _d(cam_origin), _d(cam_rot).reshape(9)
    rp = _d(refl_pow) if refl_pow is not None else refl_powers(refl, depth)
    out = {}
    u8 = np.zeros((3, w, h), np.uint8) if "u8" in want else None
    f64 = np.zeros((3, w, h), np.float64) if "f64" in want else None
    f32 = np.zeros((3, w, h), np.float32) if "f32" in want else None
    cnt = (C.c_longlong * 3)()
    fe, fkeep = _features(spheres.shape[1], lights.shape[1], planes.shape[1], materials, light_radius, shadow_samples, lens, wrong,
                            textures, light_rgb, sky)
    args = (C.byref(rg), _dp(o), _dp(R), _fp(spheres), spheres.shape[1], _fp(lights), lights.shape[1],
            _fp(planes), planes.shape[1], float(amb), float(lamb), _dp(rp), int(depth), _aa_code(aa, spp), int(flags),
            int(x0), int(x1),
            u8.ctypes.data if u8 is not None else None,
            f64.ctypes.data if f64 is not None else None,
            f32.ctypes.data if f32 is not None else None, cnt, int(nthreads), int(seed) & 0xFFFFFFFF)
    rc = L.orc_render(*args) if fe is None else L.orc_render_ex(*args, C.byref(fe))
    del fkeep
    if rc != 0:
        raise ValueError("orc_render: bad arguments")
    if u8 is not None: out["u8"] = u8
    if f64 is not None: out["f64"] = f64
    if f32 is not None: out["f32"] = f32
    out["counters"] = dict(closest=cnt[0], shadow=cnt[1], hits=cnt[2])
    return out


def render_pixels(w, h, coords, cam_origin, cam_rot, spheres, lights, planes, amb, lamb, refl, depth, aa=False, *,
                  pixel_loc=None, raygen=None, flags=0, nthreads=0, refl_pow=None, spp=0, seed=1, materials=None,
                  light_radius=None, shadow_samples=1, lens=None, wrong=0, textures=None, light_rgb=None, sky=None):
    """The same per-pixel path for an explicit (n,2) list of (x,y) pixels (the feature keywords of render()).
    Returns (u8 (n,3) in stored order [R,B,G], f64 (n,3) = pre-clip (R,G,B))."""
    L = lib()
    rg = _RayGen()
    rg.w, rg.h = int(w), int(h)
    keep = None
    if pixel_loc is not None:
        keep = _d(pixel_loc)
        assert keep.shape == (3, w, h)
        rg.pixel_loc = keep.ctypes.data
    else:
        rg.pixel_loc = None
        rg.px, rg.y0, rg.dy, rg.z0, rg.dz = [float(v) for v in raygen]
    spheres, lights, planes = _f(spheres), _f(lights), _f(planes)
    o, R = _d(cam_origin), _d(cam_rot).reshape(9)
    rp = _d(refl_pow) if refl_pow is not None else refl_powers(refl, depth)
    co = np.ascontiguousarray(coords, dtype=np.int32).reshape(-1, 2)
    n = co.shape[0]
    u8 = np.zeros((n, 3), np.uint8)
    f64 = np.zeros((n, 3), np.float64)
    fe, fkeep = _features(spheres.shape[1], lights.shape[1], planes.shape[1], materials, light_radius, shadow_samples, lens, wrong,
                            textures, light_rgb, sky)
    args = (C.byref(rg), _dp(o), _dp(R), _fp(spheres), spheres.shape[1], _fp(lights), lights.shape[1],
            _fp(planes), planes.shape[1], float(amb), float(lamb), _dp(rp), int(depth), _aa_code(aa, spp),
            int(flags), co.ctypes.data, n, u8.ctypes.data, f64.ctypes.data, int(nthreads), int(seed) & 0xFFFFFFFF)
    rc = L.orc_render_pixels(*args) if fe is None else L.orc_render_pixels_ex(*args, C.byref(fe))
    del fkeep
    if rc != 0:
        raise ValueError("orc_render_pixels: bad arguments")
    return u8, f64


def max_threads():
    return lib().orc_max_threads()
