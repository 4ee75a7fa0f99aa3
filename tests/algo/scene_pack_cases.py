"""The scenes tests/test_algorithms.py packs through tests/algo/scene_pack_check.cpp, and the ctypes side of that shim.
A case is a dict of what an rt_set_scene* entry takes (arrays, counts that may disagree with them on purpose, the entry's
name); CASES are valid scenes built from fixtures under tests/golden/, ERRORS one invalid input per rule of rt_scene.h and a
few that break two rules at once, EQUAL the degenerate inputs that must pack exactly like a lower entry's.
Run as a script (the shim is built with AddressSanitizer, whose runtime has to be loaded before Python's):
    python scene_pack_cases.py <shim.so> <out.npz>
packs every case and writes the results in the format of tests/golden/scene_pack.npz."""
import ctypes as C
import json
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
ENTRIES = ["scene", "materials", "materials_ex", "scatter", "area_lights", "textures", "lighting", "sky"]   # rt_set_scene_*
LAYOUT = ["S", "P", "L", "NC", "M", "mat_cols", "soft_n", "T", "lit", "sky", "lens_mat", "tex_off", "lit_off", "sky_off", "plane_codes"]
CLUSTER_MIN, LANES_MIN_SPHERES = 20, 161       # rt_ctx's defaults (rt::CLUSTER_MIN, MI355RT_LANES_MINS)
RT_FLAG_TYPED_BIAS = 1


class rt_texture(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("axis", (C.c_double * 3) * 3), ("dim", C.c_int32 * 3), ("reserved", C.c_int32),
                ("first", C.c_int64)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int32), ("error", C.c_char * 252), ("layout", C.c_int64 * 15), ("extent2", C.c_double),
                ("n_rec", C.c_uint64), ("n_texels", C.c_uint64), ("rec", C.POINTER(C.c_double)), ("texels", C.POINTER(C.c_float))]


def case(fixture, entry, **over):
    """The scene of tests/golden/<fixture>.npz as `entry` takes it; over: replacements (arrays, or counts S, L, P, M, T,
    n_texels, ncols that then no longer follow from the arrays)."""
    g = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    c = {"entry": entry, "flags": 0, "shadow_samples": 1}
    for k in ("spheres", "lights", "planes", "materials", "sphere_material", "plane_material", "light_radius", "sphere_texture",
              "plane_texture", "texels", "light_rgb", "sky", "tex_origin", "tex_axes", "tex_dims", "tex_first"):
        c[k] = np.array(g[k]) if k in g.files else None
    if "shadow_samples" in g.files:
        c["shadow_samples"] = int(g["shadow_samples"])
    c.update(over)
    return c


def args_of(c):
    """The arguments of rt_set_scene_sky after the context for case c, and the arrays that back them.  What c's entry does not
    take is absent (NULL / 0; shadow_samples 1), as the library's entries fill rt::SceneDesc."""
    has = lambda e: ENTRIES.index(c["entry"]) >= ENTRIES.index(e)
    keep = []

    def ptr(a, dtype, ctype):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(ctype))

    f32 = lambda a: ptr(a, np.float32, C.c_float)
    i32 = lambda a: ptr(a, np.int32, C.c_int32)
    f64 = lambda a: ptr(a, np.float64, C.c_double)
    n = lambda key, a, axis: int(c[key]) if key in c else (0 if a is None else a.shape[axis])
    sp, li, pl = c["spheres"], c["lights"], c["planes"]
    out = [f32(sp), n("S", sp, 1), f32(li), n("L", li, 1), f32(pl), n("P", pl, 1), int(c["flags"])]
    mat = c["materials"] if has("materials") else None
    ncols = int(c["ncols"]) if "ncols" in c else (3 if mat is None or mat.ndim != 2 else mat.shape[1])
    out += [f64(mat), n("M", mat, 0) if has("materials") else 0, ncols,
            i32(c["sphere_material"]) if has("materials") else None, i32(c["plane_material"]) if has("materials") else None]
    if has("area_lights"):
        rad = c["light_radius"] if c["light_radius"] is not None else np.zeros(max(out[3], 1), np.float32)   # (no radii: zeros)
        out += [f32(rad), int(c["shadow_samples"])]
    else:
        out += [None, 1]
    if has("textures") and c["tex_origin"] is not None:
        T = c["tex_origin"].shape[0]
        recs = (rt_texture * max(T, 1))()
        for t in range(T):
            for a in range(3):
                recs[t].origin[a] = c["tex_origin"][t, a]
                recs[t].dim[a] = int(c["tex_dims"][t, a])
                for i in range(3):
                    recs[t].axis[a][i] = c["tex_axes"][t, a, i]
            recs[t].first = int(c["tex_first"][t])
            recs[t].reserved = int(c.get("tex_reserved", 0))
        keep.append(recs)
        tx = c["texels"]
        out += [None if c.get("textures_null") else recs, int(c["T"]) if "T" in c else T, i32(c["sphere_texture"]), i32(c["plane_texture"]),
                None if c.get("texels_null") else f32(tx), n("n_texels", tx, 0)]
    else:
        out += [None, 0, None, None, None, 0]
    out += [f32(c["light_rgb"]) if has("lighting") else None, f64(c["sky"]) if has("sky") else None]
    return out, keep


_fp, _ip, _dp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
SKY_ARGTYPES = [_fp, C.c_int, _fp, C.c_int, _fp, C.c_int, C.c_int, _dp, C.c_int, C.c_int, _ip, _ip, _fp, C.c_int,
                C.POINTER(rt_texture), C.c_int, _ip, _ip, _fp, C.c_int64, _fp, _dp]


def bind(path):
    lib = C.CDLL(path)
    lib.scene_pack.restype = C.c_int
    lib.scene_pack.argtypes = SKY_ARGTYPES + [C.c_int, C.c_int, C.c_int, C.POINTER(Result)]
    lib.scene_pack_free.restype = None
    lib.scene_pack_free.argtypes = [C.POINTER(Result)]
    for name, nargs in (("scene_mat_offset", 4), ("scene_mat_doubles", 4), ("scene_tex_doubles", 1), ("scene_lit_doubles", 3)):
        getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_uint64, [C.c_int] * nargs
    lib.scene_block_family.restype, lib.scene_block_family.argtypes = C.c_int, [C.c_int] * 3
    return lib


def pack(lib, c, cluster_min=CLUSTER_MIN, lanes_min_spheres=LANES_MIN_SPHERES):
    """Case c through the shim: {"status", "error", "layout" int64 (15,), "extent2" float64 (1,), "rec" uint64, "texels" uint32}
    (the two buffers as their bit patterns)."""
    args, keep = args_of(c)
    r = Result()
    st = lib.scene_pack(*args, int(c["entry"] in ("lighting", "sky")), cluster_min, lanes_min_spheres, C.byref(r))
    assert st == r.status, (st, r.status)
    out = {"status": int(r.status), "error": r.error.decode(), "layout": np.array(list(r.layout), np.int64),
           "extent2": np.array([r.extent2], np.float64),
           "rec": np.ctypeslib.as_array(r.rec, shape=(int(r.n_rec),)).view(np.uint64).copy() if r.n_rec else np.zeros(0, np.uint64),
           "texels": np.ctypeslib.as_array(r.texels, shape=(int(r.n_texels),)).view(np.uint32).copy() if r.n_texels else np.zeros(0, np.uint32)}
    lib.scene_pack_free(C.byref(r))
    del keep
    return out


def _set(a, idx, v):
    a = np.array(a)
    a[idx] = v
    return a


def cases():
    """name -> case: the valid scenes."""
    tex, lit, sky, soft = "texture_everything_48_d4", "lighting_everything_48_d4", "sky_everything_48_d4", "lens_soft_glass_rough_48_d4"
    white_spec0 = dict(light_rgb=np.ones((3, 3), np.float32), materials=_set(np.load(os.path.join(GOLDEN, lit + ".npz"))["materials"], (slice(None), 6), 0.0))
    black = _set(np.load(os.path.join(GOLDEN, sky + ".npz"))["sky"], [3, 4, 5, 6, 7, 8, 9, 10, 11, 17, 18, 19, 20, 21, 22], 0.0)
    return {
        "flat": case("frame_c1_128", "scene"),                                        # no table, flat
        "mat3": case("materials_default_64_d3", "materials"),                         # 3 columns
        "refr5": case("refraction_default_64_d4", "materials_ex"),                    # 5 columns, glass
        "scat6": case("scatter_default_64_d4", "scatter"),                            # 6 columns, rough
        "soft6": case(soft, "area_lights"),                                           # area lights, 6-column table (no padded lens copy)
        "soft3": case("materials_default_64_d3", "area_lights", light_radius=np.array([0.25, 0.0, 0.5], np.float32),
                      shadow_samples=4),                                              # soft table padded from 3 columns
        "tex": case(tex, "textures"),
        "lit": case(lit, "lighting"),
        "sky": case(sky, "sky"),                                                      # all five blocks
        "sky_s64": case("sky_c4_s64_d5_sub32", "sky"),                                # clustered, not group-aligned
        "sky_s256": case("sky_c5_s256_d8_sub96", "sky"),                              # group-aligned split
        "typed_bias": case("frame_tilted_planes_48", "scene", flags=RT_FLAG_TYPED_BIAS),
        # the degenerate inputs and the lower entries they must equal (EQUAL)
        "tex_none": case(tex, "textures", sphere_texture=np.full(6, -1, np.int32), plane_texture=np.full(1, -1, np.int32)),
        "tex_none_lower": case(tex, "area_lights"),
        "lit_white": case(lit, "lighting", **white_spec0),
        "lit_white_lower": case(lit, "textures", materials=white_spec0["materials"][:, :6]),
        "sky_black": case(sky, "sky", sky=black),
        "sky_black_lower": case(sky, "lighting"),
        "radii_zero": case(soft, "area_lights", light_radius=np.zeros(3, np.float32)),
        "radii_zero_lower": case(soft, "scatter"),
    }


EQUAL = [("tex_none", "tex_none_lower"), ("lit_white", "lit_white_lower"), ("sky_black", "sky_black_lower"),
         ("radii_zero", "radii_zero_lower")]


def errors():
    """name -> case: invalid inputs, one per rule of rt_scene.h's check_* functions, then some that break two rules."""
    b = "sky_everything_48_d4"
    g = np.load(os.path.join(GOLDEN, b + ".npz"))
    sky, mat8, rgb, rad = g["sky"], g["materials"], g["light_rgb"], g["light_radius"]
    mat6, mat3 = mat8[:, :6], np.load(os.path.join(GOLDEN, "materials_default_64_d3.npz"))["materials"]
    glass = int(np.argmax(mat8[:, 3] > 0))                    # a transparent row of the fixture
    assert mat8[glass, 3] > 0
    nan, inf = float("nan"), float("inf")
    zero_rad = np.zeros(3, np.float32)
    e = {
        "sky_not_finite": case(b, "sky", sky=_set(sky, 5, nan)),
        "sky_colour_negative": case(b, "sky", sky=_set(sky, 4, -0.5)),
        "sky_up_not_unit": case(b, "sky", sky=_set(sky, slice(0, 3), 2.0 * sky[0:3])),
        "sky_sun_not_unit": case(b, "sky", sky=_set(sky, slice(13, 16), 0.5 * sky[13:16])),
        "sky_sharp": case(b, "sky", sky=_set(sky, 12, 3.0)),
        "sky_halo_shin": case(b, "sky", sky=_set(sky, 23, 2048.0)),
        "ncols_lighting": case(b, "sky", ncols=4),
        "ncols_8_textures": case(b, "textures", ncols=8),
        "ncols_scatter": case(b, "scatter", materials=mat6, ncols=4),
        "rgb_light_count": case(b, "lighting", L=65),
        "rgb_negative": case(b, "lighting", light_rgb=_set(rgb, (1, 0), -1.0)),
        "rgb_nan": case(b, "lighting", light_rgb=_set(rgb, (2, 2), nan)),
        "shadow_samples_0": case(b, "area_lights", materials=mat6, shadow_samples=0),
        "shadow_samples_17": case(b, "area_lights", materials=mat6, shadow_samples=17),
        "radius_light_count": case(b, "area_lights", materials=mat6, L=-1),
        "radius_negative": case(b, "area_lights", materials=mat6, light_radius=_set(rad, 2, -0.25)),
        "radius_inf": case(b, "area_lights", materials=mat6, light_radius=_set(rad, 0, inf)),
        "soft_without_table": case(b, "area_lights", materials=None, M=0, light_radius=np.array([0, 0.5, 0], np.float32)),
        "table_not_finite": case(b, "scatter", materials=_set(mat6, (2, 1), inf)),
        "table_trans_negative": case(b, "scatter", materials=_set(mat6, (1, 3), -0.1)),
        "table_ior_zero": case(b, "scatter", materials=_set(mat6, (0, 4), 0.0)),
        "table_glass_refl": case(b, "scatter", materials=_set(mat6, (glass, 2), 0.3)),
        "table_rough_range": case(b, "scatter", materials=_set(mat6, (0, 5), 1.5)),
        "table_glass_rough": case(b, "scatter", materials=_set(mat6, (glass, 5), 0.5)),
        "table_spec_negative": case(b, "lighting", materials=_set(mat8, (3, 6), -1.0)),
        "table_shin": case(b, "lighting", materials=_set(mat8, (4, 7), 3.0)),
        "size_spheres": case(b, "scene", S=1025),
        "size_planes": case(b, "sky", P=65),
        "null_spheres": case(b, "scene", spheres=None, S=6),
        "material_count_257": case("materials_default_64_d3", "materials", M=257),
        "material_count_negative": case("materials_default_64_d3", "materials", M=-1),
        "lighting_without_table": case(b, "lighting", materials=None, M=0, light_radius=zero_rad, tex_origin=None),
        "sky_without_table": case(b, "sky", materials=None, M=0, light_radius=zero_rad, tex_origin=None, light_rgb=None),
        "materials_null": case("materials_default_64_d3", "materials", materials=None, M=2),
        "material_ids_null": case("materials_default_64_d3", "materials", sphere_material=None),
        "table3_not_finite": case("materials_default_64_d3", "materials", materials=_set(mat3, (4, 2), nan)),
        "sphere_material_range": case(b, "sky", sphere_material=_set(g["sphere_material"], 3, 7)),
        "plane_material_range": case(b, "sky", plane_material=_set(g["plane_material"], 0, -1)),
        "texture_count_65": case(b, "textures", materials=mat6, T=65),
        "texture_count_negative": case(b, "textures", materials=mat6, T=-1),
        "texel_count_negative": case(b, "textures", materials=mat6, n_texels=-1),
        "texel_count_max": case(b, "textures", materials=mat6, n_texels=(1 << 22) + 1),
        "textures_without_table": case(b, "textures", materials=None, M=0, light_radius=zero_rad),
        "textures_null": case(b, "textures", materials=mat6, textures_null=True),
        "texels_null": case(b, "textures", materials=mat6, texels_null=True),
        "texture_reserved": case(b, "textures", materials=mat6, tex_reserved=1),
        "texture_dim_0": case(b, "textures", materials=mat6, tex_dims=_set(g["tex_dims"], (1, 2), 0)),
        "texture_dim_4097": case(b, "textures", materials=mat6, tex_dims=_set(g["tex_dims"], (0, 0), 4097)),
        "texture_axis_nan": case(b, "textures", materials=mat6, tex_axes=_set(g["tex_axes"], (1, 0, 2), nan)),
        "texture_origin_inf": case(b, "textures", materials=mat6, tex_origin=_set(g["tex_origin"], (0, 1), inf)),
        "texture_range": case(b, "textures", materials=mat6, tex_first=_set(g["tex_first"], 1, g["texels"].shape[0])),
        "texel_not_finite": case(b, "textures", materials=mat6, texels=_set(g["texels"], (5, 1), inf)),
        "sphere_texture_range": case(b, "sky", sphere_texture=_set(g["sphere_texture"], 4, 2)),
        "plane_texture_range": case(b, "sky", plane_texture=_set(g["plane_texture"], 0, -2)),
        # two rules at once: the first in rt_scene.h's order is the one reported
        "two_sky_and_ncols": case(b, "sky", sky=_set(sky, 20, inf), ncols=7),
        "two_radius_and_id": case(b, "sky", light_radius=_set(rad, 1, -1.0), sphere_material=_set(g["sphere_material"], 0, 99)),
        "two_ncols_and_rgb": case(b, "lighting", ncols=2, light_rgb=_set(rgb, (0, 0), -3.0)),
        "two_samples_and_size": case(b, "area_lights", materials=mat6, shadow_samples=0, S=5000),
        "two_table_and_texture_count": case(b, "textures", materials=_set(mat6, (1, 3), -0.1), T=70),
        "two_material_and_texture_id": case(b, "sky", sphere_material=_set(g["sphere_material"], 5, -4),
                                            sphere_texture=_set(g["sphere_texture"], 0, 9)),
        "two_rgb_and_radius": case(b, "sky", light_rgb=_set(rgb, (2, 1), nan), light_radius=_set(rad, 0, nan)),
        "two_sky_table_and_texel": case(b, "sky", sky=_set(sky, 12, 5.0), materials=_set(mat8, (0, 4), -1.0),
                                        texels=_set(g["texels"], (0, 0), nan)),
    }
    assert g["tex_origin"].shape[0] == 2 and g["texels"].shape[0] == 12 and mat8.shape == (7, 8), "the errors above are written for this fixture"
    return e


def run_all(pack_one):
    """Every case through pack_one(case) -> the arrays of tests/golden/scene_pack.npz."""
    out, errs = {}, {}
    for name, c in cases().items():
        r = pack_one(c)
        assert r["status"] == 0, (name, r["status"], r["error"])
        for k in ("rec", "texels", "layout", "extent2"):
            out[f"{name}/{k}"] = r[k]
    for name, c in errors().items():
        r = pack_one(c)
        errs[name] = [r["status"], r["error"]]
    out["errors"] = np.array(json.dumps(errs, sort_keys=True))
    return out


if __name__ == "__main__":
    lib = bind(sys.argv[1])
    np.savez_compressed(sys.argv[2], **run_all(lambda c: pack(lib, c)))
