"""ctypes binding of libmi355rt.so — one prototype per declaration in include/mi355rt.h."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("MI355RT_SO") or os.path.join(HERE, "libmi355rt.so")   # env override: A/B profiling of other builds

RT_ABI_VERSION = 7
RT_MAX_DEPTH = 16
RT_MAX_SPHERES, RT_MAX_PLANES, RT_MAX_LIGHTS = 1024, 64, 64
RT_MAX_MATERIALS = 256
RT_OK, RT_ERR_BAD_ARG, RT_ERR_HIP, RT_ERR_NO_DEVICE, RT_ERR_STATE, RT_ERR_ALLOC = 0, -1, -2, -3, -4, -5
RT_AA_NONE, RT_AA_REFERENCE, RT_AA_STOCHASTIC = 0, 1, 2
RT_MAX_SPP = 64
RT_MAX_SHADOW_SAMPLES = 16
RT_RENDER_SLOTS = 4
RT_MAX_TEXTURES, RT_MAX_TEXTURE_DIM, RT_MAX_TEXELS = 64, 4096, 1 << 22
RT_SKY_DOUBLES = 24
RT_FILM_MAX_PIXELS = 1 << 27
RT_GUIDE_PLANES = 8
RT_TEMPORAL_MAX_N = 1 << 24          # rt_film_temporal: the most passes one call blends in
RT_BLOOM_MAX_LEVELS, RT_BLOOM_WORK_PLANES, RT_BLOOM_NO_TILES = 8, 6, 1
RT_METER_LO, RT_METER_OCTAVES, RT_METER_SUB, RT_METER_BINS, RT_METER_STATE_DOUBLES = -16, 40, 8, 323, 4
RT_FLAG_TYPED_BIAS, RT_FLAG_U8_RGB, RT_FLAG_NO_FEEDBACK, RT_FLAG_U8_HWC, RT_FLAG_COUNT_RAYS, RT_FLAG_AA_PER_PIXEL, RT_FLAG_NO_BUNDLES = 1, 2, 4, 8, 16, 32, 64

STATUS_NAMES = {0: "RT_OK", -1: "RT_ERR_BAD_ARG", -2: "RT_ERR_HIP", -3: "RT_ERR_NO_DEVICE", -4: "RT_ERR_STATE", -5: "RT_ERR_ALLOC"}


class rt_params(C.Structure):
    _fields_ = [("amb", C.c_double), ("lamb", C.c_double), ("refl_pow", C.c_double * RT_MAX_DEPTH),
                ("depth", C.c_int32), ("aa_mode", C.c_int32), ("flags", C.c_int32), ("spp", C.c_int32),
                ("seed", C.c_uint32), ("reserved", C.c_int32)]


class rt_kernel_info(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("vgprs", "sgprs", "lds_static", "max_threads", "wave_size", "cu_count", "clock_khz", "reserved")]


class rt_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("launches", "frames", "launches_measuring", "launches_settled", "table_builds",
                                          "closest_queries", "hits", "shadow_traced", "shadow_skipped")] + \
               [("bounce_waves", C.c_uint64 * (RT_MAX_DEPTH + 1)), ("bounce_lanes", C.c_uint64 * (RT_MAX_DEPTH + 1))]


class rt_texture(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("axis", (C.c_double * 3) * 3), ("dim", C.c_int32 * 3), ("reserved", C.c_int32),
                ("first", C.c_int64)]


class rt_film_tone(C.Structure):
    """rt_film_resolve's tone (include/mi355rt.h; the arithmetic in numpy: film.tone_reference): exposure finite and > 0; white 0 (no
    compression) or finite and > 0, the colour that maps to 255; gamma 1 or 2; flags RT_FLAG_U8_RGB | RT_FLAG_U8_HWC only."""
    _fields_ = [("exposure", C.c_double), ("white", C.c_double), ("gamma", C.c_int32), ("flags", C.c_int32)]


class rt_denoise(C.Structure):
    """rt_film_denoise's settings (include/mi355rt.h; the arithmetic in numpy: denoise.denoise_reference): levels 0..6; normal_shin
    1, 2, 4, ..., 1024; sigma 0 (no colour weight) or finite and > 0; demodulate 0 or 1; reserved 0."""
    _fields_ = [("levels", C.c_int32), ("normal_shin", C.c_int32), ("sigma", C.c_double), ("demodulate", C.c_int32),
                ("reserved", C.c_int32)]


class rt_denoise_variance(C.Structure):
    """rt_film_denoise_variance's settings (include/mi355rt.h; the arithmetic in numpy: variance.denoise_variance_reference): levels
    0..6; normal_shin 1, 2, 4, ..., 1024; kappa and var_floor finite and >= 0; demodulate and prefilter 0 or 1.  32 bytes."""
    _fields_ = [("levels", C.c_int32), ("normal_shin", C.c_int32), ("kappa", C.c_double), ("var_floor", C.c_double),
                ("demodulate", C.c_int32), ("prefilter", C.c_int32)]


class rt_temporal(C.Structure):
    """rt_film_temporal's settings (include/mi355rt.h; the arithmetic in numpy: temporal.temporal_reference): the camera the history
    was rendered with; depth_tol finite and >= 0, relative, on the squared distance; normal_cos in [-1, 1]; max_history finite and
    >= 0, in passes (0: no history is used); reserved 0.  128 bytes."""
    _fields_ = [("prev_origin", C.c_double * 3), ("prev_rotation", C.c_double * 9), ("depth_tol", C.c_double), ("normal_cos", C.c_double),
                ("max_history", C.c_double), ("reserved", C.c_int32 * 2)]


class rt_bloom(C.Structure):
    """rt_film_bloom's settings (include/mi355rt.h; the arithmetic in numpy: bloom.bloom_reference): threshold and strength finite and
    >= 0; levels 0..RT_BLOOM_MAX_LEVELS; flags RT_BLOOM_NO_TILES only.  24 bytes."""
    _fields_ = [("threshold", C.c_double), ("strength", C.c_double), ("levels", C.c_int32), ("flags", C.c_int32)]


class rt_meter(C.Structure):
    """rt_film_meter_solve's settings (include/mi355rt.h; the arithmetic in numpy: meter.solve_reference): key finite and > 0;
    percentile 0..1; min_exposure and max_exposure finite and > 0, min_exposure <= max_exposure; rate in (0, 1]; flags and reserved
    0.  48 bytes."""
    _fields_ = [("key", C.c_double), ("percentile", C.c_double), ("min_exposure", C.c_double), ("max_exposure", C.c_double),
                ("rate", C.c_double), ("flags", C.c_int32), ("reserved", C.c_int32)]


class rt_upsample(C.Structure):
    """rt_film_upsample's settings (include/mi355rt.h; the arithmetic in numpy: upsample.upsample_reference): the closed-form grids
    (px, y0, dy, z0, dz) of the low-resolution and the output frame, finite with px, dy and dz not 0; normal_cos in [-1, 1];
    demodulate 0 or 1; reserved 0.  96 bytes."""
    _fields_ = [("lo_grid", C.c_double * 5), ("hi_grid", C.c_double * 5), ("normal_cos", C.c_double), ("demodulate", C.c_int32),
                ("reserved", C.c_int32)]


# name -> (restype, argtypes); must list every function include/mi355rt.h declares.
_dp, _fp, _vp = C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_void_p
PROTOTYPES = {
    "rt_abi_version": (C.c_int, []),
    "rt_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "rt_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "rt_destroy": (C.c_int, [_vp]),
    "rt_last_error": (C.c_char_p, [_vp]),
    "rt_set_scene": (C.c_int, [_vp, _fp, C.c_int, _fp, C.c_int, _fp, C.c_int, C.c_int]),
    "rt_set_scene_materials": (C.c_int, [_vp, _fp, C.c_int, _fp, C.c_int, _fp, C.c_int, C.c_int, _dp, C.c_int,
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rt_set_scene_materials_ex": (C.c_int, [_vp, _fp, C.c_int, _fp, C.c_int, _fp, C.c_int, C.c_int, _dp, C.c_int, C.c_int,
                                            C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rt_set_scene_materials_scatter": (C.c_int, [_vp, _fp, C.c_int, _fp, C.c_int, _fp, C.c_int, C.c_int, _dp, C.c_int,
                                                 C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rt_set_scene_area_lights": (C.c_int, [_vp, _fp, C.c_int, _fp, C.c_int, _fp, C.c_int, C.c_int, _dp, C.c_int, C.c_int,
                                           C.POINTER(C.c_int32), C.POINTER(C.c_int32), _fp, C.c_int]),
    "rt_set_scene_textures": (C.c_int, [_vp, _fp, C.c_int, _fp, C.c_int, _fp, C.c_int, C.c_int, _dp, C.c_int, C.c_int,
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32), _fp, C.c_int,
                                        C.POINTER(rt_texture), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _fp, C.c_int64]),
    "rt_set_scene_lighting": (C.c_int, [_vp, _fp, C.c_int, _fp, C.c_int, _fp, C.c_int, C.c_int, _dp, C.c_int, C.c_int,
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32), _fp, C.c_int,
                                        C.POINTER(rt_texture), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _fp, C.c_int64,
                                        _fp]),
    "rt_set_scene_sky": (C.c_int, [_vp, _fp, C.c_int, _fp, C.c_int, _fp, C.c_int, C.c_int, _dp, C.c_int, C.c_int,
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32), _fp, C.c_int,
                                   C.POINTER(rt_texture), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _fp, C.c_int64,
                                   _fp, _dp]),
    "rt_set_camera": (C.c_int, [_vp, _dp, _dp]),
    "rt_set_lens": (C.c_int, [_vp, C.c_double, C.c_double]),
    "rt_set_raygen": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]),
    "rt_set_pixel_loc": (C.c_int, [_vp, _dp, C.c_int, C.c_int]),
    "rt_render": (C.c_int, [_vp, C.POINTER(rt_params), C.c_int, C.c_int, _vp, _vp]),
    "rt_render_begin": (C.c_int, [_vp, C.POINTER(rt_params), C.c_int, C.c_int, _vp, _vp, C.c_int]),
    "rt_render_end": (C.c_int, [_vp, C.c_int]),
    "rt_render_device": (C.c_int, [_vp, C.POINTER(rt_params), C.c_int, C.c_int, _vp, _vp, C.c_int64, _vp]),
    "rt_render_sequence": (C.c_int, [_vp, C.POINTER(rt_params), C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int64, C.c_int64, _dp,
                                     C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "rt_film_accumulate": (C.c_int, [_vp, C.POINTER(rt_params), C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, _vp]),
    "rt_film_resolve": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int64, C.POINTER(rt_film_tone), _vp, _vp, C.c_int64, _vp]),
    "rt_render_guides": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int64, _vp]),
    "rt_film_denoise": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int64, _vp, C.c_int64, C.POINTER(rt_denoise), _vp, C.c_int64,
                                  _vp, C.c_int64, _vp]),
    "rt_film_temporal": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp, C.c_int64, C.POINTER(rt_temporal),
                                   _vp, C.c_int64, _vp, _vp]),
    "rt_film_accumulate_moments": (C.c_int, [_vp, C.POINTER(rt_params), C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "rt_film_denoise_variance": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int, C.c_int, C.c_int64, _vp, C.c_int64,
                                           C.POINTER(rt_denoise_variance), _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "rt_film_temporal_moments": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int64, _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp,
                                           C.c_int64, C.POINTER(rt_temporal), _vp, C.c_int64, _vp, C.c_int64, _vp, _vp]),
    "rt_film_denoise_variance_temporal": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int, C.c_int, _vp, C.c_int64,
                                                    C.POINTER(rt_denoise_variance), C.c_double, _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "rt_film_bloom": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int64, C.POINTER(rt_bloom), _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "rt_film_meter": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int, _vp, _vp]),
    "rt_film_meter_solve": (C.c_int, [_vp, _vp, C.POINTER(rt_meter), _vp, _vp]),
    "rt_film_resolve_metered": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int64, C.POINTER(rt_film_tone), _vp, _vp, _vp, C.c_int64, _vp]),
    "rt_render_guides_grid": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, _vp,
                                        C.c_int64, _vp]),
    "rt_film_upsample": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int64, _vp, C.c_int64, _vp, C.c_int64, C.c_int, C.c_int,
                                   C.POINTER(rt_upsample), _vp, C.c_int64, _vp, _vp]),
    "rt_sync": (C.c_int, [_vp]),
    "rt_stream_create": (C.c_int, [_vp, C.POINTER(C.c_void_p)]),
    "rt_stream_destroy": (C.c_int, [_vp, _vp]),
    "rt_stream_sync": (C.c_int, [_vp, _vp]),
    "rt_stream_forget": (C.c_int, [_vp, _vp]),
    "rt_timer_begin": (C.c_int, [_vp, _vp]),
    "rt_timer_end": (C.c_int, [_vp, _vp, C.POINTER(C.c_float)]),
    "rt_get_kernel_info": (C.c_int, [_vp, C.POINTER(rt_kernel_info)]),
    "rt_set_tile_stats": (C.c_int, [_vp, _vp]),
    "rt_get_stats": (C.c_int, [_vp, C.POINTER(rt_stats)]),
    "rt_reset_stats": (C.c_int, [_vp]),
    "rt_host_alloc": (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "rt_host_free": (C.c_int, [_vp, _vp]),
    "rt_malloc": (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "rt_free": (C.c_int, [_vp, _vp]),
    "rt_memcpy_h2d": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "rt_memcpy_d2h": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
}

# Entry points added without a new ABI version: a build of the same version from before them binds without them (tools/ab_bench.py
# times such a build beside this one), and Renderer raises where one is called.
LATER_ENTRIES = ("rt_render_guides", "rt_film_denoise", "rt_film_temporal", "rt_film_accumulate_moments", "rt_film_denoise_variance",
                 "rt_film_temporal_moments", "rt_film_denoise_variance_temporal", "rt_film_bloom", "rt_film_meter", "rt_film_meter_solve",
                 "rt_film_resolve_metered", "rt_render_guides_grid", "rt_film_upsample")

_lib = None


def bind(path):
    """dlopen one build of the library and attach the prototypes (tools/ab_bench.py binds two builds)."""
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          f"(or `make -C python-ray-tracer_amd/csrc`); there is no CPU fallback")
    lib = C.CDLL(path)
    for name, (res, args) in PROTOTYPES.items():
        if name in LATER_ENTRIES and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype, fn.argtypes = res, args
    if lib.rt_abi_version() != RT_ABI_VERSION:
        raise ImportError(f"{path}: ABI version {lib.rt_abi_version()} != {RT_ABI_VERSION}; rebuild")
    return lib


def load():
    """Load libmi355rt.so.  No fallback: a missing or stale library is an error."""
    global _lib
    if _lib is None:
        _lib = bind(SO_PATH)
    return _lib
