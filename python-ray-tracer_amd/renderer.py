"""Renderer — thin object wrapper over the C ABI (include/mi355rt.h).  One Renderer = one rt_ctx
= one GPU.  All pixel work happens in libmi355rt.so; this class only marshals arrays."""
import ctypes as C
import itertools
import weakref

import numpy as np

from . import _lib as L


class RenderError(RuntimeError):
    """A C-ABI call returned a non-zero rt_status."""

    def __init__(self, status, message):
        super().__init__(f"{L.STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


def refl_powers(refl, depth):
    """refl ** (i+1) evaluated on the host exactly as the reference does (trace.py:131)."""
    out = np.zeros(L.RT_MAX_DEPTH, dtype=np.float64)
    refl = float(refl)
    for i in range(min(int(depth), L.RT_MAX_DEPTH)):
        out[i] = refl ** (i + 1)
    return out


def _f32(a, rows, name):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[0] != rows:
        raise ValueError(f"{name} must have shape ({rows}, N), got {a.shape}")
    return a


def _vp(d):
    """A device address or stream handle as a C argument: 0 and None are NULL."""
    return C.c_void_p(d) if d else None


def _strides(npx, *strides):
    """Plane strides as ints, a missing one the frame's pixel count."""
    return [npx if v is None else int(v) for v in strides]


def _temporal(prev_origin, prev_rotation, depth_tol, normal_cos, max_history, reserved):
    """An rt_temporal: the camera the history was rendered with and the tap tests' settings."""
    tp = L.rt_temporal()
    tp.prev_origin[:] = [float(v) for v in np.asarray(prev_origin, dtype=np.float64).reshape(3)]
    tp.prev_rotation[:] = [float(v) for v in np.asarray(prev_rotation, dtype=np.float64).reshape(9)]
    tp.depth_tol, tp.normal_cos, tp.max_history = float(depth_tol), float(normal_cos), float(max_history)
    tp.reserved[:] = [int(v) for v in reserved]
    return tp


_serials = itertools.count(1)


class _PinnedBlock:
    """One page-locked allocation of rt_host_alloc.  It lives as long as any numpy view of it does (the view's buffer
    object holds it) and is freed when the last one goes — not when the Renderer that made it closes, whose close() would
    otherwise leave those views pointing at freed memory.  release() frees it at once (no view may be used afterwards)."""

    def __init__(self, lib, ptr):
        self.lib, self.ptr = lib, ptr

    def release(self):
        if self.ptr:
            ptr, self.ptr = self.ptr, 0
            self.lib.rt_host_free(None, C.c_void_p(ptr))     # ctx = NULL: no context needed to free page-locked memory

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def check_lens(aperture, focus_distance):
    """(aperture, focus_distance) as floats, or ValueError: aperture finite and >= 0, focus_distance finite and > 0."""
    a, f = float(aperture), float(focus_distance)
    if not (np.isfinite(a) and a >= 0.0):
        raise ValueError(f"aperture must be finite and >= 0, not {aperture!r}")
    if not (np.isfinite(f) and f > 0.0):
        raise ValueError(f"focus_distance must be finite and > 0, not {focus_distance!r}")
    return a, f


# The frames rt_set_raygen and rt_set_pixel_loc accept (include/mi355rt.h; python-ray-tracer_amd/csrc/rt_geometry.h)
MAX_FRAME_W = 2 ** 31 - 8
MAX_FRAME_H = 2 ** 29 - 32
MAX_FRAME_PIXELS = 2 ** 31


def check_frame(w, h):
    """(w, h) as ints, or ValueError: 1 <= w <= 2^31 - 8, 1 <= h <= 2^29 - 32 and w*h <= 2^31."""
    w, h = int(w), int(h)
    if not (1 <= w <= MAX_FRAME_W and 1 <= h <= MAX_FRAME_H and w * h <= MAX_FRAME_PIXELS):
        raise ValueError(f"frame {w} x {h} out of range: 1 <= w <= 2^31 - 8, 1 <= h <= 2^29 - 32 and w*h <= 2^31")
    return w, h


# The rt_set_scene* entries (include/mi355rt.h; _lib.PROTOTYPES): each takes the leading arguments of the next, up to
# rt_set_scene_sky's 23 (rt_set_scene_materials: those of rt_set_scene_materials_ex without ncols).
_SCENE_ENTRIES = {"rt_set_scene": 8, "rt_set_scene_materials": 13, "rt_set_scene_materials_ex": 13,
                  "rt_set_scene_materials_scatter": 13, "rt_set_scene_area_lights": 15, "rt_set_scene_textures": 21,
                  "rt_set_scene_lighting": 22, "rt_set_scene_sky": 23}


class Renderer:
    def __init__(self, device=0, lib=None):
        self.serial = next(_serials)     # process-unique (id() values are reused after garbage collection)
        self._lib = lib if lib is not None else L.load()
        self._ctx = C.c_void_p()
        st = self._lib.rt_create(C.byref(self._ctx), int(device))
        if st != L.RT_OK:
            raise RenderError(st, self._lib.rt_last_error(None).decode())
        self.device = int(device)
        self.w = self.h = None
        self.camera = self.raygen = None                          # (origin, rotation) and (px, y0, dy, z0, dz) as last set
        self._pinned = weakref.WeakValueDictionary()     # host_array(): data address -> _PinnedBlock (owned by the arrays)
        self.closed = False
        self.generation = {"scene": 0, "camera": 0, "grid": 0}   # bumped by every set_*: caches above this class key on it

    # -- plumbing ---------------------------------------------------------------------------
    def _check(self, st):
        if st != L.RT_OK:
            raise RenderError(st, self._lib.rt_last_error(self._ctx).decode())

    def close(self):
        # (page-locked arrays handed out by host_array() stay valid: each is freed with its last numpy view)
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._lib.rt_destroy(self._ctx)
            self._ctx = C.c_void_p()
        self.closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- inputs -----------------------------------------------------------------------------
    def set_scene(self, spheres, lights, planes, flags=0, materials=None, light_radius=None, shadow_samples=1, textures=None,
                  light_rgb=None, sky=None):
        """float32 (7,S), (3,L), (9,P) as Scene.generate_scene() returns them (scene/scene.py:96-97).
        materials: None (launches shade with their amb, lamb, refl) or (table float64 (M,3) rows amb, lamb, refl,
        sphere_ids int32 (S,), plane_ids int32 (P,)) as Scene.generate_materials() returns them — per-object shading;
        the launches' amb, lamb and refl are then ignored (rt_set_scene_materials).  A table of shape (M,5), rows
        amb, lamb, refl, trans, ior, has transparent materials (rt_set_scene_materials_ex); one of shape (M,6), rows
        amb, lamb, refl, trans, ior, rough, rough ones as well (rt_set_scene_materials_scatter).  The width of a 2-D table
        is its number of columns (the library refuses any but 3, 5 and 6); a 1-D table is read as rows of 3.
        light_radius: None, or float32 (L,) radii as Scene.get_light_radii() returns them; with a radius > 0 the lights are
        area lights with soft shadows, shadow_samples (1..RT_MAX_SHADOW_SAMPLES) points per light and trace
        (rt_set_scene_area_lights).  Area lights need a material table.
        textures: None, or (records, sphere_ids int32 (S,), plane_ids int32 (P,), texels float32 (N,3)) as
        Scene.generate_textures() returns them: records a list of (origin (3,), axes (3,3), (nx, ny, nz), first); an id of -1
        means no texture (rt_set_scene_textures).  Textures need a material table.
        light_rgb: None (every light white, (1, 1, 1)), or float32 (L,3) colours times strengths as Scene.get_light_colors()
        returns them.  A table of shape (M,8), rows amb, lamb, refl, trans, ior, rough, spec, shin, gives materials a
        Blinn-Phong highlight of strength spec (colour units) and exponent shin (1, 2, 4, ..., 1024).  Either goes through
        rt_set_scene_lighting and needs a material table.
        sky: None (a ray that hits nothing is black), or a scene.Sky or its 24 packed float64 as Scene.get_sky() returns them:
        such a ray sees the sky's gradient, sun disc and halo (rt_set_scene_sky).  A sky needs a material table."""
        s, l, p = _f32(spheres, 7, "spheres"), _f32(lights, 3, "lights"), _f32(planes, 9, "planes")
        fp = C.POINTER(C.c_float)
        rad = None
        if light_radius is not None:
            rad = np.ascontiguousarray(light_radius, dtype=np.float32).reshape(-1)
            if rad.shape[0] != l.shape[1]:
                raise ValueError(f"light_radius: {rad.shape[0]} radii for {l.shape[1]} lights")
            if materials is None and not (np.isfinite(rad) & (rad == 0.0)).all():
                raise ValueError("area lights (a light radius > 0) need a material table: pass materials=... "
                                 "(scalar-only shading has no soft shadows)")
            if materials is None:
                rad = None
        if textures is not None and materials is None:
            raise ValueError("textures need a material table: pass materials=...")
        rgb = None
        if light_rgb is not None:
            rgb = np.ascontiguousarray(light_rgb, dtype=np.float32).reshape(-1, 3)
            if rgb.shape[0] != l.shape[1]:
                raise ValueError(f"light_rgb: {rgb.shape[0]} colours for {l.shape[1]} lights")
            if materials is None:
                raise ValueError("light colours need a material table: pass materials=...")
        sk = None
        if sky is not None:
            sk = np.ascontiguousarray(sky.pack() if hasattr(sky, "pack") else sky, dtype=np.float64).reshape(-1)
            if sk.shape[0] != L.RT_SKY_DOUBLES:
                raise ValueError(f"sky: {sk.shape[0]} doubles, a packed sky has {L.RT_SKY_DOUBLES}")
            if materials is None:
                raise ValueError("a sky needs a material table: pass materials=...")
        # every entry's arguments are the leading ones of rt_set_scene_sky's (_SCENE_ENTRIES): marshal those once, then call the
        # entry of the highest feature in use
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        t = si = pi = None
        ncols = 3
        if materials is not None:
            table, sid, pid = materials
            t = np.ascontiguousarray(table, dtype=np.float64)
            ncols = t.shape[1] if t.ndim == 2 else 3
            if ncols == 3:
                t = t.reshape(-1, 3)
            si = np.ascontiguousarray(sid, dtype=np.int32).reshape(-1)
            pi = np.ascontiguousarray(pid, dtype=np.int32).reshape(-1)
            if si.shape[0] != s.shape[1] or pi.shape[0] != p.shape[1]:
                raise ValueError(f"material ids: {si.shape[0]} for {s.shape[1]} spheres, {pi.shape[0]} for {p.shape[1]} planes")
        records, tsid, tpid, texels = textures if textures is not None else (
            [], np.full(s.shape[1], -1, np.int32), np.full(p.shape[1], -1, np.int32), np.zeros((0, 3), np.float32))
        T = len(records)
        recs = (L.rt_texture * max(T, 1))()
        for k, (o, ax, dims, first) in enumerate(records):
            o = np.asarray(o, dtype=np.float64).reshape(3)
            ax = np.asarray(ax, dtype=np.float64).reshape(3, 3)
            for a in range(3):
                recs[k].origin[a] = o[a]
                recs[k].dim[a] = int(dims[a])
                for i in range(3):
                    recs[k].axis[a][i] = ax[a, i]
            recs[k].first = int(first)
        tsi = np.ascontiguousarray(tsid, dtype=np.int32).reshape(-1)
        tpi = np.ascontiguousarray(tpid, dtype=np.int32).reshape(-1)
        if tsi.shape[0] != s.shape[1] or tpi.shape[0] != p.shape[1]:
            raise ValueError(f"texture ids: {tsi.shape[0]} for {s.shape[1]} spheres, {tpi.shape[0]} for {p.shape[1]} planes")
        tx = np.ascontiguousarray(texels, dtype=np.float32).reshape(-1, 3)
        zr = rad if rad is not None else np.zeros(l.shape[1], dtype=np.float32)
        ptr = lambda a, ty: a.ctypes.data_as(ty) if a is not None else None
        args = (self._ctx, s.ctypes.data_as(fp), s.shape[1], l.ctypes.data_as(fp), l.shape[1], p.ctypes.data_as(fp), p.shape[1],
                int(flags), ptr(t, dp), t.shape[0] if t is not None else 0, ncols, ptr(si, ip), ptr(pi, ip),
                zr.ctypes.data_as(fp), int(shadow_samples), recs, T, tsi.ctypes.data_as(ip), tpi.ctypes.data_as(ip),
                tx.ctypes.data_as(fp), tx.shape[0], ptr(rgb, fp), ptr(sk, dp))
        if materials is None:
            entry = "rt_set_scene"
        elif sk is not None:
            entry = "rt_set_scene_sky"
        elif rgb is not None or ncols == 8:
            entry = "rt_set_scene_lighting"
        elif textures is not None:
            entry = "rt_set_scene_textures"
        elif rad is not None:
            entry = "rt_set_scene_area_lights"
        elif ncols not in (3, 5):
            entry = "rt_set_scene_materials_scatter"
        else:
            entry = "rt_set_scene_materials_ex" if ncols == 5 else "rt_set_scene_materials"
        args = args[:_SCENE_ENTRIES[entry]]
        if entry == "rt_set_scene_materials":
            args = args[:10] + args[11:]                     # (the one entry without ncols)
        self._check(getattr(self._lib, entry)(*args))
        self.counts = (s.shape[1], l.shape[1], p.shape[1])
        self.generation["scene"] += 1

    def set_camera(self, origin, rotation):
        """camera_origin (3,), camera_rotation (3,3); forced to float64 (an all-int position list
        would otherwise become int64)."""
        o = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        r = np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
        dp = C.POINTER(C.c_double)
        self._check(self._lib.rt_set_camera(self._ctx, o.ctypes.data_as(dp), r.ctypes.data_as(dp)))
        self.camera = (o.copy(), r.copy())                         # what Film.next_frame remembers as the history's camera
        self.generation["camera"] += 1

    def set_lens(self, aperture, focus_distance):
        """Depth of field (rt_set_lens): a thin lens of radius `aperture` (finite, >= 0; 0 is the pinhole camera) focused at
        `focus_distance` (finite, > 0) along the camera's forward axis, as Camera.lens returns them.  Applies to later launches;
        an aperture > 0 needs a scene with a material table."""
        a, f = check_lens(aperture, focus_distance)
        self._check(self._lib.rt_set_lens(self._ctx, a, f))
        self.generation["camera"] += 1

    def set_raygen(self, w, h, px, y0, dy, z0, dz):
        w, h = check_frame(w, h)
        self._check(self._lib.rt_set_raygen(self._ctx, w, h, float(px), float(y0), float(dy), float(z0), float(dz)))
        self.w, self.h = w, h
        self.raygen = (float(px), float(y0), float(dy), float(z0), float(dz))
        self.generation["grid"] += 1

    def set_pixel_loc(self, pixel_loc):
        a = np.ascontiguousarray(pixel_loc, dtype=np.float64)
        if a.ndim != 3 or a.shape[0] != 3:
            raise ValueError(f"pixel_loc must have shape (3, w, h), got {a.shape}")
        check_frame(a.shape[1], a.shape[2])
        self._check(self._lib.rt_set_pixel_loc(self._ctx, a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[1], a.shape[2]))
        self.w, self.h = a.shape[1], a.shape[2]
        self.raygen = None
        self.generation["grid"] += 1

    def set_grid(self, pixel_loc):
        """Use the closed form when the array carries one (scene.camera.PixelGrid), else upload it."""
        rg = getattr(pixel_loc, "raygen", None)
        if rg is not None:
            self.set_raygen(pixel_loc.shape[1], pixel_loc.shape[2], *rg)
        else:
            self.set_pixel_loc(pixel_loc)

    @staticmethod
    def params(amb, lamb, refl, depth, aa=False, flags=0, refl_pow=None, spp=0, seed=1):
        """aa: False/0 none, True/1 the reference's 9-tap mode, 2 (with spp, seed) stochastic supersampling."""
        p = L.rt_params()
        p.amb, p.lamb = float(amb), float(lamb)
        rp = refl_powers(refl, depth) if refl_pow is None else np.asarray(refl_pow, dtype=np.float64)
        for i in range(min(len(rp), L.RT_MAX_DEPTH)):
            p.refl_pow[i] = float(rp[i])
        p.depth, p.aa_mode, p.flags = int(depth), int(aa), int(flags)
        p.spp, p.seed = int(spp), int(seed) & 0xFFFFFFFF
        return p

    # -- launches ---------------------------------------------------------------------------
    def render(self, amb, lamb, refl, depth, aa=False, *, x0=0, x1=None, u8=True, f32=False, flags=0, refl_pow=None,
               spp=0, seed=1):
        """Synchronous render of columns [x0,x1) into new host arrays of shape (3, x1-x0, h)."""
        x1 = (self.w or 0) if x1 is None else int(x1)
        p = self.params(amb, lamb, refl, depth, aa, flags, refl_pow, spp, seed)
        n = max(x1 - int(x0), 0)     # a bad range still goes to the library, which reports it
        hwc = bool(int(flags) & L.RT_FLAG_U8_HWC)
        out8 = np.empty(((self.h or 0), n, 3) if hwc else (3, n, self.h or 0), np.uint8) if u8 else None
        out32 = np.empty((3, n, self.h or 0), np.float32) if f32 else None
        self._check(self._lib.rt_render(self._ctx, C.byref(p), int(x0), x1,
                                        out8.ctypes.data if u8 else None, out32.ctypes.data if f32 else None))
        return out8, out32

    def render_into(self, amb, lamb, refl, depth, aa, out8, out32=None, *, x0=0, x1=None, flags=0, refl_pow=None, spp=0, seed=1):
        """Synchronous render into caller-provided host arrays (C-contiguous uint8 / float32 of shape (3, x1-x0, h);
        page-locked ones from host_array() make the copy back run at the link's rate)."""
        x1 = (self.w or 0) if x1 is None else int(x1)
        p = self.params(amb, lamb, refl, depth, aa, flags, refl_pow, spp, seed)
        for a, dt in ((out8, np.uint8), (out32, np.float32)):
            if a is not None and (a.dtype != dt or not a.flags["C_CONTIGUOUS"] or a.size != 3 * (x1 - int(x0)) * (self.h or 0)):   # (3,ws,h), or (h,ws,3) with RT_FLAG_U8_HWC
                raise ValueError("output arrays must be C-contiguous uint8 / float32 with 3*(x1-x0)*h elements")
        self._check(self._lib.rt_render(self._ctx, C.byref(p), int(x0), x1,
                                        out8.ctypes.data if out8 is not None else None,
                                        out32.ctypes.data if out32 is not None else None))

    def render_begin(self, slot, amb, lamb, refl, depth, aa, out8, out32=None, *, x0=0, x1=None, flags=0, refl_pow=None, spp=0, seed=1):
        """render_into() without the wait: the frame is queued on `slot` (0 .. RENDER_SLOTS-1) and arrives in the arrays by
        render_end(slot).  Frames on different slots overlap (copy of one, rendering of the next); use page-locked
        arrays (host_array()) — a copy into pageable memory is staged by the runtime on the calling thread."""
        x1 = (self.w or 0) if x1 is None else int(x1)
        p = self.params(amb, lamb, refl, depth, aa, flags, refl_pow, spp, seed)
        for a, dt in ((out8, np.uint8), (out32, np.float32)):
            if a is not None and (a.dtype != dt or not a.flags["C_CONTIGUOUS"] or a.size != 3 * (x1 - int(x0)) * (self.h or 0)):
                raise ValueError("output arrays must be C-contiguous uint8 / float32 with 3*(x1-x0)*h elements")
        self._check(self._lib.rt_render_begin(self._ctx, C.byref(p), int(x0), x1,
                                              out8.ctypes.data if out8 is not None else None,
                                              out32.ctypes.data if out32 is not None else None, int(slot)))

    def render_end(self, slot):
        self._check(self._lib.rt_render_end(self._ctx, int(slot)))

    def host_array(self, shape, dtype):
        """A page-locked (pinned) numpy array owned by the library; give it back with release_host_array()."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = C.c_void_p()
        self._check(self._lib.rt_host_alloc(self._ctx, n, C.byref(ptr)))
        buf = (C.c_uint8 * n).from_address(ptr.value)
        buf._owner = block = _PinnedBlock(self._lib, ptr.value)     # every view of `buf` keeps the allocation alive
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned[arr.ctypes.data] = block
        return arr

    def release_host_array(self, arr):
        """Free the allocation behind `arr` now; neither `arr` nor any other view of it may be used afterwards."""
        block = self._pinned.pop(arr.ctypes.data, None)
        if block is not None:
            block.release()

    def host_arrays(self, want_f32=False, pinned=True):
        """(uint8, float32 or None) output arrays for a full frame, page-locked or plain."""
        shape = (3, self.w, self.h)
        mk = (lambda dt: self.host_array(shape, dt)) if pinned else (lambda dt: np.empty(shape, dt))
        return mk(np.uint8), (mk(np.float32) if want_f32 else None)

    def release_host_arrays(self, arrs):
        for a in arrs:
            if a is not None:
                self.release_host_array(a)

    def render_device(self, params, x0, x1, d_u8=None, d_f32=None, plane_stride=None, stream=None):
        """Asynchronous render into caller-owned device memory (raw addresses, e.g. tensor.data_ptr())."""
        if plane_stride is None:
            plane_stride = (int(x1) - int(x0)) * self.h
        self._check(self._lib.rt_render_device(self._ctx, C.byref(params), int(x0), int(x1),
                                               _vp(d_u8), _vp(d_f32),
                                               int(plane_stride), _vp(stream)))

    def render_sequence(self, params, x0, x1, n, d_u8=None, d_f32=None, plane_stride=None, frame_stride=None, cameras=None,
                        streams=None, frames_per_launch=0):
        """n frames into device memory with ONE call (rt_render_sequence): frame i at d_u8 + i*frame_stride bytes /
        d_f32 + i*frame_stride floats.  cameras=None: n frames of the current camera, `frames_per_launch` of them per launch
        (one launch's frames share a grid), launch g on streams[g % len(streams)].  cameras = float64 (n, 12) array of
        (origin, rotation) rows: one launch per frame, frame i on streams[i % len(streams)]."""
        if plane_stride is None:
            plane_stride = (int(x1) - int(x0)) * self.h
        if frame_stride is None:
            frame_stride = 3 * int(plane_stride)
        cam = None
        if cameras is not None:
            cam = np.ascontiguousarray(cameras, dtype=np.float64).reshape(-1, 12)
            if cam.shape[0] != int(n):
                raise ValueError(f"cameras must hold {n} rows of 12 doubles, got {cam.shape}")
            self.generation["camera"] += 1
        sv = tuple(int(s_) for s_ in streams) if streams else ()
        if getattr(self, "_seq_streams_key", None) != sv:       # the ctypes array of handles is built once per set of streams
            self._seq_streams_key = sv
            self._seq_streams = (C.c_void_p * len(sv))(*sv) if sv else None
        self._check(self._lib.rt_render_sequence(self._ctx, C.byref(params), int(x0), int(x1), int(n),
                                                 _vp(d_u8), _vp(d_f32),
                                                 int(plane_stride), int(frame_stride),
                                                 cam.ctypes.data_as(C.POINTER(C.c_double)) if cam is not None else None,
                                                 self._seq_streams, len(sv), int(frames_per_launch)))

    def film_accumulate(self, params, x0, x1, passes, reset, d_sum, sum_stride=None, stream=None):
        """`passes` frames of `params` with seeds seed, seed + 1, ... added to the float64 (3, x1-x0, h) sum at device address
        d_sum (rt_film_accumulate); reset: start from zero instead of the buffer's content.  Asynchronous.  film.Film owns
        such a sum and counts its passes."""
        if sum_stride is None:
            sum_stride = (int(x1) - int(x0)) * self.h
        self._check(self._lib.rt_film_accumulate(self._ctx, C.byref(params), int(x0), int(x1), int(passes), int(bool(reset)),
                                                 _vp(d_sum), int(sum_stride),
                                                 _vp(stream)))

    def film_resolve(self, d_sum, ws, h, n, d_u8=None, d_f32=None, *, exposure=1.0, white=0.0, gamma=1, flags=0, sum_stride=None,
                     out_stride=None, stream=None):
        """The sum of n passes at d_sum to a uint8 and / or float32 frame in device memory (rt_film_resolve): mean, exposure,
        highlight compression towards `white`, gamma 1 or 2.  Asynchronous."""
        if sum_stride is None:
            sum_stride = int(ws) * int(h)
        if out_stride is None:
            out_stride = int(ws) if int(flags) & L.RT_FLAG_U8_HWC else int(ws) * int(h)
        tone = L.rt_film_tone(float(exposure), float(white), int(gamma), int(flags))
        self._check(self._lib.rt_film_resolve(self._ctx, _vp(d_sum), int(sum_stride), int(ws), int(h), int(n),
                                              C.byref(tone), _vp(d_u8), _vp(d_f32),
                                              int(out_stride), _vp(stream)))

    def _later_entry(self, name):
        fn = getattr(self._lib, name, None)
        if fn is None:
            raise RenderError(L.RT_ERR_STATE, f"this build of the library has no {name}")
        return fn

    def render_guides(self, x0, x1, d_guides, plane_stride=None, stream=None):
        """The first-hit guides of columns [x0, x1) into caller-owned device memory (rt_render_guides): float32
        (RT_GUIDE_PLANES, x1-x0, h), planes normal (3), distance, albedo (3), object id, of the pinhole camera's RT_AA_NONE primary
        ray (a lens is ignored); plane_stride elements between planes.  Asynchronous.  In numpy: denoise.guides_reference."""
        if plane_stride is None:
            plane_stride = (int(x1) - int(x0)) * (self.h or 0)
        self._check(self._later_entry("rt_render_guides")(self._ctx, int(x0), int(x1), _vp(d_guides),
                                                          int(plane_stride), _vp(stream)))

    def film_denoise(self, d_sum, ws, h, n, d_guides, d_out, d_work=None, *, levels=4, normal_shin=32, sigma=0.0, demodulate=1,
                     sum_stride=None, guide_stride=None, out_stride=None, work_stride=None, stream=None, reserved=0):
        """The edge-stopping a-trous filter on the mean of the sum of n passes at d_sum, guided by d_guides, into the float64
        (3, ws, h) buffer d_out (rt_film_denoise); d_work is a second such buffer (None allowed for levels <= 1).  The result is a
        mean: resolve it with film_resolve(..., n=1).  Asynchronous.  In numpy: denoise.denoise_reference."""
        sum_stride, guide_stride, out_stride, work_stride = _strides(int(ws) * int(h), sum_stride, guide_stride, out_stride, work_stride)
        dn = L.rt_denoise(int(levels), int(normal_shin), float(sigma), int(demodulate), int(reserved))
        self._check(self._later_entry("rt_film_denoise")(self._ctx, _vp(d_sum), sum_stride, int(ws), int(h), int(n), _vp(d_guides), guide_stride,
                                                         C.byref(dn), _vp(d_out), out_stride, _vp(d_work), work_stride, _vp(stream)))

    def film_temporal(self, d_sum, n, d_guides, d_hist, d_hist_len, d_hist_guides, prev_origin, prev_rotation, d_out, d_out_len, *,
                      depth_tol, normal_cos, max_history, sum_stride=None, guide_stride=None, hist_stride=None, hist_guide_stride=None,
                      out_stride=None, stream=None, reserved=(0, 0)):
        """Temporal accumulation over the full frame of the current camera and closed-form grid (rt_film_temporal): the history
        (mean d_hist, length plane d_hist_len, guides d_hist_guides, rendered with the camera prev_origin / prev_rotation) is
        reprojected through this frame's guides d_guides and blended with the sum of n passes at d_sum into the float64
        (3, w, h) mean d_out and the float32 (w, h) length plane d_out_len.  The result is a mean: resolve or denoise it with
        n = 1.  Asynchronous.  In numpy: temporal.temporal_reference."""
        strides = _strides(int(self.w or 0) * int(self.h or 0), sum_stride, guide_stride, hist_stride, hist_guide_stride, out_stride)
        tp = _temporal(prev_origin, prev_rotation, depth_tol, normal_cos, max_history, reserved)
        self._check(self._later_entry("rt_film_temporal")(self._ctx, _vp(d_sum), strides[0], int(n), _vp(d_guides), strides[1], _vp(d_hist),
                                                          strides[2], _vp(d_hist_len), _vp(d_hist_guides), strides[3], C.byref(tp),
                                                          _vp(d_out), strides[4], _vp(d_out_len), _vp(stream)))

    def film_accumulate_moments(self, params, x0, x1, passes, reset, d_sum, d_sq, sum_stride=None, sq_stride=None, stream=None):
        """film_accumulate with the sum of the frames' squares added to a second float64 (3, x1-x0, h) buffer at d_sq
        (rt_film_accumulate_moments); d_sum receives the bits film_accumulate would give.  Asynchronous.  In numpy:
        variance.accumulate_moments_reference."""
        sum_stride, sq_stride = _strides((int(x1) - int(x0)) * (self.h or 0), sum_stride, sq_stride)
        self._check(self._later_entry("rt_film_accumulate_moments")(self._ctx, C.byref(params), int(x0), int(x1), int(passes), int(bool(reset)),
                                                                    _vp(d_sum), sum_stride, _vp(d_sq), sq_stride, _vp(stream)))

    def film_denoise_variance(self, d_sum, d_sq, ws, h, n, d_guides, d_out, d_work=None, *, levels=4, normal_shin=32, kappa=1.0, var_floor=0.0,
                              demodulate=1, prefilter=1, sum_stride=None, sq_stride=None, guide_stride=None, out_stride=None, work_stride=None,
                              stream=None):
        """The variance-guided a-trous filter on the mean of n >= 2 passes (sum at d_sum, sum of squares at d_sq), guided by d_guides,
        into the float64 (4, ws, h) buffer d_out: the filtered mean and, in plane 3, its propagated variance
        (rt_film_denoise_variance); d_work is a second such buffer (None allowed for levels == 0).  The result is a mean: resolve
        it with film_resolve(..., n=1).  Asynchronous.  In numpy: variance.denoise_variance_reference."""
        strides = _strides(int(ws) * int(h), sum_stride, sq_stride, guide_stride, out_stride, work_stride)
        dv = L.rt_denoise_variance(int(levels), int(normal_shin), float(kappa), float(var_floor), int(demodulate), int(prefilter))
        self._check(self._later_entry("rt_film_denoise_variance")(self._ctx, _vp(d_sum), strides[0], _vp(d_sq), strides[1], int(ws), int(h), int(n),
                                                                  _vp(d_guides), strides[2], C.byref(dv), _vp(d_out), strides[3], _vp(d_work),
                                                                  strides[4], _vp(stream)))

    def film_temporal_moments(self, d_sum, d_sq, n, d_guides, d_hist, d_hist_sq, d_hist_len, d_hist_guides, prev_origin, prev_rotation, d_out,
                              d_out_sq, d_out_len, *, depth_tol, normal_cos, max_history, sum_stride=None, sq_stride=None, guide_stride=None,
                              hist_stride=None, hist_sq_stride=None, hist_guide_stride=None, out_stride=None, out_sq_stride=None, stream=None,
                              reserved=(0, 0)):
        """film_temporal with the second moment carried beside the mean (rt_film_temporal_moments): d_sq is this frame's sum of squares,
        d_hist_sq the history's mean of squares, d_out_sq receives the new mean of squares, float64 (3, w, h) each; d_out and d_out_len
        receive the bits film_temporal would give.  Asynchronous.  In numpy: temporal.temporal_moments_reference."""
        strides = _strides(int(self.w or 0) * int(self.h or 0), sum_stride, sq_stride, guide_stride, hist_stride, hist_sq_stride,
                           hist_guide_stride, out_stride, out_sq_stride)
        tp = _temporal(prev_origin, prev_rotation, depth_tol, normal_cos, max_history, reserved)
        self._check(self._later_entry("rt_film_temporal_moments")(
            self._ctx, _vp(d_sum), strides[0], _vp(d_sq), strides[1], int(n), _vp(d_guides), strides[2], _vp(d_hist), strides[3], _vp(d_hist_sq),
            strides[4], _vp(d_hist_len), _vp(d_hist_guides), strides[5], C.byref(tp), _vp(d_out), strides[6], _vp(d_out_sq), strides[7],
            _vp(d_out_len), _vp(stream)))

    def film_denoise_variance_temporal(self, d_mean, d_msq, d_len, ws, h, d_guides, d_out, d_work=None, *, levels=4, normal_shin=32, kappa=1.0,
                                       var_floor=0.0, demodulate=1, prefilter=1, spatial_below=0.0, mean_stride=None, msq_stride=None,
                                       guide_stride=None, out_stride=None, work_stride=None, stream=None):
        """The variance-guided filter on a temporal mean (rt_film_denoise_variance_temporal): d_mean, d_msq and d_len are what
        film_temporal_moments wrote (mean, mean of squares, length plane); a pixel shorter than spatial_below passes takes its variance
        from its object's neighbours.  d_out and d_work as film_denoise_variance's.  Asynchronous.  In numpy:
        variance.denoise_variance_temporal_reference."""
        strides = _strides(int(ws) * int(h), mean_stride, msq_stride, guide_stride, out_stride, work_stride)
        dv = L.rt_denoise_variance(int(levels), int(normal_shin), float(kappa), float(var_floor), int(demodulate), int(prefilter))
        self._check(self._later_entry("rt_film_denoise_variance_temporal")(
            self._ctx, _vp(d_mean), strides[0], _vp(d_msq), strides[1], _vp(d_len), int(ws), int(h), _vp(d_guides), strides[2], C.byref(dv),
            float(spatial_below), _vp(d_out), strides[3], _vp(d_work), strides[4], _vp(stream)))

    def film_bloom(self, d_sum, ws, h, n, d_out, d_work=None, *, threshold=255.0, strength=0.25, levels=6, flags=0, sum_stride=None,
                   out_stride=None, work_stride=None, stream=None):
        """Bloom on the mean of the sum of n passes at d_sum (rt_film_bloom): what is brighter than threshold, blurred at `levels`
        scales and times strength, added to the mean in the float64 (3, ws, h) buffer d_out; d_work holds RT_BLOOM_WORK_PLANES
        float64 planes (None allowed for levels == 0).  The result is a mean: resolve it with film_resolve(..., n=1).  Asynchronous.
        In numpy: bloom.bloom_reference."""
        sum_stride, out_stride, work_stride = _strides(int(ws) * int(h), sum_stride, out_stride, work_stride)
        bl = L.rt_bloom(float(threshold), float(strength), int(levels), int(flags))
        self._check(self._later_entry("rt_film_bloom")(self._ctx, _vp(d_sum), sum_stride, int(ws), int(h), int(n), C.byref(bl), _vp(d_out),
                                                       out_stride, _vp(d_work), work_stride, _vp(stream)))

    def film_meter(self, d_sum, ws, h, n, d_hist, *, reset=True, sum_stride=None, stream=None):
        """The luminance histogram of the mean of the sum of n passes at d_sum into the RT_METER_BINS uint64 counts at d_hist
        (rt_film_meter); reset=False adds to the counts that are there.  Asynchronous.  In numpy: meter.histogram_reference."""
        sum_stride, = _strides(int(ws) * int(h), sum_stride)
        self._check(self._later_entry("rt_film_meter")(self._ctx, _vp(d_sum), sum_stride, int(ws), int(h), int(n), 1 if reset else 0, _vp(d_hist),
                                                       _vp(stream)))

    def film_meter_solve(self, d_hist, d_state, *, key=46.0, percentile=0.5, min_exposure=2.0 ** -10, max_exposure=2.0 ** 10, rate=1.0,
                         flags=0, reserved=0, stream=None):
        """The counts at d_hist to an exposure in the RT_METER_STATE_DOUBLES float64 at d_state, which holds the exposure before
        (rt_film_meter_solve): state = (exposure, metered luminance, pixels metered, bin).  Asynchronous.  In numpy:
        meter.solve_reference."""
        mt = L.rt_meter(float(key), float(percentile), float(min_exposure), float(max_exposure), float(rate), int(flags), int(reserved))
        self._check(self._later_entry("rt_film_meter_solve")(self._ctx, _vp(d_hist), C.byref(mt), _vp(d_state), _vp(stream)))

    def film_resolve_metered(self, d_sum, ws, h, n, d_state, d_u8=None, d_f32=None, *, exposure=1.0, white=0.0, gamma=1, flags=0,
                             sum_stride=None, out_stride=None, stream=None):
        """film_resolve with the exposure times the metered one at d_state[0] (rt_film_resolve_metered): `exposure` is the caller's
        compensation.  Asynchronous."""
        sum_stride, = _strides(int(ws) * int(h), sum_stride)
        if out_stride is None:
            out_stride = int(ws) if int(flags) & L.RT_FLAG_U8_HWC else int(ws) * int(h)
        tone = L.rt_film_tone(float(exposure), float(white), int(gamma), int(flags))
        self._check(self._later_entry("rt_film_resolve_metered")(self._ctx, _vp(d_sum), sum_stride, int(ws), int(h), int(n), C.byref(tone),
                                                                 _vp(d_state), _vp(d_u8), _vp(d_f32), int(out_stride), _vp(stream)))

    def render_guides_grid(self, w, h, raygen, x0, x1, d_guides, plane_stride=None, stream=None):
        """render_guides on the closed-form w x h grid raygen = (px, y0, dy, z0, dz) given here instead of the renderer's
        (rt_render_guides_grid): float32 (RT_GUIDE_PLANES, x1-x0, h) of the current scene and camera.  The renderer's own frame and
        grid stay as they are, and so do the dispatch orders measured for its render launches.  Asynchronous."""
        w, h = check_frame(w, h)
        px, y0, dy, z0, dz = (float(v) for v in raygen)
        if plane_stride is None:
            plane_stride = (int(x1) - int(x0)) * h
        self._check(self._later_entry("rt_render_guides_grid")(self._ctx, w, h, px, y0, dy, z0, dz, int(x0), int(x1), _vp(d_guides),
                                                               int(plane_stride), _vp(stream)))

    def film_upsample(self, d_lo, wl, hl, n, d_lo_guides, d_hi_guides, w, h, lo_grid, hi_grid, d_out, d_out_kind=None, *, normal_cos=0.95,
                      demodulate=1, lo_stride=None, lo_guide_stride=None, hi_guide_stride=None, out_stride=None, stream=None, reserved=0):
        """Guided upsampling (rt_film_upsample): the sum of n passes of the wl x hl frame at d_lo (or a mean, with n = 1) lifted along
        the guides of both frames (d_lo_guides, d_hi_guides; lo_grid, hi_grid their closed-form grids) into the float64 (3, w, h)
        buffer d_out; d_out_kind: None, or a float32 (w, h) plane that receives the stage (0, 1, 2) that wrote each pixel.  The
        result is a mean: resolve it with film_resolve(..., n=1).  Asynchronous.  In numpy: upsample.upsample_reference."""
        lo_stride, lo_guide_stride = _strides(int(wl) * int(hl), lo_stride, lo_guide_stride)
        hi_guide_stride, out_stride = _strides(int(w) * int(h), hi_guide_stride, out_stride)
        up = L.rt_upsample()
        up.lo_grid[:] = [float(v) for v in lo_grid]
        up.hi_grid[:] = [float(v) for v in hi_grid]
        up.normal_cos, up.demodulate, up.reserved = float(normal_cos), int(demodulate), int(reserved)
        self._check(self._later_entry("rt_film_upsample")(self._ctx, _vp(d_lo), lo_stride, int(wl), int(hl), int(n), _vp(d_lo_guides),
                                                          lo_guide_stride, _vp(d_hi_guides), hi_guide_stride, int(w), int(h), C.byref(up),
                                                          _vp(d_out), out_stride, _vp(d_out_kind), _vp(stream)))

    def sync(self, stream=None):
        """Wait for the context's stream, or for `stream`(a handle from stream_create / a hipStream_t address)."""
        if stream:
            self._check(self._lib.rt_stream_sync(self._ctx, C.c_void_p(stream)))
        else:
            self._check(self._lib.rt_sync(self._ctx))

    def stream_create(self):
        """An extra stream of this context's device: queue the frames of a sequence alternately on two or more
        streams (each into its own output buffers) and one frame's tail overlaps the next frame's head."""
        s = C.c_void_p()
        self._check(self._lib.rt_stream_create(self._ctx, C.byref(s)))
        return s.value

    def stream_destroy(self, stream):
        if stream and self._ctx.value:
            self._check(self._lib.rt_stream_destroy(self._ctx, C.c_void_p(stream)))

    def stream_forget(self, stream):
        """Before the owner of a foreign stream (e.g. a torch.cuda.Stream) destroys it: wait for it and drop the
        context's reference to its handle."""
        if stream and self._ctx.value:
            self._check(self._lib.rt_stream_forget(self._ctx, C.c_void_p(stream)))

    def timer_begin(self, stream=None):
        self._check(self._lib.rt_timer_begin(self._ctx, _vp(stream)))

    def timer_end(self, stream=None):
        ms = C.c_float()
        self._check(self._lib.rt_timer_end(self._ctx, _vp(stream), C.byref(ms)))
        return ms.value

    def set_tile_stats(self, dptr):
        """Device buffer (uint32 per 8x8 tile) that later launches fill with per-tile wave cycles; None = off."""
        self._check(self._lib.rt_set_tile_stats(self._ctx, _vp(dptr)))

    def stats(self):
        """rt_stats as a dict: launch counters, and the ray counters of RT_FLAG_COUNT_RAYS launches."""
        st = L.rt_stats()
        self._check(self._lib.rt_get_stats(self._ctx, C.byref(st)))
        return {n: (int(getattr(st, n)) if not n.startswith("bounce_") else [int(v) for v in getattr(st, n)]) for n, _ in st._fields_}

    def reset_stats(self):
        self._check(self._lib.rt_reset_stats(self._ctx))

    def kernel_info(self):
        info = L.rt_kernel_info()
        self._check(self._lib.rt_get_kernel_info(self._ctx, C.byref(info)))
        return {n: getattr(info, n) for n, _ in info._fields_ if n != "reserved"}

    # -- raw device memory (used by the cuda facade) ------------------------------------------
    def malloc(self, nbytes):
        p = C.c_void_p()
        self._check(self._lib.rt_malloc(self._ctx, int(nbytes), C.byref(p)))
        return p.value

    def free(self, dptr):
        if dptr and self._ctx.value:
            self._check(self._lib.rt_free(self._ctx, C.c_void_p(dptr)))

    def h2d(self, dptr, host):
        self._check(self._lib.rt_memcpy_h2d(self._ctx, C.c_void_p(dptr), host.ctypes.data, host.nbytes))

    def d2h(self, host, dptr):
        self._check(self._lib.rt_memcpy_d2h(self._ctx, host.ctypes.data, C.c_void_p(dptr), host.nbytes))


def device_count():
    n = C.c_int()
    L.load().rt_device_count(C.byref(n))
    return n.value
