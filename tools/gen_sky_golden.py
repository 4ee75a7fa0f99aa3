#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — fixtures of the sky (rt_set_scene_sky; runs only where the reference checkout is, as
oracle/gen_golden.py does; it changes nothing under oracle/).

Everything is tools/gen_lighting_golden.py's, imported: the trace is its lit_trace(), whose miss returns (sky_color(d), the
reference's 404 sentinels) under a sky (python_ray_tracer_amd/scene/sky.py: numpy float64, the arithmetic of include/mi355rt.h;
it imports nothing from the reference).

Writes tests/golden/sky_<case>.npz: the keys of the lighting_*.npz fixtures plus sky (24 doubles), u8_plain (the same pixels
with sky = None: the same lights and materials) and events, the counts of EVENTS over the sampled traces that missed;
sharp_extremes_32_d1 also has sky_b, rgb64_b and u8_b, the same pixels under a second sky.
Before a file is written:
  * with a black sky every sampled trace that misses returns +0.0 three times, what gen_lighting_golden's lit_trace() returns, and
    that pass (white lights, spec = 0) compares every trace with the reference's own trace();
  * at least a quarter of the sampled pixels differ from u8_plain;
  * events_48_d4 has each of EVENTS at least 8 times;
  * the file is no larger than tests/golden/lens_c4_s64_d5_sub32.npz.

Usage:  python tools/gen_sky_golden.py [--only NAME ...] [--jobs 8]
"""
import argparse
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "tools")
for _p in (REPO, TOOLS):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import gen_lighting_golden as gl  # noqa: E402
from python_ray_tracer_amd.scene import sky as S  # noqa: E402
from python_ray_tracer_amd.scene.sky import Sky, sky_color  # noqa: E402

OUT = gl.OUT
EVENTS = ("primary_miss", "reflected_miss", "refracted_miss", "scattered_miss", "below_horizon", "inside_disc",
          "halo_outside_disc", "t_clipped_to_1")
_K = {}


def _init():
    gl._init()


def black(packed):
    """The packed sky with its five colours zero."""
    k = np.array(packed, dtype=np.float64)
    for c in S.COLOURS:
        k[c:c + 3] = 0.0
    return k


def _miss(d):
    """gen_lighting_golden's miss hook: sky(d) as a tuple of float64, and the events of this miss."""
    k, ev = _K["sky"], _K["events"]
    g = sky_color(np.array(d, dtype=np.float64), k)
    if _K["black"] and not np.array_equal(g.view(np.uint64), np.zeros(3, np.uint64)):
        raise RuntimeError(f"a black sky gave {g.tolist()} for d = {d}")
    ev[gl._W["ray"] + "_miss"] += 1
    h = float(d[0]) * k[0] + float(d[1]) * k[1] + float(d[2]) * k[2]
    s = float(d[0]) * k[13] + float(d[1]) * k[14] + float(d[2]) * k[15]
    ev["below_horizon"] += h < 0
    ev["t_clipped_to_1"] += abs(h) > 1
    ev["inside_disc"] += s >= k[16]
    ev["halo_outside_disc"] += 0 < s < k[16]
    return (g[0], g[1], g[2])


def _run(job):
    """gen_lighting_golden._run with the sky (or None) as the job's first element; the event counts are its own."""
    sky, is_black, inner = job
    _K.update(sky=sky, black=is_black, events={e: 0 for e in EVENTS})
    gl._W["miss"] = None if sky is None else _miss
    try:
        rgb64, u8, _ = gl._run(inner)
    finally:
        gl._W["miss"] = None
    return rgb64, u8, np.array([_K["events"][e] for e in EVENTS], dtype=np.int64)


def render_pixels(pool, jobs, mods, *args, **kw):
    """gen_lighting_golden.render_pixels with render(lit, sky): sky a packed sky or None."""
    class Capture:                                  # the pool stand-in that gen_lighting_golden's render() maps its jobs through
        sky, is_black = None, False

        def map(self, fn, inner):
            return pool.map(_run, [(self.sky, self.is_black, j) for j in inner])

    cap = Capture()
    d, render_lit = gl.render_pixels(cap, jobs, mods, *args, **kw)

    def render(lit, sky, is_black=False):
        cap.sky, cap.is_black = (None if sky is None else np.array(sky, dtype=np.float64)), is_black
        return render_lit(lit)

    return d, render


def case(pool, jobs, mods, name, *args, tex, light_rgb, sky, scalars=(0.0, 0.6, 0.3), sky_b=None, **kw):
    t0 = time.time()
    if tex is None:
        tex = gl.no_textures(args[2].shape[1], args[6].shape[1])
    packed = sky.pack() if hasattr(sky, "pack") else S.check_packed(sky)
    d, render = render_pixels(pool, jobs, mods, *args, tex if len(tex[3]) else None, light_rgb, **kw)
    rgb64, u8, ev = render(True, packed)
    _, u8p, _ = render(True, None)
    render(False, black(packed), True)   # every miss +0.0, and every trace of the restatement equal to the reference's trace()
    amb, lamb, refl = scalars
    depth = int(d["depth"])
    d.update(amb=amb, lamb=lamb, refl=refl,
             refl_pow=np.array([np.float64(refl) ** (i + 1) for i in range(max(depth, 1))], dtype=np.float64),
             rgb64=rgb64, u8=u8, u8_plain=u8p, events=np.asarray(ev, dtype=np.int64), sky=packed,
             tex_origin=tex[0], tex_axes=tex[1], tex_dims=tex[2], tex_first=tex[3], sphere_texture=tex[4], plane_texture=tex[5],
             texels=tex[6])
    if sky_b is not None:                # the same scene under a second sky: sky_b, rgb64_b, u8_b
        packed_b = S.check_packed(sky_b.pack() if hasattr(sky_b, "pack") else sky_b)
        rgb64_b, u8_b, _ = render(True, packed_b)
        d.update(sky_b=packed_b, rgb64_b=rgb64_b, u8_b=u8_b)
    differ = int((u8 != u8p).any(axis=1).sum())
    if 4 * differ < len(u8):
        raise SystemExit(f"{name}: only {differ} of {len(u8)} pixels differ from the scene without a sky (a quarter is required)")
    if name == "events_48_d4" and min(ev) < 8:
        raise SystemExit(f"{name}: events {dict(zip(EVENTS, ev.tolist()))} (8 of each are required)")
    path = os.path.join(OUT, f"sky_{name}.npz")
    tmp = path + ".tmp.npz"
    np.savez_compressed(tmp, **d)
    size, limit = os.path.getsize(tmp), os.path.getsize(gl.SIZE_LIMIT_FILE)
    if size > limit:
        os.remove(tmp)
        raise SystemExit(f"{name}: {size} bytes, more than {os.path.basename(gl.SIZE_LIMIT_FILE)} ({limit})")
    os.replace(tmp, path)
    print(f"  wrote {path} ({size / 1024:.0f} KiB, {len(u8)} px, differ from plain {differ}, events {dict(zip(EVENTS, ev.tolist()))}, "
          f"{time.time() - t0:.1f} s)", flush=True)


def scenes(gg, workloads):
    """name -> (positional arguments of render_pixels after mods, up to focus_point; tex or None; light_rgb; sky; keywords)."""
    from gen_scatter_golden import DEFAULT_TABLE, GRID_TABLE, grid_ids
    lit = gl.scenes(gg, workloads)
    L3, P1, P0 = gg.lig(gg.DEFAULT_LIGHTS), gg.pla([gg.DEFAULT_PLANE]), gg.pla([])
    S6 = gg.sph(gg.DEFAULT_SPHERES)
    CAM = ([-2, 0, 2.0], [0, -30, 0])
    Z3 = [0.0, 0.0, 0.0]
    C0 = gg.DEFAULT_SPHERES[0][0]
    WHITE3 = [(1.0, 1.0, 1.0)] * 3
    MIRRORS = [(0.05, 0.7, 0.0), (0.0, 0.5, 0.5), (0.1, 0.6, 0.1), (0.0, 0.3, 0.8)]
    DAY = Sky((40, 90, 200), (170, 200, 230), (60, 55, 50), sharpness=2, sun_direction=(1.0, 0.35, 0.25), sun_angle_deg=4.0,
              sun_color=(255, 240, 200), halo_color=(120, 90, 40), halo_shininess=32)
    DUSK = Sky((20, 20, 70), (240, 120, 60), (30, 20, 20), sharpness=4, sun_direction=(1.0, -0.2, 0.05), sun_angle_deg=3.0,
               sun_color=(255, 200, 120), halo_color=(160, 70, 20), halo_shininess=8)
    out = {}
    # white lights and no spec row: the sky alone makes it a sky scene
    out["default_64_d4"] = ((64, 64, S6, L3, Z3, 1, P1, *CAM, gl.pad8(MIRRORS), [3, 1, 0, 2, 1, 3], [3], 4, 0.0, C0), None, WHITE3,
                            DAY, dict(seed=11))
    a, tex, rgb, kw = lit["aa_48_d2"]
    out["aa_48_d2"] = (a, tex, rgb, DUSK, kw)
    a, tex, rgb, kw = lit["stoch_40x24_spp3_seed7"]
    out["stoch_40x24_spp3_seed7"] = (a, tex, rgb, DAY, kw)
    # events_48_d4: the camera looks along the horizon at the low sun, past glass and rough metal, over a window plane (a pane
    # of glass for a floor: what looks down passes through it and misses below the horizon).  t_clipped_to_1 needs directions
    # within rounding of +-up: |up|^2 is 1 + 9e-7, the most the contract takes, and the glass ball of ior 1.5 above the camera
    # has it at its focal point, 1.5 radii from the centre, so the rays through its middle leave it parallel, along up.
    EV = np.array([(0.0, 0.05, 0.0, 0.9, 1.5, 0.0, 0.0, 1.0),      # 0 glass
                   (0.05, 0.3, 0.8, 0.0, 1.0, 0.6, 0.0, 1.0),      # 1 rough metal
                   (0.0, 0.2, 0.85, 0.0, 1.0, 0.0, 0.0, 1.0),      # 2 mirror
                   (0.0, 0.05, 0.0, 0.85, 1.0, 0.0, 0.0, 1.0),     # 3 the window plane
                   (0.05, 0.7, 0.0, 0.0, 1.0, 0.0, 60.0, 16.0)])   # 4 matte, glossy
    ev_cam = ([-2.0, 0.0, 1.0], [0, 40, 0])
    ball_r = 0.5
    up = np.array([0.0, 0.0, 1.0]) * math.sqrt(1.0 + 9e-7)
    ev_sph = gg.sph([([-2.0, 0.0, 1.0 + 1.5 * ball_r], ball_r, gg.GREY),          # the ball lens above the camera
                     ([1.5, 0.9, 1.0], 0.6, gg.DEFAULT_SPHERES[1][2]), ([1.2, -0.9, 0.8], 0.5, gg.DEFAULT_SPHERES[2][2]),
                     ([2.5, 0.0, 1.6], 0.7, gg.DEFAULT_SPHERES[3][2]), ([0.6, 0.2, 0.45], 0.3, gg.DEFAULT_SPHERES[4][2])])
    ev_sky = np.array(Sky((30, 80, 190), (200, 190, 170), (50, 45, 60), sharpness=8, sun_direction=(1.0, 0.1, 0.12),
                          sun_angle_deg=14.0, sun_color=(255, 230, 180), halo_color=(140, 100, 50), halo_shininess=16).pack())
    ev_sky[S.UP:S.UP + 3] = up
    out["events_48_d4"] = ((48, 48, ev_sph, L3, Z3, 1, P1, *ev_cam, EV, [0, 1, 0, 2, 4], [3], 4, 0.0, C0), None,
                           [(1.0, 0.9, 0.7), (0.5, 0.6, 1.0), (0.6, 0.6, 0.6)], ev_sky, dict(seed=23, fov=120.0))
    a, tex, rgb, kw = lit["everything_48_d4"]
    out["everything_48_d4"] = (a, tex, rgb, DAY, kw)
    # no plane: most rays miss
    out["spheres_only_32_d3"] = ((32, 32, S6, L3, Z3, 1, P0, *CAM, gl.glossy(DEFAULT_TABLE, [0, 90], [1, 32]), range(6), [], 3, 0.0, C0),
                                 None, WHITE3, DUSK, dict(seed=5))
    # sharp 16 with halo_shin 1 and no disc (sun_cos > 1); the same scene under a second sky, sky_b: sharp 1 and halo_shin 1024
    ext = np.array(Sky((10, 60, 220), (250, 250, 250), (90, 60, 30), sharpness=16, sun_direction=(1.0, 0.0, 0.4), sun_angle_deg=1.0,
                       sun_color=(255, 255, 255), halo_color=(80, 60, 20), halo_shininess=1).pack())
    ext[S.SUN_COS] = 1.5
    out["sharp_extremes_32_d1"] = ((32, 32, S6, L3, Z3, 1, P1, *CAM, gl.pad8(MIRRORS), [3, 1, 0, 2, 1, 3], [1], 1, 0.0, C0), None,
                                   WHITE3, ext, dict(seed=19, sky_b=Sky((10, 60, 220), (250, 250, 250), (90, 60, 30), sharpness=1,
                                                                        sun_direction=(1.0, 0.0, 0.4), sun_angle_deg=3.0,
                                                                        sun_color=(200, 200, 200), halo_color=(255, 220, 150),
                                                                        halo_shininess=1024)))
    # (c4 and c5: the lighting fixtures' scenes with the camera raised towards the horizon, so that the frame's top sees the sky; c4
    # under a grey sky, as it is under grey lights, for the size limit)
    a, tex, rgb, kw = lit["c4_s64_d5_sub32"]
    a = a[:8] + ([0, -12, 0],) + a[9:]
    out["c4_s64_d5_sub32"] = (a, tex, rgb, Sky((60, 60, 60), (200, 200, 200), (30, 30, 30), sharpness=2), kw)
    a, tex, rgb, kw = lit["c5_s256_d8_sub96"]
    a = a[:8] + ([0, -12, 0],) + a[9:]
    out["c5_s256_d8_sub96"] = (a, tex, rgb, DAY, kw)
    return out


def main():
    import multiprocessing as mp
    from oracle import gen_golden as gg
    from python_ray_tracer_amd import workloads
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    mods = gg._import_reference()
    with mp.Pool(a.jobs, initializer=_init) as pool:
        for name, (args, tex, light_rgb, sky, kw) in scenes(gg, workloads).items():
            if a.only is None or name in a.only:
                case(pool, a.jobs, mods, name, *args, tex=tex, light_rgb=light_rgb, sky=sky, **kw)


if __name__ == "__main__":
    main()
