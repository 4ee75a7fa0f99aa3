#!/usr/bin/env python3
"""Render a frame with the `Renderer` API and save it as a PNG.

    python examples/render_png.py [--size 1000x1000] [--depth 4] [--aa | --spp N] [--frames 50] [--materials | --glass | --scatter]
                                  [--soft [--shadow-samples 4]] [--dof APERTURE [--focus-on-sphere K]]
                                  [--checker [--texture IMAGE]] [--lights] [--sky] [--out output/render.png]
                                  [--passes N [--exposure E] [--white W] [--gamma2]]
                                  [--denoise [--denoise-levels N]] [--guides PREFIX]
                                  [--denoise-variance [--kappa K]]
                                  [--bloom [STRENGTH] [--bloom-threshold T] [--bloom-levels N]]
                                  [--orbit K --temporal [--orbit-step DEG] [--denoise-variance [--spatial-below L]]]
                                  [--auto-exposure [KEY] [--adapt RATE]]

--materials renders the scene with per-object materials (rt_set_scene_materials): a mirror floor under matte spheres.
--scatter renders rough materials (rt_set_scene_materials_scatter): brushed-metal spheres and a satin floor; with --spp N
(stochastic anti-aliasing, N samples per pixel) the scattered reflections average out.
--soft makes the default scene's lights area lights of radius 0.5 (rt_set_scene_area_lights): soft shadows, --shadow-samples
points per light and trace, over the --materials scene unless --glass or --scatter is given; --spp N averages the penumbrae.
--dof APERTURE gives the camera a thin lens of that radius (rt_set_lens: depth of field), focused on the centre of sphere K
(--focus-on-sphere, default 0), over the --materials scene unless --glass or --scatter is given: that sphere is sharp, the floor
in front of it and behind it blurred.  Use it with --spp 16, which averages the lens samples.
--checker gives the floor a checkerboard of 0.5 x 0.5 squares and sphere 0 a solid checker (rt_set_scene_textures), over the
--materials scene unless --glass or --scatter is given; --texture IMAGE also lays that picture (read with PIL) on the floor in
front of the camera, 2 units wide.  --spp N averages the texel edges.
--lights lights the default scene with one warm light, one cool light and one dim light, and gives it glossy spheres and glass
with a highlight (rt_set_scene_lighting), over the --glass scene unless --scatter is given.
--sky puts the default scene with a mirror floor, two glass spheres and two of brushed metal under a blue gradient with a low sun
and its halo (rt_set_scene_sky), and raises the camera so that the horizon is in the picture; --spp N smooths the sun's edge.
--passes N renders the picture through a Film (rt_film_accumulate, rt_film_resolve): N passes with seeds 1, 2, ..., N summed on the
device, each a frame of the launch the other options describe, and their mean resolved there with --exposure E (default 1),
highlights compressed so that --white W (colour units; default 0: none, values clip at 255) maps to 255, and --gamma2 (a square
root for display).  For example --sky --dof 0.1 --passes 64 --white 400: 64 lens samples per pixel and a sun that is not flat white.

--denoise filters the film's mean before it is resolved (rt_render_guides, rt_film_denoise: an edge-stopping filter guided by
what the pinhole camera hits first), with --denoise-levels N iterations (default 4); without --passes it takes four passes.  For
example --sky --soft --shadow-samples 1 --passes 4 --denoise --white 400.  --guides PREFIX writes the guides as PREFIX_normal.png,
PREFIX_depth.png, PREFIX_albedo.png and PREFIX_id.png.

--denoise-variance filters with the variance-guided denoiser instead (rt_film_accumulate_moments, rt_film_denoise_variance: the film
keeps a sum of squares and every pixel's colour tolerance is --kappa standard deviations of its mean, default the library's), with
--denoise-levels N iterations; without --passes it takes four passes.  For example --sky --soft --shadow-samples 1 --passes 8
--denoise-variance --white 400.

--bloom [STRENGTH] adds glare before the tone curve (rt_film_bloom): the light above --bloom-threshold T (default 255) is blurred at
--bloom-levels N scales (default 6) and STRENGTH of it (default 0.25) is added to the mean, filtered or not; without --passes it takes
four passes.  For example --sky --dof 0.1 --passes 64 --white 400 --bloom: the sun glows instead of ending in a hard-edged white disc.

--orbit K --passes N --temporal renders K camera steps of an orbit about the point the camera looks at (--orbit-step degrees each,
default 2), N passes per step, and carries the film through every move (rt_film_temporal: the previous mean reprojected through
the first-hit guides and blended with the new passes); the last frame is written, filtered when --denoise is given.  For example
--sky --soft --shadow-samples 1 --orbit 8 --passes 4 --temporal --denoise --white 400.  With --denoise-variance in place of --denoise the
film carries its second moment through the moves as well (rt_film_temporal_moments) and the temporal mean is filtered with a colour
tolerance per pixel (rt_film_denoise_variance_temporal): tight where the history survived, wide where the move uncovered something;
pixels whose history is shorter than --spatial-below passes (default the library's) take their variance from their neighbours, so
--passes 1 is enough.  For example --sky --soft --shadow-samples 1 --orbit 8 --passes 1 --temporal --denoise-variance --white 400.

--auto-exposure [KEY] meters the picture on the device (rt_film_meter, rt_film_meter_solve, rt_film_resolve_metered): the median
luminance of what the resolve shows (filtered, bloomed or plain) is mapped to KEY colour units (default 46, 18 % of 255) and
--exposure becomes a compensation on top; without --passes it takes four passes.  With --orbit K the exposure moves --adapt RATE of
the way to each step's own (default 1: it jumps), as an eye adapts; --orbit then also works without --temporal (every step a
fresh film, so with --dof).  For example --sky --dof 0.1 --passes 16 --white 400 --bloom --auto-exposure, and the same with
--orbit 8 --adapt 0.25.

The device writes the interleaved (h, w, 3) image directly (RT_FLAG_U8_HWC | RT_FLAG_U8_RGB) into page-locked host
memory; the frame time is measured with HIP events over `--frames` launches.  For the numba-shaped call the
reference's driver makes, see INTEGRATION.md §1 and tests/test_gpu_parity.py::test_facade_matches_reference_call_shape.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import python_ray_tracer_amd as pkg
from python_ray_tracer_amd import _lib as L
from python_ray_tracer_amd.scene import Scene, Camera, Light, Material, Plane, Sky, Texture
from python_ray_tracer_amd.viewer import convert_array_to_image


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1000x1000")
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--aa", action="store_true", help="the reference's 9-tap anti-aliasing")
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--materials", action="store_true", help="mirror floor, matte spheres (per-object materials)")
    ap.add_argument("--glass", action="store_true",
                    help="two glass spheres (ior 1.5 and 2.4) over the --materials mirror floor (refraction)")
    ap.add_argument("--scatter", action="store_true",
                    help="brushed-metal spheres (roughness 0.1 and 0.3) and a satin floor (roughness 0.2): rough reflections")
    ap.add_argument("--soft", action="store_true", help="area lights of radius 0.5: soft shadows")
    ap.add_argument("--shadow-samples", type=int, default=4, help="--soft: shadow samples per light and trace")
    ap.add_argument("--spp", type=int, default=0, help="stochastic anti-aliasing with this many samples per pixel")
    ap.add_argument("--dof", type=float, default=0.0, metavar="APERTURE", help="depth of field: a thin lens of this radius")
    ap.add_argument("--focus-on-sphere", type=int, default=0, metavar="K", help="--dof: focus on the centre of sphere K")
    ap.add_argument("--checker", action="store_true", help="a checkered floor and a solid checker on sphere 0 (textures)")
    ap.add_argument("--texture", default=None, metavar="IMAGE", help="--checker: also lay this picture on the floor")
    ap.add_argument("--lights", action="store_true", help="a warm, a cool and a dim light; glossy spheres and glass (lighting)")
    ap.add_argument("--sky", action="store_true", help="a blue gradient with a low sun behind a mirror floor, glass and metal (sky)")
    ap.add_argument("--passes", type=int, default=0, metavar="N", help="accumulate N passes (seeds 1..N) in a film and resolve their mean")
    ap.add_argument("--exposure", type=float, default=1.0, help="--passes: the mean is multiplied by this")
    ap.add_argument("--white", type=float, default=0.0, help="--passes: compress highlights so that this value maps to 255 (0: clip)")
    ap.add_argument("--gamma2", action="store_true", help="--passes: square-root display gamma")
    ap.add_argument("--denoise", action="store_true", help="filter the film's mean with the edge-stopping denoiser (four passes unless --passes)")
    ap.add_argument("--denoise-levels", type=int, default=4, metavar="N", help="--denoise: filter iterations, 0..6")
    ap.add_argument("--denoise-variance", action="store_true", help="filter the film's mean with the variance-guided denoiser (four passes unless --passes)")
    ap.add_argument("--kappa", type=float, default=None, metavar="K", help="--denoise-variance: colour tolerance in standard deviations of the mean")
    ap.add_argument("--spatial-below", type=float, default=None, metavar="L",
                    help="--temporal --denoise-variance: pixels with a history shorter than L passes take their variance from their neighbours")
    ap.add_argument("--bloom", type=float, nargs="?", const=0.25, default=None, metavar="STRENGTH",
                    help="glare around what is brighter than --bloom-threshold: this share of its light is spread (four passes unless --passes)")
    ap.add_argument("--bloom-threshold", type=float, default=255.0, metavar="T", help="--bloom: what is brighter than this glows")
    ap.add_argument("--bloom-levels", type=int, default=6, metavar="N", help="--bloom: scales of the blur, 0..8")
    ap.add_argument("--guides", default=None, metavar="PREFIX", help="write the first-hit guides as PREFIX_normal/_depth/_albedo/_id.png")
    ap.add_argument("--orbit", type=int, default=0, metavar="K", help="--temporal: render K camera steps of an orbit and write the last frame")
    ap.add_argument("--orbit-step", type=float, default=2.0, metavar="DEG", help="--orbit: degrees per camera step")
    ap.add_argument("--temporal", action="store_true", help="carry the film through the camera moves of --orbit (temporal accumulation)")
    ap.add_argument("--auto-exposure", type=float, nargs="?", const=46.0, default=None, metavar="KEY",
                    help="meter the picture on the device: its median luminance maps to KEY (four passes unless --passes)")
    ap.add_argument("--adapt", type=float, default=1.0, metavar="RATE", help="--auto-exposure --orbit: the share of the way the exposure moves per step, (0, 1]")
    ap.add_argument("--upsample", type=int, default=1, metavar="R",
                    help="accumulate and filter a film at w/R x h/R and lift it to w x h along full-resolution guides (four passes unless --passes)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "output", "render.png"))
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.lower().split("x"))
    if a.upsample < 1 or w // a.upsample < 2 or h // a.upsample < 2:
        ap.error("--upsample takes a ratio R >= 1 that leaves a low-resolution frame of at least 2 x 2")
    if (a.denoise or a.temporal or a.denoise_variance or a.bloom is not None or a.auto_exposure is not None or a.upsample > 1) and a.passes <= 0:
        a.passes = 4
    if a.denoise_variance and a.denoise:
        ap.error("--denoise-variance stands in place of --denoise")
    if a.denoise_variance and a.passes < 2 and not a.temporal:
        ap.error("--denoise-variance needs at least two passes, or --temporal")
    if a.spatial_below is not None and not (a.temporal and a.denoise_variance):
        ap.error("--spatial-below goes with --temporal --denoise-variance")
    if a.temporal and a.orbit < 1:
        a.orbit = 8
    if a.orbit > 0 and not a.temporal and a.auto_exposure is None:
        ap.error("--orbit renders through --temporal, or with --auto-exposure")
    if a.adapt != 1.0 and a.auto_exposure is None:
        ap.error("--adapt goes with --auto-exposure")
    if a.temporal and a.dof > 0:
        ap.error("--temporal reprojects the pinhole camera's guides: not with --dof")
    euler = [0, -12, 0] if a.sky else [0, -30, 0]                   # --sky: the horizon a third of the way down the picture
    cam = Camera(resolution=(w, h), position=[-2, 0, 2.0], euler=euler)
    with pkg.Renderer(0) as r:
        scene = Scene.default_scene()
        mats = None
        if a.scatter:
            for p in scene.planes:
                p.material = Material(0.0, 0.3, 0.7, roughness=0.2)                  # a satin floor
            scene.spheres[0].material = Material(0.05, 0.3, 0.8, roughness=0.1)     # brushed metal
            scene.spheres[2].material = Material(0.05, 0.3, 0.8, roughness=0.3)
            scene.spheres[4].material = Material(0.0, 0.2, 0.9, roughness=0.05)
            mats = scene.generate_materials(Material(0.05, 0.8, 0.0))
        elif a.materials or a.glass or a.soft or a.dof > 0 or a.checker or a.lights or a.sky:
            for p in scene.planes:
                p.material = Material(0.0, 0.3, 0.8)                # a mirror floor
            if a.glass or a.lights or a.sky:                        # clear glass; ior 2.4 (diamond) shows total internal reflection
                scene.spheres[0].material = Material(0.0, 0.0, 0.0, transparency=0.9, ior=1.5)
                scene.spheres[5].material = Material(0.0, 0.0, 0.0, transparency=0.9, ior=2.4)
            if a.lights:                                            # a highlight on the glass, and two glossy spheres
                scene.spheres[0].material = Material(0.0, 0.0, 0.0, transparency=0.9, ior=1.5, specular=220.0, shininess=256)
                scene.spheres[5].material = Material(0.0, 0.0, 0.0, transparency=0.9, ior=2.4, specular=220.0, shininess=256)
                scene.spheres[1].material = Material(0.05, 0.7, 0.1, specular=160.0, shininess=64)
                scene.spheres[2].material = Material(0.05, 0.7, 0.1, specular=90.0, shininess=8)
            if a.sky:                                               # brushed metal, as --scatter's
                scene.spheres[2].material = Material(0.05, 0.3, 0.8, roughness=0.3)
                scene.spheres[4].material = Material(0.0, 0.2, 0.9, roughness=0.05)
            mats = scene.generate_materials(Material(0.05, 0.8, 0.0))   # matte spheres: no reflection
        colors = None
        if a.lights:                                                # a warm key light, a cool fill, a dim third
            if a.scatter:
                scene.spheres[1].material = Material(0.05, 0.7, 0.1, specular=160.0, shininess=64)
                mats = scene.generate_materials(Material(0.05, 0.8, 0.0))
            for li, (color, intensity) in zip(scene.lights, (((1.0, 0.8, 0.55), 1.3), ((0.5, 0.7, 1.0), 0.7), ((1.0, 1.0, 1.0), 0.25))):
                li.color, li.intensity = color, intensity
            scene.lights = [Light(li.origin, li.radius, li.color, li.intensity) for li in scene.lights]   # (validated)
            colors = scene.get_light_colors()
        if a.sky:                                                   # the sky lights nothing: the scene keeps its three lights
            scene.sky = Sky(zenith=(25, 70, 190), horizon=(190, 215, 240), nadir=(70, 65, 60), sharpness=2,
                            sun_direction=(1.0, 0.25, 0.12), sun_angle_deg=2.5, sun_color=(255, 240, 200),
                            halo_color=(130, 100, 50), halo_shininess=64)
        radii = None
        if a.soft:
            for li in scene.lights:
                li.radius = 0.5
            radii = scene.get_light_radii()
        textures = None
        if a.checker:
            scene.planes[0].texture = Texture.checker((230, 230, 230), (40, 40, 40), 0.5)
            scene.spheres[0].texture = Texture.checker((230, 60, 40), (250, 220, 120), 0.25, solid=True)
            if a.texture:                                       # a poster on a second plane just above the floor: the picture 2 units
                from PIL import Image                           # wide in front of the camera, repeating beyond it
                img = np.asarray(Image.open(a.texture).convert("RGB"), dtype=np.float32)
                hgt = 2.0 * img.shape[0] / img.shape[1]
                poster = Texture.image(img, (1.0 + hgt, 1.0, 0.0), (0.0, -2.0, 0.0), (-hgt, 0.0, 0.0))
                scene.planes.append(Plane([0, 0, 0.001], [0, 0, 1], [125, 125, 125], material=scene.planes[0].material, texture=poster))
                mats = scene.generate_materials(Material(0.05, 0.8, 0.0))
            textures = scene.generate_textures()
        r.set_scene(*scene.generate_scene(), materials=mats, light_radius=radii, shadow_samples=a.shadow_samples, textures=textures,
                    light_rgb=colors, sky=scene.get_sky())
        r.set_camera(cam.position, cam.rotation)
        if a.dof > 0:
            focus = cam.focus_on(scene.spheres[a.focus_on_sphere].origin)
            cam = Camera(resolution=(w, h), position=[-2, 0, 2.0], euler=euler, aperture=a.dof, focus_distance=focus)
            r.set_lens(*cam.lens)
        r.set_raygen(w, h, *cam.raygen())
        lifter = lambda film: None
        if a.upsample > 1:                                      # the film runs on the low grid of the same field of view; the picture stays w x h
            from python_ray_tracer_amd.upsample import Upsampler, hi_raygen
            fw, fh, full_grid = w, h, tuple(cam.raygen())
            w, h = fw // a.upsample, fh // a.upsample
            r.set_raygen(w, h, *hi_raygen(full_grid, fw, fh, w, h))
            lifter = lambda film: Upsampler(film, fw, fh, raygen=full_grid)
        image = r.host_array((h, w, 3), np.uint8)
        flags = L.RT_FLAG_U8_HWC | L.RT_FLAG_U8_RGB
        aa = 2 if a.spp > 0 else a.aa
        p = r.params(0.0, 0.6, 0.3, a.depth, aa, flags=flags, spp=a.spp)
        auto = a.auto_exposure is not None
        meter_kw = dict(key=a.auto_exposure, rate=a.adapt) if auto else {}
        if a.temporal or a.orbit > 0:                           # a film carried through the camera moves of an orbit
            from python_ray_tracer_amd.temporal import orbit
            start = (np.asarray(cam.position, np.float64), np.asarray(cam.rotation, np.float64))
            pivot = start[0] + 4.0 * start[1][:, 0]             # a point the camera looks at
            tone = dict(exposure=a.exposure, white=a.white, gamma=2 if a.gamma2 else 1, flags=flags)
            var_kw = {**({} if a.kappa is None else dict(kappa=a.kappa)), **({} if a.spatial_below is None else dict(spatial_below=a.spatial_below))}
            with pkg.Film(r, moments=a.denoise_variance) as film:
                r.timer_begin()
                for k in range(a.orbit):
                    r.set_camera(*orbit(start, pivot, a.orbit_step * k))
                    if a.temporal:
                        film.next_frame()
                    else:                                       # (--auto-exposure alone: every step a fresh film; the exposure stays)
                        film.clear()
                    p.seed = 1 + k * a.passes
                    film.accumulate(p, a.passes)
                    src = dict(denoised=a.denoise or a.denoise_variance, temporal=a.temporal)
                    if a.temporal:
                        film.temporal()
                    if a.denoise:
                        film.denoise(levels=a.denoise_levels, temporal=a.temporal)
                    if a.denoise_variance:
                        film.denoise(variance=True, temporal=a.temporal, levels=a.denoise_levels, **var_kw)
                    if auto:                                    # every step is metered: the exposure adapts along the orbit
                        if a.bloom is not None:
                            film.bloom(a.bloom_threshold, a.bloom, a.bloom_levels, **src)
                        film.meter(bloom=a.bloom is not None, **src, **meter_kw)
                ms = r.timer_end() / (a.orbit * a.passes)
                if a.bloom is not None and not auto:
                    film.bloom(a.bloom_threshold, a.bloom, a.bloom_levels, **src)
                up = lifter(film)
                if up:                                          # the low-resolution source of that resolve, lifted to the full frame
                    up.upsample(bloom=a.bloom is not None, **src)
                image = (up or film).resolve(bloom=a.bloom is not None, auto_exposure=auto, **src, **tone)[0]
                if up:
                    up.close()
                if auto:
                    print("auto-exposure: exposure {:.6g}, metered luminance {:.6g}, {:.0f} pixels, bin {:.0f}".format(*film.exposure()))
        elif a.passes > 0:                                      # a film: the passes summed and resolved on the device
            with pkg.Film(r, moments=a.denoise_variance) as film:
                film.accumulate(p, a.passes)
                if a.denoise:
                    film.denoise(levels=a.denoise_levels)
                if a.denoise_variance:
                    film.denoise(variance=True, levels=a.denoise_levels, **({} if a.kappa is None else dict(kappa=a.kappa)))
                if a.bloom is not None:                         # the glow of the source that the resolve shows, before the tone curve
                    film.bloom(a.bloom_threshold, a.bloom, a.bloom_levels, denoised=a.denoise or a.denoise_variance)
                if auto:                                        # the exposure of the source that the resolve shows, solved on the device
                    film.meter(denoised=a.denoise or a.denoise_variance, bloom=a.bloom is not None, **meter_kw)
                up = lifter(film)
                if up:
                    up.upsample(denoised=a.denoise or a.denoise_variance, bloom=a.bloom is not None)
                image = (up or film).resolve(exposure=a.exposure, white=a.white, gamma=2 if a.gamma2 else 1, flags=flags,
                                             denoised=a.denoise or a.denoise_variance, bloom=a.bloom is not None, auto_exposure=auto)[0]
                if up:
                    up.close()
                if auto:
                    print("auto-exposure: exposure {:.6g}, metered luminance {:.6g}, {:.0f} pixels, bin {:.0f}".format(*film.exposure()))
                r.timer_begin()
                for _ in range(a.frames):                       # (timed: one more pass into the sum, per pass)
                    film.accumulate(p, 1)
                ms = r.timer_end() / a.frames
        else:
            r.render_into(0.0, 0.6, 0.3, a.depth, aa, image, flags=flags, spp=a.spp)
            dev = r.malloc(3 * w * h)
            for _ in range(3):
                r.render_device(p, 0, w, dev, None, w)
            r.timer_begin()
            for _ in range(a.frames):
                r.render_device(p, 0, w, dev, None, w)
            ms = r.timer_end() / a.frames
            r.free(dev)
        if a.guides:                                            # normal, depth, albedo and id of what the pinhole camera hits first
            from PIL import Image
            with pkg.Film(r) as film:
                g = film.guides()                               # float32 (8, w, h)
            hit = g[7] >= 0
            far = float(g[3][hit].max()) if hit.any() else 1.0
            ids = g[7].astype(np.int64) + 1                     # (0: nothing)
            pictures = {"normal": np.where(hit, (g[0:3] * 0.5 + 0.5) * 255.0, 0.0), "depth": np.where(hit, (1.0 - g[3] / far) * 255.0, 0.0)[None].repeat(3, 0),
                        "albedo": g[4:7], "id": np.stack([(ids * 97) % 256, (ids * 57) % 256, (ids * 181) % 256]) * (ids > 0)}
            os.makedirs(os.path.dirname(os.path.abspath(a.guides)), exist_ok=True)
            for kind, pic in pictures.items():
                Image.fromarray(np.clip(np.rint(pic), 0, 255).astype(np.uint8).transpose(2, 1, 0)).save(f"{a.guides}_{kind}.png")
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        convert_array_to_image(np.array(image)).save(a.out)
        if a.upsample > 1:
            print(f"upsample: the film ran at {w}x{h}, the picture is {fw}x{fh}")
        print(f"{w}x{h} depth {a.depth} aa={a.aa} spp={a.spp} materials={a.materials} glass={a.glass} scatter={a.scatter} soft={a.soft} dof={a.dof} checker={a.checker} lights={a.lights} sky={a.sky} passes={a.passes} denoise={a.denoise} denoise_variance={a.denoise_variance} temporal={a.temporal} orbit={a.orbit}: {ms:.4f} ms per {'pass' if a.passes > 0 else 'frame'} on the device; wrote {a.out}")


if __name__ == "__main__":
    main()
