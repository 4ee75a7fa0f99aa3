/*
 * mi355rt.h — C ABI of libmi355rt.so, the MI355X (gfx950) replacement for the per-pixel
 * ray-trace path of peter-seres/python-ray-tracer.
 *
 * The boundary being replaced is the numba kernel launch (reference paths are relative to
 * /root/reference/src):
 *
 *     render[blockspergrid, threadsperblock](pixel_loc, result, camera_origin, camera_rotation,
 *                                            spheres, lights, planes, amb, lamb, refl,
 *                                            refl_depth, aliasing)          main.py:41-42
 *     signature                                                             ray_tracing/kernels.py:7
 *     exported name  `from ray_tracing import render`                       ray_tracing/__init__.py:1
 *
 * plus the data movement around it: `cuda.to_device(...)` x7 (main.py:19-32) and
 * `result.copy_to_host()` (main.py:51).  Each entry point below names the piece of that call it
 * stands for.  Plain pointers and sizes only; no C++ or torch types cross this boundary; no
 * exception crosses it (every function returns an rt_status).
 *
 * Threading: a context is not thread-safe; use one context per host thread / per GPU.
 * Streams: rt_render_device may be called for one context on several streams (frames of a sequence in flight
 * together); the scheduler feedback inside the context is safe under that use.  rt_set_camera, rt_set_lens, rt_set_raygen and
 * rt_set_scene apply to LATER launches only: camera, lens and ray grid travel with every launch by value, and the scene
 * lives in a ring of device buffers — a launch keeps reading the buffer that was current when it was queued, so frames
 * in flight on any stream finish with the scene they were launched with.  rt_set_pixel_loc (the explicit grid of the
 * literal drop-in) rewrites ONE device buffer: it waits for the whole device before it does.
 * The library has no CPU fallback: without a usable HIP device rt_create fails.
 */
#ifndef MI355RT_H
#define MI355RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 7
#define RT_MAX_DEPTH 16      /* entries of rt_params.refl_pow (reflection bounces) */
#define RT_MAX_SPHERES 1024  /* scene limits: the packed scene must fit one workgroup's LDS */
#define RT_MAX_PLANES 64
#define RT_MAX_LIGHTS 64
#define RT_MAX_MATERIALS 256  /* entries of a scene's material table (rt_set_scene_materials) */

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_BAD_ARG = -1,   /* NULL pointer, size out of range, x-range outside the frame ... */
    RT_ERR_HIP = -2,       /* a HIP runtime call failed; see rt_last_error */
    RT_ERR_NO_DEVICE = -3, /* no HIP device / device index out of range */
    RT_ERR_STATE = -4,     /* render called before scene / camera / ray grid were set */
    RT_ERR_ALLOC = -5      /* host or device allocation failed */
} rt_status;

/* aa_mode */
#define RT_AA_NONE 0      /* aliasing=False                                        kernels.py:26 only */
#define RT_AA_REFERENCE 1 /* aliasing=True: the reference's 3x3 half-pixel taps incl. its G/B
                             accumulation order (kernels.py:29-65) on 1<=x<=w-2, 1<=y<=h-2; the
                             frame border, where the reference indexes out of bounds, gets one tap.
                             With the closed-form grid (rt_set_raygen) neighbouring pixels' shared taps are
                             traced once: see RT_FLAG_AA_PER_PIXEL */
#define RT_AA_STOCHASTIC 2 /* build-defined (the reference has no such mode; README "anti aliasing" to-do):
                             rt_params.spp samples per pixel at P + u*dy*y^ + v*dz*z^ with (u,v) in [-1/2,1/2)^2
                             from a counter hash of (x, y, sample, seed) — rt_device.h:jitter(); plain mean of the
                             samples' (R,G,B).  Needs the closed-form ray grid (rt_set_raygen).  Each sample is
                             the reference's sample() (trace.py:115-133) on that direction. */
#define RT_MAX_SPP 64
#define RT_MAX_SHADOW_SAMPLES 16 /* rt_set_scene_area_lights: shadow samples per light and trace */

/* flags */
#define RT_FLAG_TYPED_BIAS 1 /* evaluate BIAS*N of a plane hit (trace.py:82-83) in float64 (numba
                                typing) instead of float32 (NumPy>=2 simulator promotion; default,
                                the variant pinned by the golden vectors) */
#define RT_FLAG_U8_RGB 2     /* store the uint8 frame as (R,G,B); default is the reference's
                                (R,B,G) order (common.py:60-63) */
#define RT_FLAG_U8_HWC 8     /* store the uint8 frame as an image, [y][x][3] interleaved (what viewer/image.py:7-19
                                builds on the host from the (3,w,h) frame); plane_stride is then the row pitch in
                                pixels (x1-x0 for a compact slab); uint8 output only */
#define RT_FLAG_NO_FEEDBACK 4 /* dispatch tiles in plain order; by default a launch dispatches its workgroups
                                longest-first using the per-tile cycles the previous launch of the same
                                geometry recorded (same pixels either way).  Once two consecutive launches
                                have measured the same scene, camera, grid, range, depth and AA mode the
                                order is kept and measuring stops until an rt_set_* call or another
                                range/depth/mode/stream starts it again */

#define RT_FLAG_AA_PER_PIXEL 32 /* RT_AA_REFERENCE: trace all nine taps of every pixel (what the reference does, kernels.py:29-65)
                                  instead of tracing each half-pixel lattice sample once and summing nine per pixel — the
                                  default on the closed-form grid, same bytes, 4 instead of 9 samples per pixel */
#define RT_FLAG_NO_BUNDLES 64 /* use the plain wave-uniform cull where the library would pick the lane-owned traversal (clustered scenes
                                with 161 spheres or more; rt_device.h).  Same pixels; for A/B timing.  (The name dates from round 2's
                                bundle pre-cull, which the flag also switched off; that variant was removed in round 3.) */
#define RT_FLAG_COUNT_RAYS 16 /* run the counting instantiation of the kernel (slower: registers instead of LDS-parked
                                state): adds this launch's ray counts to the context's rt_stats.  Same pixels.
                                Refused (RT_ERR_BAD_ARG) for a scene with materials: the counting instantiations exist
                                for the shading scalars of rt_params only. */

typedef struct rt_ctx rt_ctx;

/* Shader scalars of the launch (main.py:11, kernels.py:7 args amb, lamb, refl, refl_depth, aliasing).
 * refl_pow[i] must hold refl ** (i+1) as the host language evaluates it (trace.py:131). */
typedef struct rt_params {
    double amb;
    double lamb;
    double refl_pow[RT_MAX_DEPTH];
    int32_t depth;   /* refl_depth, 0..RT_MAX_DEPTH */
    int32_t aa_mode; /* RT_AA_* */
    int32_t flags;   /* RT_FLAG_* */
    int32_t spp;     /* RT_AA_STOCHASTIC: samples per pixel, 1..RT_MAX_SPP (ignored otherwise) */
    uint32_t seed;   /* RT_AA_STOCHASTIC: hash seed (and, in every mode, of rt_set_scene_materials_scatter's rough rows and
                        rt_set_scene_area_lights' shadow samples and rt_set_lens' lens samples) */
    int32_t reserved;
} rt_params;

/* Static facts about the compiled kernel (for reports). */
typedef struct rt_kernel_info {
    int32_t vgprs;          /* numRegs of the render kernel */
    int32_t sgprs;
    int32_t lds_static;     /* bytes */
    int32_t max_threads;    /* per workgroup */
    int32_t wave_size;
    int32_t cu_count;
    int32_t clock_khz;
    int32_t reserved;
} rt_kernel_info;

/* What the context has done since rt_create / rt_reset_stats (SURVEY.md §5 "metrics": rays counted).
 * The ray counters are those of launches made with RT_FLAG_COUNT_RAYS, in the reference's terms:
 *   closest_queries = calls of get_intersection for a closest hit (trace.py:53), hits = those that hit,
 *   shadow_traced + shadow_skipped = shadow queries the reference issues (trace.py:92, one per light and hit);
 *   skipped ones are those whose answer the reference discards (Lambert term <= 0, trace.py:101): the kernel does
 *   not trace them.  With RT_AA_REFERENCE the kernel traces every lattice sample once where the reference
 *   re-traces shared taps, so its counts are lower than the reference algorithm's. */
typedef struct rt_stats {
    uint64_t launches;            /* render launches */
    uint64_t frames;              /* frames those launches rendered (rt_render_sequence: several per launch) */
    uint64_t launches_measuring;  /* ... that timed their tiles and rebuilt the dispatch order */
    uint64_t launches_settled;    /* ... that dispatched in a settled (kept) order */
    uint64_t table_builds;        /* cull-table sets built (one per new scene / camera position / depth bound) */
    uint64_t closest_queries;
    uint64_t hits;
    uint64_t shadow_traced;
    uint64_t shadow_skipped;
    /* per bounce b (0 = primary rays): wavefronts that traced it and the lanes of those that carried a ray —
     * bounce_lanes[b] / (64 bounce_waves[b]) is the SIMD lane utilisation of that bounce */
    uint64_t bounce_waves[RT_MAX_DEPTH + 1];
    uint64_t bounce_lanes[RT_MAX_DEPTH + 1];
} rt_stats;

int rt_abi_version(void);

/* Number of HIP devices visible to this process. */
int rt_device_count(int *count);

/* Create / destroy a context bound to one GPU (owns a stream, scene/camera buffers, timing events).
 * Replaces numba's implicit CUDA context creation at first `cuda.to_device` (main.py:19). */
int rt_create(rt_ctx **ctx, int device);
int rt_destroy(rt_ctx *ctx);

/* Message for the last error on this context (or, with ctx == NULL, for a failed rt_create). */
const char *rt_last_error(const rt_ctx *ctx);

/* Scene arrays exactly as Scene.generate_scene() returns them (scene/scene.py:69-97):
 *   spheres float32 (7,S) C-order, rows cx,cy,cz,r,R,G,B     replaces cuda.to_device(spheres_host) main.py:19
 *   lights  float32 (3,L) rows x,y,z                          replaces cuda.to_device(light_host)   main.py:20
 *   planes  float32 (9,P) rows ox,oy,oz,nx,ny,nz,R,G,B        replaces cuda.to_device(planes_host)  main.py:21
 * Any of S, L, P may be 0 (the pointer is then ignored). */
int rt_set_scene(rt_ctx *ctx, const float *spheres, int S, const float *lights, int L,
                 const float *planes, int P, int flags);

/* The same scene with per-object materials (the reference's "more robust way of defining materials", README to-do list).
 *   materials        float64 (M,3) C-order, rows (amb, lamb, refl); finite; 0 <= M <= RT_MAX_MATERIALS
 *   sphere_material  int32 (S,), plane_material int32 (P,): each object's row of the table, in [0, M)
 * A launch on such a scene ignores rt_params.amb, lamb and refl_pow.  Trace k of a sample (k = 0 the primary ray, 1..depth
 * the bounces) that hits an object of material (amb_k, lamb_k, refl_k) is the reference's trace() (trace.py:44-112) with
 * ambient_int = amb_k and lambert_int = lamb_k, and its colour is added with the weight W_k = ((refl_0 * refl_1) * ...) *
 * refl_{k-1} (float64, left to right) in place of reflection_int ** k (trace.py:131); a trace that misses ends the path.
 * With one material (amb, lamb, r) for every object and r = 0, 1 or a power of two the frame is byte-identical to
 * rt_set_scene and the scalars (amb, lamb, r); for other r, r*r*r may differ from the host's r**3 in the last bit.
 * M == 0 is rt_set_scene (the id arrays are then ignored).  Invalid ids, coefficients or NULL arrays: RT_ERR_BAD_ARG, and
 * the previous scene stays current.  Table and ids travel with the scene (see "Streams" above).  RT_FLAG_COUNT_RAYS is
 * refused for such a scene. */
int rt_set_scene_materials(rt_ctx *ctx, const float *spheres, int S, const float *lights, int L,
                           const float *planes, int P, int flags,
                           const double *materials, int M,
                           const int32_t *sphere_material, const int32_t *plane_material);

/* The same with transparent materials (refraction; the reference's README to-do list).  ncols is 3 or 5:
 *   ncols == 3   exactly rt_set_scene_materials.
 *   ncols == 5   materials float64 (M,5) C-order, rows (amb, lamb, refl, trans, ior): trans finite and >= 0, ior finite and
 *                > 0, and a row with trans > 0 must have refl == 0 (one continuation cannot carry both).  A table without a
 *                row trans > 0 is the 3-column table of its first three columns (same kernels, same bytes); only a scene
 *                with a transparent row runs the refraction kernels.
 * A transparent hit (trans > 0) is shaded exactly like an opaque one (ambient, Lambert, full shadows; a sphere hit from the
 * inside with the outward normal N and P + BIAS*N), but the ray continues through the surface instead of being reflected.
 * float64, no fused multiply-add, in this order, with P = o + t*d the unbiased hit point, N the outward normal (trace.py:63-71),
 * BIAS = 0.0002 and linear_comb / normalize of common.py:
 *   c = dot(d, N); c < 0 (entering): eta = 1.0/ior, ci = -c, n = N; otherwise (leaving): eta = ior, ci = c, n = -N.
 *   sphere: k = 1.0 - (eta*eta)*(1.0 - ci*ci).
 *     k >= 0: T = normalize(linear_comb(d, n, eta, eta*ci - sqrt(k))), next origin
 *             linear_comb(linear_comb(P, n, 1.0, -BIAS), T, 1.0, BIAS)   (the far side of the surface);
 *     k < 0 (total internal reflection): R = get_reflection(d, N), next origin
 *             linear_comb(linear_comb(P, n, 1.0, BIAS), R, 1.0, BIAS)    (the incoming side).
 *   plane (a thin sheet, ior ignored): direction d, next origin linear_comb(linear_comb(P, n, 1.0, -BIAS), d, 1.0, BIAS), with
 *     BIAS*N rounded as trace.py:82-83 rounds it (RT_FLAG_TYPED_BIAS applies).
 * Bounce k+1 is weighted with W_{k+1} = W_k * c_k, c_k = trans_k for a transparent hit (total internal reflection included)
 * and refl_k otherwise; a miss ends the path.  Transparent objects cast full shadows.  Invalid input (a bad id, a NULL array,
 * ncols not 3 or 5, a coefficient outside the rules above): RT_ERR_BAD_ARG, and the previous scene stays current.
 * RT_FLAG_COUNT_RAYS is refused for such a scene.  RT_ABI_VERSION is unchanged: callers detect this entry point by its symbol. */
int rt_set_scene_materials_ex(rt_ctx *ctx, const float *spheres, int S, const float *lights, int L,
                              const float *planes, int P, int flags,
                              const double *materials, int M, int ncols,
                              const int32_t *sphere_material, const int32_t *plane_material);

/* The same with rough materials (scatter; the reference's README to-do list).  ncols is 3, 5 or 6:
 *   ncols == 3 or 5   exactly rt_set_scene_materials_ex.
 *   ncols == 6        materials float64 (M,6) C-order, rows (amb, lamb, refl, trans, ior, rough): the rules of ncols == 5, and
 *                     rough finite and in [0, 1]; a row with trans > 0 must have rough == 0 (frosted glass is not supported).
 *                     A table without a row rough > 0 is the 5-column table of its first five columns (same kernels, same
 *                     bytes); only a scene with a rough row runs the scatter kernels.
 * A hit on a rough object (rough > 0) is shaded exactly like any other (ambient, Lambert, shadows; the weights W_k do not
 * change), but for trace b < depth (b = 0: the primary ray) its next ray leaves along the mirror direction R perturbed by
 * rough times a point in the unit ball.  float64, no fused multiply-add, in this order, with R = get_reflection(d, N)
 * (common.py:113-120), N the outward normal, Pt the biased hit point of trace.py:82-83, linear_comb / normalize / dot of
 * common.py and jitter_hash the 32-bit counter hash of rt_params.seed (rt_device.h):
 *   key of a sample (X, Y, s): X, Y on the half-pixel lattice, pixel (x, y) at (2x, 2y) with x the absolute column, the
 *     RT_AA_REFERENCE tap towards neighbour (dx, dy) at (2x+dx, 2y+dy); s the RT_AA_STOCHASTIC sample index, else 0.  (The
 *     lattice path, RT_FLAG_AA_PER_PIXEL, an explicit grid and column slabs give the same bytes.)
 *   candidate j = 0..7, component c = 0..2:  h = jitter_hash(X, Y, ((s*16 + b)*8 + j)*4 + c, seed ^ 0x5CA77E12),
 *     q_c = (double)(h >> 8) * 2^-23 + (2^-24 - 1)   (exact); q is the first candidate with dot(q, q) < 1 (exact).
 *   D = normalize(linear_comb(R, q, 1.0, rough)), or D = R if none of the eight candidates is inside the ball.
 *   sR = dot(R, N), sD = dot(D, N): unless both are > 0 or both < 0 (NaN included) the path ends after this trace, like a
 *     miss (absorption).
 *   next origin linear_comb(Pt, D, 1.0, BIAS), weight W_{k+1} = W_k * refl_k as for a mirror.
 * rt_params.seed is read in every aa_mode for such a scene.  Invalid input (as rt_set_scene_materials_ex, ncols not 3, 5 or
 * 6, rough outside [0, 1] or NaN, a rough transparent row): RT_ERR_BAD_ARG, and the previous scene stays current.
 * RT_FLAG_COUNT_RAYS is refused for such a scene.  RT_ABI_VERSION is unchanged: callers detect this entry point by its symbol. */
int rt_set_scene_materials_scatter(rt_ctx *ctx, const float *spheres, int S, const float *lights, int L,
                                   const float *planes, int P, int flags,
                                   const double *materials, int M, int ncols,
                                   const int32_t *sphere_material, const int32_t *plane_material);

/* The same with area lights: soft shadows from spherical lights with a radius.  light_radius float32 (L,), radius rho_m of
 * light m (finite, >= 0; the (3,L) lights array is unchanged and holds the centres c_m); shadow_samples n, 1..RT_MAX_SHADOW_SAMPLES.
 *   Every rho_m == 0:  exactly rt_set_scene_materials_scatter (the same kernels and bytes, whatever n is).
 *   Some rho_m > 0:    every light is sampled n times per trace, lights of radius 0 included.  For trace b (b = 0: the primary
 *     ray) of sample (X, Y, s) (the key of rt_set_scene_materials_scatter), light m and shadow sample i = 0..n-1:
 *       candidate j = 0..7, component c = 0..2:  h = jitter_hash(X, Y, t, seed ^ 0x50F7117E) with
 *         t = ((((s*32 + b)*64 + m)*16 + i)*8 + j)*4 + c   (injective for s < 64, b <= 16, m < 64, i < 16; below 2^26),
 *         q_c = (double)(h >> 8) * 2^-23 + (2^-24 - 1)   (exact); q is the first candidate with dot(q, q) < 1 (exact).
 *       Q = c_m + rho_m * q, float64 with c_m the float32 centre widened and rho_m the float32 radius widened, no fused
 *         multiply-add; Q = c_m if none of the eight candidates is inside the ball.
 *     Trace b is the reference's trace() (trace.py:44-112) with two changes: its lights array is the L*n points Q in the order
 *     (m, i), m-major, and lambert_int is lamb_b / n (a float64 division, exact for a power-of-two n).  Everything else is as
 *     before: the ambient term, get_vector_to_light(Pt, Q), the shadow query's 0 < t < 999 any-hit (an occluder beyond Q
 *     counts), no query where the Lambert term is <= 0, refraction, scatter and the weights W_k.  Every AA mode, the lattice
 *     path, RT_FLAG_AA_PER_PIXEL, an explicit grid and column slabs give the same bytes.  rt_params.seed is read in every
 *     aa_mode for such a scene.
 *   Soft lights need a material table (M >= 1; ncols 3, 5 or 6, the rules of rt_set_scene_materials_scatter): scalar-only
 *   shading has no area-light kernels.  Invalid input (as rt_set_scene_materials_scatter, a radius > 0 with M == 0, a NULL
 *   light_radius with L > 0, a radius NaN, infinite or < 0, shadow_samples outside 1..RT_MAX_SHADOW_SAMPLES): RT_ERR_BAD_ARG,
 *   and the previous scene stays current.  RT_FLAG_COUNT_RAYS is refused for such a scene.  RT_ABI_VERSION is unchanged:
 *   callers detect this entry point by its symbol. */
int rt_set_scene_area_lights(rt_ctx *ctx, const float *spheres, int S, const float *lights, int L,
                             const float *planes, int P, int flags,
                             const double *materials, int M, int ncols,
                             const int32_t *sphere_material, const int32_t *plane_material,
                             const float *light_radius, int shadow_samples);

/* The same with textures: a hit object's colour looked up at the hit point in a wrapped, nearest-neighbour grid of texels
 * projected along up to three world-space axes (a checkered floor is a 2x2x1 grid, a solid checker 2x2x2, stripes 2x1x1, an
 * image on a plane or projected onto a sphere like a slide W x H x 1).
 *   textures        rt_texture (T,), 0 <= T <= RT_MAX_TEXTURES
 *   sphere_texture  int32 (S,), plane_texture int32 (P,): the object's texture, or -1 for none; a NULL array means all -1
 *   texels          float32 (n_texels, 3) C-order, true (R,G,B), finite; 0 <= n_texels <= RT_MAX_TEXELS.  Texture k owns texels
 *                   first .. first + nx*ny*nz - 1, x fastest, then y, then z; the range must lie inside the array.  Ranges may
 *                   overlap (two textures may share texels).
 * T == 0, or every id -1:  exactly rt_set_scene_area_lights (the same kernels and bytes).  Only a scene with a textured object
 * runs the texture kernels.
 * A trace whose closest hit is an object with texture k uses, in place of the object's colour (RGB_obj, trace.py:65/70) for the
 * ambient term and for every Lambert term of that trace, the texel chosen as follows.  Pt is the unbiased hit point of
 * trace.py:60.  float64, no fused multiply-add, in this order:
 *   for a = 0..2 with dim[a] > 1:
 *       d   = (Pt.x - origin.x, Pt.y - origin.y, Pt.z - origin.z)
 *       g   = ((d.x * axis[a][0]) + (d.y * axis[a][1])) + (d.z * axis[a][2])
 *       f   = floor(g)
 *       i_a = -2^30 if f is NaN or f < -2^30;  2^30 - 1 if f > 2^30 - 1;  else (integer) f
 *       j_a = i_a mod dim[a], Euclidean (0 <= j_a < dim[a])
 *   for an axis with dim[a] == 1:  j_a = 0, and g is not evaluated
 *   texel index = first + (j_2 * ny + j_1) * nx + j_0
 *   colour      = the three float32 of that texel, widened to float64
 * Everything else is unchanged: normals, bias, shadows, refraction, scatter, area lights, the lens, the weights W_k.  A
 * transparent or rough object may be textured.  Every AA mode, the lattice path, RT_FLAG_AA_PER_PIXEL, an explicit grid, column
 * slabs, rt_render, rt_render_begin/end, rt_render_device and rt_render_sequence give the same bytes.
 * Textures need a material table (M >= 1), like area lights and the lens.  Invalid input (as rt_set_scene_area_lights, an id
 * outside [-1, T), a dimension outside 1..RT_MAX_TEXTURE_DIM, reserved != 0, a non-finite origin, axis or texel, a texel range outside the
 * array, T > RT_MAX_TEXTURES, n_texels > RT_MAX_TEXELS, T > 0 with M == 0, NULL where an array is needed): RT_ERR_BAD_ARG, and the
 * previous scene stays current.  Textures and texels travel with the scene (see "Streams" at the top): a frame in flight keeps
 * the textures it was launched with.  Every call uploads its texels again.  RT_FLAG_COUNT_RAYS is refused for such a scene.
 * RT_ABI_VERSION is unchanged: callers detect this entry point by its symbol. */
#define RT_MAX_TEXTURES     64
#define RT_MAX_TEXTURE_DIM  4096
#define RT_MAX_TEXELS       (1 << 22)   /* four 1024 x 1024 images; 64 MB on the device */

typedef struct rt_texture {
    double  origin[3];   /* world point that maps to grid coordinate (0,0,0)        */
    double  axis[3][3];  /* U, V, W: grid cells per world unit along each axis       */
    int32_t dim[3];      /* nx, ny, nz, each 1..RT_MAX_TEXTURE_DIM                   */
    int32_t reserved;    /* 0                                                        */
    int64_t first;       /* index of texel (0,0,0) in the texel array                */
} rt_texture;

int rt_set_scene_textures(rt_ctx *ctx, const float *spheres, int S, const float *lights, int L,
                          const float *planes, int P, int flags,
                          const double *materials, int M, int ncols,
                          const int32_t *sphere_material, const int32_t *plane_material,
                          const float *light_radius, int shadow_samples,
                          const rt_texture *textures, int T,
                          const int32_t *sphere_texture, const int32_t *plane_texture,
                          const float *texels, int64_t n_texels);

/* The same with lighting: a colour and strength per light, and a Blinn-Phong highlight per material.
 *   light_rgb  float32 (L, 3) C-order: e_m = (e_r, e_g, e_b), the colour times the strength of light m; every component finite
 *              and >= 0.  NULL: every light is (1, 1, 1).
 *   ncols      3, 5, 6 or 8.  Rows of 8 are (amb, lamb, refl, trans, ior, rough, spec, shin): spec finite and >= 0, in colour
 *              units (the 0..255 scale of the objects' colours); shin, the Blinn-Phong exponent, one of 1, 2, 4, ..., 1024, so
 *              that the power is log2(shin) exact squarings and no pow() is involved.  Every rule for the first six columns holds.
 * ncols 3, 5 or 6 with light_rgb NULL is exactly rt_set_scene_textures.
 * A scene runs the lighting kernels when some e_m is not bitwise (1, 1, 1) or some table row has spec > 0 (by row, whether or not
 * an object uses it, as the rough and transparent tests).  Every other scene is exactly rt_set_scene_textures': the same kernels
 * and bytes.  In a scene that runs them, trace b adds per light m (and per shadow sample under area lights), float64, no fused
 * multiply-add, in this order; d is the incoming unit direction, N the outward normal, Pt the biased point of trace.py:82-83, col
 * the object's colour or its texel, Ld the unit vector from Pt to light m (to the sample point Q under area lights), n the scene's
 * shadow_samples with area lights and 1 without, lamb_n = lamb / n as before and spec_n = spec / n (a float64 division):
 *   cN = dot(Ld, N)
 *   k  = lamb_n * cN                                                       (trace.py:99)
 *   wantL = k > 0;  wantS = spec > 0 and cN > 0
 *   neither: no shadow query, next light
 *   occluded (the same shadow ray and any-hit rule as before): next light
 *   wantL:  rgb_c = rgb_c + ((k * e_c) * col_c)                            c = r, g, b
 *   wantS:  Hs = (Ld.x + (-d.x), Ld.y + (-d.y), Ld.z + (-d.z));  H = normalize(Hs);  s = dot(N, H)
 *           s > 0:  q = s;  log2(shin) times q = q * q;  a = spec_n * q
 *                   rgb_c = rgb_c + (a * e_c)                              c = r, g, b, after this light's Lambert term
 * A NaN compares false everywhere: Hs == 0 gives s = NaN and no highlight.  (The kernels decide wantS on spec_n > 0.  That differs
 * from spec > 0 only where spec / n underflows to 0, and there the bytes are the same: a = 0 * q is +0, e_c >= 0, and rgb_c, which
 * starts as 0 + amb * col_c, is never -0, so adding a * e_c changes nothing, nor does the shadow query that is not asked.)
 * The highlight has the light's colour, not the
 * texel's.  Everything else is unchanged: ambient, bias, the continuation rays and the weights W_k, the scatter, light and lens
 * hashes, the texel lookup.  A transparent or rough object may have spec > 0.  Every AA mode, the lattice path,
 * RT_FLAG_AA_PER_PIXEL, an explicit grid, column slabs, rt_render, rt_render_begin/end, rt_render_device and rt_render_sequence
 * give the same bytes.
 * Lighting needs a material table (M >= 1).  Invalid input (as rt_set_scene_textures, a light_rgb component that is negative or not
 * finite, a spec that is negative or not finite, a shin that is not one of the eleven values, a coloured light or spec > 0 with
 * M == 0): RT_ERR_BAD_ARG, and the previous scene stays current.  Light colours travel with the scene, as texture records do: a
 * frame in flight keeps the lights it was launched with.  RT_FLAG_COUNT_RAYS is refused for such a scene.  RT_ABI_VERSION is
 * unchanged: callers detect this entry point by its symbol. */
int rt_set_scene_lighting(rt_ctx *ctx, const float *spheres, int S, const float *lights, int L,
                          const float *planes, int P, int flags,
                          const double *materials, int M, int ncols,
                          const int32_t *sphere_material, const int32_t *plane_material,
                          const float *light_radius, int shadow_samples,
                          const rt_texture *textures, int T,
                          const int32_t *sphere_texture, const int32_t *plane_texture,
                          const float *texels, int64_t n_texels,
                          const float *light_rgb);

/* The same with a sky: the colour of a ray that hits nothing, a gradient with a sun disc and a halo around it.
 *   sky   NULL, or RT_SKY_DOUBLES = 24 float64:
 *           0..2    up         unit vector towards the zenith
 *           3..5    zenith     RGB in colour units (the 0..255 scale of the objects' colours)
 *           6..8    horizon    RGB
 *           9..11   nadir      RGB
 *           12      sharp      1, 2, 4, 8 or 16: how fast the gradient leaves the horizon colour
 *           13..15  sun_dir    unit vector towards the sun
 *           16      sun_cos    the disc is where dot(d, sun_dir) >= sun_cos; a value > 1 means no disc
 *           17..19  sun_rgb    colour added inside the disc
 *           20..22  halo_rgb   colour of the glow around the sun
 *           23      halo_shin  1, 2, 4, ..., 1024: the halo's exponent
 * A scene has a sky when sky != NULL and some component of the five colours is not zero.  Every other scene is exactly
 * rt_set_scene_lighting's: the same kernels and bytes.  In a scene with a sky, a trace that is made and finds nothing
 * (get_intersection reports 404, trace.py:56-57) returns sky(d) instead of (0, 0, 0).  It still returns the 404 sentinels for point
 * and direction, so the path ends as before and its colour is weighted like any other trace's: trace 0 sets the sample to sky(d),
 * trace b >= 1 adds W_b * sky(d).  d is the direction the trace was called with: the primary or lens ray, the reflected, refracted
 * or scattered direction, or the straight continuation through a window; it is unit to rounding and is not normalised again.
 * float64, no fused multiply-add, in this order, per channel c (dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z, common.py:35-37):
 *   h   = dot(d, up)
 *   a   = h < 0 ? -h : h;   t = a > 1 ? 1 : a;   far = h < 0 ? nadir : zenith      (h = -0.0 takes zenith with t = 0)
 *   sharp = 2^j, j > 0:     q = 1 - t;  j times q = q * q;  t = 1 - q               (j = 0: t as it is)
 *   g_c = horizon_c + (t * (far_c - horizon_c))
 *   s   = dot(d, sun_dir)
 *   s > 0:          q = s;  log2(halo_shin) times q = q * q;   g_c = g_c + (halo_c * q)
 *   s >= sun_cos:   g_c = g_c + sun_c
 * (far_c - horizon_c is a float64 subtraction; the library forms it once per scene, which gives the same bits.)  There is no
 * pow(), no atan2 and no image lookup.  A uniform sky (zenith == horizon == nadir, black sun and halo) is exactly its colour in
 * every direction.  The sky is seen through glass and in mirrors.  It gives no light: shadow rays, the ambient and Lambert terms
 * and the highlights are unchanged (a caller who wants sunlight adds a light along sun_dir).  A ray that scatter sends through its
 * surface traces nothing, so it adds nothing, as before.  Every AA mode, the lattice path, RT_FLAG_AA_PER_PIXEL, an explicit grid,
 * column slabs, rt_render, rt_render_begin/end, rt_render_device and rt_render_sequence give the same bytes.
 * Invalid input (anything rt_set_scene_lighting refuses, a sky component that is not finite, a negative colour, |up|^2 or
 * |sun_dir|^2 outside 1 +- 1e-6, a sharp or halo_shin that is not one of the listed values, a sky with M == 0): RT_ERR_BAD_ARG, and
 * the previous scene stays current.  The sky travels with the scene: a frame in flight keeps the sky it was launched with.
 * RT_FLAG_COUNT_RAYS is refused for such a scene.  RT_ABI_VERSION is unchanged: callers detect this entry point by its symbol. */
#define RT_SKY_DOUBLES 24
int rt_set_scene_sky(rt_ctx *ctx, const float *spheres, int S, const float *lights, int L,
                     const float *planes, int P, int flags,
                     const double *materials, int M, int ncols,
                     const int32_t *sphere_material, const int32_t *plane_material,
                     const float *light_radius, int shadow_samples,
                     const rt_texture *textures, int T,
                     const int32_t *sphere_texture, const int32_t *plane_texture,
                     const float *texels, int64_t n_texels,
                     const float *light_rgb, const double *sky);

/* camera_origin float64 (3,) and camera_rotation float64 (3,3) C-order   main.py:27-28 */
int rt_set_camera(rt_ctx *ctx, const double origin[3], const double rotation[9]);

/* Depth of field: a thin-lens camera.  aperture a: the lens radius in world units (finite, >= 0); focus_distance f: the distance
 * from cam_o to the plane of sharp focus along the camera's forward axis R e_x (finite, > 0).  Invalid values: RT_ERR_BAD_ARG,
 * and the previous lens stays.  A new context has a = 0.  Like the camera, the lens applies to LATER launches only and travels
 * with every launch by value (frames in flight keep theirs); a changed lens starts dispatch-order measuring again, the same lens
 * again changes nothing.  rt_render_sequence uses the context's lens for every frame (cameras != NULL included).
 *   a == 0:  the pinhole camera, exactly as without this call (the same kernels and bytes, whatever f is).
 *   a > 0:   the primary ray of every sample is a lens ray; shading, bounces, refraction, scatter and shadow rays are unchanged.
 *     float64, no fused multiply-add, in this order, with linear_comb / normalize / vector_difference of common.py, O = cam_o,
 *     R = cam_R and jitter_hash the 32-bit counter hash of rt_params.seed (rt_device.h):
 *       P: the sample's pixel point as without a lens (pixel_loc / the closed-form grid, the RT_AA_REFERENCE midpoint, the
 *         RT_AA_STOCHASTIC jittered point); v = R P with the products and sums of kernels.py:22, before its normalize.
 *       focal point F = linear_comb(O, v, 1.0, f / P.x)  (P.x = px on the closed-form grid; an explicit grid's own first row).
 *       key (X, Y, s): the key of rt_set_scene_materials_scatter (half-pixel lattice, s the stochastic sample index, else 0).
 *       candidate j = 0..7, component c = 0..1:  h = jitter_hash(X, Y, (s*8 + j)*2 + c, seed ^ 0x1E45D0F5),
 *         u_c = (double)(h >> 8) * 2^-23 + (2^-24 - 1)   (exact); u is the first candidate with u_0*u_0 + u_1*u_1 < 1 (exact),
 *         u = (0, 0) if none of the eight is inside the disk.
 *       lens point L = (O + (a*u_0)*ey) + (a*u_1)*ez per component, ey = (R[1], R[4], R[7]) and ez = (R[2], R[5], R[8]) the
 *         images of the camera's y and z axes.
 *       primary ray (L, normalize(vector_difference(L, F))).
 *     Every AA mode, the lattice path, RT_FLAG_AA_PER_PIXEL, an explicit grid and column slabs give the same bytes.
 *     rt_params.seed is read in every aa_mode.  With RT_AA_NONE every pixel gets one lens sample; RT_AA_STOCHASTIC averages.
 *     A lens needs a scene with a material table (M >= 1): a launch with a > 0 on a scene without one fails with RT_ERR_STATE.
 *     RT_FLAG_COUNT_RAYS stays refused (as for every scene with materials).  RT_ABI_VERSION is unchanged: callers detect this
 *     entry point by its symbol. */
int rt_set_lens(rt_ctx *ctx, double aperture, double focus_distance);

/* The pixel grid of Camera.generate_pixel_locations() (scene/camera.py:18-26) in closed form:
 *   pixel_loc[:, x, y] = (px, x*dy + y0, y*dz + z0)      (one multiply, one add, as np.mgrid does)
 * The kernel generates primary rays from this; no (3,w,h) array is read.   replaces main.py:29
 * Frame size (here and in rt_set_pixel_loc): 1 <= w <= 2^31 - 8, 1 <= h <= 2^29 - 32 and w*h <= 2^31, else RT_ERR_BAD_ARG.
 * (The kernel forms a tile's columns x0 + 8 tx + 7, up to w + 6, as a signed 32-bit int; and a dispatch holds at most 2^32 - 1
 * work-items: launches wider than that go out as column slabs, and one column of 8x8 tiles must fit.)  Every such frame renders
 * with every entry point; RT_AA_REFERENCE traces the half-pixel lattice while (2w-1)(2h-1) < 2^31, 2w-1 <= 2^31 - 8 and
 * 2h-1 <= 2^29 - 32, else nine taps per pixel (RT_FLAG_AA_PER_PIXEL): the same bytes. */
int rt_set_raygen(rt_ctx *ctx, int w, int h, double px, double y0, double dy, double z0, double dz);

/* Drop-in alternative: an explicit float64 (3,w,h) C-order pixel_loc array (host pointer), uploaded
 * and read by the kernel as kernels.py:19 does.                          replaces main.py:29 */
int rt_set_pixel_loc(rt_ctx *ctx, const double *pixel_loc, int w, int h);

/* One launch of the render path for frame columns x0 <= x < x1 (x1 - x0 need not be a multiple of
 * the tile size), into HOST buffers; synchronous (includes the D2H copy — main.py:41-42 + :51).
 *   out_u8  : uint8   (3, x1-x0, h) C-order, index [c, x-x0, y]; channel order per flags; or NULL
 *   out_f32 : float32 (3, x1-x0, h) the (R,G,B) handed to clip_color_vector (kernels.py:69),
 *             true channel order, unclamped; or NULL */
int rt_render(rt_ctx *ctx, const rt_params *params, int x0, int x1, uint8_t *out_u8, float *out_f32);
/* (Frames of half a megapixel and more are rendered in four column chunks whose copies to the host overlap the
 * rendering of the chunks behind them; the result is the same bytes.) */

/* Page-locked host memory for rt_render's outputs: the device-to-host copy of a frame then runs at the link's rate
 * (with pageable memory the runtime stages it).  Any host pointer is accepted by rt_render; these are an offer.
 * (The reference's `result.copy_to_host()` allocates its own pageable array, main.py:51.) */
int rt_host_alloc(rt_ctx *ctx, size_t bytes, void **hptr);
int rt_host_free(rt_ctx *ctx, void *hptr);   /* ctx may be NULL: page-locked memory may outlive the context that allocated it */

/* rt_render in two halves, for SEQUENCES of frames into host memory (an animation: main.py:41-51 in a loop).
 * rt_render_begin queues the launch and the copies of one frame on the stream of `slot` (0 <= slot < RT_RENDER_SLOTS)
 * and returns; rt_render_end(slot) returns when everything queued on that slot has arrived in the host buffers.  Frames
 * begun on different slots render and travel side by side — the copy of one frame overlaps the rendering of the next, so
 * with page-locked destinations (rt_host_alloc) a sequence runs at the slower of the two rates instead of their sum.
 * A second frame begun on a slot before its rt_render_end simply queues behind the first.  The camera, the closed-form ray
 * grid and the scene may be changed between two begins (camera and grid travel with the launch by value; the scene of a
 * launch in flight stays in its own buffer of the context's ring, see "Streams" at the top); the host buffers of a slot
 * must stay untouched until its rt_render_end.  Arguments and results as rt_render (same bytes). */
#define RT_RENDER_SLOTS 4
int rt_render_begin(rt_ctx *ctx, const rt_params *params, int x0, int x1, uint8_t *out_u8, float *out_f32, int slot);
int rt_render_end(rt_ctx *ctx, int slot);

/* The same launch into DEVICE buffers, asynchronous on `stream` (a hipStream_t; NULL = the
 * context's own stream).  Element [c, x, y] (x0 <= x < x1) is stored at
 *   base[c * plane_stride + (x - x0) * h + y]
 * so plane_stride = (x1-x0)*h gives a compact slab and, with base pointing at column x0 of a full
 * frame, plane_stride = w*h renders the slab in place.  Either pointer may be NULL. */
int rt_render_device(rt_ctx *ctx, const rt_params *params, int x0, int x1, void *d_u8, void *d_f32,
                     int64_t plane_stride, void *stream);

/* A SEQUENCE of n frames into device buffers with one call (the reference's driver launches frame after frame,
 * main.py:41-47): frame i is stored at d_u8 + i * frame_stride bytes / d_f32 + i * frame_stride floats, each frame laid
 * out as rt_render_device describes (frame_stride >= 3 * plane_stride; for RT_FLAG_U8_HWC >= 3 * row pitch * h).
 *   cameras == NULL: n frames of the context's camera.  They are rendered by launches of `frames_per_launch` frames each
 *     (0 = a default of 8; one launch renders its frames back to back in one grid, so one frame's last workgroups run
 *     beside the next frame's first and the host pays one launch for all of them), launch g on streams[g % n_streams].
 *   cameras != NULL: float64 (n, 12) — origin[3] then rotation[9] per frame (an animation).  One launch per frame, frame i
 *     on streams[i % n_streams]; afterwards the context's camera is the last one.  The dispatch order measured under an
 *     earlier camera is kept and refreshed every few frames (any order renders the same pixels).
 * streams == NULL or n_streams == 0: everything on the context's stream.  Asynchronous like rt_render_device; the same
 * pixels as n calls of it. */
int rt_render_sequence(rt_ctx *ctx, const rt_params *params, int x0, int x1, int n, void *d_u8, void *d_f32,
                       int64_t plane_stride, int64_t frame_stride, const double *cameras, void *const *streams,
                       int n_streams, int frames_per_launch);

/* The film: passes accumulated in device memory and resolved to a frame there (the device half of the reference's "real-time
 * display" to-do item: progressive refinement).  One launch averages at most RT_MAX_SPP samples, and only under RT_AA_STOCHASTIC;
 * a film takes any number of passes in any aa_mode, and its resolve compresses what clip_color would cut off.
 *   d_sum   caller-owned device buffer of float64, true (R,G,B) planes: element [c, x, y] (x0 <= x < x1) at
 *           d_sum[c * sum_stride + (x - x0) * h + y], the addressing of rt_render_device; a full-frame sum (sum_stride = w*h, d_sum
 *           pointing at column x0) can be filled slab by slab in place.
 * rt_film_accumulate: for pass i = 0..passes-1 let f_i be the float32 colours rt_render_device would store for *params with
 * seed = (params->seed + i) mod 2^32, everything else unchanged (every aa_mode; the RT_FLAG_U8_* bits are ignored).  Per element e,
 * float64, in this order:
 *   s = reset ? +0.0 : sum[e];   for i in 0..passes-1:  s = s + (double)f_i[e];   sum[e] = s
 * (reset != 0 does not read the buffer: it may hold anything.)  The library renders the passes with the unchanged render kernels
 * into its own scratch and folds up to four of them into the sum per add kernel; the result does not depend on that grouping.
 * Asynchronous on `stream` (NULL = the context's stream) like rt_render_device; scene, camera, lens and grid are those current
 * at the call.  RT_ERR_BAD_ARG for passes < 1, d_sum NULL, sum_stride < (x1-x0)*h, (x1-x0)*h > RT_FILM_MAX_PIXELS, and whatever
 * rt_render_device refuses (which keeps its status); the sum is then untouched.  Two accumulates into the same sum on different
 * streams are the caller's race; into different sums on different streams they are safe (the scratch is per stream).
 * rt_film_resolve: the sum of n >= 1 passes (the caller keeps n) of a ws x h frame or slab to a frame.  Per pixel and channel c,
 * float64, no fused multiply-add, in this order, with s the sum:
 *   v = (s / (double)n) * exposure
 *   white > 0:   wn = white / 255.0 (once);  x = v / 255.0;
 *                x > 0:  y = (x * (1.0 + x / (wn*wn))) / (1.0 + x);  v = y * 255.0      (x <= 0 or NaN: v unchanged)
 *   gamma == 2:  t = v / 255.0;   t > 0:  v = sqrt(t) * 255.0                           (t <= 0 or NaN: v unchanged)
 *   d_f32: (float)v        d_u8: clip_color(v), the rule of rt_device.h (NaN -> 0, round half to even, clamp)
 * The compression is the extended Reinhard curve per channel: a value equal to white comes out as 255.  (In exact arithmetic; the
 * float64 v is exactly 255.0 for white = 1e-3 and 255 and within two units in the last place of it for every white, so the float32
 * output is exactly 255.0f and the byte 255: white = 1e6 gives v = 254.99999999999997.)  Gamma 2 is a square root: there is
 * no pow(), so the bytes do not depend on a math library (as shin and sharp).  The outputs are laid out as rt_render_device's:
 * planar (3, ws, h) with out_stride between planes, float32 in true (R,G,B) order, uint8 in the reference's (R,B,G) order unless
 * RT_FLAG_U8_RGB; RT_FLAG_U8_HWC stores the uint8 frame as [y][x][3] with out_stride the row pitch in pixels, uint8 only (d_f32
 * must then be NULL, as for rt_render_device).  Either output pointer may be NULL, but not both.
 * With n = 1, exposure 1, white 0 and gamma 1 the float32 output is the pass's float32 frame bit for bit, and the uint8 output is
 * clip_color of that float32 (a colour of -0.0, which no scene renders, comes out as +0.0 + -0.0 = +0.0).  rt_render_device's own uint8 frame clips the float64 colour before it is rounded to float32, so the
 * two may differ by one at a rounding tie (a colour within float32 rounding of k + 0.5).
 * RT_ERR_BAD_ARG for a NULL d_sum or tone, n < 1, exposure not finite or <= 0, white not 0 and not (finite and > 0), gamma not 1
 * or 2, a flag bit other than the two above, ws < 1, h < 1, ws*h > RT_FILM_MAX_PIXELS, sum_stride < ws*h, out_stride < ws*h (with
 * RT_FLAG_U8_HWC: < ws), both outputs NULL.  Asynchronous on `stream`; it needs no scene.
 * RT_ABI_VERSION is unchanged: callers detect these entry points by their symbols. */
#define RT_FILM_MAX_PIXELS (1 << 27)   /* (x1-x0)*h of one film call */

int rt_film_accumulate(rt_ctx *ctx, const rt_params *params, int x0, int x1, int passes, int reset,
                       void *d_sum, int64_t sum_stride, void *stream);

typedef struct rt_film_tone {
    double  exposure;  /* finite, > 0 */
    double  white;     /* 0: no compression; else finite, > 0, colour units: the value that maps to 255 */
    int32_t gamma;     /* 1 or 2 */
    int32_t flags;     /* RT_FLAG_U8_RGB, RT_FLAG_U8_HWC; every other bit must be 0 */
} rt_film_tone;

int rt_film_resolve(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n,
                    const rt_film_tone *tone, void *d_u8, void *d_f32, int64_t out_stride, void *stream);

/* The denoiser: a few passes, then a filter that knows where the geometry's edges are.  Two entry points: the first-hit guides of
 * a frame (also useful on their own, as masks and for compositing), and an edge-stopping a-trous filter on a film's mean.
 * RT_ABI_VERSION is unchanged: callers detect these entry points by their symbols.
 *
 * rt_render_guides: what the pinhole camera sees first.  The output is float32: element [g, x, y] (x0 <= x < x1) is at
 * d_guides[g*plane_stride + (x-x0)*h + y], the addressing of rt_render_device, so a full-frame buffer can be filled slab by slab
 * in place.  The call uses the scene, camera and grid that are current at the call (they travel by value, as in every launch);
 * it needs no rt_params and no material table, and works on scenes set through every rt_set_scene* entry.
 * For pixel (x, y) the ray is the RT_AA_NONE primary ray without a lens: P the pixel point (the closed form of rt_set_raygen or the
 * explicit grid of rt_set_pixel_loc), d = normalize(R P), o = the camera origin.  A lens set with rt_set_lens is ignored: the
 * guides are those of the sharp image.  (t, idx, type) = get_intersection(o, d) (trace.py:7-41), exactly as the render kernels
 * evaluate it: the same query with the same culls, not a second intersection routine.
 *   plane   hit                                      miss (404)
 *   0..2    (float)N                                 +0.0f
 *   3       (float)t                                 +0.0f
 *   4..6    albedo                                   +0.0f
 *   7       object id                                -1.0f
 * N is the float64 normal trace() uses (trace.py:66/71): for a sphere normalize(Pt - c) with Pt = linear_comb(o, d, 1.0, t), for a
 * plane the normalised float32 normal as the render kernels form it.  Albedo is the object's own float32 colour; when the scene
 * has textures and the object's texture id is >= 0 it is the texel the render kernels' first trace would use: the same point Pt
 * and the same texel index (rt_set_scene_textures).  Object id: a sphere has (float)k with k the caller's sphere index, a plane
 * (float)(S + k); ids stay below 2^24, so they are exact in float32.
 * Asynchronous on `stream` (NULL = the context's stream).  RT_ERR_BAD_ARG for a NULL buffer, plane_stride < (x1-x0)*h, and whatever
 * rt_render_device refuses for x0, x1; RT_ERR_STATE without a scene, camera or grid; the buffer is then untouched.
 * What the guides are not: a pixel that shows a mirror or glass carries the mirror's or the glass's own normal, albedo and id, not
 * those of what is seen in or through it, and under a lens the guides stay those of the pinhole image.
 *
 * rt_film_denoise: an edge-stopping a-trous filter on the film's mean.  d_sum is a film sum of n passes of a ws x h frame;
 * d_guides that frame's guides (planes 0..2 and 7 are always read, planes 4..6 when demodulate is set); d_out a float64 buffer of
 * three planes laid out like a sum, which receives the filtered MEAN: the caller tone-maps it with rt_film_resolve and n = 1
 * (filtering happens in linear colour, before compression).  d_work is a second such buffer, owned by the caller (the library
 * allocates nothing); it may be NULL when levels <= 1.  Which of the two holds which level is the library's business; the result
 * always ends in d_out.  d_out and d_work must not overlap d_sum, d_guides or each other: equal pointers are refused, partial
 * overlap is the caller's error.
 * Per pixel p in float64, no fused multiply-add, in this order (x is the slow axis of the layout, so taps at dy are neighbours in
 * memory):
 *   m_0[c][p] = s[c][p] / (double)n
 *   demodulate:  a[c][p] = max((double)albedo_c[p], 1.0);   m_0[c][p] = m_0[c][p] / a[c][p]
 *   levels == 0 (with or without demodulate):  out[c][p] = s[c][p] / (double)n, and nothing else is evaluated
 *   for i = 0 .. levels-1:      step = 1 << i;   q_i = sigma / 2^i  (exact)
 *       W = +0.0; A_c = +0.0
 *       for dx = -2..2 (outer), dy = -2..2 (inner):   q = (p.x + step*dx, p.y + step*dy)
 *           q outside [0,ws) x [0,h):  skip
 *           id[q] != id[p]:            skip
 *           id[p] >= 0:  cn = ((nx_p*nx_q) + (ny_p*ny_q)) + (nz_p*nz_q)   (float32 normals widened to double)
 *                        !(cn > 0):  skip;    log2(normal_shin) times:  cn = cn*cn
 *           id[p] <  0:  cn = 1.0                                          (sky pixels: the colour weight alone)
 *           sigma > 0:   e_c = (m_i[c][q] - m_i[c][p]) / q_i;  d2 = (e_0*e_0 + e_1*e_1) + e_2*e_2;  wc = 1.0 / (1.0 + d2)
 *           else:        wc = 1.0
 *           w = ((k[dx] * k[dy]) * cn) * wc          k = (1/16, 1/4, 3/8, 1/4, 1/16)  (the B3 spline)
 *           W = W + w;   A_c = A_c + w * m_i[c][q]
 *       m_{i+1}[c][p] = A_c / W                       (the centre tap always contributes 9/64, so W > 0)
 *   out[c][p] = demodulate ? m_levels[c][p] * a[c][p] : m_levels[c][p]
 * max(v, 1.0) is v > 1.0 ? v : 1.0.  The colour weight is rational rather than exp(), and the normal weight is squarings rather than
 * pow(): the bytes do not depend on a math library (as shin, sharp and gamma 2).  Sums are assumed finite: a non-finite sum (or
 * guide) gives unspecified values but does not fault.
 * The filter sees only the buffer it is given: taps do not cross a slab's edge, so a multi-rank caller denoises the assembled frame.
 * RT_ERR_BAD_ARG for a NULL d_sum, d_guides, dn or d_out; n < 1; levels outside 0..6; a normal_shin that is not one of the eleven
 * powers of two 1..1024; a sigma that is not 0 and not (finite and > 0); a demodulate that is not 0 or 1; a reserved that is not 0;
 * ws < 1, h < 1 or ws*h > RT_FILM_MAX_PIXELS; any of the four strides < ws*h (work_stride counts when d_work is given);
 * d_work == NULL with levels >= 2; equal buffers.  The outputs are then untouched.  Asynchronous on `stream`; it needs no scene. */
#define RT_GUIDE_PLANES 8

int rt_render_guides(rt_ctx *ctx, int x0, int x1, void *d_guides, int64_t plane_stride, void *stream);

typedef struct rt_denoise {
    int32_t levels;       /* 0..6: filter iterations; iteration i has taps step 2^i apart */
    int32_t normal_shin;  /* 1, 2, 4, ..., 1024: exponent of the normal weight, as log2 exact squarings */
    double  sigma;        /* 0: no colour weight; else finite, > 0, colour units at level 0, halved per level */
    int32_t demodulate;   /* 0 or 1: filter colour / albedo and multiply back */
    int32_t reserved;     /* must be 0 */
} rt_denoise;

int rt_film_denoise(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n,
                    const void *d_guides, int64_t guide_stride, const rt_denoise *dn,
                    void *d_out, int64_t out_stride, void *d_work, int64_t work_stride, void *stream);

/* Temporal accumulation: the film through a camera move.  rt_film_temporal carries the previous frame's mean to where its surfaces
 * are under the current camera, rejects what has become visible, and blends in the new passes.  RT_ABI_VERSION is unchanged:
 * callers detect this entry point by its symbol.
 * The call works on the full w x h frame of the context's current camera (rt_set_camera) and closed-form grid (rt_set_raygen); both
 * travel by value, as in every launch.  d_sum is a film sum of n passes of this frame (float64, 3 planes); d_guides this frame's
 * guides (float32, 8 planes, rt_render_guides); d_hist the previous frame's mean (float64, 3 planes laid out like a sum);
 * d_hist_len one float32 plane of w*h: how many passes each history pixel stands for; d_hist_guides the previous frame's guides;
 * tp->prev_origin and tp->prev_rotation the camera the history was rendered with.  d_out (float64, 3 planes) receives the new mean
 * and d_out_len (float32, w*h) the new length plane: the next call's history, and what rt_film_denoise / rt_film_resolve take with
 * n = 1.  The history frame is assumed to have the same grid and the same, static scene: moving objects are out of scope (a moved
 * object's pixels pass the tests against its old position or fail them by accident).  Mirrors and glass carry their own guides, not
 * those of what is seen in them, and highlights depend on the view: such shading lags behind the camera.
 * Per pixel p = (x, y), e = x*h + y, in float64 without fused multiply-add, in this order; o, R are the current camera, o', R' the
 * previous one, px, y0, dy, z0, dz the grid:
 *   fresh:   out[k][e] = s[k][e] / (double)n   (k = 0..2);   out_len[e] = (float)n
 *   idp = guides[7][e];     idp < 0 (a miss) or max_history == 0:  fresh
 *   P = (px, (double)x*dy + y0, (double)y*dz + z0);  d = normalize(R P) exactly as rt_render_guides forms it;  t = (double)guides[3][e]
 *   Pt_k = o_k + t*d_k;     u_k = Pt_k - o'_k
 *   q_j = (R'[j]*u_0 + R'[3+j]*u_1) + R'[6+j]*u_2      (j = 0..2: R' transposed times u)
 *   !(q_0 > 0):  fresh
 *   r2 = (u_0*u_0 + u_1*u_1) + u_2*u_2;   sc = px / q_0;   fx = (q_1*sc - y0) / dy;   fy = (q_2*sc - z0) / dz
 *   snap:  rx = floor(fx + 0.5);  |fx - rx| <= 2^-20:  fx = rx        (the same for fy)
 *   !(fx > -1 && fx < w && fy > -1 && fy < h):  fresh                 (NaN lands here)
 *   ix = floor(fx); ax = fx - ix;   iy = floor(fy); ay = fy - iy;    W = H_k = Lh = +0.0
 *   for a = 0, 1 (outer), b = 0, 1 (inner):   q = (ix + a, iy + b);   bw = (a ? ax : 1.0 - ax) * (b ? ay : 1.0 - ay)
 *       bw == 0, or q outside [0,w) x [0,h):  skip
 *       hist_guides[7][q] != idp:  skip
 *       tq = (double)hist_guides[3][q];   !(fabs(tq*tq - r2) <= depth_tol * r2):  skip
 *       cn = ((nx_p*nx_q) + (ny_p*ny_q)) + (nz_p*nz_q)   (float32 normals widened; p from guides, q from hist_guides);  !(cn >= normal_cos): skip
 *       lq = (double)hist_len[q];   !(lq > 0):  skip
 *       W = W + bw;   H_k = H_k + bw * hist[k][q];   Lh = Lh + bw * lq
 *   !(W > 0):  fresh
 *   hm_k = H_k / W;   L = Lh / W;   L > max_history:  L = max_history
 *   out[k][e] = (L * hm_k + s[k][e]) / (L + (double)n);      out_len[e] = (float)(L + (double)n)
 * The snap makes a still camera read exactly one history pixel: a still camera gives the running mean and nothing is blurred.  With
 * a large max_history the result is the cumulative mean, with a small one an exponential average.  No sqrt or pow() beyond the
 * normalize the guides already use: the bytes do not depend on a math library.  A non-finite sum, history or guide gives
 * unspecified values but does not fault: every tap index is range-checked before it is read.
 * Taps cross column slabs, so a multi-rank caller reprojects the assembled frame.
 * RT_ERR_BAD_ARG for a NULL buffer or tp; n < 1 or n > 2^24; a stride < w*h; w*h > RT_FILM_MAX_PIXELS; non-finite camera entries
 * (either camera); depth_tol or max_history not finite or < 0; normal_cos outside [-1, 1]; reserved != 0; d_out or d_out_len equal to
 * any input (or to each other).  RT_ERR_STATE without a camera or a grid, with an explicit rt_set_pixel_loc grid, or with a grid
 * whose dy or dz is 0.  The outputs are then untouched.  Asynchronous on `stream`; it needs no scene. */
typedef struct rt_temporal {
    double  prev_origin[3];    /* the camera the history was rendered with */
    double  prev_rotation[9];
    double  depth_tol;         /* finite, >= 0: relative tolerance on the SQUARED distance */
    double  normal_cos;        /* in [-1, 1] */
    double  max_history;       /* finite, >= 0: cap on a pixel's history length, in passes; 0: no history is used */
    int32_t reserved[2];       /* must be 0 */
} rt_temporal;                 /* 128 bytes */

int rt_film_temporal(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, int64_t n,
                     const void *d_guides, int64_t guide_stride,
                     const void *d_hist, int64_t hist_stride, const void *d_hist_len,
                     const void *d_hist_guides, int64_t hist_guide_stride,
                     const rt_temporal *tp,
                     void *d_out, int64_t out_stride, void *d_out_len, void *stream);

/* The variance-guided denoiser: the film keeps a sum of squares beside its sum, and the filter takes every pixel's colour tolerance
 * from the estimated variance of its mean instead of one global sigma, so it fades out by itself as the film converges.
 * RT_ABI_VERSION is unchanged: callers detect these two entry points by their symbols.
 *
 * rt_film_accumulate_moments: rt_film_accumulate with a second buffer.  Everything rt_film_accumulate does stays: the pass seeds,
 * the scratch, the batches of up to four passes, the slab addressing, the status codes; d_sum receives the same bits.  d_sq is a
 * second float64 buffer of three planes with the same addressing (element [c, x, y] at d_sq[c * sq_stride + (x - x0) * h + y]).
 * Per element e, float64, in pass order:
 *   q = reset ? +0.0 : sq[e];  for i: g = (double)f_i[e]; q = q + g*g;  sq[e] = q
 * (the product of two widened float32 values is exact in float64).  RT_ERR_BAD_ARG as rt_film_accumulate, and for d_sq NULL,
 * sq_stride < (x1-x0)*h and d_sq == d_sum; both buffers are then untouched.
 *
 * rt_film_denoise_variance: rt_film_denoise's a-trous filter with a per-pixel colour tolerance.  d_sum and d_sq are a film's sum
 * and sum of squares of n >= 2 passes of a ws x h frame, d_guides that frame's guides.  d_out and d_work are float64 buffers of
 * FOUR planes (RT_DENOISE_VAR_PLANES) laid out like a sum: planes 0..2 receive the filtered MEAN, which rt_film_resolve takes with
 * n = 1 (it reads three planes), plane 3 the propagated variance of that mean.  d_work may be NULL only for levels == 0.  Which of
 * the two holds which level is the library's business; the result always ends in d_out.  The library allocates nothing.  d_out and
 * d_work must not overlap an input or each other: equal pointers are refused, partial overlap is the caller's error.
 * Per pixel p in float64, no fused multiply-add, in this order (k[] is the B3 spline of rt_film_denoise, which is why the tolerance
 * is called kappa):
 *   m_0[c][p] = s[c][p] / (double)n;    r = sq[c][p] / (double)n - m_0[c][p]*m_0[c][p];    r > 0 ? r : 0   (NaN: 0)
 *   var_c = r / (double)(n - 1)                                   (the variance of the MEAN, per channel)
 *   demodulate:  a[c][p] = max((double)albedo_c[p], 1.0);   m_0[c][p] = m_0[c][p] / a[c][p];   var_c = var_c / (a[c][p]*a[c][p])
 *   v_0[p] = (var_0 + var_1) + var_2
 *   levels == 0:  out[c][p] = s[c][p] / (double)n;  out[3][p] = v_0[p] computed WITHOUT demodulation;  nothing else is evaluated
 *   for i = 0 .. levels-1:    step = 1 << i
 *       prefilter:  gw = gv = +0.0;  for dx = -1..1 (outer), dy = -1..1 (inner):  q = (p.x+dx, p.y+dy)   (step 1 at every level)
 *                       q outside the frame, or id[q] != id[p]:  skip
 *                       t = g[dx]*g[dy]   g = (1/4, 1/2, 1/4);    gw = gw + t;   gv = gv + t * v_i[q]
 *                   vp = gv / gw                                   (the centre contributes 1/4, so gw > 0)
 *       else:       vp = v_i[p]
 *       den = (kappa*kappa) * vp + var_floor
 *       W = +0.0; A_c = +0.0; V = +0.0
 *       for dx = -2..2 (outer), dy = -2..2 (inner):   q = (p.x + step*dx, p.y + step*dy)
 *           outside, id, normal test and cn:  exactly the lines of rt_film_denoise
 *           e_c = m_i[c][q] - m_i[c][p];   d2 = (e_0*e_0 + e_1*e_1) + e_2*e_2
 *           den > 0:  wc = 1.0 / (1.0 + d2 / den)        else:  wc = d2 > 0 ? 0.0 : 1.0
 *           w = ((k[dx] * k[dy]) * cn) * wc
 *           W = W + w;   A_c = A_c + w * m_i[c][q];   V = V + (w*w) * v_i[q]
 *       m_{i+1}[c][p] = A_c / W;     v_{i+1}[p] = V / (W*W)
 *   out[c][p] = demodulate ? m_levels[c][p] * a[c][p] : m_levels[c][p];     out[3][p] = v_levels[p]   (filter units)
 * kappa is the colour tolerance in standard deviations of the mean; var_floor is added to the scaled variance, in squared filter
 * units (colour / albedo with demodulate, colour without).  With kappa = 0 and var_floor = 0, or where a pixel's variance is 0 (n
 * identical passes), only taps of exactly the centre's colour are mixed in.  No exp(), no pow(), no sqrt: the bytes do not depend on
 * a math library.  A non-finite sum, sum of squares or guide gives unspecified values but does not fault: every tap index is
 * range-checked before it is read.  Taps do not cross the edge of the buffer, so a multi-rank caller denoises the assembled frame.
 * A temporal mean (rt_film_temporal) has no second moment of its own, and this filter takes a film's own sum and sum of squares only:
 * rt_film_temporal_moments carries a second moment through the history beside the mean, and rt_film_denoise_variance_temporal
 * filters what it wrote (below).
 * RT_ERR_BAD_ARG as rt_film_denoise (NULL d_sum, d_guides, dv or d_out; levels; normal_shin; demodulate; ws, h), and for d_sq NULL;
 * n < 2; a kappa or var_floor that is not finite or is negative; a prefilter that is not 0 or 1; any of the five strides < ws*h
 * (work_stride counts when d_work is given); d_work == NULL with levels >= 1; equal buffers among d_out, d_work and any input.  The
 * outputs are then untouched.  Asynchronous on `stream`; it needs no scene. */
#define RT_DENOISE_VAR_PLANES 4

int rt_film_accumulate_moments(rt_ctx *ctx, const rt_params *params, int x0, int x1, int passes, int reset,
                               void *d_sum, int64_t sum_stride, void *d_sq, int64_t sq_stride, void *stream);

typedef struct rt_denoise_variance {
    int32_t levels;       /* 0..6 */
    int32_t normal_shin;  /* 1, 2, 4, ..., 1024 */
    double  kappa;        /* finite, >= 0: colour tolerance in standard deviations of the mean */
    double  var_floor;    /* finite, >= 0: added to the scaled variance, in squared filter units */
    int32_t demodulate;   /* 0 or 1 */
    int32_t prefilter;    /* 0 or 1: 3x3 smoothing of the variance before it is used */
} rt_denoise_variance;    /* 32 bytes */

int rt_film_denoise_variance(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, const void *d_sq, int64_t sq_stride,
                             int ws, int h, int64_t n, const void *d_guides, int64_t guide_stride,
                             const rt_denoise_variance *dv, void *d_out, int64_t out_stride,
                             void *d_work, int64_t work_stride, void *stream);

/* The two together: a second moment carried through the history, and the variance-guided filter on the temporal mean, so that a moving
 * camera's frame of 1 to 4 passes gets a colour tolerance per pixel (tight where the history survived, wide at a disocclusion) instead
 * of one global sigma.  RT_ABI_VERSION is unchanged: callers detect these two entry points by their symbols.
 *
 * rt_film_temporal_moments: rt_film_temporal with three more buffers.  Every line of rt_film_temporal holds, in the same order; d_out
 * and d_out_len receive the same bits as rt_film_temporal on the same inputs.  d_sq is the frame's sum of squares
 * (rt_film_accumulate_moments); d_hist_sq the history's MEAN of squares (float64, 3 planes); d_out_sq receives the new mean of squares:
 * the next call's d_hist_sq.  Per pixel, float64, no fused multiply-add:
 *   fresh:                         out_sq[k][e] = sq[k][e] / (double)n
 *   in the tap loop, after H_k:    Q_k = Q_k + bw * hist_sq[k][q]
 *   after hm_k:                    hq_k = Q_k / W
 *                                  out_sq[k][e] = (L * hq_k + sq[k][e]) / (L + (double)n)
 * With max_history == 0 it writes sum / n, sq / n and the length n.  Every error rt_film_temporal raises, with the same statuses;
 * RT_ERR_BAD_ARG for a NULL d_sq, d_hist_sq or d_out_sq, for sq_stride, hist_sq_stride or out_sq_stride < w*h, and for d_out_sq equal
 * to any other buffer (d_out or d_out_len equal to d_sq or d_hist_sq is refused as well).  The outputs are then untouched. */
int rt_film_temporal_moments(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, const void *d_sq, int64_t sq_stride, int64_t n,
                             const void *d_guides, int64_t guide_stride,
                             const void *d_hist, int64_t hist_stride, const void *d_hist_sq, int64_t hist_sq_stride, const void *d_hist_len,
                             const void *d_hist_guides, int64_t hist_guide_stride, const rt_temporal *tp,
                             void *d_out, int64_t out_stride, void *d_out_sq, int64_t out_sq_stride, void *d_out_len, void *stream);

/* rt_film_denoise_variance_temporal: rt_film_denoise_variance on what rt_film_temporal_moments wrote.  d_mean is the mean (float64, 3
 * planes), d_msq the mean of squares (3 planes), d_len the per-pixel length (float32, one plane of ws*h).  Only the prepare pass
 * differs: the levels, the plan of which buffer gets which write, d_out and d_work (four planes each) are rt_film_denoise_variance's.
 * Per pixel p, float64, no fused multiply-add, in this order:
 *   Lp = (double)len[p];   m_c = mean[c][p]
 *   Lp >= spatial_below  (own):
 *       r_c = msq[c][p] - m_c*m_c;  r_c > 0 ? r_c : 0 (NaN: 0)
 *       Lp > 1:  var_c = r_c / (Lp - 1.0)        else:  var_c = 0
 *   else  (pooled; a NaN length lands here):
 *       SL = M_c = Q_c = +0.0
 *       for dx = -2..2 (outer), dy = -2..2 (inner), step 1:   q = (p.x+dx, p.y+dy)
 *           q outside the frame, or id[q] != id[p]:  skip
 *           lq = (double)len[q];   !(lq > 0):  skip
 *           SL = SL + lq;   M_c = M_c + lq * mean[c][q];   Q_c = Q_c + lq * msq[c][q]
 *       !(SL > 1) or !(Lp > 0):  var_c = 0
 *       else:  pm = M_c / SL;   r_c = Q_c / SL - pm*pm  (clamped as above);   var_c = (r_c / (SL - 1.0)) * (SL / Lp)
 *   demodulate, v_0, levels == 0 (out = mean, out[3] = v_0 without demodulation), the levels and the output:
 *       exactly rt_film_denoise_variance's lines
 * The pooled path is for a disocclusion: a pixel with 1 to 3 passes has no usable variance of its own, so it takes the spread of its
 * object's neighbours, weighted by how many passes each stands for, scaled from "one sample" to "a mean of Lp samples".  The own path
 * makes a frame of fresh pixels (len == (float)n, mean == s/n, msq == sq/n) rt_film_denoise_variance's filter bit for bit: then
 * Lp - 1.0 == (double)(n - 1).  spatial_below = 0 pools nowhere.
 * RT_ERR_BAD_ARG as rt_film_denoise_variance (no n exists), and for a NULL d_msq or d_len; a spatial_below that is not finite or is
 * negative; a stride < ws*h; equal buffers among d_out, d_work and any input.  The outputs are then untouched.  Every index is
 * range-checked before it is read: non-finite inputs give unspecified values and do not fault.  Asynchronous on `stream`. */
int rt_film_denoise_variance_temporal(rt_ctx *ctx, const void *d_mean, int64_t mean_stride, const void *d_msq, int64_t msq_stride,
                                      const void *d_len, int ws, int h, const void *d_guides, int64_t guide_stride,
                                      const rt_denoise_variance *dv, double spatial_below,
                                      void *d_out, int64_t out_stride, void *d_work, int64_t work_stride, void *stream);

/* Bloom: glare around what is brighter than white.  After rt_film_resolve's tone curve a sun of 5000 colour units and a wall of
 * 400 are the same white; rt_film_bloom spreads a share of the light above a threshold into its neighbourhood, in linear colour,
 * before the curve.  RT_ABI_VERSION is unchanged: callers detect this entry point by its symbol.
 *
 * rt_film_bloom: d_sum is a film sum of n passes of a ws x h frame or slab: three float64 planes, element [c, x, y] at
 * c*sum_stride + x*h + y, like every film buffer; with n = 1 it is a mean, what rt_film_denoise* or rt_film_temporal* wrote (a
 * four-plane buffer is fine: only planes 0..2 are read).  d_out, three float64 planes, receives the mean plus the glow: the caller
 * tone-maps it with rt_film_resolve and n = 1.  d_work is the caller's and holds RT_BLOOM_WORK_PLANES float64 planes of work_stride
 * (the library allocates nothing); it may be NULL when levels == 0.  Which work planes hold what at which level is the library's
 * business.  d_out and d_work must not overlap d_sum or each other: equal pointers are refused, partial overlap is the caller's
 * error.
 * Per pixel p = (x, y) and channel c in float64, no fused multiply-add, in this order:
 *   m_c = s[c][p] / (double)n;      out[c][p] = m_c
 *   levels == 0:  nothing else is evaluated
 *   mx = m_0 > m_1 ? m_0 : m_1;   mx = mx > m_2 ? mx : m_2
 *   mx > threshold:  g = (mx - threshold) / mx;   b_0[c][p] = m_c > 0 ? m_c * g : +0.0        else:  b_0[c][p] = +0.0
 *   wl = strength / (double)levels   (once)
 *   for i = 0 .. levels-1:    step = 1 << i;     k = (1/16, 1/4, 3/8, 1/4, 1/16)
 *       t[c][x,y]       = T after:  T = +0.0;  for d = -2..2:  qx = x + step*d;  0 <= qx < ws:  T = T + k[d] * b_i[c][qx, y]
 *       b_{i+1}[c][x,y] = B after:  B = +0.0;  for d = -2..2:  qy = y + step*d;  0 <= qy < h:   B = B + k[d] * t[c][x, qy]
 *       out[c][p] = out[c][p] + wl * b_{i+1}[c][p]
 * The bright pass scales the pixel by its brightest channel, so the glow keeps the pixel's hue.  A tap outside the frame is skipped
 * and not renormalised: light that leaves the frame is lost.  Each level is the separable B3 a-trous blur the denoisers use, without
 * any edge-stopping.  The glow is the mean of the `levels` scales times strength: a tight core and a wide tail, which away from
 * the borders carries exactly strength times the bright light.  There is no exp(), pow() or sqrt(): the bytes do not depend on a
 * math library.  Sums are assumed finite: a non-finite sum gives unspecified values but does not fault.
 * The call sees only the buffer it is given: taps do not cross its edge, so a multi-rank caller blooms the assembled frame.
 * RT_BLOOM_NO_TILES makes every level run as two gather kernels; without it the levels with small steps run as one kernel that
 * stages a tile in LDS.  The bytes are the same either way: the flag is for A/B measurements and tests.
 * RT_ERR_BAD_ARG, in this order, for: a NULL d_sum, bl or d_out; ws*h outside 1..RT_FILM_MAX_PIXELS; n < 1; levels outside
 * 0..RT_BLOOM_MAX_LEVELS; a threshold that is not (finite and >= 0); a strength that is not (finite and >= 0); an unknown flag
 * bit; d_work == NULL with levels >= 1; sum_stride, out_stride or (when d_work is given) work_stride < ws*h; d_out or d_work equal
 * to d_sum or to each other.  The outputs are then untouched.  Asynchronous on `stream`; it needs no scene. */
#define RT_BLOOM_MAX_LEVELS  8
#define RT_BLOOM_WORK_PLANES 6
#define RT_BLOOM_NO_TILES    1      /* rt_bloom.flags: gather at every level (A/B and tests) */

typedef struct rt_bloom {
    double  threshold;   /* colour units, finite, >= 0: what is brighter than this glows */
    double  strength;    /* finite, >= 0: the share of the bright light that is spread */
    int32_t levels;      /* 0..RT_BLOOM_MAX_LEVELS */
    int32_t flags;       /* RT_BLOOM_NO_TILES; every other bit 0 */
} rt_bloom;              /* 24 bytes */

int rt_film_bloom(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, const rt_bloom *bl,
                  void *d_out, int64_t out_stride, void *d_work, int64_t work_stride, void *stream);

/* Metering: a luminance histogram of the film and an exposure solved from it, on the device.  rt_film_resolve takes its exposure
 * by value from the host; a caller who wanted one that suits the picture had to copy the float64 mean back.  The three entries
 * below are queued on one stream (meter, solve, resolve) and never synchronise with the host.  RT_ABI_VERSION is unchanged: callers
 * detect these entry points by their symbols.
 *
 * rt_film_meter: d_sum is three float64 planes like every film buffer, element [c, x, y] at c*sum_stride + x*h + y: a sum of n
 * passes, or a mean with n = 1 (a four-plane buffer is fine: only planes 0..2 are read).  d_hist is RT_METER_BINS uint64 counts,
 * 8-byte aligned.  reset != 0 zeroes the counts first; reset == 0 adds to what is there, so slabs, ranks and frames add up exactly
 * (integers).  Per pixel p, in float64 without fused multiply-add:
 *   m_c = s[c][p] / (double)n
 *   Y = (0.2126 * m_0 + 0.7152 * m_1) + 0.0722 * m_2
 *   !(Y > 0)  (zero, negative, NaN):  bin 0
 *   else  u = the 64 bits of Y;   k = (int64)(u >> 49) - 8056        (8056 = (1023 + RT_METER_LO) * 8)
 *         k < 0: bin 1        k >= 320: bin 322  (+Inf included)        else: bin 2 + k
 *   hist[bin] = hist[bin] + 1
 * So bins 2..321 cover [2^-16, 2^24) colour units, eight per octave: bin b is [edge(b), edge(b+1)) with edge(b) the float64 whose
 * bits are (uint64)(b - 2 + 8056) << 49, which is (1 + j/8) * 2^E, exact.  Bin 0 holds what has no luminance, bin 1 what is below
 * 2^-16, bin 322 what is at or above 2^24.  There is no log(): the bins come from the bits of a float64 and the counts are
 * integers, so the bytes depend neither on a math library nor on the order in which lanes arrive.
 * RT_ERR_BAD_ARG, in this order, for: a NULL d_sum or d_hist; ws*h outside 1..RT_FILM_MAX_PIXELS; n < 1; sum_stride < ws*h; a
 * d_hist that is not 8-byte aligned or equals d_sum.  The counts are then untouched.  Asynchronous on `stream`; it needs no scene.
 *
 * rt_film_meter_solve: a histogram to an exposure.  mt holds the settings; d_state is RT_METER_STATE_DOUBLES float64 that the call
 * reads and writes (8-byte aligned); a state of zeros means "no history".
 *   N = hist[1] + ... + hist[322]                    (bin 0 is not metered)
 *   prev = state[0];   usable = prev is finite and > 0
 *   N == 0:  e = usable ? prev : clamp(1.0);   state = (e, +0.0, 0.0, 0.0);   done
 *   r = (uint64)(percentile * (double)N);   r > N-1: r = N-1
 *   b = the smallest bin in 1..322 with C_b > r,  C_b = hist[1] + ... + hist[b];   below = C_{b-1}
 *   b == 1: Ym = 2^-16     b == 322: Ym = 2^24
 *   else  lo = edge(b); hi = edge(b+1);  Ym = lo + (hi - lo) * ((double)(r - below) / (double)hist[b])
 *   t = clamp(key / Ym)                      clamp(v): v < min_exposure ? min_exposure : (v > max_exposure ? max_exposure : v)
 *   e = (usable and rate < 1) ? clamp(prev + (t - prev) * rate) : t
 *   state = (e, Ym, (double)N, (double)b)
 * key is the luminance the metered value is mapped to; the interpolation inside the bin keeps the exposure from moving in steps
 * of an eighth of an octave; rate is the eye's adaptation from frame to frame (1 jumps).  Float64 without fused multiply-add; the
 * counts are assumed to add up below 2^63.
 * RT_ERR_BAD_ARG, in this order, for: a NULL d_hist, mt or d_state; a key that is not (finite and > 0); a percentile outside 0..1;
 * a min_exposure that is not (finite and > 0); a max_exposure that is not (finite and > 0); min_exposure > max_exposure; a rate
 * outside (0, 1]; flags != 0; reserved != 0; d_state equal to d_hist.  The state is then untouched.  Asynchronous on `stream`.
 *
 * rt_film_resolve_metered: rt_film_resolve with one line changed.  The exposure used is E = tone->exposure * x, one float64
 * product, formed once; x = state[0] when that is finite and > 0, otherwise x = 1.0; tone->exposure becomes the user's
 * compensation.  With state[0] == 1.0 the outputs are rt_film_resolve's bit for bit.  The refusals are rt_film_resolve's, in its
 * order, and a NULL d_state (behind a NULL tone). */
#define RT_METER_LO            (-16)   /* log2 of the lower edge of bin 2 */
#define RT_METER_OCTAVES       40
#define RT_METER_SUB           8       /* bins per octave */
#define RT_METER_BINS          323     /* 40 * 8 + 3 */
#define RT_METER_STATE_DOUBLES 4       /* exposure, metered luminance, pixels metered, the bin it fell in */

typedef struct rt_meter {
    double  key;            /* finite, > 0, colour units: the luminance the metered value is mapped to */
    double  percentile;     /* 0..1 */
    double  min_exposure;   /* finite, > 0, min_exposure <= max_exposure */
    double  max_exposure;   /* finite, > 0 */
    double  rate;           /* in (0, 1]; 1 jumps */
    int32_t flags;          /* must be 0 */
    int32_t reserved;       /* must be 0 */
} rt_meter;                 /* 48 bytes */

int rt_film_meter(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, int reset, void *d_hist,
                  void *stream);
int rt_film_meter_solve(rt_ctx *ctx, const void *d_hist, const rt_meter *mt, void *d_state, void *stream);
int rt_film_resolve_metered(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n,
                            const rt_film_tone *tone, const void *d_state, void *d_u8, void *d_f32, int64_t out_stride,
                            void *stream);

/* Guided upsampling: run the film at low resolution, show it at full.  Accumulate, reproject and filter on a coarse grid, render the
 * guides alone at display resolution, and lift the filtered mean to the display grid along those guides: edges come from the
 * full-resolution ids and normals, texture detail from the full-resolution albedo.  RT_ABI_VERSION is unchanged: callers detect
 * these two entry points by their symbols.
 *
 * rt_render_guides_grid: rt_render_guides on the closed-form w x h grid (px, y0, dy, z0, dz) given in the call instead of the
 * context's grid.  Scene, camera, kernels, table modes, slab splitting and addressing are rt_render_guides': element [g, x, y]
 * (x0 <= x < x1) is at d_guides[g*plane_stride + (x-x0)*h + y] with this call's h.  The call leaves the context's grid as it is and
 * does not count as a change of view: a caller alternates low-resolution passes and full-resolution guides every frame, and the
 * dispatch orders measured for the render launches stay.  The context need not have a grid of its own.  Refusals carry texts
 * prefixed "rt_render_guides_grid: ", checked in this order: RT_ERR_BAD_ARG for a NULL d_guides and for a frame size that
 * rt_set_raygen refuses; RT_ERR_STATE without a scene or without a camera; RT_ERR_BAD_ARG unless 0 <= x0 < x1 <= w and for
 * plane_stride < (x1-x0)*h.  The buffer is then untouched.  Asynchronous on `stream`.
 *
 * rt_film_upsample: the lift.  d_lo is a film sum of n passes of the wl x hl frame, or with n = 1 a mean that rt_film_temporal, a
 * denoiser or rt_film_bloom wrote (planes 0..2 are read, so four-plane buffers work); d_lo_guides and d_hi_guides are the float32
 * guides of the two frames for the same camera and scene (planes 0..2, 4..6 and 7 are read, plane 3 is not); d_out receives three
 * float64 planes w x h laid out like a sum, which rt_film_resolve, rt_film_bloom and rt_film_meter take with n = 1; d_out_kind is
 * NULL or one float32 plane of w*h that says per pixel which stage wrote it (0, 1 or 2).  lo_grid and hi_grid are (px, y0, dy, z0,
 * dz) of the two frames, as rt_set_raygen and rt_render_guides_grid take them.  The call needs no scene, camera or grid state, and
 * the library allocates nothing.
 * Per output pixel p = (X, Y), E = X*h + Y, in float64 without fused multiply-add, in this order; q is a pixel of the low frame,
 * read at q.x*hl + q.y:
 *   m[c][q] = lo[c][q] / (double)n;   a_lo[c][q] = max((double)lo_guides[4+c][q], 1.0);   a_hi[c] = max((double)hi_guides[4+c][E], 1.0)
 *   sc = lo_px / hi_px;   fx = (((double)X*hi_dy + hi_y0) * sc - lo_y0) / lo_dy;   fy = (((double)Y*hi_dz + hi_z0) * sc - lo_z0) / lo_dz
 *   snap as rt_film_temporal:  rx = floor(fx + 0.5);  |fx - rx| <= 2^-20:  fx = rx        (the same for fy)
 *   !(fx >= 0):  fx = 0;   fx > wl-1:  fx = wl-1;     the same for fy with hl              (so NaN becomes 0)
 *   ix = floor(fx); ax = fx - ix;   iy = floor(fy); ay = fy - iy;    idp = hi_guides[7][E]
 *   stage 0   W = A_c = +0.0;  for a = 0, 1 (outer), b = 0, 1 (inner):  q = (ix+a, iy+b);  bw = (a ? ax : 1.0 - ax) * (b ? ay : 1.0 - ay)
 *               bw == 0, or q outside [0,wl) x [0,hl):  skip;      lo_guides[7][q] != idp:  skip
 *               idp >= 0:  cn = ((nx_p*nx_q) + (ny_p*ny_q)) + (nz_p*nz_q)  (float32 normals widened; p from hi_guides, q from lo_guides);
 *                          !(cn >= normal_cos):  skip
 *               v_c = demodulate ? m[c][q] / a_lo[c][q] : m[c][q];     W = W + bw;   A_c = A_c + bw * v_c
 *             W > 0:  out[c][E] = demodulate ? (A_c / W) * a_hi[c] : A_c / W;   kind 0
 *   stage 1   else W = A_c = +0.0;  for a = -1..2 (outer), b = -1..2 (inner):  q = (ix+a, iy+b)
 *               q outside the frame:  skip;      lo_guides[7][q] != idp:  skip                (no normal test)
 *               ex = (double)(ix+a) - fx;  ey = (double)(iy+b) - fy;   wq = 1.0 / (1.0 + (ex*ex + ey*ey))
 *               v_c as above;     W = W + wq;   A_c = A_c + wq * v_c
 *             W > 0:  the same output line;   kind 1
 *   stage 2   else W = A_c = +0.0;  the taps and weights bw of stage 0 (bw == 0 or q outside: skip), no test, no demodulation:
 *               W = W + bw;   A_c = A_c + bw * m[c][q]
 *             out[c][E] = A_c / W;   kind 2                 (after the clamp the tap (ix, iy) is inside and its bw > 0, so W > 0)
 * max(v, 1.0) is v > 1.0 ? v : 1.0.  No exp(), pow() or sqrt: the bytes do not depend on a math library.  With equal grids and
 * demodulate == 0 every pixel reads one tap of weight 1.0 (the snap), so out is lo / n bit for bit and every kind is 0 (for a
 * normal_cos that a float32 unit normal passes against itself: its squared length is 1 only to a few 2^-24, so up to 0.999, not 1).
 * A non-finite mean or guide gives unspecified values but does not fault: every tap index is range-checked before it is read.
 * The limitations stay where the guides' are: what a mirror or glass shows is interpolated inside the mirror's own id; under a lens
 * the sharp guides mask a blurred edge; taps do not cross the buffer's edge, so a multi-rank caller upsamples the assembled frame.
 * RT_ERR_BAD_ARG with texts prefixed "rt_film_upsample: ", checked in this order: a NULL d_lo, d_lo_guides, d_hi_guides, d_out or up;
 * wl*hl outside 1..RT_FILM_MAX_PIXELS, then w*h; n < 1; lo_stride or lo_guide_stride < wl*hl, hi_guide_stride or out_stride < w*h;
 * a grid entry that is not finite, or a px, dy or dz of 0 in either grid; normal_cos outside [-1, 1]; a demodulate that is not 0 or 1;
 * reserved != 0; d_out or d_out_kind equal to an input or to each other.  The outputs are then untouched.  Asynchronous on `stream`. */
int rt_render_guides_grid(rt_ctx *ctx, int w, int h, double px, double y0, double dy, double z0, double dz,
                          int x0, int x1, void *d_guides, int64_t plane_stride, void *stream);

typedef struct rt_upsample {
    double  lo_grid[5];    /* px, y0, dy, z0, dz of the low-resolution frame */
    double  hi_grid[5];    /* the same of the output frame */
    double  normal_cos;    /* in [-1, 1]: least cosine between the output pixel's normal and a tap's */
    int32_t demodulate;    /* 0 or 1: interpolate colour / albedo_lo, multiply by albedo_hi */
    int32_t reserved;      /* must be 0 */
} rt_upsample;             /* 96 bytes */

int rt_film_upsample(rt_ctx *ctx, const void *d_lo, int64_t lo_stride, int wl, int hl, int64_t n,
                     const void *d_lo_guides, int64_t lo_guide_stride,
                     const void *d_hi_guides, int64_t hi_guide_stride, int w, int h,
                     const rt_upsample *up, void *d_out, int64_t out_stride, void *d_out_kind, void *stream);

/* Device memory owned by the caller (the DeviceNDArray that `cuda.to_device(np.zeros((3,w,h)))`
 * returns, main.py:32, and `result.copy_to_host()`, main.py:51).  The copies are ordered on the
 * context's stream and return when the bytes have arrived. */
int rt_malloc(rt_ctx *ctx, size_t bytes, void **dptr);
int rt_free(rt_ctx *ctx, void *dptr);
int rt_memcpy_h2d(rt_ctx *ctx, void *dst_device, const void *src_host, size_t bytes);
int rt_memcpy_d2h(rt_ctx *ctx, void *dst_host, const void *src_device, size_t bytes);

/* Block until everything queued on the context's stream is done (the implicit sync of
 * copy_to_host, main.py:51). */
int rt_sync(rt_ctx *ctx);

/* Extra streams for callers that do not link HIP themselves: frames of a sequence can be queued alternately on two
 * or more streams (each into its own output buffers) so that one frame's last workgroups overlap the next frame's
 * first — the reference launches one frame and waits (main.py:41-51).  The handle is a hipStream_t; any
 * hipStream_t of the context's device is equally valid wherever this header takes a `stream`. */
int rt_stream_create(rt_ctx *ctx, void **stream);
int rt_stream_destroy(rt_ctx *ctx, void *stream);
int rt_stream_sync(rt_ctx *ctx, void *stream);   /* NULL = context stream */
/* A stream the caller owns (a torch / HIP stream passed to rt_render_device) must be forgotten before its owner
 * destroys it: the context keeps the handles of streams that launched on it, to fence them when the dispatch order
 * or a cull-table set they may still read is rebuilt.  Waits for the stream's queued work, then drops the handle;
 * the stream may be used with the context again afterwards.  rt_stream_destroy does this by itself. */
int rt_stream_forget(rt_ctx *ctx, void *stream);

/* hipEvent pair on `stream` (NULL = context stream) around whatever is launched in between;
 * rt_timer_end synchronises on the second event and returns elapsed milliseconds. */
int rt_timer_begin(rt_ctx *ctx, void *stream);
int rt_timer_end(rt_ctx *ctx, void *stream, float *ms);

int rt_get_kernel_info(rt_ctx *ctx, rt_kernel_info *info);

/* rt_get_stats waits for the device when counting launches have been made (the counters live in device memory). */
int rt_get_stats(rt_ctx *ctx, rt_stats *stats);
int rt_reset_stats(rt_ctx *ctx);

/* Statistics: with a non-NULL device buffer of ceil((x1-x0)/8) * ceil(h/8) uint32, every later rt_render_device /
 * rt_render_sequence launch stores the shader-clock cycles each 8x8 tile's wavefront took, tile index =
 * tile_x * ceil(h/8) + tile_y with tile_x counted from the launch's x0 (what the reference's unused `timed` decorator,
 * viewer/image.py:22-34, gestures at).  Defined for launches of the pixel frame into device buffers: the host-buffer
 * entry points split large frames into column chunks (each chunk records from ITS first column into its own part of the
 * buffer, so the frame's tiles still land at the indices above), and RT_AA_REFERENCE on the closed-form grid traces a
 * half-pixel lattice instead of pixels and records nothing.  NULL turns it off. */
int rt_set_tile_stats(rt_ctx *ctx, void *d_cycles);

#ifdef __cplusplus
}
#endif
#endif /* MI355RT_H */
