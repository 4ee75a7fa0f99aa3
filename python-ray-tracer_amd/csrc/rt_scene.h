// rt_scene.h — what every rt_set_scene* entry does before it touches the device: validate the caller's scene and pack it into
// the float64 scene buffer and the float32 texel array the render kernels read (layout: rt_layout.h, rt_device.h).
// HIP-free, like rt_geometry.h and for the same reason: all of this is host arithmetic whose every bit reaches the frames, so
// it must be testable where there is no GPU.  mi355rt.hip calls pack_scene and uploads what it returns;
// tests/algo/scene_pack_check.cpp calls it under AddressSanitizer and UBSan and compares the bytes with recorded ones.
// Compile with -ffp-contract=off (the float32 sub-expressions below are the reference's, rounding by rounding).
#pragma once
#include "../../include/mi355rt.h"
#include "rt_layout.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace rt {

// Every input of every rt_set_scene* entry (include/mi355rt.h describes them); the defaults are "absent".
struct SceneDesc {
    const float *spheres = nullptr, *lights = nullptr, *planes = nullptr;   // (7,S), (3,L), (9,P)
    int S = 0, L = 0, P = 0;
    int flags = 0;
    const double *materials = nullptr;     // (M, ncols), or nullptr with M == 0: the launch's shading scalars
    int M = 0, ncols = 3;
    const int32_t *sphere_material = nullptr, *plane_material = nullptr;
    const float *light_radius = nullptr;   // nullptr (no area lights) or the (L,) radii of rt_set_scene_area_lights
    int shadow_samples = 1;
    const rt_texture *textures = nullptr;  // the arguments of rt_set_scene_textures (T == 0: none)
    int T = 0;
    const int32_t *sphere_texture = nullptr, *plane_texture = nullptr;
    const float *texels = nullptr;
    int64_t n_texels = 0;
    const float *light_rgb = nullptr;      // nullptr or the (L, 3) colours of rt_set_scene_lighting
    bool lighting = false;                 // the entry is rt_set_scene_lighting or rt_set_scene_sky: the ones that take a table of 8 columns
    const double *sky = nullptr;           // nullptr or the RT_SKY_DOUBLES of rt_set_scene_sky
};

// What a launch needs to know about the packed scene.
struct SceneLayout {
    int S = 0, P = 0, L = 0;
    int NC = 0;                   // sphere clusters (0 = flat scene)
    int M = 0;                    // materials of the scene (rt_set_scene_materials; 0 = the launch's shading scalars)
    int mat_cols = 3;             // doubles per row of its table: 6 with a rough row (the scatter kernels), else 5 with a
                                  // transparent row (the refraction kernels), else 3
    int soft_n = 0;               // shadow samples per light of a scene with a light radius > 0 (the area-light kernels), else 0
    int T = 0;                    // texture records of a scene with a textured object (the texture kernels), else 0
    bool lit = false;             // the scene runs the lighting kernels (a light colour that is not (1, 1, 1), or a row with spec > 0)
    bool sky = false;             // the scene runs the sky kernels (rt_set_scene_sky with a colour that is not zero); lit is set too
    long long lens_mat = 0;       // offset (doubles) in the scene buffer of its material block with rows of 6 (the lens kernels')
    long long tex_off = 0;        // ... of its texture block (rt::tex_doubles)
    long long lit_off = 0;        // ... of its lighting block (rt::lit_doubles)
    long long sky_off = 0;        // ... of its sky block (rt::SKY_DOUBLES)
    unsigned plane_codes = 0;     // axis codes of planes 0..3 (rt_device.h: KParams::plane_codes)
    double extent2 = 0.0;         // max squared distance of lights / sphere surfaces from the world origin
};

struct PackedScene {
    int status = RT_OK;
    std::string error;            // the rt_last_error text of a status that is not RT_OK
    SceneLayout layout;
    std::vector<double> rec;      // the scene buffer
    std::vector<float> texels;    // {R,G,B, texture id} of the S + P object slots, then {R,G,B,-} of the scene's texels (textured or lit scenes)
};

// The family whose material block a scene buffer starts with: rows of `cols`, and an area-light scene's shadow_samples behind it.
inline Family block_family(int M, int cols, bool soft)
{
    if (M <= 0) return Family::PLAIN;
    return soft ? Family::SOFT : cols == 6 ? Family::SCAT : cols == 5 ? Family::REFR : Family::MAT;
}

namespace detail {

// common.py:104-110 on float32 inputs (float32 squares/sum, sqrt of that sum rounded to float32,
// float32 divisions) — the shading normal of a plane, hoisted to scene-upload time.
inline void plane_normal_f32(const float n[3], float out[3])
{
    const float s = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    const float norm = (float)std::sqrt((double)s);
    out[0] = n[0] / norm; out[1] = n[1] / norm; out[2] = n[2] / norm;
}

// M rows of `cols` columns of a material table into dst, from a table of `ncols` columns: its first columns, and where it has
// fewer, trans 0, ior 1 and rough 0.
inline void put_rows(double *dst, int cols, const double *src, int ncols, int M)
{
    static const double pad[6] = {0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    for (int m = 0; m < M; ++m)
        for (int i = 0; i < cols; ++i) dst[(size_t)cols * m + i] = i < ncols ? src[(size_t)ncols * m + i] : pad[i];
}

// One pack_scene call: the description, the two thresholds, the result, and what validation learns on the way to packing.
// The check_* functions return false with out.status and out.error set; pack_scene calls them in a fixed order, so an input
// that breaks two rules always reports the same one.
struct Packer {
    const SceneDesc &d;
    const int cluster_min, lanes_min_spheres;
    PackedScene out;

    bool has_sky = false;
    int sky_sharp = 0, sky_shin = 0;            // log2(sharp), log2(halo_shin)
    bool lit = false, soft = false, textured = false;
    int cols = 3;                               // columns of the table that travels
    const double *materials = nullptr;          // that table: the caller's, `packed` or `soft_table`
    std::vector<double> packed, soft_table;
    std::vector<double> spec_shin;              // ncols == 8: {spec, log2(shin)} per row
    std::vector<int> order;                     // slot -> the caller's sphere index
    size_t mat_off = 0, matd = 0, lens_off = 0, tex_off = 0, lit_off = 0, sky_off = 0;

    Packer(const SceneDesc &desc, int cmin, int lmin) : d(desc), cluster_min(cmin), lanes_min_spheres(lmin), materials(desc.materials) {}

    bool fail(int code, const std::string &msg) { out.status = code; out.error = msg; return false; }

    // ---- validation -------------------------------------------------------------------------------------------------------

    // the sky: one whose five colours are all zero is no sky (has_sky stays false: exactly rt_set_scene_lighting), any other
    // runs the sky kernels, which are lighting kernels (check_sizes_ids sets lit)
    bool check_sky()
    {
        const double *sky = d.sky;
        if (!sky) return true;
        for (int i = 0; i < RT_SKY_DOUBLES; ++i)
            if (!std::isfinite(sky[i])) return fail(RT_ERR_BAD_ARG, "sky[" + std::to_string(i) + "] is not finite");
        for (int i : {3, 4, 5, 6, 7, 8, 9, 10, 11, 17, 18, 19, 20, 21, 22}) {
            if (sky[i] < 0.0) return fail(RT_ERR_BAD_ARG, "sky[" + std::to_string(i) + "]: a colour must be >= 0");
            has_sky = has_sky || sky[i] != 0.0;
        }
        for (int v : {0, 13}) {
            const double n2 = sky[v] * sky[v] + sky[v + 1] * sky[v + 1] + sky[v + 2] * sky[v + 2];
            if (!(n2 >= 1.0 - 1e-6 && n2 <= 1.0 + 1e-6))
                return fail(RT_ERR_BAD_ARG, v == 0 ? "sky: up must be a unit vector" : "sky: sun_dir must be a unit vector");
        }
        sky_sharp = sky_shin = -1;
        for (int i = 0; i <= 4; ++i) if (sky[12] == (double)(1 << i)) sky_sharp = i;
        for (int i = 0; i <= 10; ++i) if (sky[23] == (double)(1 << i)) sky_shin = i;
        if (sky_sharp < 0) return fail(RT_ERR_BAD_ARG, "sky: sharp must be one of 1, 2, 4, 8, 16");
        if (sky_shin < 0) return fail(RT_ERR_BAD_ARG, "sky: halo_shin must be one of 1, 2, 4, ..., 1024");
        return true;
    }

    bool check_table_width()
    {
        if (d.ncols != 3 && d.ncols != 5 && d.ncols != 6 && !(d.lighting && d.ncols == 8))
            return fail(RT_ERR_BAD_ARG, d.lighting ? "ncols must be 3, 5, 6 or 8" : "ncols must be 3, 5 or 6");
        return true;
    }

    // lighting: validated here and in check_table (the spec and shin columns); a scene whose lights are all bitwise (1, 1, 1) and
    // whose rows all have spec 0 is exactly rt_set_scene_textures' (lit stays false), any other runs the lighting kernels
    bool check_light_colours()
    {
        const float *light_rgb = d.light_rgb;
        if (!light_rgb) return true;
        if (d.L < 0 || d.L > RT_MAX_LIGHTS) return fail(RT_ERR_BAD_ARG, "scene size outside RT_MAX_SPHERES / RT_MAX_LIGHTS / RT_MAX_PLANES");
        static const float one = 1.0f;
        for (int i = 0; i < 3 * d.L; ++i) {
            if (!(std::isfinite(light_rgb[i]) && light_rgb[i] >= 0.0f))
                return fail(RT_ERR_BAD_ARG, "light_rgb[" + std::to_string(i / 3) + "] must be finite and >= 0");
            lit = lit || std::memcmp(&light_rgb[i], &one, sizeof one) != 0;
        }
        return true;
    }

    // area lights (light_radius: nullptr from the entries before rt_set_scene_area_lights): a scene with every radius 0 is
    // exactly rt_set_scene_materials_scatter's (soft stays false), one with a radius > 0 runs the area-light kernels
    bool check_radii()
    {
        const float *light_radius = d.light_radius;
        if (!light_radius) return true;
        if (d.shadow_samples < 1 || d.shadow_samples > RT_MAX_SHADOW_SAMPLES)
            return fail(RT_ERR_BAD_ARG, "shadow_samples outside 1..RT_MAX_SHADOW_SAMPLES");
        if (d.L < 0 || d.L > RT_MAX_LIGHTS) return fail(RT_ERR_BAD_ARG, "scene size outside RT_MAX_SPHERES / RT_MAX_LIGHTS / RT_MAX_PLANES");
        for (int k = 0; k < d.L; ++k) {
            if (!(std::isfinite(light_radius[k]) && light_radius[k] >= 0.0f))
                return fail(RT_ERR_BAD_ARG, "light_radius[" + std::to_string(k) + "] must be finite and >= 0");
            soft = soft || light_radius[k] > 0.0f;
        }
        if (soft && !(d.M > 0 && materials))
            return fail(RT_ERR_BAD_ARG, "a light radius > 0 needs a material table (M >= 1)");
        return true;
    }

    // a table of 5 or more columns: validated here; it travels with the columns its rows use: all six with a rough row (the scatter
    // kernels), else the first five with a transparent row (the refraction kernels), else the first three (the material kernels).
    // The area-light kernels are scatter kernels: their table travels with all six columns (a 3- or 5-column table padded with
    // trans 0, ior 1, rough 0), and with lamb / n in place of lamb (the reference's lambert_int of a trace with n points per light)
    bool check_table()
    {
        const int M = d.M, ncols = d.ncols;
        if (ncols >= 5 && M > 0 && M <= RT_MAX_MATERIALS && materials) {
            bool glass = false, rough = false;
            for (int m = 0; m < M; ++m) {
                const double *r = materials + (size_t)ncols * m;
                for (int i = 0; i < ncols; ++i)
                    if (!std::isfinite(r[i]))
                        return fail(RT_ERR_BAD_ARG, "material " + std::to_string(m) + " has a coefficient that is not finite");
                if (!(r[3] >= 0.0)) return fail(RT_ERR_BAD_ARG, "material " + std::to_string(m) + ": trans must be >= 0");
                if (!(r[4] > 0.0)) return fail(RT_ERR_BAD_ARG, "material " + std::to_string(m) + ": ior must be > 0");
                if (r[3] > 0.0 && r[2] != 0.0)
                    return fail(RT_ERR_BAD_ARG, "material " + std::to_string(m) + ": a transparent row must have refl == 0");
                if (ncols >= 6) {
                    if (!(r[5] >= 0.0 && r[5] <= 1.0)) return fail(RT_ERR_BAD_ARG, "material " + std::to_string(m) + ": rough must be in [0, 1]");
                    if (r[3] > 0.0 && r[5] > 0.0)
                        return fail(RT_ERR_BAD_ARG, "material " + std::to_string(m) + ": a transparent row must have rough == 0");
                    rough = rough || r[5] > 0.0;
                }
                glass = glass || r[3] > 0.0;
                if (ncols == 8) {
                    if (!(r[6] >= 0.0)) return fail(RT_ERR_BAD_ARG, "material " + std::to_string(m) + ": spec must be >= 0");
                    int lg = -1;
                    for (int i = 0; i <= 10; ++i) if (r[7] == (double)(1 << i)) lg = i;
                    if (lg < 0) return fail(RT_ERR_BAD_ARG, "material " + std::to_string(m) + ": shin must be one of 1, 2, 4, ..., 1024");
                    lit = lit || r[6] > 0.0;
                }
            }
            cols = rough ? 6 : (glass ? 5 : 3);
            if (ncols == 8) {
                spec_shin.resize((size_t)2 * M);
                for (int m = 0; m < M; ++m) {
                    spec_shin[(size_t)2 * m] = materials[(size_t)8 * m + 6];
                    spec_shin[(size_t)2 * m + 1] = std::log2(materials[(size_t)8 * m + 7]);   // (exact: a power of two)
                }
            }
            packed.resize((size_t)cols * M);
            put_rows(packed.data(), cols, materials, ncols, M);
            materials = packed.data();
        }
        if (soft && M <= RT_MAX_MATERIALS) {
            soft_table.resize((size_t)6 * M);
            put_rows(soft_table.data(), 6, materials, cols, M);
            for (int m = 0; m < M; ++m) soft_table[(size_t)6 * m + 1] /= (double)d.shadow_samples;
            materials = soft_table.data();
            cols = 6;
        }
        return true;
    }

    bool check_sizes_ids()
    {
        const int S = d.S, L = d.L, P = d.P, M = d.M;
        if (S < 0 || S > RT_MAX_SPHERES || L < 0 || L > RT_MAX_LIGHTS || P < 0 || P > RT_MAX_PLANES)
            return fail(RT_ERR_BAD_ARG, "scene size outside RT_MAX_SPHERES / RT_MAX_LIGHTS / RT_MAX_PLANES");
        if ((S && !d.spheres) || (L && !d.lights) || (P && !d.planes)) return fail(RT_ERR_BAD_ARG, "NULL scene array with non-zero count");
        if (M < 0 || M > RT_MAX_MATERIALS) return fail(RT_ERR_BAD_ARG, "material count outside 0..RT_MAX_MATERIALS");
        if (lit && !(M > 0 && materials)) return fail(RT_ERR_BAD_ARG, "lighting needs a material table (M >= 1)");
        if (has_sky && !(M > 0 && materials)) return fail(RT_ERR_BAD_ARG, "a sky needs a material table (M >= 1)");
        lit = lit || has_sky;                                           // (white lights and spec 0 where the scene gave none)
        if (M > 0) {
            if (!materials) return fail(RT_ERR_BAD_ARG, "materials is NULL with M > 0");
            if ((S && !d.sphere_material) || (P && !d.plane_material)) return fail(RT_ERR_BAD_ARG, "NULL material id array with non-zero count");
            for (int i = 0; i < cols * M; ++i)
                if (!std::isfinite(materials[i]))
                    return fail(RT_ERR_BAD_ARG, "material " + std::to_string(i / cols) + " has a coefficient that is not finite");
            for (int k = 0; k < S; ++k)
                if (d.sphere_material[k] < 0 || d.sphere_material[k] >= M)
                    return fail(RT_ERR_BAD_ARG, "sphere_material[" + std::to_string(k) + "] outside 0..M-1");
            for (int k = 0; k < P; ++k)
                if (d.plane_material[k] < 0 || d.plane_material[k] >= M)
                    return fail(RT_ERR_BAD_ARG, "plane_material[" + std::to_string(k) + "] outside 0..M-1");
        }
        return true;
    }

    // textures: a scene without a textured object (T == 0, or every id -1) is exactly rt_set_scene_area_lights' (textured stays
    // false), one with a textured object runs the texture kernels
    bool check_textures()
    {
        const int S = d.S, P = d.P, M = d.M, T = d.T;
        const int64_t n_texels = d.n_texels;
        if (T < 0 || T > RT_MAX_TEXTURES) return fail(RT_ERR_BAD_ARG, "texture count outside 0..RT_MAX_TEXTURES");
        if (n_texels < 0 || n_texels > RT_MAX_TEXELS) return fail(RT_ERR_BAD_ARG, "texel count outside 0..RT_MAX_TEXELS");
        if (T > 0) {
            if (!(M > 0)) return fail(RT_ERR_BAD_ARG, "textures need a material table (M >= 1)");
            if (!d.textures) return fail(RT_ERR_BAD_ARG, "textures is NULL with T > 0");
            if (!d.texels) return fail(RT_ERR_BAD_ARG, "texels is NULL with T > 0");
            for (int t = 0; t < T; ++t) {
                const rt_texture &x = d.textures[t];
                long long cells = 1;
                if (x.reserved != 0) return fail(RT_ERR_BAD_ARG, "texture " + std::to_string(t) + ": reserved must be 0");
                for (int a = 0; a < 3; ++a) {
                    if (x.dim[a] < 1 || x.dim[a] > RT_MAX_TEXTURE_DIM)
                        return fail(RT_ERR_BAD_ARG, "texture " + std::to_string(t) + ": a dimension outside 1..RT_MAX_TEXTURE_DIM");
                    cells *= x.dim[a];
                    if (!std::isfinite(x.origin[a]) || !std::isfinite(x.axis[a][0]) || !std::isfinite(x.axis[a][1]) || !std::isfinite(x.axis[a][2]))
                        return fail(RT_ERR_BAD_ARG, "texture " + std::to_string(t) + ": origin or axis not finite");
                }
                if (x.first < 0 || x.first > n_texels || cells > n_texels - x.first)
                    return fail(RT_ERR_BAD_ARG, "texture " + std::to_string(t) + ": texel range outside the texel array");
            }
            for (int64_t i = 0; i < 3 * n_texels; ++i)
                if (!std::isfinite(d.texels[i])) return fail(RT_ERR_BAD_ARG, "texel " + std::to_string(i / 3) + " is not finite");
        }
        for (int k = 0; k < S && d.sphere_texture; ++k) {
            if (d.sphere_texture[k] < -1 || d.sphere_texture[k] >= T)
                return fail(RT_ERR_BAD_ARG, "sphere_texture[" + std::to_string(k) + "] outside -1..T-1");
            textured = textured || d.sphere_texture[k] >= 0;
        }
        for (int k = 0; k < P && d.plane_texture; ++k) {
            if (d.plane_texture[k] < -1 || d.plane_texture[k] >= T)
                return fail(RT_ERR_BAD_ARG, "plane_texture[" + std::to_string(k) + "] outside -1..T-1");
            textured = textured || d.plane_texture[k] >= 0;
        }
        return true;
    }

    // ---- packing ----------------------------------------------------------------------------------------------------------

    // Recursive median split of the centres in order[a, b) along the longest axis of their bounding box, the left part always a
    // whole number of clusters: every cluster but the last has exactly rt::CLUSTER spheres and is a compact block
    // of neighbours.  (Until late in round 2: Morton order cut into runs of 8 — first with every axis scaled to its own
    // span, which sorted a flat layer of spheres by radius; then with one scale; the split is tighter still.)
    // Ties are broken by the caller's index, so the order is the same on every host.
    void split(int a, int b)
    {
        const float *spheres = d.spheres;
        const int S = d.S;
        const bool group_aligned = S >= lanes_min_spheres;
        const int n = b - a;
        if (n <= rt::CLUSTER) return;
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
        for (int j = a; j < b; ++j)
            for (int i = 0; i < 3; ++i) { const double v = spheres[i * S + order[j]]; lo[i] = std::min(lo[i], v); hi[i] = std::max(hi[i], v); }
        int ax = 0;
        for (int i = 1; i < 3; ++i) if (hi[i] - lo[i] > hi[ax] - lo[ax]) ax = i;
        const int nc = (n + rt::CLUSTER - 1) / rt::CLUSTER;
        // scenes whose kernels test GROUPS of rt::SUPER consecutive clusters first (the lane-owned traversal's): the left
        // part is a whole number of groups as well, so that every group is a subtree of this split
        const int left = (group_aligned && nc > rt::SUPER) ? rt::SUPER * ((nc / rt::SUPER + 1) / 2) : (nc + 1) / 2;
        const int mid = a + left * rt::CLUSTER;
        auto key = [&](int x) { const float v = spheres[ax * S + x]; return v == v ? v : 3.0e38f; };   // (a NaN sorts last)
        std::sort(order.begin() + a, order.begin() + b, [&](int x, int y) {
            const float vx = key(x), vy = key(y);
            return vx < vy || (vx == vy && x < y);
        });
        split(a, mid);
        split(mid, b);
    }

    // Scenes with more than cluster_min (rt::CLUSTER_MIN) spheres are stored in clusters of rt::CLUSTER spatially close
    // spheres, each with a bounding sphere the kernel culls first.  Slot
    // order is a permutation of the caller's order; every record keeps the caller's index so that the
    // reference's tie rule (the lower index wins an exact tie, trace.py:26) is unaffected.
    void cluster_order()
    {
        order.resize(d.S);
        std::iota(order.begin(), order.end(), 0);
        if (d.S > cluster_min) {
            split(0, d.S);
            out.layout.NC = (d.S + rt::CLUSTER - 1) / rt::CLUSTER;
        }
    }

    // where the blocks lie, and the buffer itself
    void block_offsets()
    {
        const int S = d.S, P = d.P, L = d.L, M = d.M, NC = out.layout.NC;
        mat_off = rt::mat_offset(S, P, L, NC);      // (records, cluster records, one spare double)
        // the lens kernels are scatter kernels: a table of 3 or 5 columns gets a copy padded to six (trans 0, ior 1, rough 0)
        // behind its block, with the same ids; a 6-column one (an area-light scene's included) serves them as it is
        matd = rt::mat_doubles(M, S, P, block_family(M, cols, soft));
        lens_off = (M > 0 && cols < 6) ? mat_off + matd : mat_off;
        // the texture block (rt::tex_doubles) behind everything else
        tex_off = mat_off + matd + (lens_off != mat_off ? rt::mat_doubles(M, S, P, rt::Family::LENS) : 0);
        // and the lighting block (rt::lit_doubles) behind that
        lit_off = tex_off + (textured ? rt::tex_doubles(d.T) : 0);
        // and the sky block (rt::SKY_DOUBLES) last
        sky_off = lit_off + (lit ? rt::lit_doubles(S, P, L) : 0);
        out.rec.assign(sky_off + (has_sky ? rt::SKY_DOUBLES : 0), 0.0);
    }

    // Packed float64 records (layout: rt_device.h).  All float32 sub-expressions of the reference
    // are evaluated here, once, in float32: r*r (intersections.py:21), the plane shading normal
    // (common.py:104-110) and BIAS*N of a plane hit (trace.py:82-83).
    void object_records()
    {
        const float *spheres = d.spheres, *planes = d.planes, *lights = d.lights;
        const int S = d.S, P = d.P, L = d.L;
        double *sp = out.rec.data();
        unsigned codes = 0;
        for (int slot = 0; slot < S; ++slot, sp += rt::SPH_STRIDE) {
            const int k = order[slot];
            sp[7] = (double)k;                                   // the caller's index of this sphere
            const float r = spheres[3 * S + k];
            const float r2 = r * r;
            sp[0] = spheres[0 * S + k]; sp[1] = spheres[1 * S + k]; sp[2] = spheres[2 * S + k]; sp[3] = (double)r2;
            sp[4] = spheres[4 * S + k]; sp[5] = spheres[5 * S + k]; sp[6] = spheres[6 * S + k];
        }
        for (int k = 0; k < P; ++k, sp += rt::PL_STRIDE) {
            for (int i = 0; i < 6; ++i) sp[i] = planes[i * P + k];
            const float nraw[3] = {planes[3 * P + k], planes[4 * P + k], planes[5 * P + k]};
            float nf[3];
            plane_normal_f32(nraw, nf);
            const double BIAS = 0.0002;
            const float bf = (float)BIAS;
            {   // axis code: the stored normal is exactly +-e_i (intersection shortcut in rt_device.h:plane_den_num)
                int axis = -1, nonzero = 0;
                for (int i = 0; i < 3; ++i) if (nraw[i] != 0.0f) { ++nonzero; axis = i; }
                sp[15] = (nonzero == 1 && (nraw[axis] == 1.0f || nraw[axis] == -1.0f)) ? (double)(axis + 1) * (double)nraw[axis] : 0.0;
                if (k < 4) codes |= (unsigned)(unsigned char)(signed char)sp[15] << (8 * k);
            }
            for (int i = 0; i < 3; ++i) {
                sp[6 + i] = (double)nf[i];
                sp[9 + i] = (d.flags & RT_FLAG_TYPED_BIAS) ? BIAS * (double)nf[i] : (double)(bf * nf[i]);
                sp[12 + i] = planes[(6 + i) * P + k];
            }
        }
        for (int k = 0; k < L; ++k, sp += rt::LT_STRIDE) {
            sp[0] = lights[0 * L + k]; sp[1] = lights[1 * L + k]; sp[2] = lights[2 * L + k];
            if (soft) sp[3] = d.light_radius[k];                    // (the pad slot: the area-light kernels' radius)
        }
        out.layout.plane_codes = codes;
    }

    // bounding sphere (float64, inflated) of the spheres in slots [j0, j1): around the centroid of the centres or the centre of
    // their bounding box, whichever gives the smaller sphere
    void bound(int j0, int j1, double *dst) const
    {
        const float *spheres = d.spheres;
        const int S = d.S;
        double Cc[2][3] = {{0, 0, 0}, {0, 0, 0}}, blo[3] = {1e300, 1e300, 1e300}, bhi[3] = {-1e300, -1e300, -1e300};
        for (int j = j0; j < j1; ++j)
            for (int i = 0; i < 3; ++i) {
                const double v = spheres[i * S + order[j]], rr = std::fabs((double)spheres[3 * S + order[j]]);
                Cc[0][i] += v; blo[i] = std::min(blo[i], v - rr); bhi[i] = std::max(bhi[i], v + rr);
            }
        for (int i = 0; i < 3; ++i) { Cc[0][i] /= (j1 - j0); Cc[1][i] = 0.5 * (blo[i] + bhi[i]); }
        double C[3] = {0, 0, 0}, R = 1e300;
        for (int t = 0; t < 2; ++t) {
            double Rt = 0;
            for (int j = j0; j < j1; ++j) {
                const int k = order[j];
                const double dx = spheres[0 * S + k] - Cc[t][0], dy = spheres[1 * S + k] - Cc[t][1], dz = spheres[2 * S + k] - Cc[t][2];
                Rt = std::max(Rt, std::sqrt(dx * dx + dy * dy + dz * dz) + std::fabs((double)spheres[3 * S + k]));
            }
            if (Rt < R || t == 0) { R = Rt; for (int i = 0; i < 3; ++i) C[i] = Cc[t][i]; }   // (NaN: keeps the centroid's)
        }
        R = R * (1.0 + 1e-6) + 1e-9;
        dst[0] = C[0]; dst[1] = C[1]; dst[2] = C[2]; dst[3] = R * R;
    }

    void bounding_spheres()
    {
        const int S = d.S, NC = out.layout.NC;
        double *sp = out.rec.data() + rt::lds_doubles(S, d.P, d.L);
        for (int c = 0; c < NC; ++c, sp += rt::CL_STRIDE)                   // clusters of rt::CLUSTER spheres
            bound(c * rt::CLUSTER, std::min(S, (c + 1) * rt::CLUSTER), sp);
        for (int g = 0; g < rt::supers(NC); ++g, sp += rt::CL_STRIDE)      // groups of rt::SUPER clusters
            bound(g * rt::SUPER * rt::CLUSTER, std::min(S, (g + 1) * rt::SUPER * rt::CLUSTER), sp);
    }

    // the material block (rt::mat_offset): M, the table, the ids of the sphere SLOTS (cluster_order) and of the planes; behind it
    // the lens kernels' copy with rows of six, where the table has fewer columns
    void material_block()
    {
        const int S = d.S, P = d.P, M = d.M;
        if (!(M > 0)) return;
        std::vector<double> &rec = out.rec;
        rec[mat_off] = (double)M;
        std::memcpy(rec.data() + mat_off + 1, materials, (size_t)cols * M * sizeof(double));
        std::vector<int32_t> ids((size_t)S + P);
        for (int slot = 0; slot < S; ++slot) ids[slot] = d.sphere_material[order[slot]];
        for (int k = 0; k < P; ++k) ids[(size_t)S + k] = d.plane_material[k];
        if (!ids.empty()) std::memcpy(rec.data() + mat_off + 1 + (size_t)cols * M, ids.data(), ids.size() * sizeof(int32_t));
        if (soft) rec[mat_off + matd - 1] = (double)d.shadow_samples;   // (rt::mat_doubles: the block's last double)
        if (lens_off != mat_off) {
            rec[lens_off] = (double)M;
            put_rows(rec.data() + lens_off + 1, 6, materials, cols, M);
            if (!ids.empty()) std::memcpy(rec.data() + lens_off + 1 + (size_t)6 * M, ids.data(), ids.size() * sizeof(int32_t));
        }
    }

    // textures: the records with what texel_of reads (dimensions and their reciprocals as doubles, the first texel's entry of
    // the texel array); the texel array starts with the S + P slots' own colours (exact: the scene is float32) and texture
    // ids (-1: none), so that a hit without a texture reads its colour the same way
    // (a lit scene without a textured object has the array too, every id -1: the lighting kernels are texture kernels)
    void texture_block()
    {
        if (!(textured || lit)) return;
        const float *spheres = d.spheres, *planes = d.planes;
        const int S = d.S, P = d.P, T = d.T;
        const int64_t n_texels = d.n_texels;
        std::vector<float> &tx = out.texels;
        double *tb = out.rec.data() + tex_off;
        if (textured) tb[0] = (double)T;
        for (int t = 0; t < T && textured; ++t) {
            double *r = tb + 1 + (size_t)rt::TEX_STRIDE * t;
            const rt_texture &x = d.textures[t];
            for (int a = 0; a < 3; ++a) {
                r[a] = x.origin[a];
                for (int i = 0; i < 3; ++i) r[3 + 3 * a + i] = x.axis[a][i];
                r[12 + a] = (double)x.dim[a];
                r[15 + a] = 1.0 / (double)x.dim[a];
            }
            r[18] = (double)((long long)S + P + x.first);
        }
        tx.assign(4 * ((size_t)S + P + (size_t)(textured ? n_texels : 0)), 0.0f);
        for (int slot = 0; slot < S; ++slot) {
            for (int c = 0; c < 3; ++c) tx[4 * (size_t)slot + c] = spheres[(4 + c) * S + order[slot]];
            tx[4 * (size_t)slot + 3] = (textured && d.sphere_texture) ? (float)d.sphere_texture[order[slot]] : -1.0f;
        }
        for (int k = 0; k < P; ++k) {
            for (int c = 0; c < 3; ++c) tx[4 * ((size_t)S + k) + c] = planes[(6 + c) * P + k];
            tx[4 * ((size_t)S + k) + 3] = (textured && d.plane_texture) ? (float)d.plane_texture[k] : -1.0f;
        }
        for (int64_t i = 0; i < n_texels && textured; ++i)
            for (int c = 0; c < 3; ++c) tx[4 * ((size_t)S + P + (size_t)i) + c] = d.texels[3 * i + c];
    }

    // lighting: the lights' colours (widened: exact), then per object slot its row's spec / n (n: the shadow samples of an
    // area-light scene, else 1; a float64 division, as lamb / n) and log2(shin)
    void lighting_block()
    {
        if (!lit) return;
        const int S = d.S, P = d.P, L = d.L;
        double *lb = out.rec.data() + lit_off;
        for (int k = 0; k < L; ++k)
            for (int c = 0; c < 3; ++c) lb[(size_t)rt::LT_STRIDE * k + c] = d.light_rgb ? (double)d.light_rgb[3 * k + c] : 1.0;
        double *ob = lb + (size_t)rt::LT_STRIDE * L;
        const double n = soft ? (double)d.shadow_samples : 1.0;
        for (size_t j = 0; j < (size_t)S + P; ++j) {
            const int m = j < (size_t)S ? d.sphere_material[order[j]] : d.plane_material[j - S];
            ob[2 * j] = spec_shin.empty() ? 0.0 : spec_shin[(size_t)2 * m] / n;
            ob[2 * j + 1] = spec_shin.empty() ? 0.0 : spec_shin[(size_t)2 * m + 1];
        }
    }

    // the sky, laid out for rt::sky_color: the gradient as the horizon's colour and the two differences from it, the two
    // exponents as numbers of squarings (int64)
    void sky_block()
    {
        if (!has_sky) return;
        const double *sky = d.sky;
        double *kb = out.rec.data() + sky_off;
        for (int c = 0; c < 3; ++c) {
            kb[c] = sky[c];
            kb[3 + c] = sky[6 + c];
            kb[6 + c] = sky[3 + c] - sky[6 + c];
            kb[9 + c] = sky[9 + c] - sky[6 + c];
            kb[13 + c] = sky[13 + c];
            kb[17 + c] = sky[17 + c];
            kb[20 + c] = sky[20 + c];
        }
        kb[16] = sky[16];
        const long long nsq[2] = {sky_sharp, sky_shin};         // the two counts are int64 words: scalar loop counters
        std::memcpy(&kb[12], &nsq[0], sizeof(double));
        std::memcpy(&kb[23], &nsq[1], sizeof(double));
    }

    // max squared distance of the sphere surfaces and the lights (an area light: its ball) from the world origin
    void extent()
    {
        const float *spheres = d.spheres, *lights = d.lights;
        const int S = d.S, L = d.L;
        double ext2 = 0.0;
        for (int k = 0; k < S; ++k) {
            const double cx = spheres[0 * S + k], cy = spheres[1 * S + k], cz = spheres[2 * S + k], r = std::fabs((double)spheres[3 * S + k]);
            const double e = std::sqrt(cx * cx + cy * cy + cz * cz) + r;
            if (e * e > ext2) ext2 = e * e;
        }
        for (int k = 0; k < L; ++k) {
            const double x = lights[0 * L + k], y = lights[1 * L + k], z = lights[2 * L + k];
            if (soft) {                                                 // (the light's ball)
                const double e = std::sqrt(x * x + y * y + z * z) + (double)d.light_radius[k];
                if (e * e > ext2) ext2 = e * e;
            } else
            if (x * x + y * y + z * z > ext2) ext2 = x * x + y * y + z * z;
        }
        out.layout.extent2 = ext2;
    }

    void run()
    {
        if (!(check_sky() && check_table_width() && check_light_colours() && check_radii() && check_table() && check_sizes_ids() &&
              check_textures()))
            return;
        cluster_order();
        block_offsets();
        object_records();
        bounding_spheres();
        material_block();
        texture_block();
        lighting_block();
        sky_block();
        extent();
        SceneLayout &l = out.layout;
        l.S = d.S; l.P = d.P; l.L = d.L;
        l.M = d.M;
        l.mat_cols = cols;
        l.soft_n = soft ? d.shadow_samples : 0;
        l.T = textured ? d.T : 0;
        l.lit = lit;
        l.sky = has_sky;
        l.lens_mat = (long long)lens_off;
        l.tex_off = (long long)tex_off;
        l.lit_off = (long long)lit_off;
        l.sky_off = (long long)sky_off;
    }
};

}  // namespace detail

// Validates and packs one scene.  cluster_min: scenes with more spheres are stored in clusters; lanes_min_spheres: from that many
// on the cluster order is aligned to groups of rt::SUPER clusters (the lane-owned traversal's).  A status other than RT_OK
// comes with its error text and nothing else.
inline PackedScene pack_scene(const SceneDesc &desc, int cluster_min, int lanes_min_spheres)
{
    detail::Packer p(desc, cluster_min, lanes_min_spheres);
    try {
        p.run();
    } catch (const std::bad_alloc &) {
        p.fail(RT_ERR_ALLOC, "out of host memory");
    }
    if (p.out.status != RT_OK) { p.out.layout = SceneLayout(); p.out.rec.clear(); p.out.texels.clear(); }
    return std::move(p.out);
}

}  // namespace rt
