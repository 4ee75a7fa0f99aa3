/* The CPU oracle under AddressSanitizer + UndefinedBehaviorSanitizer (sanitizers run on the CPU build
 * only).  Reads one scene dump written by tests/test_algorithms.py, renders it through orc_render (all AA modes,
 * whole frame and an unaligned slab, explicit pixel grid and closed form) and orc_render_pixels, and writes the bytes
 * back, then the same through the feature path (orc_render_ex, orc_render_pixels_ex) with the dump's material table,
 * light radii and lens, and once more with the dump's texture records, ids and texels (a texel range that ends exactly at the
 * array's end, axes that clamp), light colours, 8-column table and sky; the test compares them with the regular build.  Any
 * sanitizer report aborts the run (exit != 0). */
#include "../../oracle/rt_oracle.c"
#include <stdio.h>

static void *slurp(FILE *f, size_t n) { void *p = malloc(n ? n : 1); if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } return p; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[8];   /* w h S L P depth spp seed */
    if (fread(hdr, sizeof hdr, 1, f) != 1) return 2;
    const int w = hdr[0], h = hdr[1], S = hdr[2], L = hdr[3], P = hdr[4], depth = hdr[5], spp = hdr[6];
    double *cam = slurp(f, 12 * sizeof(double));          /* origin[3], rotation[9] */
    double *rg = slurp(f, 5 * sizeof(double));            /* px y0 dy z0 dz */
    double *sc = slurp(f, (3 + depth) * sizeof(double));  /* amb lamb refl, refl_pow[depth] */
    float *sp = slurp(f, 7 * (size_t)S * 4), *li = slurp(f, 3 * (size_t)L * 4), *pl = slurp(f, 9 * (size_t)P * 4);
    orc_raygen g = { w, h, NULL, rg[0], rg[1], rg[2], rg[3], rg[4] };
    const size_t n = (size_t)3 * w * h;
    uint8_t *u8 = malloc(n); double *f64 = malloc(n * 8); float *f32 = malloc(n * 4);
    long long counters[3];
    FILE *o = fopen(argv[2], "wb");
    const int modes[3] = { 0, 1, 0x100 | spp };
    for (int m = 0; m < 3; ++m) {
        memset(u8, 0, n);
        if (orc_render(&g, cam, cam + 3, sp, S, li, L, pl, P, sc[0], sc[1], sc + 3, depth, modes[m], 0, 0, w, u8, f64, f32, counters, 2, (uint32_t)hdr[7])) return 3;
        fwrite(u8, 1, n, o); fwrite(f32, 4, n, o);
    }
    /* an unaligned slab with the typed-bias flag; only columns [x0,x1) are written */
    memset(u8, 0, n);
    if (orc_render(&g, cam, cam + 3, sp, S, li, L, pl, P, sc[0], sc[1], sc + 3, depth, 1, ORC_FLAG_TYPED_BIAS, w / 3, w - 2, u8, NULL, NULL, NULL, 1, 0)) return 3;
    fwrite(u8, 1, n, o);
    /* explicit pixel grid */
    double *grid = malloc(n * 8);
    for (int x = 0; x < w; ++x) for (int y = 0; y < h; ++y) {
        grid[(size_t)x * h + y] = rg[0]; grid[(size_t)w * h + (size_t)x * h + y] = x * rg[2] + rg[1]; grid[(size_t)2 * w * h + (size_t)x * h + y] = y * rg[4] + rg[3];
    }
    orc_raygen ge = { w, h, grid, 0, 0, 0, 0, 0 };
    memset(u8, 0, n);
    if (orc_render(&ge, cam, cam + 3, sp, S, li, L, pl, P, sc[0], sc[1], sc + 3, depth, 1, 0, 0, w, u8, NULL, NULL, NULL, 2, 0)) return 3;
    fwrite(u8, 1, n, o);
    /* sparse pixels, incl. the frame's corners */
    int32_t co[8] = { 0, 0, w - 1, h - 1, w / 2, h / 2, w - 1, 0 };
    uint8_t px[12]; double pf[12];
    if (orc_render_pixels(&g, cam, cam + 3, sp, S, li, L, pl, P, sc[0], sc[1], sc + 3, depth, 1, 0, co, 4, px, pf, 1, 0)) return 3;
    fwrite(px, 1, 12, o);
    /* rejected arguments must not touch memory */
    if (orc_render(&g, cam, cam + 3, sp, S, li, L, pl, P, sc[0], sc[1], sc + 3, depth, 0, 0, 5, w + 1, u8, NULL, NULL, NULL, 1, 0) != -1) return 4;
    co[0] = w;
    if (orc_render_pixels(&g, cam, cam + 3, sp, S, li, L, pl, P, sc[0], sc[1], sc + 3, depth, 0, 0, co, 4, px, pf, 1, 0) != -1) return 4;
    /* the feature path (orc_render_ex / orc_render_pixels_ex): the dump's material table, ids, light radii, shadow samples
     * and lens, every AA mode, the explicit grid, an unaligned typed-bias slab, sparse pixels and refused input */
    int fh[3];   /* M ncols n */
    if (fread(fh, sizeof fh, 1, f) != 1) return 2;
    double *tab = slurp(f, (size_t)fh[0] * fh[1] * sizeof(double));
    int32_t *sid = slurp(f, (size_t)S * 4), *pid = slurp(f, (size_t)P * 4);
    float *rad = slurp(f, (size_t)L * 4);
    double *lens = slurp(f, 2 * sizeof(double));
    /* textures, lighting and the sky: T, the records, n_texels, the ids, the texels, light_rgb, M8 and an 8-column table, the sky */
    int T, M8;
    int64_t n_texels;
    if (fread(&T, sizeof T, 1, f) != 1) return 2;
    orc_texture *recs = slurp(f, (size_t)T * sizeof(orc_texture));
    if (fread(&n_texels, sizeof n_texels, 1, f) != 1) return 2;
    int32_t *tsid = slurp(f, (size_t)S * 4), *tpid = slurp(f, (size_t)P * 4);
    float *texels = slurp(f, (size_t)n_texels * 12);            /* exactly n_texels texels: one read past the end is a report */
    float *lrgb = slurp(f, (size_t)L * 12);
    if (fread(&M8, sizeof M8, 1, f) != 1) return 2;
    double *tab8 = slurp(f, (size_t)M8 * 8 * sizeof(double));
    double *sky = slurp(f, ORC_SKY_DOUBLES * sizeof(double));
    fclose(f);
    orc_features fe = { fh[0], fh[1], tab, sid, pid, L ? rad : NULL, fh[2], lens[0], lens[1], 0 };
    for (int m = 0; m < 3; ++m) {
        memset(u8, 0, n);
        if (orc_render_ex(&g, cam, cam + 3, sp, S, li, L, pl, P, 0, 0, sc + 3, depth, modes[m], 0, 0, w, u8, f64, f32, counters, 2, (uint32_t)hdr[7], &fe)) return 5;
        fwrite(u8, 1, n, o); fwrite(f32, 4, n, o);
    }
    memset(u8, 0, n);
    if (orc_render_ex(&g, cam, cam + 3, sp, S, li, L, pl, P, 0, 0, sc + 3, depth, 1, ORC_FLAG_TYPED_BIAS, w / 3, w - 2, u8, NULL, NULL, NULL, 1, 3, &fe)) return 5;
    fwrite(u8, 1, n, o);
    memset(u8, 0, n);
    if (orc_render_ex(&ge, cam, cam + 3, sp, S, li, L, pl, P, 0, 0, sc + 3, depth, 1, 0, 0, w, u8, NULL, NULL, NULL, 2, 3, &fe)) return 5;
    fwrite(u8, 1, n, o);
    co[0] = 0;
    if (orc_render_pixels_ex(&g, cam, cam + 3, sp, S, li, L, pl, P, 0, 0, sc + 3, depth, 0x100 | spp, 0, co, 4, px, pf, 1, 3, &fe)) return 5;
    fwrite(px, 1, 12, o); fwrite(pf, 8, 12, o);
    fe.shadow_samples = 17;                                 /* refused: nothing is written */
    if (orc_render_ex(&g, cam, cam + 3, sp, S, li, L, pl, P, 0, 0, sc + 3, depth, 0, 0, 0, w, u8, NULL, NULL, NULL, 1, 0, &fe) != -1) return 6;
    fe.shadow_samples = fh[2]; fe.M = 0;                    /* a lens without a table */
    if (fe.aperture > 0 && orc_render_pixels_ex(&g, cam, cam + 3, sp, S, li, L, pl, P, 0, 0, sc + 3, depth, 0, 0, co, 4, px, pf, 1, 0, &fe) != -1) return 6;
    /* textures, coloured lights, highlights and the sky through the same entry points */
    orc_features fl = { M8, 8, tab8, sid, pid, L ? rad : NULL, fh[2], lens[0], lens[1], 0, T, recs, tsid, tpid, texels, n_texels,
                        L ? lrgb : NULL, sky };
    for (int m = 0; m < 3; ++m) {
        memset(u8, 0, n);
        if (orc_render_ex(&g, cam, cam + 3, sp, S, li, L, pl, P, 0, 0, sc + 3, depth, modes[m], 0, 0, w, u8, f64, f32, counters, 2, (uint32_t)hdr[7], &fl)) return 7;
        fwrite(u8, 1, n, o); fwrite(f32, 4, n, o);
    }
    memset(u8, 0, n);
    if (orc_render_ex(&ge, cam, cam + 3, sp, S, li, L, pl, P, 0, 0, sc + 3, depth, 1, ORC_FLAG_TYPED_BIAS, w / 3, w - 2, u8, NULL, NULL, NULL, 1, 3, &fl)) return 7;
    fwrite(u8, 1, n, o);
    co[0] = 0;
    if (orc_render_pixels_ex(&g, cam, cam + 3, sp, S, li, L, pl, P, 0, 0, sc + 3, depth, 0x100 | spp, 0, co, 4, px, pf, 1, 3, &fl)) return 7;
    fwrite(px, 1, 12, o); fwrite(pf, 8, 12, o);
    fl.textures = NULL; fl.sphere_texture = fl.plane_texture = NULL; fl.T = 0;   /* NULL id arrays: every id -1 */
    if (orc_render_pixels_ex(&g, cam, cam + 3, sp, S, li, L, pl, P, 0, 0, sc + 3, depth, 0, 0, co, 4, px, pf, 1, 3, &fl)) return 7;
    fwrite(px, 1, 12, o); fwrite(pf, 8, 12, o);
    fl.textures = recs; fl.sphere_texture = tsid; fl.plane_texture = tpid; fl.T = T;
    /* refused input returns -1 and touches nothing: the outputs keep their fill */
    memset(u8, 0xAB, n); memset(px, 0xCD, sizeof px);
#define REFUSED(code) do { \
        if (orc_render_ex(&g, cam, cam + 3, sp, S, li, L, pl, P, 0, 0, sc + 3, depth, 0, 0, 0, w, u8, NULL, NULL, NULL, 1, 0, &fl) != -1) return code; \
        if (orc_render_pixels_ex(&g, cam, cam + 3, sp, S, li, L, pl, P, 0, 0, sc + 3, depth, 0, 0, co, 4, px, NULL, 1, 0, &fl) != -1) return code; \
        for (size_t i = 0; i < n; ++i) if (u8[i] != 0xAB) return code; \
        for (size_t i = 0; i < sizeof px; ++i) if (px[i] != 0xCD) return code; } while (0)
    if (T > 0) {
        const orc_texture keep = recs[T - 1];                   /* the record whose range ends exactly at the array's end */
        if (keep.first + (int64_t)keep.dim[0] * keep.dim[1] * keep.dim[2] != n_texels) return 8;
        recs[T - 1].first += 1; REFUSED(8);                     /* one texel past the end */
        recs[T - 1] = keep; recs[T - 1].first = -1; REFUSED(8);
        recs[T - 1] = keep; recs[T - 1].dim[2] = 4097; REFUSED(8);
        recs[T - 1] = keep; recs[T - 1].dim[0] = 0; REFUSED(8);
        recs[T - 1] = keep; recs[T - 1].reserved = 1; REFUSED(8);
        recs[T - 1] = keep; recs[T - 1].axis[1][2] = NAN; REFUSED(8);
        recs[T - 1] = keep;
        fl.n_texels = n_texels - 1; REFUSED(8);                 /* the same range against a shorter array */
        fl.n_texels = ((int64_t)1 << 22) + 1; REFUSED(8);
        fl.n_texels = n_texels;
        fl.T = 65; REFUSED(8);
        fl.T = T;
        fl.texels = NULL; REFUSED(8);
        fl.texels = texels;
        if (S > 0) { const int32_t id = tsid[0]; tsid[0] = T; REFUSED(8); tsid[0] = -2; REFUSED(8); tsid[0] = id; }
        if (P > 0) { const int32_t id = tpid[P - 1]; tpid[P - 1] = T; REFUSED(8); tpid[P - 1] = id; }
        fl.M = 0; REFUSED(8);                                   /* textures without a table */
        fl.M = M8;
    }
    if (L > 0) {
        const float e = lrgb[3 * L - 1];
        lrgb[3 * L - 1] = -1.0f; REFUSED(9);
        lrgb[3 * L - 1] = INFINITY; REFUSED(9);
        lrgb[3 * L - 1] = e;
    }
    { const double v = tab8[7]; tab8[7] = 3.0; REFUSED(9); tab8[7] = 2048.0; REFUSED(9); tab8[7] = v; }
    { const double v = tab8[6]; tab8[6] = -1.0; REFUSED(9); tab8[6] = v; }
    fl.ncols = 7; REFUSED(9);
    fl.ncols = 8;
    { const double v = sky[12]; sky[12] = 3.0; REFUSED(10); sky[12] = v; }
    { const double v = sky[23]; sky[23] = 2048.0; REFUSED(10); sky[23] = v; }
    { const double v = sky[1]; sky[1] = v + 0.5; REFUSED(10); sky[1] = v; }
    { const double v = sky[14]; sky[14] = v + 0.5; REFUSED(10); sky[14] = v; }
    { const double v = sky[20]; sky[20] = -1.0; REFUSED(10); sky[20] = NAN; REFUSED(10); sky[20] = v; }
    fl.M = 0; fl.T = 0; REFUSED(10);                            /* a sky (and coloured lights) without a table */
    fl.M = M8; fl.T = T;
    if (orc_render_pixels_ex(&g, cam, cam + 3, sp, S, li, L, pl, P, 0, 0, sc + 3, depth, 0, 0, co, 4, px, pf, 1, 3, &fl)) return 11;   /* restored: accepted */
    fwrite(px, 1, 12, o);
    fclose(o);
    free(recs); free(tsid); free(tpid); free(texels); free(lrgb); free(tab8); free(sky);
    free(tab); free(sid); free(pid); free(rad); free(lens);
    free(u8); free(f64); free(f32); free(grid); free(cam); free(rg); free(sc); free(sp); free(li); free(pl);
    printf("ok\n");
    return 0;
}
