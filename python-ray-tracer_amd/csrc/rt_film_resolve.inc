// rt_film_resolve.inc — the body of the film's two resolve kernels (rt_film.h: film_resolve_kernel, film_resolve_metered_kernel), included
// once in each with the kernel's argument `a` (FilmResolveArgs) in scope.  Text and not a function: behind a __forceinline__ function
// (film_add_body's way) the compiler orders and allocates film_resolve_kernel's instructions differently (16 to 44 of its 3 111 lines,
// depending on the form tried; DESIGN.md: Metering), and that kernel's instruction stream is kept as it was.
// A thread resolves groups of four consecutive elements of a column run (all three channels: the image layout interleaves them)
// in a grid-stride loop; the first npx mod 4 threads of block 0 the pixels behind the last group.
    const double *const s0 = a.sum, *const s1 = a.sum + a.sum_stride, *const s2 = a.sum + 2 * a.sum_stride;
    const bool v0 = film_aligned(s0, 16), v1 = film_aligned(s1, 16), v2 = film_aligned(s2, 16);
    // the uint8 planes in stored order: (R,B,G) unless RT_FLAG_U8_RGB
    float *const f0 = a.f32, *const f1 = a.f32 + a.out_stride, *const f2 = a.f32 + 2 * a.out_stride;
    const bool w0 = film_aligned(f0, 16), w1 = film_aligned(f1, 16), w2 = film_aligned(f2, 16);
    uint8_t *const u0 = a.u8, *const u1 = a.u8 + a.out_stride, *const u2 = a.u8 + 2 * a.out_stride;
    const bool b0 = film_aligned(u0, 4), b1 = film_aligned(u1, 4), b2 = film_aligned(u2, 4);
    const long long ngroups = a.npx >> 2, step = (long long)gridDim.x * FILM_THREADS;
    for (long long g = (long long)blockIdx.x * FILM_THREADS + threadIdx.x; g < ngroups; g += step) {
        const long long e = g << 2;
        double R[4], G[4], B[4];
        film_load4(s0 + e, v0, R);
        film_load4(s1 + e, v1, G);
        film_load4(s2 + e, v2, B);
#pragma unroll
        for (int i = 0; i < 4; ++i) { R[i] = film_tone(R[i], a.tone); G[i] = film_tone(G[i], a.tone); B[i] = film_tone(B[i], a.tone); }
        if (a.f32) {
            film_store_f32x4(f0 + e, w0, R);
            film_store_f32x4(f1 + e, w1, G);
            film_store_f32x4(f2 + e, w2, B);
        }
        if (a.u8) {
            if (a.hwc) {
#pragma unroll
                for (int i = 0; i < 4; ++i) film_store_u8_pixel(a, e + i, R[i], G[i], B[i]);
            } else {
                film_store_u8x4(u0 + e, b0, R);
                film_store_u8x4(u1 + e, b1, a.rgb ? G : B);
                film_store_u8x4(u2 + e, b2, a.rgb ? B : G);
            }
        }
    }
    if (blockIdx.x == 0 && (long long)threadIdx.x < (a.npx & 3)) {
        const long long e = (ngroups << 2) + threadIdx.x;
        const double R = film_tone(s0[e], a.tone), G = film_tone(s1[e], a.tone), B = film_tone(s2[e], a.tone);
        if (a.f32) { f0[e] = (float)R; f1[e] = (float)G; f2[e] = (float)B; }
        if (a.u8) film_store_u8_pixel(a, e, R, G, B);
    }
