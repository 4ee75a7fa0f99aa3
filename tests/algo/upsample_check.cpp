/* Guided upsampling's arithmetic (python-ray-tracer_amd/csrc/rt_upsample.h: upsample_pixel and what it calls, the text the upsample
 * kernel compiles) without HIP, over a table of frame pairs.  Built with AddressSanitizer and UndefinedBehaviorSanitizer and run by
 * tests/test_upsample.py, which writes the table and compares what this writes, bit for bit, with the numpy restatement
 * upsample_reference of python-ray-tracer_amd/upsample.py.
 *
 *   upsample_check IN OUT
 * IN:  int64 K; then K cases: int64 wl, hl, w, h, n, pad, demodulate, planes (every plane is pad elements longer than its frame; the
 *      low mean has `planes` planes, 3 or 4); float64 lo_grid[5], hi_grid[5], normal_cos; float64 lo[planes][wl*hl + pad];
 *      float32 lo_guides[8][wl*hl + pad]; float32 hi_guides[8][w*h + pad].
 * OUT: per case float64 out[3][w*h], float32 kind[w*h].
 * Every buffer is allocated at exactly its padded planes, so a tap outside a frame is an AddressSanitizer report, and the padding of
 * the outputs must come back as it was.  Each case runs a second time without the kind plane and must write the same bytes.  Prints
 * "cases=K ok". */
#include "../../python-ray-tracer_amd/csrc/rt_upsample.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

struct CaseHeader {
    int64_t wl, hl, w, h, n, pad, demodulate, planes;
    double lo_grid[5], hi_grid[5], normal_cos;
};
static_assert(sizeof(CaseHeader) == 8 * 8 + 11 * 8, "the table's records are packed");

template <class T> static bool read_all(std::FILE *in, std::vector<T> &v) { return std::fread(v.data(), sizeof(T), v.size(), in) == v.size(); }

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: upsample_check IN OUT\n"); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 2; }
    int64_t K = 0;
    if (std::fread(&K, sizeof K, 1, in) != 1 || K < 0 || K > (1 << 16)) { std::fprintf(stderr, "bad header\n"); return 2; }
    for (int64_t k = 0; k < K; ++k) {
        CaseHeader c;
        if (std::fread(&c, sizeof c, 1, in) != 1 || c.wl < 1 || c.hl < 1 || c.wl * c.hl > (1 << 20) || c.w < 1 || c.h < 1 ||
            c.w * c.h > (1 << 20) || c.pad < 0 || c.pad > 64 || c.n < 1 || (c.planes != 3 && c.planes != 4) ||
            (c.demodulate != 0 && c.demodulate != 1)) {
            std::fprintf(stderr, "bad case %lld\n", (long long)k);
            return 2;
        }
        const size_t nlo = (size_t)(c.wl * c.hl), slo = nlo + (size_t)c.pad, npx = (size_t)(c.w * c.h), stride = npx + (size_t)c.pad;
        std::vector<double> lo((size_t)c.planes * slo), res(3 * stride, -1.0), res2(3 * stride, -1.0);
        std::vector<float> lo_guides(8 * slo), hi_guides(8 * stride), kind(stride, -2.0f);
        if (!read_all(in, lo) || !read_all(in, lo_guides) || !read_all(in, hi_guides)) {
            std::fprintf(stderr, "short table\n");
            return 2;
        }
        rt::UpsampleArgs a = {};
        a.lo = lo.data(); a.lo_guides = lo_guides.data(); a.hi_guides = hi_guides.data(); a.out = res.data(); a.kind = kind.data();
        a.lo_stride = a.lo_guide_stride = (long long)slo; a.hi_guide_stride = a.out_stride = (long long)stride;
        a.wl = (int)c.wl; a.hl = (int)c.hl; a.w = (int)c.w; a.h = (int)c.h; a.n = (double)c.n;
        a.lo_px = c.lo_grid[0]; a.lo_y0 = c.lo_grid[1]; a.lo_dy = c.lo_grid[2]; a.lo_z0 = c.lo_grid[3]; a.lo_dz = c.lo_grid[4];
        a.hi_px = c.hi_grid[0]; a.hi_y0 = c.hi_grid[1]; a.hi_dy = c.hi_grid[2]; a.hi_z0 = c.hi_grid[3]; a.hi_dz = c.hi_grid[4];
        a.normal_cos = c.normal_cos; a.demod = (int)c.demodulate;
        for (int x = 0; x < a.w; ++x)
            for (int y = 0; y < a.h; ++y) rt::upsample_pixel(a, x, y);
        a.out = res2.data(); a.kind = nullptr;
        for (int x = 0; x < a.w; ++x)
            for (int y = 0; y < a.h; ++y) rt::upsample_pixel(a, x, y);
        if (std::memcmp(res.data(), res2.data(), res.size() * sizeof(double)) != 0) {
            std::fprintf(stderr, "the kind plane changes the output in case %lld\n", (long long)k);
            return 1;
        }
        for (size_t e = npx; e < stride; ++e) {
            if (res[e] != -1.0 || res[stride + e] != -1.0 || res[2 * stride + e] != -1.0 || kind[e] != -2.0f) {
                std::fprintf(stderr, "padding written in case %lld\n", (long long)k);
                return 1;
            }
        }
        for (int p = 0; p < 3; ++p)
            if (std::fwrite(res.data() + p * stride, sizeof(double), npx, out) != npx) { std::fprintf(stderr, "write failed\n"); return 2; }
        if (std::fwrite(kind.data(), sizeof(float), npx, out) != npx) { std::fprintf(stderr, "write failed\n"); return 2; }
    }
    std::fclose(in);
    if (std::fclose(out) != 0) { std::fprintf(stderr, "write failed\n"); return 2; }
    std::printf("cases=%lld ok\n", (long long)K);
    return 0;
}
