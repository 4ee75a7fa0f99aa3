/* The film's arithmetic (python-ray-tracer_amd/csrc/rt_film.h: film_add, film_tone, film_clip, the text the two film kernels
 * compile) without HIP, over a table of cases.  Built with AddressSanitizer and UndefinedBehaviorSanitizer and run by
 * tests/test_film.py, which writes the table and compares what this writes, bit for bit, with the numpy restatement of
 * python-ray-tracer_amd/film.py.
 *
 *   film_check IN OUT
 * IN:  int64 T, int64 A; T tone cases {float64 s, int64 n, float64 exposure, float64 white, int64 gamma} (40 bytes each); A add
 *      cases {float64 sum, int64 count (0..9), int64 reset, float32 addend[9], 4 bytes of padding} (64 bytes each).
 * OUT: float64 v[T] (film_tone), float32 f[T] ((float)v), uint8 u[T] (film_clip(v)), then float64 s[A] (film_add, left to right,
 *      from +0.0 where reset is set).
 * Prints "tone=T add=A ok". */
#include "../../python-ray-tracer_amd/csrc/rt_film.h"

#include <cstdint>
#include <cstdio>
#include <vector>

struct ToneCase { double s; int64_t n; double exposure, white; int64_t gamma; };
struct AddCase { double sum; int64_t count, reset; float addend[9]; float pad; };
static_assert(sizeof(ToneCase) == 40 && sizeof(AddCase) == 64, "the table's records are packed");

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: film_check IN OUT\n"); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    int64_t counts[2] = {0, 0};
    if (std::fread(counts, sizeof counts, 1, in) != 1 || counts[0] < 0 || counts[1] < 0 || counts[0] > (1 << 24) || counts[1] > (1 << 24)) {
        std::fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<ToneCase> tone((size_t)counts[0]);
    std::vector<AddCase> add((size_t)counts[1]);
    if ((!tone.empty() && std::fread(tone.data(), sizeof(ToneCase), tone.size(), in) != tone.size()) ||
        (!add.empty() && std::fread(add.data(), sizeof(AddCase), add.size(), in) != add.size())) {
        std::fprintf(stderr, "short table\n");
        return 2;
    }
    std::fclose(in);

    std::vector<double> v(tone.size()), s(add.size());
    std::vector<float> f(tone.size());
    std::vector<uint8_t> u(tone.size());
    for (size_t i = 0; i < tone.size(); ++i) {
        const rt::FilmTone t = rt::film_tone_of(tone[i].n, tone[i].exposure, tone[i].white, (int)tone[i].gamma);
        v[i] = rt::film_tone(tone[i].s, t);
        f[i] = (float)v[i];
        u[i] = rt::film_clip(v[i]);
    }
    for (size_t i = 0; i < add.size(); ++i) {
        if (add[i].count < 0 || add[i].count > 9) { std::fprintf(stderr, "bad addend count\n"); return 2; }
        double acc = add[i].reset ? 0.0 : add[i].sum;
        for (int64_t k = 0; k < add[i].count; ++k) acc = rt::film_add(acc, add[i].addend[k]);
        s[i] = acc;
    }

    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 2; }
    bool ok = true;
    if (!v.empty()) ok = std::fwrite(v.data(), sizeof(double), v.size(), out) == v.size() &&
                         std::fwrite(f.data(), sizeof(float), f.size(), out) == f.size() &&
                         std::fwrite(u.data(), 1, u.size(), out) == u.size();
    if (ok && !s.empty()) ok = std::fwrite(s.data(), sizeof(double), s.size(), out) == s.size();
    if (std::fclose(out) != 0 || !ok) { std::fprintf(stderr, "write failed\n"); return 2; }
    std::printf("tone=%zu add=%zu ok\n", tone.size(), add.size());
    return 0;
}
