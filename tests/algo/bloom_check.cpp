/* The bloom's text without HIP (python-ray-tracer_amd/csrc/rt_bloom.h, and rt_film_bloom's check and arguments in rt_film_launch.h),
 * built with AddressSanitizer and UndefinedBehaviorSanitizer and run by tests/test_bloom.py.
 *
 *   bloom_check IN OUT   IN: int64 ncases, then per case int64 {ws, h, n, levels, pad_sum, pad_out, pad_work, compare}, float64
 *                        {threshold, strength} and the sum, 3 planes of ws*h + pad_sum float64.  OUT: per case the 3 * ws*h float64 of
 *                        `out` that the per-element functions give when the gather plan drives them.  Prints "cases=N ok".
 * Per case the program
 *   - walks bloom_plan(levels, RT_BLOOM_NO_TILES) with bloom_bright, bloom_x_pixel and bloom_y_pixel over heap buffers of exactly
 *     3 (out) and RT_BLOOM_WORK_PLANES (work) planes of ws*h + pad elements: the work planes start as NaN, the pads as a sentinel that
 *     must survive;
 *   - walks the plans that tile up to step 1, 2 and 4 with the tile kernel's phases, one emulated workgroup after another (a loop over
 *     the thread index in place of the workgroup, a barrier where one phase's loop ends) over a fresh heap "LDS" of exactly
 *     BLOOM_LDS_DOUBLES doubles, and fails unless `out` has the gather plan's bits (compare == 0: non-finite sums, run for the
 *     sanitizers only).
 * Once, it checks every plan (levels 0..8, both flag values, every max_step): a launch reads what an earlier one wrote and never what
 * it writes, out is written first and then updated once per level in level order; and every refusal of check_film_bloom with its
 * literal text, in the header's order. */
#include "../../python-ray-tracer_amd/csrc/rt_film_launch.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

static void die(const std::string &what)
{
    std::fprintf(stderr, "%s\n", what.c_str());
    std::exit(1);
}

static const double SENTINEL = -7.25e77;

struct Case {
    int ws, h, levels;
    int64_t n;
    long long pad_sum, pad_out, pad_work;
    int compare;
    rt_bloom bl;
    std::unique_ptr<double[]> sum;      // exactly 3 * (npx + pad_sum)
};

struct Buffers {
    std::unique_ptr<double[]> out, work;
    long long out_stride, work_stride;
};

static Buffers fresh(const Case &c)
{
    const long long npx = (long long)c.ws * c.h;
    Buffers b;
    b.out_stride = npx + c.pad_out; b.work_stride = npx + c.pad_work;
    b.out.reset(new double[3 * b.out_stride]);
    b.work.reset(new double[RT_BLOOM_WORK_PLANES * b.work_stride]);
    for (long long i = 0; i < 3 * b.out_stride; ++i) b.out[i] = SENTINEL;
    for (int p = 0; p < RT_BLOOM_WORK_PLANES; ++p)
        for (long long i = 0; i < b.work_stride; ++i) b.work[p * b.work_stride + i] = i < npx ? std::numeric_limits<double>::quiet_NaN() : SENTINEL;
    return b;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static void pads_intact(const Case &c, const Buffers &b, const char *what)
{
    const long long npx = (long long)c.ws * c.h;
    for (int p = 0; p < 3; ++p)
        for (long long i = npx; i < b.out_stride; ++i) if (!same_bits(b.out[p * b.out_stride + i], SENTINEL)) die(std::string(what) + ": a pad of out was written");
    for (int p = 0; p < RT_BLOOM_WORK_PLANES; ++p)
        for (long long i = npx; i < b.work_stride; ++i) if (!same_bits(b.work[p * b.work_stride + i], SENTINEL)) die(std::string(what) + ": a pad of work was written");
}

// One launch on the CPU: the per-element functions over the frame, or the tile phases workgroup by workgroup.
static void run_launch(const rt::BloomLaunch &l, const rt::BloomArgs &a)
{
    if (l.kind == rt::BLOOM_TILE) {
        const int threads = 256;
        for (int tx = 0; tx < rt::bloom_tiles_x(a.ws); ++tx)
            for (int ty = 0; ty < rt::bloom_tiles_y(a.h); ++ty) {
                std::unique_ptr<double[]> lds(new double[rt::BLOOM_LDS_DOUBLES]);
                for (int i = 0; i < rt::BLOOM_LDS_DOUBLES; ++i) lds[i] = std::numeric_limits<double>::quiet_NaN();
                const int x0 = tx * rt::BLOOM_TX, y0 = ty * rt::BLOOM_TY;
                for (int c = 0; c < 3; ++c) {
                    for (int t = threads - 1; t >= 0; --t) rt::bloom_tile_load(a, lds.get(), t, threads, x0, y0, c);
                    for (int t = 0; t < threads; ++t) rt::bloom_tile_xpass(a, lds.get(), t, threads, x0, y0, c);
                    for (int t = threads - 1; t >= 0; --t) rt::bloom_tile_ypass(a, lds.get(), t, threads, x0, y0, c);
                }
            }
        return;
    }
    for (int x = 0; x < a.ws; ++x)
        for (int y = 0; y < a.h; ++y) {
            if (l.kind == rt::BLOOM_BRIGHT) rt::bloom_bright(a, (long long)x * a.h + y);
            else if (l.kind == rt::BLOOM_X) rt::bloom_x_pixel(a, x, y);
            else rt::bloom_y_pixel(a, x, y);
        }
}

static Buffers run_plan(const Case &c, int flags, int max_step)
{
    Buffers b = fresh(c);
    rt_bloom bl = c.bl;
    bl.flags = flags;
    const rt::Refusal r = rt::check_film_bloom(c.sum.get(), (long long)c.ws * c.h + c.pad_sum, c.ws, c.h, c.n, &bl, b.out.get(), b.out_stride,
                                               b.work.get(), b.work_stride);
    if (r.code != RT_OK) die(std::string("a case was refused: ") + r.msg);
    const rt::BloomPlan plan = rt::bloom_plan(bl.levels, bl.flags, max_step);
    for (int k = 0; k < plan.count; ++k)
        run_launch(plan.l[k], rt::bloom_args(plan.l[k], c.sum.get(), (long long)c.ws * c.h + c.pad_sum, c.ws, c.h, c.n, &bl, b.out.get(), b.out_stride,
                                             b.work.get(), b.work_stride));
    pads_intact(c, b, flags ? "gather" : "tile");
    return b;
}

// ---- every plan ------------------------------------------------------------------------------------------------------------------
static void check_plans()
{
    for (int levels = 0; levels <= RT_BLOOM_MAX_LEVELS; ++levels)
        for (int flags = 0; flags <= 1; ++flags)
            for (int max_step : {0, 1, 2, 4, rt::BLOOM_TILE_MAX_STEP}) {
                const rt::BloomPlan p = rt::bloom_plan(levels, flags, max_step);
                const std::string id = "plan(" + std::to_string(levels) + "," + std::to_string(flags) + "," + std::to_string(max_step) + ")";
                if (p.count < 1 || p.count > 1 + 2 * RT_BLOOM_MAX_LEVELS) die(id + ": count");
                // what each set holds: 0 nothing, else 1 + 2 * level + (1: t of the level, 0: b of the level)
                int holds[2] = {0, 0};
                int out_level = -2;                               // -2: out not written; -1: the mean; i: updated by level i
                for (int k = 0; k < p.count; ++k) {
                    const rt::BloomLaunch &l = p.l[k];
                    if (l.src >= 0 && l.src == l.dst) die(id + ": a launch reads the set it writes");
                    if (l.src > 1 || l.dst > 1) die(id + ": a set outside the work planes");
                    if (k == 0) {
                        if (l.kind != rt::BLOOM_BRIGHT || l.src != -1 || !l.out || l.dst != (levels > 0 ? 0 : -1)) die(id + ": the bright pass");
                        out_level = -1;
                        if (l.dst >= 0) holds[l.dst] = 1;         // b_0
                        continue;
                    }
                    if (l.kind == rt::BLOOM_BRIGHT || l.level < 0 || l.level >= levels || l.step != (1 << l.level)) die(id + ": level or step");
                    const bool tiled = l.step <= max_step && !flags;
                    const int b_i = 1 + 2 * l.level, t_i = b_i + 1, b_next = b_i + 2;
                    if (l.src < 0) die(id + ": no source");
                    if (l.kind == rt::BLOOM_X) {
                        if (tiled || holds[l.src] != b_i || l.out || l.dst < 0) die(id + ": the x pass");
                        holds[l.dst] = t_i;
                    } else {
                        if ((l.kind == rt::BLOOM_TILE) != tiled) die(id + ": tile or gather");
                        if (holds[l.src] != (tiled ? b_i : t_i)) die(id + ": a launch reads what no earlier one wrote");
                        if (!l.out || out_level != l.level - 1) die(id + ": out is not updated once per level in level order");
                        out_level = l.level;
                        if ((l.dst < 0) != (l.level == levels - 1)) die(id + ": only the last level stores no b");
                        if (l.dst >= 0) holds[l.dst] = b_next;
                    }
                }
                if (out_level != levels - 1) die(id + ": a level is missing");
            }
}

// ---- the refusals ----------------------------------------------------------------------------------------------------------------
struct BloomCall {
    const void *sum; int64_t sum_stride; int ws, h; int64_t n; rt_bloom bl; bool have_bl; const void *out; int64_t out_stride;
    const void *work; int64_t work_stride;
};

static void refused(const BloomCall &c, const char *want, const char *name)
{
    const rt::Refusal r = rt::check_film_bloom(c.sum, c.sum_stride, c.ws, c.h, c.n, c.have_bl ? &c.bl : nullptr, c.out, c.out_stride, c.work, c.work_stride);
    if (!want) {
        if (r.code != RT_OK) die(std::string(name) + ": refused: " + r.msg);
        return;
    }
    if (r.code != RT_ERR_BAD_ARG || !r.msg || std::strcmp(r.msg, want) != 0 || !r.entry || std::strcmp(r.entry, "rt_film_bloom") != 0)
        die(std::string(name) + ": got '" + (r.msg ? r.msg : "(accepted)") + "', want '" + want + "'");
}

static void check_refusals()
{
    static double s[4], o[4], w[4];
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const BloomCall good = {s, 12, 4, 3, 1, {255.0, 0.25, 6, 0}, true, o, 12, w, 12};
    refused(good, nullptr, "good");
    // the texts, in the header's order: case k breaks rule k and every rule behind it, and rule k's text comes back
    const char *const text[] = {"d_sum is NULL", "bl is NULL", "d_out is NULL", "ws*h outside 1..RT_FILM_MAX_PIXELS", "n < 1", "levels outside 0..8",
                                "threshold must be finite and >= 0", "strength must be finite and >= 0", "unknown flag bit",
                                "d_work is NULL with levels >= 1", "a plane stride is smaller than the frame",
                                "d_out and d_work must be buffers of their own"};
    const int rules = (int)(sizeof text / sizeof *text);
    for (int k = 0; k < rules; ++k) {
        BloomCall c = good;
        // (what breaks rule j; the buffers become equal, so the last rule is broken from the start)
        c.work = o;
        if (k <= 10) { c.sum_stride = 11; c.out_stride = 11; c.work_stride = 11; }
        if (k <= 9) c.work = nullptr;
        if (k <= 8) c.bl.flags = 2;
        if (k <= 7) c.bl.strength = -1.0;
        if (k <= 6) c.bl.threshold = nan;
        if (k <= 5) c.bl.levels = 9;
        if (k <= 4) c.n = 0;
        if (k <= 3) c.ws = 0;
        if (k <= 2) c.out = nullptr;
        if (k <= 1) c.have_bl = false;
        if (k <= 0) c.sum = nullptr;
        if (k == 9) c.out = w;                                    // (d_work NULL: the last rule cannot be broken through it; harmless)
        refused(c, text[k], text[k]);
    }
    // every rule alone, and its edges
    BloomCall c = good;
    c.ws = 1 << 14; c.h = (1 << 13) + 1; c.sum_stride = c.out_stride = c.work_stride = (int64_t)c.ws * c.h; refused(c, text[3], "area above");
    c.h = 1 << 13; c.sum_stride = c.out_stride = c.work_stride = (int64_t)1 << 27; refused(c, nullptr, "area at the limit");
    c = good; c.h = 0; refused(c, text[3], "h 0");
    c = good; c.ws = -1; refused(c, text[3], "ws -1");
    c = good; c.n = -3; refused(c, text[4], "n -3");
    c = good; c.bl.levels = -1; refused(c, text[5], "levels -1");
    c = good; c.bl.levels = 8; refused(c, nullptr, "levels 8");
    for (double v : {nan, inf, -inf, -1e-300}) {
        c = good; c.bl.threshold = v; refused(c, text[6], "threshold");
        c = good; c.bl.strength = v; refused(c, text[7], "strength");
    }
    c = good; c.bl.threshold = 0.0; c.bl.strength = 0.0; refused(c, nullptr, "zeros");
    c = good; c.bl.flags = RT_BLOOM_NO_TILES; refused(c, nullptr, "no tiles");
    c = good; c.bl.flags = -2; refused(c, text[8], "flags -2");
    c = good; c.bl.flags = 3; refused(c, text[8], "flags 3");
    c = good; c.work = nullptr; refused(c, text[9], "no work, levels 6");
    c.bl.levels = 0; c.work_stride = 0; refused(c, nullptr, "no work, levels 0: its stride does not count");
    c = good; c.sum_stride = 11; refused(c, text[10], "sum_stride");
    c = good; c.out_stride = 11; refused(c, text[10], "out_stride");
    c = good; c.work_stride = 11; refused(c, text[10], "work_stride");
    c = good; c.out = s; refused(c, text[11], "out == sum");
    c = good; c.work = s; refused(c, text[11], "work == sum");
    c = good; c.work = o; refused(c, text[11], "work == out");
}

// ---- the cases -------------------------------------------------------------------------------------------------------------------
int main(int argc, char **argv)
{
    if (argc != 3) die("usage: bloom_check IN OUT");
    static_assert(sizeof(rt_bloom) == 24, "rt_bloom is 24 bytes");
    static_assert(rt::BLOOM_LDS_BYTES == 51200 && 3 * rt::BLOOM_LDS_BYTES <= rt::CU_LDS, "three workgroups' tiles fit a CU's LDS");
    check_plans();
    check_refusals();
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) die("cannot open the files");
    int64_t ncases = 0;
    if (std::fread(&ncases, sizeof ncases, 1, in) != 1) die("short input");
    for (int64_t k = 0; k < ncases; ++k) {
        int64_t head[8];
        double set[2];
        if (std::fread(head, sizeof head, 1, in) != 1 || std::fread(set, sizeof set, 1, in) != 1) die("short input");
        Case c;
        c.ws = (int)head[0]; c.h = (int)head[1]; c.n = head[2]; c.levels = (int)head[3];
        c.pad_sum = head[4]; c.pad_out = head[5]; c.pad_work = head[6]; c.compare = (int)head[7];
        c.bl.threshold = set[0]; c.bl.strength = set[1]; c.bl.levels = c.levels; c.bl.flags = 0;
        const long long npx = (long long)c.ws * c.h, total = 3 * (npx + c.pad_sum);
        c.sum.reset(new double[total]);
        if ((long long)std::fread(c.sum.get(), sizeof(double), total, in) != total) die("short input");
        const Buffers g = run_plan(c, RT_BLOOM_NO_TILES, 0);
        for (int p = 0; p < 3; ++p)
            if (std::fwrite(g.out.get() + p * g.out_stride, sizeof(double), npx, out) != (size_t)npx) die("short write");
        for (int max_step : {1, 2, 4}) {
            if (c.levels == 0 && max_step > 1) continue;
            const Buffers t = run_plan(c, 0, max_step);
            if (!c.compare) continue;
            for (int p = 0; p < 3; ++p)
                for (long long e = 0; e < npx; ++e)
                    if (!same_bits(t.out[p * t.out_stride + e], g.out[p * g.out_stride + e])) {
                        char msg[256];
                        std::snprintf(msg, sizeof msg, "case %lld (%d x %d, levels %d), tiles up to step %d: plane %d element %lld is %.17g, the gather form's %.17g",
                                      (long long)k, c.ws, c.h, c.levels, max_step, p, e, t.out[p * t.out_stride + e], g.out[p * g.out_stride + e]);
                        die(msg);
                    }
        }
    }
    std::fclose(in);
    if (std::fclose(out) != 0) die("short write");
    std::printf("cases=%lld ok\n", (long long)ncases);
    return 0;
}
