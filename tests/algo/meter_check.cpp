/* The meter's text without HIP (python-ray-tracer_amd/csrc/rt_meter.h, and the checks and arguments of rt_film_meter, rt_film_meter_solve
 * and rt_film_resolve_metered in rt_film_launch.h), built with AddressSanitizer and UndefinedBehaviorSanitizer and run by
 * tests/test_meter.py.
 *
 *   meter_check IN OUT   IN: int64 ncases, then per case int64 {ws, h, n, pad_sum, nblocks} and the sum, 3 planes of ws*h + pad_sum
 *                        float64; then int64 nsolves, and per solve RT_METER_BINS uint64 counts, RT_METER_STATE_DOUBLES float64 of state
 *                        and float64 {key, percentile, min_exposure, max_exposure, rate}.
 *                        OUT: per case the RT_METER_BINS uint64 counts; per solve the state after it.  Prints "cases=N solves=M ok".
 * Per case the program emulates meter_hist_kernel: `nblocks` workgroups one after another, each over a fresh heap "LDS" of exactly
 * METER_LDS_WORDS uint32 that starts as garbage, its three phases as loops over the thread index (a barrier where one phase's loop
 * ends), into counts that stand between two sentinel words.  The sum is a heap buffer of exactly 3 * (ws*h + pad_sum) float64 whose
 * pads hold 1e300, which would land in bin 322.  The frame is then metered again as two column slabs without a reset, with another
 * number of workgroups, and must give the same counts.
 * Once, it checks meter_bin and meter_edge on the contract's examples, and every refusal of the three checks with its literal text, in
 * the header's order. */
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

static const uint64_t SENTINEL = 0xfeedfacecafebeefull;
static const int THREADS = rt::METER_THREADS;

/* counts between two sentinel words */
struct Counts {
    std::unique_ptr<uint64_t[]> words;
    Counts() : words(new uint64_t[RT_METER_BINS + 2])
    {
        for (int i = 0; i < RT_METER_BINS + 2; ++i) words[i] = SENTINEL;       /* (a reset must zero what is there) */
    }
    uint64_t *hist() { return words.get() + 1; }
    void intact(const char *what) const
    {
        if (words[0] != SENTINEL || words[RT_METER_BINS + 1] != SENTINEL) die(std::string(what) + ": a word beside the counts was written");
    }
};

/* rt_film_meter on the CPU: the check, the reset, then the kernel's phases workgroup by workgroup */
static void meter(const double *sum, int64_t sum_stride, int ws, int h, int64_t n, int reset, uint64_t *hist, int nblocks)
{
    const rt::Refusal r = rt::check_film_meter(sum, sum_stride, ws, h, n, hist);
    if (r.code != RT_OK) die(std::string("a case was refused: ") + r.msg);
    const rt::MeterHistArgs a = rt::meter_hist_args(sum, sum_stride, ws, h, n, hist);
    if (reset) for (int b = 0; b < RT_METER_BINS; ++b) hist[b] = 0;
    for (int block = 0; block < nblocks; ++block) {
        std::unique_ptr<uint32_t[]> lds(new uint32_t[rt::METER_LDS_WORDS]);
        for (int i = 0; i < rt::METER_LDS_WORDS; ++i) lds[i] = 0xdeadbeefu;
        for (int t = THREADS - 1; t >= 0; --t) rt::meter_lds_clear(lds.get(), t, THREADS);
        for (int t = 0; t < THREADS; ++t) rt::meter_count(a, lds.get(), t, THREADS, block, nblocks);
        for (int t = THREADS - 1; t >= 0; --t) rt::meter_flush(a, lds.get(), t, THREADS);
    }
}

/* ---- the contract's examples ------------------------------------------------------------------------------------------------------ */
static void check_bins()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double lo = std::ldexp(1.0, -16), hi = std::ldexp(1.0, 24);
    struct { double y; int bin; } ex[] = {{lo, 2}, {std::nextafter(lo, 0.0), 1}, {1.0, 130}, {1.125, 131}, {255.0, 193}, {hi, 322}, {inf, 322},
                                          {std::nextafter(hi, 0.0), 321}, {5e-324, 1}, {0.0, 0}, {-0.0, 0}, {-1.0, 0}, {-inf, 0}, {nan, 0}};
    for (const auto &e : ex)
        if (rt::meter_bin(e.y) != e.bin) die("meter_bin(" + std::to_string(e.y) + ") is " + std::to_string(rt::meter_bin(e.y)) + ", not " + std::to_string(e.bin));
    if (rt::meter_edge(2) != lo || rt::meter_edge(322) != hi || rt::meter_edge(130) != 1.0 || rt::meter_edge(131) != 1.125) die("meter_edge");
    for (int b = 2; b < RT_METER_BINS; ++b) {
        const double e = rt::meter_edge(b);
        if (rt::meter_bin(e) != b || rt::meter_bin(std::nextafter(e, 0.0)) != b - 1) die("edge " + std::to_string(b) + " does not open its bin");
        int ex2 = 0;
        const double f = std::frexp(e, &ex2) * 16.0;                  /* (1 + j/8) * 2^E: sixteenths of the leading power of two */
        if (f != std::floor(f) || f < 8.0 || f >= 16.0) die("edge " + std::to_string(b) + " is not (1 + j/8) 2^E");
    }
    if (rt::meter_luminance(1.0, 1.0, 1.0) != (0.2126 + 0.7152) + 0.0722) die("meter_luminance");
    static_assert(rt::METER_LDS_BYTES == (size_t)rt::METER_COPIES * 323 * 4 && 8 * rt::METER_LDS_BYTES <= rt::CU_LDS, "eight workgroups' counters fit a CU's LDS");
}

/* ---- the refusals ----------------------------------------------------------------------------------------------------------------- */
static void expect(const rt::Refusal &r, const char *want, const char *entry, const std::string &name)
{
    if (!want) {
        if (r.code != RT_OK) die(name + ": refused: " + r.msg);
        return;
    }
    if (r.code != RT_ERR_BAD_ARG || !r.msg || std::strcmp(r.msg, want) != 0) die(name + ": got '" + (r.msg ? r.msg : "(accepted)") + "', want '" + want + "'");
    if (entry && (!r.entry || std::strcmp(r.entry, entry) != 0)) die(name + ": the refusal does not carry " + entry);
    if (!entry && r.entry) die(name + ": the refusal names an entry");
}

struct MeterCall { const void *sum; int64_t stride; int ws, h; int64_t n; const void *hist; };
struct SolveCall { const void *hist; rt_meter mt; bool have_mt; const void *state; };
struct ResolveCall { const void *sum; int64_t stride; int ws, h; int64_t n; rt_film_tone tone; bool have_tone; const void *state, *u8, *f32; int64_t out_stride; };

static rt::Refusal run(const MeterCall &c) { return rt::check_film_meter(c.sum, c.stride, c.ws, c.h, c.n, c.hist); }
static rt::Refusal run(const SolveCall &c) { return rt::check_film_meter_solve(c.hist, c.have_mt ? &c.mt : nullptr, c.state); }
static rt::Refusal run(const ResolveCall &c)
{
    return rt::check_film_resolve_metered(c.sum, c.stride, c.ws, c.h, c.n, c.have_tone ? &c.tone : nullptr, c.state, c.u8, c.f32, c.out_stride);
}

static void check_refusals()
{
    alignas(16) static double s[4];
    alignas(16) static uint64_t hs[4];
    alignas(16) static double st[4];
    alignas(16) static unsigned char o8[4];
    alignas(16) static float o32[4];
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const char *const M = "rt_film_meter", *const S = "rt_film_meter_solve", *const R = "rt_film_resolve_metered";

    /* rt_film_meter: case k breaks rule k and every rule behind it, and rule k's text comes back */
    const MeterCall mgood = {s, 12, 4, 3, 1, hs};
    expect(run(mgood), nullptr, M, "meter good");
    const char *const mtext[] = {"d_sum is NULL", "d_hist is NULL", "ws*h outside 1..RT_FILM_MAX_PIXELS", "n < 1", "sum_stride smaller than the frame",
                                 "d_hist is not 8-byte aligned", "d_hist and d_sum must be buffers of their own"};
    for (int k = 0; k < 7; ++k) {
        MeterCall c = mgood;
        c.hist = s;                                                   /* the last rule is broken from the start */
        if (k <= 5) c.hist = (const char *)s + 4;
        if (k <= 4) c.stride = 11;
        if (k <= 3) c.n = 0;
        if (k <= 2) c.ws = 0;
        if (k <= 1) c.hist = nullptr;
        if (k <= 0) c.sum = nullptr;
        expect(run(c), mtext[k], M, std::string("meter: ") + mtext[k]);
    }
    MeterCall m = mgood;
    m.ws = 1 << 14; m.h = (1 << 13) + 1; m.stride = (int64_t)m.ws * m.h; expect(run(m), mtext[2], M, "meter area above");
    m.h = 1 << 13; m.stride = (int64_t)1 << 27; expect(run(m), nullptr, M, "meter area at the limit");
    m = mgood; m.h = -1; expect(run(m), mtext[2], M, "meter h -1");
    m = mgood; m.n = -5; expect(run(m), mtext[3], M, "meter n -5");
    m = mgood; m.stride = 12; expect(run(m), nullptr, M, "meter stride at the frame");
    for (int off = 1; off < 8; ++off) { m = mgood; m.hist = (const char *)hs + off; expect(run(m), mtext[5], M, "meter misaligned counts"); }

    /* rt_film_meter_solve */
    const SolveCall sgood = {hs, {46.0, 0.5, 1.0 / 1024, 1024.0, 1.0, 0, 0}, true, st};
    expect(run(sgood), nullptr, S, "solve good");
    const char *const stext[] = {"d_hist is NULL", "mt is NULL", "d_state is NULL", "key must be finite and > 0", "percentile outside 0..1",
                                 "min_exposure must be finite and > 0", "max_exposure must be finite and > 0", "min_exposure above max_exposure",
                                 "rate outside (0, 1]", "flags must be 0", "reserved must be 0", "d_state and d_hist must be buffers of their own"};
    for (int k = 0; k < 12; ++k) {
        SolveCall c = sgood;
        c.state = hs;
        if (k <= 10) c.mt.reserved = 1;
        if (k <= 9) c.mt.flags = 1;
        if (k <= 8) c.mt.rate = 0.0;
        if (k <= 7) { c.mt.min_exposure = 4.0; c.mt.max_exposure = 2.0; }
        if (k <= 6) c.mt.max_exposure = inf;
        if (k <= 5) c.mt.min_exposure = 0.0;
        if (k <= 4) c.mt.percentile = 1.5;
        if (k <= 3) c.mt.key = nan;
        if (k <= 2) c.state = nullptr;
        if (k <= 1) c.have_mt = false;
        if (k <= 0) c.hist = nullptr;
        expect(run(c), stext[k], S, std::string("solve: ") + stext[k]);
    }
    SolveCall c = sgood;
    for (double v : {nan, inf, -inf, 0.0, -1.0}) {
        c = sgood; c.mt.key = v; expect(run(c), stext[3], S, "solve key");
        c = sgood; c.mt.min_exposure = v; expect(run(c), stext[5], S, "solve min_exposure");
        c = sgood; c.mt.max_exposure = v; expect(run(c), stext[6], S, "solve max_exposure");
    }
    for (double v : {nan, -1e-300, 1.0000000000000002, inf}) { c = sgood; c.mt.percentile = v; expect(run(c), stext[4], S, "solve percentile"); }
    for (double v : {0.0, 1.0}) { c = sgood; c.mt.percentile = v; expect(run(c), nullptr, S, "solve percentile at an end"); }
    for (double v : {nan, 0.0, -0.5, 1.0000000000000002, inf}) { c = sgood; c.mt.rate = v; expect(run(c), stext[8], S, "solve rate"); }
    c = sgood; c.mt.rate = 5e-324; expect(run(c), nullptr, S, "solve the least rate");
    c = sgood; c.mt.min_exposure = c.mt.max_exposure = 2.0; expect(run(c), nullptr, S, "solve equal clamps");
    c = sgood; c.mt.flags = -1; expect(run(c), stext[9], S, "solve flags -1");
    c = sgood; c.mt.reserved = -1; expect(run(c), stext[10], S, "solve reserved -1");

    /* rt_film_resolve_metered: rt_film_resolve's rules under its own name, and a state behind the tone */
    const ResolveCall rgood = {s, 12, 4, 3, 1, {1.0, 0.0, 1, 0}, true, st, o8, o32, 12};
    expect(run(rgood), nullptr, R, "resolve good");
    struct { const char *text; bool named; } rtext[] = {{"d_sum is NULL", true}, {"tone is NULL", true}, {"d_state is NULL", true},
        {"ws*h outside 1..RT_FILM_MAX_PIXELS", true}, {"n < 1", true}, {"exposure must be finite and > 0", true},
        {"white must be 0, or finite and > 0", true}, {"gamma must be 1 or 2", true}, {"unknown flag bit", true},
        {"both output pointers are NULL", false}, {"sum_stride smaller than the frame", true}, {"out_stride smaller than the frame", false}};
    for (int k = 0; k < 12; ++k) {
        ResolveCall q = rgood;
        q.out_stride = 11;
        if (k <= 10) q.stride = 11;
        if (k <= 9) { q.u8 = nullptr; q.f32 = nullptr; }
        if (k <= 8) q.tone.flags = 1 << 20;
        if (k <= 7) q.tone.gamma = 3;
        if (k <= 6) q.tone.white = -1.0;
        if (k <= 5) q.tone.exposure = 0.0;
        if (k <= 4) q.n = 0;
        if (k <= 3) q.h = 0;
        if (k <= 2) q.state = nullptr;
        if (k <= 1) q.have_tone = false;
        if (k <= 0) q.sum = nullptr;
        expect(run(q), rtext[k].text, rtext[k].named ? R : nullptr, std::string("resolve: ") + rtext[k].text);
        if (k != 2) {                                                 /* and rt_film_resolve says the same, under its own name */
            const rt::Refusal plain = rt::check_film_resolve(q.sum, q.stride, q.ws, q.h, q.n, q.have_tone ? &q.tone : nullptr, q.u8, q.f32, q.out_stride);
            expect(plain, rtext[k].text, rtext[k].named ? "rt_film_resolve" : nullptr, std::string("plain resolve: ") + rtext[k].text);
        }
    }
    ResolveCall q = rgood;
    q.tone.flags = RT_FLAG_U8_HWC; expect(run(q), "RT_FLAG_U8_HWC re-uses out_stride as the image row pitch: resolve the float32 buffer in a separate call", nullptr, "resolve hwc with f32");
    q.f32 = nullptr; q.out_stride = 3; expect(run(q), "row pitch smaller than the frame width", nullptr, "resolve hwc pitch");
    q.out_stride = 4; expect(run(q), nullptr, R, "resolve hwc");
}

/* ---- film_metered_exposure ------------------------------------------------------------------------------------------------------- */
static void check_exposure()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    if (rt::film_metered_exposure(1.5, 1.0) != 1.5 || rt::film_metered_exposure(1.5, 4.0) != 6.0) die("film_metered_exposure");
    for (double x : {0.0, -0.0, -2.0, nan, inf, -inf}) if (rt::film_metered_exposure(1.5, x) != 1.5) die("an unusable state must count as 1.0");
    if (rt::film_metered_exposure(2.0, 5e-324) != 1e-323 || !rt::film_exposure_usable(std::numeric_limits<double>::max())) die("the ends of the usable range");
}

int main(int argc, char **argv)
{
    if (argc != 3) die("usage: meter_check IN OUT");
    static_assert(sizeof(rt_meter) == 48, "rt_meter is 48 bytes");
    check_bins();
    check_refusals();
    check_exposure();
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) die("cannot open the files");
    int64_t ncases = 0, nsolves = 0;
    if (std::fread(&ncases, sizeof ncases, 1, in) != 1) die("short input");
    for (int64_t k = 0; k < ncases; ++k) {
        int64_t head[5];
        if (std::fread(head, sizeof head, 1, in) != 1) die("short input");
        const int ws = (int)head[0], h = (int)head[1], nblocks = (int)head[4];
        const int64_t n = head[2], pad = head[3];
        const long long npx = (long long)ws * h, stride = npx + pad, total = 3 * stride;
        std::unique_ptr<double[]> sum(new double[total]);
        if ((long long)std::fread(sum.get(), sizeof(double), total, in) != total) die("short input");
        Counts whole, slabs;
        meter(sum.get(), stride, ws, h, n, 1, whole.hist(), nblocks);
        whole.intact("whole frame");
        uint64_t seen = 0;
        for (int b = 0; b < RT_METER_BINS; ++b) seen += whole.hist()[b];
        if (seen != (uint64_t)npx) die("case " + std::to_string(k) + ": the counts add up to " + std::to_string(seen) + ", not ws*h (a pad was read?)");
        /* two column slabs, no reset between them, another number of workgroups */
        const int cut = ws / 2;
        if (cut > 0) {
            meter(sum.get(), stride, cut, h, n, 1, slabs.hist(), nblocks + 1);
            meter(sum.get() + (long long)cut * h, stride, ws - cut, h, n, 0, slabs.hist(), 1);
        } else {
            meter(sum.get(), stride, ws, h, n, 1, slabs.hist(), 3);
        }
        slabs.intact("slabs");
        if (std::memcmp(whole.hist(), slabs.hist(), RT_METER_BINS * sizeof(uint64_t)) != 0) die("case " + std::to_string(k) + ": two slabs do not add up to the frame");
        if (std::fwrite(whole.hist(), sizeof(uint64_t), RT_METER_BINS, out) != RT_METER_BINS) die("short write");
    }
    if (std::fread(&nsolves, sizeof nsolves, 1, in) != 1) die("short input");
    for (int64_t k = 0; k < nsolves; ++k) {
        std::unique_ptr<uint64_t[]> hist(new uint64_t[RT_METER_BINS]);
        std::unique_ptr<double[]> state(new double[RT_METER_STATE_DOUBLES]);
        double set[5];
        if (std::fread(hist.get(), sizeof(uint64_t), RT_METER_BINS, in) != RT_METER_BINS ||
            std::fread(state.get(), sizeof(double), RT_METER_STATE_DOUBLES, in) != RT_METER_STATE_DOUBLES || std::fread(set, sizeof set, 1, in) != 1)
            die("short input");
        const rt_meter mt = {set[0], set[1], set[2], set[3], set[4], 0, 0};
        const rt::Refusal r = rt::check_film_meter_solve(hist.get(), &mt, state.get());
        if (r.code != RT_OK) die(std::string("a solve was refused: ") + r.msg);
        rt::meter_solve(hist.get(), mt, state.get());
        if (std::fwrite(state.get(), sizeof(double), RT_METER_STATE_DOUBLES, out) != RT_METER_STATE_DOUBLES) die("short write");
    }
    std::fclose(in);
    if (std::fclose(out) != 0) die("short write");
    std::printf("cases=%lld solves=%lld ok\n", (long long)ncases, (long long)nsolves);
    return 0;
}
