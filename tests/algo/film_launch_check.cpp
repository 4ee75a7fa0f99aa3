/* What the film entries decide before they touch the device (python-ray-tracer_amd/csrc/rt_film_launch.h), without HIP: their checks,
 * their kernels' arguments and their filters' ping-pong plans.  Built with AddressSanitizer and UndefinedBehaviorSanitizer and run by
 * tests/test_algorithms.py, which compares what this writes with tests/golden/film_launch_args.npz and with literals.
 *
 *   film_launch_check OUT CHECKS   writes int64 rows of 4 + MAXF words to OUT: {kind, case, sub, fields} and every field of one argument
 *                                  struct, field by field in the struct's order (floats and doubles as raw bits; a pointer as its made-up
 *                                  address, buffer number << 44 plus the byte offset, NULL as -1), zeros behind the last field; and to
 *                                  CHECKS one line "name<TAB>code<TAB>text" per entry-check case; prints "records=N checks=M ok".
 * Kinds: 0 TemporalArgs, 1 TemporalMomentsArgs (case: view * 2 + previous camera); 2 FilmResolveArgs (case: planar RGB, planar BGR,
 * HWC); 3 the film's batch plan {fplane, pass_bytes, batch}, 4 FilmAddArgs and 5 FilmAdd2Args of every add launch (sub: the first
 * pass of the batch); 6 DenoiseArgs, 7 rt_film_denoise_variance's DenoiseVarArgs, 8 DenoiseVarLenArgs and 9
 * rt_film_denoise_variance_temporal's DenoiseVarArgs of every write (case: levels * 2 + demodulate, sub: the write).
 * The device buffers are never touched.  The program itself fails if, for any `levels`, a filter's last write does not land in d_out,
 * a write reads the buffer it writes, or a write does not read what the write before it wrote. */
#include "../../python-ray-tracer_amd/csrc/rt_film_launch.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

enum { SUM = 1, SQ, GUIDES, HIST, HIST_SQ, HIST_LEN, HIST_GUIDES, OUT, WORK, OUT_SQ, OUT_LEN, U8, F32, FRAMES };
static void *buf(int id, size_t bytes = 0) { return (void *)(((uintptr_t)id << 44) + bytes); }

static std::vector<int64_t> g_out;
static long g_records = 0;
static const int MAXF = 53;

static int64_t ptr(const void *p) { return p ? (int64_t)(uintptr_t)p : -1; }
static int64_t bits(double d) { int64_t b; std::memcpy(&b, &d, sizeof b); return b; }

static void die(const char *what)
{
    std::fprintf(stderr, "%s\n", what);
    std::exit(1);
}

static void put(int kind, int cs, int sub, const std::vector<int64_t> &f)
{
    if (f.size() > (size_t)MAXF) die("MAXF is too small");
    for (int64_t v : {(int64_t)kind, (int64_t)cs, (int64_t)sub, (int64_t)f.size()}) g_out.push_back(v);
    g_out.insert(g_out.end(), f.begin(), f.end());
    g_out.insert(g_out.end(), MAXF - f.size(), 0);
    ++g_records;
}

static std::vector<int64_t> fields(const rt::TemporalArgs &a)
{
    std::vector<int64_t> f = {ptr(a.sum), ptr(a.guides), ptr(a.hist), ptr(a.hist_len), ptr(a.hist_guides), ptr(a.out), ptr(a.out_len),
                              a.sum_stride, a.guide_stride, a.hist_stride, a.hist_guide_stride, a.out_stride, a.w, a.h, bits(a.n),
                              bits(a.px), bits(a.y0), bits(a.dy), bits(a.z0), bits(a.dz)};
    for (double d : a.o) f.push_back(bits(d));
    for (double d : a.R) f.push_back(bits(d));
    for (double d : a.po) f.push_back(bits(d));
    for (double d : a.pR) f.push_back(bits(d));
    for (double d : {a.depth_tol, a.normal_cos, a.max_history}) f.push_back(bits(d));
    return f;
}

static std::vector<int64_t> fields(const rt::TemporalMomentsArgs &m)
{
    std::vector<int64_t> f = fields(m.t);
    for (int64_t v : {ptr(m.sq), ptr(m.hist_sq), ptr(m.out_sq), (int64_t)m.sq_stride, (int64_t)m.hist_sq_stride, (int64_t)m.out_sq_stride}) f.push_back(v);
    return f;
}

static std::vector<int64_t> fields(const rt::FilmResolveArgs &a)
{
    return {ptr(a.sum), ptr(a.u8), ptr(a.f32), a.sum_stride, a.out_stride, a.npx, a.h, a.rgb, a.hwc,
            bits(a.tone.n), bits(a.tone.exposure), bits(a.tone.white), bits(a.tone.wn2), a.tone.gamma};
}

static std::vector<int64_t> fields(const rt::FilmAddArgs &a) { return {ptr(a.sum), ptr(a.frames), a.sum_stride, a.fplane, a.npx, a.nb, a.reset}; }

static std::vector<int64_t> fields(const rt::FilmAdd2Args &a)
{
    return {ptr(a.sum), ptr(a.sq), ptr(a.frames), a.sum_stride, a.sq_stride, a.fplane, a.npx, a.nb, a.reset};
}

static std::vector<int64_t> fields(const rt::DenoiseArgs &a)
{
    return {ptr(a.src), ptr(a.guides), ptr(a.dst), a.src_stride, a.guide_stride, a.dst_stride, a.ws, a.h, a.step, a.nsq, a.first, a.last,
            a.demod, a.copy, bits(a.n), bits(a.q)};
}

static std::vector<int64_t> fields(const rt::DenoiseVarArgs &a)
{
    return {ptr(a.sum), ptr(a.sq), ptr(a.src), ptr(a.guides), ptr(a.dst), a.sum_stride, a.sq_stride, a.src_stride, a.guide_stride, a.dst_stride,
            a.ws, a.h, a.step, a.nsq, a.last, a.demod, a.prefilter, a.copy, bits(a.n), bits(a.n1), bits(a.k2), bits(a.var_floor)};
}

static std::vector<int64_t> fields(const rt::DenoiseVarLenArgs &a)
{
    return {ptr(a.mean), ptr(a.msq), ptr(a.len), ptr(a.guides), ptr(a.dst), a.mean_stride, a.msq_stride, a.guide_stride, a.dst_stride,
            a.ws, a.h, a.demod, a.copy, bits(a.spatial_below)};
}

/* one write of a filter's ping-pong: what the program itself asks of the plan */
static const void *g_prev_dst = nullptr;
static void note_write(int k, int nwrites, const void *src, const void *dst, const void *d_out, const void *d_work)
{
    if (dst != d_out && dst != d_work) die("a write lands in neither d_out nor d_work");
    if (src == dst) die("a write reads the buffer it writes");
    if (k > 0 && src != g_prev_dst) die("a write does not read what the write before it wrote");
    if (k == nwrites - 1 && dst != d_out) die("the last write does not land in d_out");
    g_prev_dst = dst;
}

static const int W = 16, H = 8;
static const long long NPX = W * H;

static rt::View view_of(int i)
{
    rt::View v;
    const double o[2][3] = {{0.0, 0.0, 0.0}, {0.3, -1.7, 2.9}};
    const double R[2][9] = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0.36, 0.48, -0.8, -0.8, 0.6, 0.0, 0.48, 0.64, 0.6}};
    std::memcpy(v.cam_o, o[i], sizeof v.cam_o);
    std::memcpy(v.cam_R, R[i], sizeof v.cam_R);
    v.w = i ? 40 : W; v.h = i ? 24 : H;
    v.px = 1.5 - i; v.y0 = -0.9875; v.dy = 0.025 * (i + 1); v.z0 = 0.7375; v.dz = -0.0625;
    if (i) { v.lens_a = 0.125; v.lens_f = 6.5; }
    v.have_cam = v.have_grid = true;
    return v;
}

static rt_temporal temporal_of(int i)
{
    rt_temporal tp;
    std::memset(&tp, 0, sizeof tp);
    const double o[2][3] = {{0.25, 0.0, 0.0}, {-3.5, 0.125, 7.0}};
    const double R[2][9] = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0.6, 0.0, 0.8, 0.0, 1.0, 0.0, -0.8, 0.0, 0.6}};
    std::memcpy(tp.prev_origin, o[i], sizeof tp.prev_origin);
    std::memcpy(tp.prev_rotation, R[i], sizeof tp.prev_rotation);
    tp.depth_tol = i ? 0.0 : 0.01; tp.normal_cos = i ? -1.0 : 0.9; tp.max_history = i ? 0.0 : 32.0;
    return tp;
}

/* ---- the arguments, as the entries of mi355rt.hip build them ---- */

static void temporal_rows(int cs, const rt::View &v, const rt_temporal &tp)
{
    const long long npx = (long long)v.w * v.h;
    const int64_t n = 3 + cs;
    rt::TemporalArgs a;
    rt::temporal_args(a, v, buf(SUM, 8 * cs), npx + 1, n, buf(GUIDES), npx + 2, buf(HIST, 16), npx + 3, buf(HIST_LEN), buf(HIST_GUIDES, 4), npx + 4, &tp,
                      buf(OUT), npx + 5, buf(OUT_LEN, 4 * cs));
    put(0, cs, 0, fields(a));
    rt::TemporalMomentsArgs m;
    rt::temporal_args(m.t, v, buf(SUM, 8 * cs), npx + 1, n, buf(GUIDES), npx + 2, buf(HIST, 16), npx + 3, buf(HIST_LEN), buf(HIST_GUIDES, 4), npx + 4, &tp,
                      buf(OUT), npx + 5, buf(OUT_LEN, 4 * cs));
    rt::temporal_moments_args(m, buf(SQ, 8), npx + 6, buf(HIST_SQ), npx + 7, buf(OUT_SQ, 24), npx + 8);
    put(1, cs, 0, fields(m));
}

static void resolve_rows(int cs, int flags, void *d_u8, void *d_f32, int64_t out_stride)
{
    const rt_film_tone tone = {cs ? 1.75 : 1.0, cs == 1 ? 0.0 : 640.0, cs == 2 ? 2 : 1, flags};
    put(2, cs, 0, fields(rt::film_resolve_args(buf(SUM, 8 * cs), NPX + cs, W, H, 5 + cs, &tone, d_u8, d_f32, out_stride)));
}

/* film_queue_passes: every add launch of `passes` passes over npx pixels, onto the sum alone and onto both moments */
static void add_rows(int cs, long long npx, int passes, int reset)
{
    const rt::FilmBatch fb = rt::film_batch(npx, passes);
    put(3, cs, 0, {fb.fplane, (int64_t)fb.pass_bytes, fb.batch});
    const float *const frames = (const float *)buf(FRAMES);
    for (int i = 0; i < passes; i += fb.batch) {
        const int nb = std::min(fb.batch, passes - i);
        put(4, cs, i, fields(rt::film_add_args(buf(SUM, 8), npx + 1, frames, fb.fplane, npx, nb, (reset && i == 0) ? 1 : 0)));
        put(5, cs, i, fields(rt::film_add2_args(buf(SUM, 8), npx + 1, buf(SQ), npx + 2, frames, fb.fplane, npx, nb, (reset && i == 0) ? 1 : 0)));
    }
}

/* the three filters: every write of `levels` levels */
static void filter_rows(int cs, int levels, int demodulate)
{
    const rt::FilmPingPong pp = {buf(OUT), NPX + 3, buf(WORK, 32), NPX + 4};
    const int64_t n = 7;
    {
        const rt_denoise dn = {levels, 1 << (levels + 1), levels & 1 ? 0.0 : 12.5, demodulate, 0};
        const int nwrites = levels ? levels : 1;
        for (int i = 0; i < nwrites; ++i) {
            const rt::FilmWrite w = rt::film_write(false, levels, i, buf(SUM, 8), NPX + 1, pp);
            const rt::DenoiseArgs a = rt::denoise_args(w, buf(GUIDES), NPX + 2, W, H, n, &dn, levels + 1, i);
            note_write(i, nwrites, a.src, a.dst, pp.d_out, pp.d_work);
            put(6, cs, i, fields(a));
        }
    }
    const rt_denoise_variance dv = {levels, 1 << levels, 1.5, 0x1p-20, demodulate, levels & 1};
    {
        rt::DenoiseVarArgs base = rt::denoise_var_common(buf(GUIDES), NPX + 2, W, H, &dv, levels);
        rt::denoise_var_inputs(base, buf(SUM, 8), NPX + 1, buf(SQ), NPX + 5, n, levels);
        for (int k = 0; k <= levels; ++k) {
            const rt::DenoiseVarArgs a = rt::denoise_var_write(base, rt::film_write(true, levels, k, nullptr, 0, pp), levels, k);
            note_write(k, levels + 1, a.src, a.dst, pp.d_out, pp.d_work);
            put(7, cs, k, fields(a));
        }
    }
    {
        const rt::DenoiseVarArgs base = rt::denoise_var_common(buf(GUIDES), NPX + 2, W, H, &dv, levels);
        for (int k = 0; k <= levels; ++k) {
            const rt::FilmWrite w = rt::film_write(true, levels, k, nullptr, 0, pp);
            note_write(k, levels + 1, w.src, w.dst, pp.d_out, pp.d_work);
            if (k == 0) put(8, cs, k, fields(rt::denoise_var_len_args(w, buf(HIST), NPX + 1, buf(HIST_SQ), NPX + 5, buf(HIST_LEN), W, H, buf(GUIDES), NPX + 2, &dv, 2.5)));
            else put(9, cs, k, fields(rt::denoise_var_write(base, w, levels, k)));
        }
    }
}

/* ---- the entry checks ---- */

static FILE *g_checks = nullptr;
static long g_nchecks = 0;
static void check(const std::string &name, const rt::Refusal &r)
{
    if ((r.code == RT_OK) != (r.msg == nullptr) || (r.code == RT_OK && r.entry)) die("a refusal without a message, or a message without a refusal");
    const std::string text = r.code == RT_OK ? "" : (r.entry ? std::string(r.entry) + ": " + r.msg : std::string(r.msg));
    std::fprintf(g_checks, "%s\t%d\t%s\n", name.c_str(), r.code, text.c_str());
    ++g_nchecks;
}

/* the arguments of each entry: good ones, each replaceable */
struct Accumulate {
    bool have_scene = true;
    rt::View v = view_of(0);
    rt::SceneLayout lay;
    rt_params params;
    const rt_params *p = &params;
    int x0 = 0, x1 = W, passes = 2;
    const void *d_sum = buf(SUM), *d_sq = buf(SQ);
    int64_t sum_stride = NPX, sq_stride = NPX;
    Accumulate() { std::memset(&params, 0, sizeof params); params.depth = 2; }
    rt::Refusal run(bool moments) const
    {
        return rt::check_film_accumulate(moments ? "rt_film_accumulate_moments" : "rt_film_accumulate", have_scene, v, lay, p, x0, x1, passes, d_sum,
                                         sum_stride, moments, d_sq, sq_stride);
    }
};

struct Resolve {
    const void *d_sum = buf(SUM), *d_u8 = buf(U8), *d_f32 = buf(F32);
    int64_t sum_stride = NPX, n = 4, out_stride = NPX;
    int ws = W, h = H;
    rt_film_tone tone = {1.0, 0.0, 1, 0};
    const rt_film_tone *t = &tone;
    rt::Refusal run() const { return rt::check_film_resolve(d_sum, sum_stride, ws, h, n, t, d_u8, d_f32, out_stride); }
};

struct Filter {                       /* the three filters: d_sum / d_sq / d_len are d_mean / d_msq / d_len of the temporal one */
    const void *d_sum = buf(SUM), *d_sq = buf(SQ), *d_len = buf(HIST_LEN), *d_guides = buf(GUIDES), *d_out = buf(OUT), *d_work = buf(WORK);
    int64_t sum_stride = NPX, sq_stride = NPX, guide_stride = NPX, out_stride = NPX, work_stride = NPX, n = 4;
    int ws = W, h = H, nsq = -2;
    double spatial_below = 4.0;
    rt_denoise dn_ = {2, 32, 0.0, 1, 0};
    rt_denoise_variance dv_ = {2, 32, 1.0, 0.0, 1, 1};
    const rt_denoise *dn = &dn_;
    const rt_denoise_variance *dv = &dv_;
    rt::Refusal denoise() { return rt::check_film_denoise(d_sum, sum_stride, ws, h, n, d_guides, guide_stride, dn, d_out, out_stride, d_work, work_stride, nsq); }
    rt::Refusal variance()
    {
        return rt::check_film_denoise_variance(d_sum, sum_stride, d_sq, sq_stride, ws, h, n, d_guides, guide_stride, dv, d_out, out_stride, d_work,
                                               work_stride, nsq);
    }
    rt::Refusal variance_temporal()
    {
        return rt::check_film_denoise_variance_temporal(d_sum, sum_stride, d_sq, sq_stride, d_len, ws, h, d_guides, guide_stride, dv, spatial_below, d_out,
                                                        out_stride, d_work, work_stride, nsq);
    }
};

struct Temporal {
    rt::View v = view_of(0);
    const void *d_sum = buf(SUM), *d_sq = buf(SQ), *d_guides = buf(GUIDES), *d_hist = buf(HIST), *d_hist_sq = buf(HIST_SQ), *d_hist_len = buf(HIST_LEN),
               *d_hist_guides = buf(HIST_GUIDES), *d_out = buf(OUT), *d_out_sq = buf(OUT_SQ), *d_out_len = buf(OUT_LEN);
    int64_t sum_stride = NPX, sq_stride = NPX, guide_stride = NPX, hist_stride = NPX, hist_sq_stride = NPX, hist_guide_stride = NPX, out_stride = NPX,
            out_sq_stride = NPX, n = 4;
    rt_temporal tp_ = temporal_of(0);
    const rt_temporal *tp = &tp_;
    rt::Refusal run(bool moments) const
    {
        if (!moments)
            return rt::check_film_temporal("rt_film_temporal", v, d_sum, sum_stride, n, d_guides, guide_stride, d_hist, hist_stride, d_hist_len,
                                           d_hist_guides, hist_guide_stride, tp, d_out, out_stride, d_out_len);
        return rt::check_film_temporal_moments(v, d_sum, sum_stride, d_sq, sq_stride, n, d_guides, guide_stride, d_hist, hist_stride, d_hist_sq,
                                               hist_sq_stride, d_hist_len, d_hist_guides, hist_guide_stride, tp, d_out, out_stride, d_out_sq,
                                               out_sq_stride, d_out_len);
    }
};

static const double NaN = __builtin_nan(""), Inf = __builtin_inf();

static void entry_checks()
{
    /* rt_film_accumulate and rt_film_accumulate_moments */
    for (int m = 0; m < 2; ++m) {
        const std::string s = m ? "moments/" : "accumulate/";
        auto A = [&](auto edit) { Accumulate a; edit(a); return a.run(m != 0); };
        check(s + "ok", A([](Accumulate &) {}));
        check(s + "params_null", A([](Accumulate &a) { a.p = nullptr; a.passes = 0; }));
        check(s + "no_scene", A([](Accumulate &a) { a.have_scene = false; a.passes = 0; }));
        check(s + "columns", A([](Accumulate &a) { a.x1 = W + 1; a.d_sum = nullptr; }));
        check(s + "passes", A([](Accumulate &a) { a.passes = 0; }));
        check(s + "passes_and_sum_null", A([](Accumulate &a) { a.passes = 0; a.d_sum = nullptr; }));
        check(s + "sum_null", A([](Accumulate &a) { a.d_sum = nullptr; a.d_sq = nullptr; }));
        check(s + "sq_null", A([](Accumulate &a) { a.d_sq = nullptr; }));
        check(s + "sq_is_sum", A([](Accumulate &a) { a.d_sq = a.d_sum; }));
        check(s + "sq_is_sum_and_sum_stride", A([](Accumulate &a) { a.d_sq = a.d_sum; a.sum_stride = NPX - 1; }));
        check(s + "above_max", A([](Accumulate &a) { a.v.w = a.v.h = a.x1 = 1 << 14; a.sum_stride = 0; }));
        check(s + "sum_stride", A([](Accumulate &a) { a.sum_stride = NPX - 1; a.sq_stride = 0; }));
        check(s + "sum_stride_of_a_slab", A([](Accumulate &a) { a.x0 = 8; a.sum_stride = 8 * H - 1; }));
        check(s + "sq_stride", A([](Accumulate &a) { a.sq_stride = NPX - 1; }));
        check(s + "slab_ok", A([](Accumulate &a) { a.x0 = 8; a.sum_stride = a.sq_stride = 8 * H; }));
    }
    /* rt_film_resolve */
    {
        auto R = [&](auto edit) { Resolve r; edit(r); return r.run(); };
        check("resolve/ok", R([](Resolve &) {}));
        check("resolve/sum_null", R([](Resolve &r) { r.d_sum = nullptr; r.t = nullptr; }));
        check("resolve/tone_null", R([](Resolve &r) { r.t = nullptr; r.ws = 0; }));
        check("resolve/ws", R([](Resolve &r) { r.ws = 0; }));
        check("resolve/h", R([](Resolve &r) { r.h = 0; }));
        check("resolve/above_max", R([](Resolve &r) { r.ws = r.h = 1 << 14; }));
        check("resolve/at_max_ok", R([](Resolve &r) { r.ws = 1 << 14; r.h = 1 << 13; r.sum_stride = r.out_stride = 1 << 27; }));
        check("resolve/ws_and_n", R([](Resolve &r) { r.ws = 0; r.n = 0; }));
        check("resolve/n", R([](Resolve &r) { r.n = 0; r.tone.exposure = 0.0; }));
        check("resolve/exposure_zero", R([](Resolve &r) { r.tone.exposure = 0.0; r.tone.white = -1.0; }));
        check("resolve/exposure_inf", R([](Resolve &r) { r.tone.exposure = Inf; }));
        check("resolve/exposure_nan", R([](Resolve &r) { r.tone.exposure = NaN; }));
        check("resolve/white_negative", R([](Resolve &r) { r.tone.white = -1.0; r.tone.gamma = 3; }));
        check("resolve/white_nan", R([](Resolve &r) { r.tone.white = NaN; }));
        check("resolve/white_ok", R([](Resolve &r) { r.tone.white = 640.0; r.tone.gamma = 2; }));
        check("resolve/gamma", R([](Resolve &r) { r.tone.gamma = 3; r.tone.flags = 1; }));
        check("resolve/flags", R([](Resolve &r) { r.tone.flags = RT_FLAG_COUNT_RAYS; r.d_u8 = r.d_f32 = nullptr; }));
        check("resolve/both_null", R([](Resolve &r) { r.d_u8 = r.d_f32 = nullptr; r.sum_stride = 0; }));
        check("resolve/sum_stride", R([](Resolve &r) { r.sum_stride = NPX - 1; r.out_stride = 0; }));
        check("resolve/hwc_f32", R([](Resolve &r) { r.tone.flags = RT_FLAG_U8_HWC; r.out_stride = W - 1; }));
        check("resolve/hwc_pitch", R([](Resolve &r) { r.tone.flags = RT_FLAG_U8_HWC; r.d_f32 = nullptr; r.out_stride = W - 1; }));
        check("resolve/hwc_ok", R([](Resolve &r) { r.tone.flags = RT_FLAG_U8_HWC | RT_FLAG_U8_RGB; r.d_f32 = nullptr; r.out_stride = W; }));
        check("resolve/out_stride", R([](Resolve &r) { r.out_stride = NPX - 1; }));
    }
    /* the three filters */
    for (int which = 0; which < 3; ++which) {
        const std::string s = which == 0 ? "denoise/" : (which == 1 ? "variance/" : "variance_temporal/");
        auto F = [&](auto edit) {
            Filter f;
            edit(f);
            const rt::Refusal r = which == 0 ? f.denoise() : (which == 1 ? f.variance() : f.variance_temporal());
            if (r.code == RT_OK && f.nsq != 5 && f.nsq != 0) die("an accepted filter call without nsq");
            return r;
        };
        auto levels = [&](Filter &f, int v) { f.dn_.levels = f.dv_.levels = v; };
        auto shin = [&](Filter &f, int v) { f.dn_.normal_shin = f.dv_.normal_shin = v; };
        auto demod = [&](Filter &f, int v) { f.dn_.demodulate = f.dv_.demodulate = v; };
        check(s + "ok", F([](Filter &) {}));
        check(s + "sum_null", F([](Filter &f) { f.d_sum = nullptr; f.d_sq = nullptr; f.d_guides = nullptr; }));
        if (which) check(s + "sq_null", F([](Filter &f) { f.d_sq = nullptr; f.d_len = nullptr; f.d_guides = nullptr; }));
        if (which == 2) check(s + "len_null", F([](Filter &f) { f.d_len = nullptr; f.d_guides = nullptr; }));
        check(s + "guides_null", F([](Filter &f) { f.d_guides = nullptr; f.dn = nullptr; f.dv = nullptr; }));
        check(s + "settings_null", F([](Filter &f) { f.dn = nullptr; f.dv = nullptr; f.d_out = nullptr; }));
        check(s + "out_null", F([](Filter &f) { f.d_out = nullptr; f.n = 0; }));
        if (which == 0) check(s + "n", F([&](Filter &f) { f.n = 0; levels(f, 7); }));
        if (which == 1) check(s + "n", F([&](Filter &f) { f.n = 1; levels(f, -1); }));
        check(s + "levels_below", F([&](Filter &f) { levels(f, -1); }));
        check(s + "levels_above", F([&](Filter &f) { levels(f, 7); shin(f, 3); }));
        check(s + "levels_six_ok", F([&](Filter &f) { levels(f, 6); shin(f, 1); }));
        check(s + "normal_shin_three", F([&](Filter &f) { shin(f, 3); f.dn_.sigma = -1.0; f.dv_.kappa = -1.0; }));
        check(s + "normal_shin_above", F([&](Filter &f) { shin(f, 2048); }));
        check(s + "normal_shin_zero", F([&](Filter &f) { shin(f, 0); }));
        if (which == 0) {
            check(s + "sigma_negative", F([&](Filter &f) { f.dn_.sigma = -1.0; demod(f, 2); }));
            check(s + "sigma_nan", F([](Filter &f) { f.dn_.sigma = NaN; }));
            check(s + "sigma_inf", F([](Filter &f) { f.dn_.sigma = Inf; }));
            check(s + "sigma_ok", F([](Filter &f) { f.dn_.sigma = 12.5; }));
            check(s + "demodulate", F([&](Filter &f) { demod(f, 2); f.dn_.reserved = 1; }));
            check(s + "reserved", F([](Filter &f) { f.dn_.reserved = 1; f.ws = 0; }));
        } else {
            check(s + "kappa_negative", F([](Filter &f) { f.dv_.kappa = -1.0; f.dv_.var_floor = -1.0; }));
            check(s + "kappa_nan", F([](Filter &f) { f.dv_.kappa = NaN; }));
            check(s + "var_floor_negative", F([&](Filter &f) { f.dv_.var_floor = -1.0; demod(f, 2); }));
            check(s + "var_floor_inf", F([](Filter &f) { f.dv_.var_floor = Inf; }));
            check(s + "demodulate", F([&](Filter &f) { demod(f, 2); f.dv_.prefilter = 2; }));
            check(s + "prefilter", F([](Filter &f) { f.dv_.prefilter = 2; f.spatial_below = -1.0; f.ws = 0; }));
        }
        if (which == 2) {
            check(s + "spatial_below_negative", F([](Filter &f) { f.spatial_below = -1.0; f.ws = 0; }));
            check(s + "spatial_below_nan", F([](Filter &f) { f.spatial_below = NaN; }));
            check(s + "spatial_below_inf", F([](Filter &f) { f.spatial_below = Inf; }));
        }
        check(s + "ws", F([](Filter &f) { f.ws = 0; f.sum_stride = -1; }));
        check(s + "h", F([](Filter &f) { f.h = 0; }));
        check(s + "above_max", F([](Filter &f) { f.ws = f.h = 1 << 14; }));
        check(s + "sum_stride", F([](Filter &f) { f.sum_stride = NPX - 1; }));
        if (which) check(s + "sq_stride", F([](Filter &f) { f.sq_stride = NPX - 1; }));
        check(s + "guide_stride", F([](Filter &f) { f.guide_stride = NPX - 1; }));
        check(s + "out_stride", F([](Filter &f) { f.out_stride = NPX - 1; f.d_work = nullptr; }));
        check(s + "work_stride", F([](Filter &f) { f.work_stride = NPX - 1; f.d_work = f.d_out; }));
        check(s + "no_work", F([&](Filter &f) { f.d_work = nullptr; f.work_stride = 0; f.d_out = f.d_sum; levels(f, which ? 1 : 2); }));
        check(s + "no_work_ok", F([&](Filter &f) { f.d_work = nullptr; f.work_stride = 0; levels(f, which ? 0 : 1); }));
        check(s + "out_is_sum", F([](Filter &f) { f.d_out = f.d_sum; }));
        if (which) check(s + "out_is_sq", F([](Filter &f) { f.d_out = f.d_sq; }));
        if (which == 2) check(s + "out_is_len", F([](Filter &f) { f.d_out = f.d_len; }));
        check(s + "out_is_guides", F([](Filter &f) { f.d_out = f.d_guides; }));
        check(s + "work_is_sum", F([](Filter &f) { f.d_work = f.d_sum; }));
        if (which) check(s + "work_is_sq", F([](Filter &f) { f.d_work = f.d_sq; }));
        if (which == 2) check(s + "work_is_len", F([](Filter &f) { f.d_work = f.d_len; }));
        check(s + "work_is_guides", F([](Filter &f) { f.d_work = f.d_guides; }));
        check(s + "work_is_out", F([](Filter &f) { f.d_work = f.d_out; }));
        if (which < 2) check(s + "len_is_no_input_ok", F([](Filter &f) { f.d_out = f.d_len; }));
    }
    /* rt_film_temporal and rt_film_temporal_moments */
    for (int m = 0; m < 2; ++m) {
        const std::string s = m ? "temporal_moments/" : "temporal/";
        auto T = [&](auto edit) { Temporal t; edit(t); return t.run(m != 0); };
        check(s + "ok", T([](Temporal &) {}));
        check(s + "sum_null", T([](Temporal &t) { t.d_sum = nullptr; t.tp = nullptr; }));
        check(s + "guides_null", T([](Temporal &t) { t.d_guides = nullptr; }));
        check(s + "hist_null", T([](Temporal &t) { t.d_hist = nullptr; }));
        check(s + "hist_len_null", T([](Temporal &t) { t.d_hist_len = nullptr; }));
        check(s + "hist_guides_null", T([](Temporal &t) { t.d_hist_guides = nullptr; }));
        check(s + "out_null", T([](Temporal &t) { t.d_out = nullptr; }));
        check(s + "out_len_null", T([](Temporal &t) { t.d_out_len = nullptr; t.n = 0; }));
        check(s + "tp_null", T([](Temporal &t) { t.tp = nullptr; t.n = 0; }));
        check(s + "n_zero", T([](Temporal &t) { t.n = 0; t.tp_.depth_tol = -1.0; t.d_sq = nullptr; }));
        check(s + "n_above", T([](Temporal &t) { t.n = (1 << 24) + 1; }));
        check(s + "n_at_max_ok", T([](Temporal &t) { t.n = 1 << 24; }));
        check(s + "depth_tol_negative", T([](Temporal &t) { t.tp_.depth_tol = -1.0; t.tp_.normal_cos = 2.0; }));
        check(s + "depth_tol_nan", T([](Temporal &t) { t.tp_.depth_tol = NaN; }));
        check(s + "normal_cos_above", T([](Temporal &t) { t.tp_.normal_cos = 1.5; t.tp_.max_history = -1.0; }));
        check(s + "normal_cos_nan", T([](Temporal &t) { t.tp_.normal_cos = NaN; }));
        check(s + "max_history_negative", T([](Temporal &t) { t.tp_.max_history = -1.0; t.tp_.reserved[0] = 1; }));
        check(s + "max_history_inf", T([](Temporal &t) { t.tp_.max_history = Inf; }));
        check(s + "reserved0", T([](Temporal &t) { t.tp_.reserved[0] = 1; t.v.have_cam = false; }));
        check(s + "reserved1", T([](Temporal &t) { t.tp_.reserved[1] = 1; }));
        check(s + "no_camera", T([](Temporal &t) { t.v.have_cam = false; t.v.have_grid = false; }));
        check(s + "no_grid", T([](Temporal &t) { t.v.have_grid = false; t.v.explicit_grid = true; }));
        check(s + "explicit_grid", T([](Temporal &t) { t.v.explicit_grid = true; t.v.dy = 0.0; }));
        check(s + "dy_zero", T([](Temporal &t) { t.v.dy = 0.0; t.tp_.prev_origin[0] = NaN; }));
        check(s + "dz_zero", T([](Temporal &t) { t.v.dz = 0.0; }));
        check(s + "camera_nan", T([](Temporal &t) { t.v.cam_o[1] = NaN; t.v.w = t.v.h = 1 << 14; }));
        check(s + "rotation_inf", T([](Temporal &t) { t.v.cam_R[8] = Inf; }));
        check(s + "prev_origin_nan", T([](Temporal &t) { t.tp_.prev_origin[2] = NaN; }));
        check(s + "prev_rotation_inf", T([](Temporal &t) { t.tp_.prev_rotation[0] = -Inf; }));
        check(s + "above_max", T([](Temporal &t) { t.v.w = t.v.h = 1 << 14; t.sum_stride = 0; t.d_out = t.d_sum; }));
        check(s + "sum_stride", T([](Temporal &t) { t.sum_stride = NPX - 1; }));
        check(s + "guide_stride", T([](Temporal &t) { t.guide_stride = NPX - 1; }));
        check(s + "hist_stride", T([](Temporal &t) { t.hist_stride = NPX - 1; }));
        check(s + "hist_guide_stride", T([](Temporal &t) { t.hist_guide_stride = NPX - 1; }));
        check(s + "out_stride", T([](Temporal &t) { t.out_stride = NPX - 1; t.d_out = t.d_sum; }));
        check(s + "out_is_sum", T([](Temporal &t) { t.d_out = t.d_sum; }));
        check(s + "out_is_guides", T([](Temporal &t) { t.d_out = t.d_guides; }));
        check(s + "out_is_hist", T([](Temporal &t) { t.d_out = t.d_hist; t.d_sq = nullptr; }));
        check(s + "out_is_hist_len", T([](Temporal &t) { t.d_out = t.d_hist_len; }));
        check(s + "out_is_hist_guides", T([](Temporal &t) { t.d_out = t.d_hist_guides; }));
        check(s + "out_len_is_sum", T([](Temporal &t) { t.d_out_len = t.d_sum; }));
        check(s + "out_len_is_guides", T([](Temporal &t) { t.d_out_len = t.d_guides; }));
        check(s + "out_len_is_hist", T([](Temporal &t) { t.d_out_len = t.d_hist; }));
        check(s + "out_len_is_hist_len", T([](Temporal &t) { t.d_out_len = t.d_hist_len; }));
        check(s + "out_len_is_hist_guides", T([](Temporal &t) { t.d_out_len = t.d_hist_guides; }));
        check(s + "out_len_is_out", T([](Temporal &t) { t.d_out_len = t.d_out; }));
        if (!m) continue;
        /* the second moment's rules, after every rule shared with rt_film_temporal */
        check(s + "sq_null", T([](Temporal &t) { t.d_sq = nullptr; t.sq_stride = 0; }));
        check(s + "hist_sq_null", T([](Temporal &t) { t.d_hist_sq = nullptr; }));
        check(s + "out_sq_null", T([](Temporal &t) { t.d_out_sq = nullptr; }));
        check(s + "sq_stride", T([](Temporal &t) { t.sq_stride = NPX - 1; t.d_out_sq = t.d_sum; }));
        check(s + "hist_sq_stride", T([](Temporal &t) { t.hist_sq_stride = NPX - 1; }));
        check(s + "out_sq_stride", T([](Temporal &t) { t.out_sq_stride = NPX - 1; }));
        const char *const others[] = {"sum", "sq", "guides", "hist", "hist_sq", "hist_len", "hist_guides", "out", "out_len"};
        for (int i = 0; i < 9; ++i)
            check(s + "out_sq_is_" + others[i], T([i](Temporal &t) {
                const void *const o[] = {t.d_sum, t.d_sq, t.d_guides, t.d_hist, t.d_hist_sq, t.d_hist_len, t.d_hist_guides, t.d_out, t.d_out_len};
                t.d_out_sq = o[i];
                if (i == 0) t.d_out = t.d_sq;
            }));
        check(s + "out_is_sq", T([](Temporal &t) { t.d_out = t.d_sq; }));
        check(s + "out_is_hist_sq", T([](Temporal &t) { t.d_out = t.d_hist_sq; }));
        check(s + "out_len_is_sq", T([](Temporal &t) { t.d_out_len = t.d_sq; }));
        check(s + "out_len_is_hist_sq", T([](Temporal &t) { t.d_out_len = t.d_hist_sq; }));
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    for (int view = 0; view < 2; ++view) for (int prev = 0; prev < 2; ++prev) temporal_rows(view * 2 + prev, view_of(view), temporal_of(prev));
    resolve_rows(0, RT_FLAG_U8_RGB, buf(U8, 3), buf(F32, 4), NPX + 7);
    resolve_rows(1, 0, buf(U8), nullptr, NPX);
    resolve_rows(2, RT_FLAG_U8_HWC, buf(U8, 1), nullptr, W + 2);
    int cs = 0;
    for (long long npx : {1ll, 5ll, 128ll}) for (int passes : {1, 4, 9}) { add_rows(cs, npx, passes, cs & 1); ++cs; }
    {
        const long long npx = 6000001;                           /* four passes of 72 MB: beyond FILM_SCRATCH_MAX, so one by one */
        if (rt::film_batch(npx, 5).batch != 1 || rt::film_batch(npx, 3).batch != 3) die("the large frame does not send its passes one by one");
        add_rows(cs, npx, 5, 1);
    }
    for (int levels = 0; levels <= 6; ++levels) for (int demod = 0; demod < 2; ++demod) filter_rows(levels * 2 + demod, levels, demod);
    FILE *fo = std::fopen(argv[1], "wb");
    if (!fo || std::fwrite(g_out.data(), sizeof(int64_t), g_out.size(), fo) != g_out.size() || std::fclose(fo) != 0) return 1;
    g_checks = std::fopen(argv[2], "w");
    if (!g_checks) return 1;
    entry_checks();
    if (std::fclose(g_checks) != 0) return 1;
    std::printf("records=%ld checks=%ld ok\n", g_records, g_nchecks);
    return 0;
}
