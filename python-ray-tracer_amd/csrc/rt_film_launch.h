// rt_film_launch.h — what the film entries (rt_film_accumulate to rt_film_upsample) decide before they touch the device:
//   * the entry checks (check_film_*): each entry's rules in its own order, each shared rule written once (film_*); a film refusal
//     carries its entry's name, which rt_last_error puts before the text;
//   * the kernels' arguments: the film's batch plan, the add, resolve and temporal kernels', the filters' (film_batch, *_args);
//   * the filters' ping-pong between d_out and d_work as data: which buffer write k reads and which it writes (film_write).
// HIP-free, like rt_launch.h and for the same reason; tests/algo/film_launch_check.cpp walks these functions under AddressSanitizer and
// UBSan and compares every refusal with its literal text and every field with the recorded one.
#pragma once
#include <cstddef>
#include <initializer_list>

#include "rt_launch.h"
#include "rt_film.h"
#include "rt_denoise.h"
#include "rt_denoise_var.h"
#include "rt_temporal.h"
#include "rt_bloom.h"
#include "rt_meter.h"
#include "rt_upsample.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace rt {

// Entry `e` refuses with the text "e: msg".
inline Refusal film_refusal(const char *e, const char *msg, int code = RT_ERR_BAD_ARG)
{
    Refusal r;
    r.code = code; r.msg = msg; r.entry = e;
    return r;
}

// One rule of entry `e`, and the rules of a shared piece: the function returns the first refusal.
#define RT_FILM_RULE(ok, ...) do { if (!(ok)) return film_refusal(e, __VA_ARGS__); } while (0)
#define RT_FILM_RULES(call) do { const Refusal r_ = (call); if (r_.code != RT_OK) return r_; } while (0)

inline Refusal film_levels(const char *e, int levels) { return levels >= 0 && levels <= 6 ? Refusal{} : film_refusal(e, "levels outside 0..6"); }

// nsq = log2(normal_shin): the squarings of the normal's cosine
inline Refusal film_normal_shin(const char *e, int normal_shin, int &nsq)
{
    nsq = -1;
    for (int i = 0; i <= 10; ++i) if (normal_shin == (1 << i)) nsq = i;
    RT_FILM_RULE(nsq >= 0, "normal_shin must be 1, 2, 4, ..., 1024");
    return {};
}

inline Refusal film_area(const char *e, int ws, int h)
{
    return ws >= 1 && h >= 1 && (long long)ws * h <= RT_FILM_MAX_PIXELS ? Refusal{} : film_refusal(e, "ws*h outside 1..RT_FILM_MAX_PIXELS");
}

inline Refusal film_strides(const char *e, long long npx, std::initializer_list<int64_t> strides, const char *msg = "a plane stride is smaller than the frame")
{
    for (int64_t s : strides) RT_FILM_RULE(s >= npx, msg);
    return {};
}

// "outputs must be buffers of their own": no output (NULL: not given) is one of the inputs, or another output.
inline Refusal film_own(const char *e, std::initializer_list<const void *> outs, std::initializer_list<const void *> ins, const char *msg)
{
    for (const void *const *o = outs.begin(); o != outs.end(); ++o) {
        if (!*o) continue;
        for (const void *in : ins) RT_FILM_RULE(*o != in, msg);
        for (const void *const *p = outs.begin(); p != o; ++p) RT_FILM_RULE(*o != *p, msg);
    }
    return {};
}

// rt_film_accumulate and, with `moments`, rt_film_accumulate_moments: check_params' rules, then the film's.
inline Refusal check_film_accumulate(const char *e, bool have_scene, const View &v, const SceneLayout &lay, const rt_params *p, int x0, int x1,
                                     int passes, const void *d_sum, int64_t sum_stride, bool moments, const void *d_sq, int64_t sq_stride)
{
    RT_FILM_RULES(check_params(have_scene, v, lay, p, x0, x1));
    RT_FILM_RULE(passes >= 1, "passes < 1");
    RT_FILM_RULE(d_sum, "d_sum is NULL");
    if (moments) {
        RT_FILM_RULE(d_sq, "d_sq is NULL");
        RT_FILM_RULES(film_own(e, {d_sq}, {d_sum}, "d_sq and d_sum must be buffers of their own"));
    }
    const long long npx = (long long)(x1 - x0) * v.h;
    RT_FILM_RULE(npx <= RT_FILM_MAX_PIXELS, "(x1-x0)*h above RT_FILM_MAX_PIXELS");
    RT_FILM_RULE(sum_stride >= npx, "sum_stride smaller than the slab");
    if (moments) RT_FILM_RULE(sq_stride >= npx, "sq_stride smaller than the slab");
    return {};
}

// rt_film_resolve's rules under entry `e`; metered: rt_film_resolve_metered's, which asks for a state behind the tone.
// (the texts about the outputs name no entry, as rt_render_device's do not)
inline Refusal film_resolve_rules(const char *e, const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, const rt_film_tone *tone,
                                  bool metered, const void *d_state, const void *d_u8, const void *d_f32, int64_t out_stride)
{
    RT_FILM_RULE(d_sum, "d_sum is NULL");
    RT_FILM_RULE(tone, "tone is NULL");
    RT_FILM_RULE(!metered || d_state, "d_state is NULL");
    RT_FILM_RULES(film_area(e, ws, h));
    RT_FILM_RULE(n >= 1, "n < 1");
    RT_FILM_RULE(std::isfinite(tone->exposure) && tone->exposure > 0.0, "exposure must be finite and > 0");
    RT_FILM_RULE(tone->white == 0.0 || (std::isfinite(tone->white) && tone->white > 0.0), "white must be 0, or finite and > 0");
    RT_FILM_RULE(tone->gamma == 1 || tone->gamma == 2, "gamma must be 1 or 2");
    RT_FILM_RULE(!(tone->flags & ~(RT_FLAG_U8_RGB | RT_FLAG_U8_HWC)), "unknown flag bit");
    if (!d_u8 && !d_f32) return {RT_ERR_BAD_ARG, "both output pointers are NULL"};
    const long long npx = (long long)ws * h;
    RT_FILM_RULE(sum_stride >= npx, "sum_stride smaller than the frame");
    if (tone->flags & RT_FLAG_U8_HWC) {
        if (d_f32) return {RT_ERR_BAD_ARG, "RT_FLAG_U8_HWC re-uses out_stride as the image row pitch: resolve the float32 buffer in a separate call"};
        if (out_stride < (int64_t)ws) return {RT_ERR_BAD_ARG, "row pitch smaller than the frame width"};
    } else if (out_stride < npx) return {RT_ERR_BAD_ARG, "out_stride smaller than the frame"};
    return {};
}

inline Refusal check_film_resolve(const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, const rt_film_tone *tone, const void *d_u8,
                                  const void *d_f32, int64_t out_stride)
{
    return film_resolve_rules("rt_film_resolve", d_sum, sum_stride, ws, h, n, tone, false, nullptr, d_u8, d_f32, out_stride);
}

inline Refusal check_film_resolve_metered(const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, const rt_film_tone *tone,
                                          const void *d_state, const void *d_u8, const void *d_f32, int64_t out_stride)
{
    return film_resolve_rules("rt_film_resolve_metered", d_sum, sum_stride, ws, h, n, tone, true, d_state, d_u8, d_f32, out_stride);
}

// What the three filters ask of their frame and buffers, behind their settings: `strides` are the inputs' and d_out's, `ins` the
// inputs; d_work may be NULL below `need_work` levels (no_work: the text for a NULL one at or above).
inline Refusal film_filter_buffers(const char *e, int ws, int h, std::initializer_list<int64_t> strides, std::initializer_list<const void *> ins,
                                   const void *d_out, const void *d_work, int64_t work_stride, int levels, int need_work, const char *no_work)
{
    RT_FILM_RULES(film_area(e, ws, h));
    const long long npx = (long long)ws * h;
    RT_FILM_RULES(film_strides(e, npx, strides));
    if (d_work) RT_FILM_RULES(film_strides(e, npx, {work_stride}));
    RT_FILM_RULE(d_work || levels < need_work, no_work);
    return film_own(e, {d_out, d_work}, ins, "d_out and d_work must be buffers of their own");
}

inline Refusal check_film_denoise(const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, const void *d_guides, int64_t guide_stride,
                                  const rt_denoise *dn, const void *d_out, int64_t out_stride, const void *d_work, int64_t work_stride, int &nsq)
{
    const char *const e = "rt_film_denoise";
    RT_FILM_RULE(d_sum, "d_sum is NULL");
    RT_FILM_RULE(d_guides, "d_guides is NULL");
    RT_FILM_RULE(dn, "dn is NULL");
    RT_FILM_RULE(d_out, "d_out is NULL");
    RT_FILM_RULE(n >= 1, "n < 1");
    RT_FILM_RULES(film_levels(e, dn->levels));
    RT_FILM_RULES(film_normal_shin(e, dn->normal_shin, nsq));
    RT_FILM_RULE(dn->sigma == 0.0 || (std::isfinite(dn->sigma) && dn->sigma > 0.0), "sigma must be 0, or finite and > 0");
    RT_FILM_RULE(dn->demodulate == 0 || dn->demodulate == 1, "demodulate must be 0 or 1");
    RT_FILM_RULE(dn->reserved == 0, "reserved must be 0");
    return film_filter_buffers(e, ws, h, {sum_stride, guide_stride, out_stride}, {d_sum, d_guides}, d_out, d_work, work_stride, dn->levels, 2,
                               "d_work is NULL with levels >= 2");
}

// rt_denoise_variance as both variance filters read it.
inline Refusal film_variance_settings(const char *e, const rt_denoise_variance *dv, int &nsq)
{
    RT_FILM_RULES(film_levels(e, dv->levels));
    RT_FILM_RULES(film_normal_shin(e, dv->normal_shin, nsq));
    RT_FILM_RULE(std::isfinite(dv->kappa) && dv->kappa >= 0.0, "kappa must be finite and >= 0");
    RT_FILM_RULE(std::isfinite(dv->var_floor) && dv->var_floor >= 0.0, "var_floor must be finite and >= 0");
    RT_FILM_RULE(dv->demodulate == 0 || dv->demodulate == 1, "demodulate must be 0 or 1");
    RT_FILM_RULE(dv->prefilter == 0 || dv->prefilter == 1, "prefilter must be 0 or 1");
    return {};
}

inline Refusal check_film_denoise_variance(const void *d_sum, int64_t sum_stride, const void *d_sq, int64_t sq_stride, int ws, int h, int64_t n,
                                           const void *d_guides, int64_t guide_stride, const rt_denoise_variance *dv, const void *d_out,
                                           int64_t out_stride, const void *d_work, int64_t work_stride, int &nsq)
{
    const char *const e = "rt_film_denoise_variance";
    RT_FILM_RULE(d_sum, "d_sum is NULL");
    RT_FILM_RULE(d_sq, "d_sq is NULL");
    RT_FILM_RULE(d_guides, "d_guides is NULL");
    RT_FILM_RULE(dv, "dv is NULL");
    RT_FILM_RULE(d_out, "d_out is NULL");
    RT_FILM_RULE(n >= 2, "n < 2");
    RT_FILM_RULES(film_variance_settings(e, dv, nsq));
    return film_filter_buffers(e, ws, h, {sum_stride, sq_stride, guide_stride, out_stride}, {d_sum, d_sq, d_guides}, d_out, d_work, work_stride,
                               dv->levels, 1, "d_work is NULL with levels >= 1");
}

inline Refusal check_film_denoise_variance_temporal(const void *d_mean, int64_t mean_stride, const void *d_msq, int64_t msq_stride, const void *d_len,
                                                    int ws, int h, const void *d_guides, int64_t guide_stride, const rt_denoise_variance *dv,
                                                    double spatial_below, const void *d_out, int64_t out_stride, const void *d_work,
                                                    int64_t work_stride, int &nsq)
{
    const char *const e = "rt_film_denoise_variance_temporal";
    RT_FILM_RULE(d_mean, "d_mean is NULL");
    RT_FILM_RULE(d_msq, "d_msq is NULL");
    RT_FILM_RULE(d_len, "d_len is NULL");
    RT_FILM_RULE(d_guides, "d_guides is NULL");
    RT_FILM_RULE(dv, "dv is NULL");
    RT_FILM_RULE(d_out, "d_out is NULL");
    RT_FILM_RULES(film_variance_settings(e, dv, nsq));
    RT_FILM_RULE(std::isfinite(spatial_below) && spatial_below >= 0.0, "spatial_below must be finite and >= 0");
    return film_filter_buffers(e, ws, h, {mean_stride, msq_stride, guide_stride, out_stride}, {d_mean, d_msq, d_len, d_guides}, d_out, d_work,
                               work_stride, dv->levels, 1, "d_work is NULL with levels >= 1");
}

// rt_temporal's numbers and the pass count (the previous camera: film_reprojectable).
inline Refusal film_temporal_settings(const char *e, const rt_temporal *tp, int64_t n)
{
    RT_FILM_RULE(tp, "tp is NULL");
    RT_FILM_RULE(n >= 1 && n <= (1 << 24), "n outside 1..2^24");
    RT_FILM_RULE(std::isfinite(tp->depth_tol) && tp->depth_tol >= 0.0, "depth_tol must be finite and >= 0");
    RT_FILM_RULE(tp->normal_cos >= -1.0 && tp->normal_cos <= 1.0, "normal_cos outside [-1, 1]");
    RT_FILM_RULE(std::isfinite(tp->max_history) && tp->max_history >= 0.0, "max_history must be finite and >= 0");
    RT_FILM_RULE(tp->reserved[0] == 0 && tp->reserved[1] == 0, "reserved must be 0");
    return {};
}

// A view whose pixels can be carried to the previous camera's: a camera, a closed-form grid that is no line, finite cameras.
inline Refusal film_reprojectable(const char *e, const View &v, const rt_temporal *tp)
{
    RT_FILM_RULE(v.have_cam, "rt_set_camera has not been called", RT_ERR_STATE);
    RT_FILM_RULE(v.have_grid, "rt_set_raygen has not been called", RT_ERR_STATE);
    RT_FILM_RULE(!v.explicit_grid, "an explicit rt_set_pixel_loc grid cannot be reprojected", RT_ERR_STATE);
    RT_FILM_RULE(v.dy != 0.0 && v.dz != 0.0, "the grid's dy or dz is 0", RT_ERR_STATE);
    bool finite = true;
    for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(v.cam_o[i]) && std::isfinite(tp->prev_origin[i]);
    for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(v.cam_R[i]) && std::isfinite(tp->prev_rotation[i]);
    RT_FILM_RULE(finite, "a camera entry is not finite");
    return {};
}

// rt_film_temporal (e: its name), and what rt_film_temporal_moments (e: its own) asks before it looks at its second moment.
inline Refusal check_film_temporal(const char *e, const View &v, const void *d_sum, int64_t sum_stride, int64_t n, const void *d_guides,
                                   int64_t guide_stride, const void *d_hist, int64_t hist_stride, const void *d_hist_len, const void *d_hist_guides,
                                   int64_t hist_guide_stride, const rt_temporal *tp, const void *d_out, int64_t out_stride, const void *d_out_len)
{
    RT_FILM_RULE(d_sum && d_guides && d_hist && d_hist_len && d_hist_guides && d_out && d_out_len, "a buffer is NULL");
    RT_FILM_RULES(film_temporal_settings(e, tp, n));
    RT_FILM_RULES(film_reprojectable(e, v, tp));
    const long long npx = (long long)v.w * v.h;
    RT_FILM_RULE(npx <= RT_FILM_MAX_PIXELS, "w*h above RT_FILM_MAX_PIXELS");
    RT_FILM_RULES(film_strides(e, npx, {sum_stride, guide_stride, hist_stride, hist_guide_stride, out_stride}));
    return film_own(e, {d_out, d_out_len}, {d_sum, d_guides, d_hist, d_hist_len, d_hist_guides}, "d_out and d_out_len must be buffers of their own");
}

inline Refusal check_film_temporal_moments(const View &v, const void *d_sum, int64_t sum_stride, const void *d_sq, int64_t sq_stride, int64_t n,
                                           const void *d_guides, int64_t guide_stride, const void *d_hist, int64_t hist_stride,
                                           const void *d_hist_sq, int64_t hist_sq_stride, const void *d_hist_len, const void *d_hist_guides,
                                           int64_t hist_guide_stride, const rt_temporal *tp, const void *d_out, int64_t out_stride,
                                           const void *d_out_sq, int64_t out_sq_stride, const void *d_out_len)
{
    const char *const e = "rt_film_temporal_moments";
    RT_FILM_RULES(check_film_temporal(e, v, d_sum, sum_stride, n, d_guides, guide_stride, d_hist, hist_stride, d_hist_len, d_hist_guides,
                                      hist_guide_stride, tp, d_out, out_stride, d_out_len));
    RT_FILM_RULE(d_sq && d_hist_sq && d_out_sq, "d_sq, d_hist_sq or d_out_sq is NULL");
    RT_FILM_RULES(film_strides(e, (long long)v.w * v.h, {sq_stride, hist_sq_stride, out_sq_stride},
                               "a plane stride of the second moment is smaller than the frame"));
    RT_FILM_RULES(film_own(e, {d_out_sq}, {d_sum, d_sq, d_guides, d_hist, d_hist_sq, d_hist_len, d_hist_guides, d_out, d_out_len},
                           "d_out_sq must be a buffer of its own"));
    return film_own(e, {d_out, d_out_len}, {d_sq, d_hist_sq}, "d_out and d_out_len must be buffers of their own");
}

#undef RT_FILM_RULE
#undef RT_FILM_RULES

// The film's batches: pass planes padded to a multiple of four floats (every plane of the scratch is 16-byte aligned whatever npx
// is), up to FILM_BATCH passes per add kernel, one by one where a batch of frames would not fit FILM_SCRATCH_MAX.
struct FilmBatch { long long fplane; size_t pass_bytes; int batch; };

inline FilmBatch film_batch(long long npx, int passes)
{
    FilmBatch b;
    b.fplane = (npx + 3) & ~3ll;
    b.pass_bytes = (size_t)b.fplane * 3 * sizeof(float);
    b.batch = passes < FILM_BATCH ? passes : FILM_BATCH;
    if (b.batch * b.pass_bytes > FILM_SCRATCH_MAX) b.batch = 1;
    return b;
}

// One add kernel: nb pass frames at `frames` onto the sum (reset: from zero).
inline FilmAddArgs film_add_args(void *d_sum, int64_t sum_stride, const float *frames, long long fplane, long long npx, int nb, int reset)
{
    return {(double *)d_sum, frames, sum_stride, fplane, npx, nb, reset};
}

inline FilmAdd2Args film_add2_args(void *d_sum, int64_t sum_stride, void *d_sq, int64_t sq_stride, const float *frames, long long fplane,
                                   long long npx, int nb, int reset)
{
    return {(double *)d_sum, (double *)d_sq, frames, sum_stride, sq_stride, fplane, npx, nb, reset};
}

inline FilmResolveArgs film_resolve_args(const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, const rt_film_tone *tone, void *d_u8,
                                         void *d_f32, int64_t out_stride)
{
    FilmResolveArgs a;
    a.sum = (const double *)d_sum; a.u8 = (uint8_t *)d_u8; a.f32 = (float *)d_f32;
    a.sum_stride = sum_stride; a.out_stride = out_stride; a.npx = (long long)ws * h;
    a.h = h; a.rgb = (tone->flags & RT_FLAG_U8_RGB) ? 1 : 0; a.hwc = (tone->flags & RT_FLAG_U8_HWC) ? 1 : 0;
    a.tone = film_tone_of(n, tone->exposure, tone->white, tone->gamma);
    return a;
}

// The temporal kernel's argument: the view's camera and closed-form grid and the previous camera by value.
inline void temporal_args(TemporalArgs &a, const View &v, const void *d_sum, int64_t sum_stride, int64_t n, const void *d_guides,
                          int64_t guide_stride, const void *d_hist, int64_t hist_stride, const void *d_hist_len, const void *d_hist_guides,
                          int64_t hist_guide_stride, const rt_temporal *tp, void *d_out, int64_t out_stride, void *d_out_len)
{
    a.sum = (const double *)d_sum; a.guides = (const float *)d_guides; a.hist = (const double *)d_hist;
    a.hist_len = (const float *)d_hist_len; a.hist_guides = (const float *)d_hist_guides;
    a.out = (double *)d_out; a.out_len = (float *)d_out_len;
    a.sum_stride = sum_stride; a.guide_stride = guide_stride; a.hist_stride = hist_stride; a.hist_guide_stride = hist_guide_stride;
    a.out_stride = out_stride;
    a.w = v.w; a.h = v.h; a.n = (double)n;
    a.px = v.px; a.y0 = v.y0; a.dy = v.dy; a.z0 = v.z0; a.dz = v.dz;
    std::memcpy(a.o, v.cam_o, sizeof a.o); std::memcpy(a.R, v.cam_R, sizeof a.R);
    std::memcpy(a.po, tp->prev_origin, sizeof a.po); std::memcpy(a.pR, tp->prev_rotation, sizeof a.pR);
    a.depth_tol = tp->depth_tol; a.normal_cos = tp->normal_cos; a.max_history = tp->max_history;
}

// m.t is temporal_args' (the caller fills it); the second moment's three buffers beside it.
inline void temporal_moments_args(TemporalMomentsArgs &m, const void *d_sq, int64_t sq_stride, const void *d_hist_sq, int64_t hist_sq_stride,
                                  void *d_out_sq, int64_t out_sq_stride)
{
    m.sq = (const double *)d_sq; m.hist_sq = (const double *)d_hist_sq; m.out_sq = (double *)d_out_sq;
    m.sq_stride = sq_stride; m.hist_sq_stride = hist_sq_stride; m.out_sq_stride = out_sq_stride;
}

// A filter's two buffers, and one write of its ping-pong between them.
struct FilmPingPong { void *d_out; int64_t out_stride; void *d_work; int64_t work_stride; };
struct FilmWrite { const double *src; long long src_stride; double *dst; long long dst_stride; };

// Write k of a filter: it writes d_out or d_work by the filter's plan (denoise_to_out: rt_film_denoise's level k; `variance`:
// denoise_var_to_out, k = 0 the prepare pass and k = i + 1 level i) and reads what write k - 1 wrote.  Write 0 reads `first`
// (rt_film_denoise: the sum; the prepare passes read their own inputs: NULL).
inline FilmWrite film_write(bool variance, int levels, int k, const void *first, int64_t first_stride, const FilmPingPong &b)
{
    const auto to_out = [&](int j) { return variance ? denoise_var_to_out(levels, j) : denoise_to_out(levels, j); };
    const auto side = [&](bool out, long long &stride) { stride = out ? b.out_stride : b.work_stride; return (double *)(out ? b.d_out : b.d_work); };
    FilmWrite w;
    w.dst = side(to_out(k), w.dst_stride);
    if (k == 0) { w.src = (const double *)first; w.src_stride = first_stride; }
    else w.src = side(to_out(k - 1), w.src_stride);
    return w;
}

// Level i of rt_film_denoise.
inline DenoiseArgs denoise_args(const FilmWrite &w, const void *d_guides, int64_t guide_stride, int ws, int h, int64_t n, const rt_denoise *dn,
                                int nsq, int i)
{
    DenoiseArgs a;
    std::memset(&a, 0, sizeof a);
    a.guides = (const float *)d_guides; a.guide_stride = guide_stride;
    a.ws = ws; a.h = h; a.nsq = nsq; a.demod = dn->demodulate; a.n = (double)n;
    a.src = w.src; a.src_stride = w.src_stride; a.dst = w.dst; a.dst_stride = w.dst_stride;
    denoise_level(a, dn->levels, i, dn->sigma);
    return a;
}

// What every write of a variance filter shares: the guides, the frame, the settings.
inline DenoiseVarArgs denoise_var_common(const void *d_guides, int64_t guide_stride, int ws, int h, const rt_denoise_variance *dv, int nsq)
{
    DenoiseVarArgs a;
    std::memset(&a, 0, sizeof a);
    a.guides = (const float *)d_guides; a.guide_stride = guide_stride;
    a.ws = ws; a.h = h; a.nsq = nsq; a.demod = dv->demodulate; a.prefilter = dv->prefilter;
    a.k2 = dv->kappa * dv->kappa; a.var_floor = dv->var_floor;
    return a;
}

// rt_film_denoise_variance: what its prepare pass reads, carried by every write.
inline void denoise_var_inputs(DenoiseVarArgs &a, const void *d_sum, int64_t sum_stride, const void *d_sq, int64_t sq_stride, int64_t n, int levels)
{
    a.sum = (const double *)d_sum; a.sum_stride = sum_stride; a.sq = (const double *)d_sq; a.sq_stride = sq_stride;
    a.copy = levels == 0; a.n = (double)n; a.n1 = (double)(n - 1);
}

// Write k of a variance filter (film_write): the prepare pass of rt_film_denoise_variance, or level k - 1 of either.
inline DenoiseVarArgs denoise_var_write(DenoiseVarArgs a, const FilmWrite &w, int levels, int k)
{
    a.src = w.src; a.src_stride = w.src_stride; a.dst = w.dst; a.dst_stride = w.dst_stride;
    if (k > 0) denoise_var_level(a, levels, k - 1);
    return a;
}

// The prepare pass of rt_film_denoise_variance_temporal (write 0).
inline DenoiseVarLenArgs denoise_var_len_args(const FilmWrite &w, const void *d_mean, int64_t mean_stride, const void *d_msq, int64_t msq_stride,
                                              const void *d_len, int ws, int h, const void *d_guides, int64_t guide_stride,
                                              const rt_denoise_variance *dv, double spatial_below)
{
    DenoiseVarLenArgs p;
    std::memset(&p, 0, sizeof p);
    p.mean = (const double *)d_mean; p.mean_stride = mean_stride; p.msq = (const double *)d_msq; p.msq_stride = msq_stride;
    p.len = (const float *)d_len; p.guides = (const float *)d_guides; p.guide_stride = guide_stride;
    p.dst = w.dst; p.dst_stride = w.dst_stride;
    p.ws = ws; p.h = h; p.demod = dv->demodulate; p.copy = dv->levels == 0; p.spatial_below = spatial_below;
    return p;
}

// rt_film_bloom: its rules in the header's order (the rule macros again: this entry was added behind the filters' arguments).
#define RT_FILM_RULE(ok, ...) do { if (!(ok)) return film_refusal(e, __VA_ARGS__); } while (0)
#define RT_FILM_RULES(call) do { const Refusal r_ = (call); if (r_.code != RT_OK) return r_; } while (0)

inline Refusal check_film_bloom(const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, const rt_bloom *bl, const void *d_out,
                                int64_t out_stride, const void *d_work, int64_t work_stride)
{
    const char *const e = "rt_film_bloom";
    RT_FILM_RULE(d_sum, "d_sum is NULL");
    RT_FILM_RULE(bl, "bl is NULL");
    RT_FILM_RULE(d_out, "d_out is NULL");
    RT_FILM_RULES(film_area(e, ws, h));
    RT_FILM_RULE(n >= 1, "n < 1");
    RT_FILM_RULE(bl->levels >= 0 && bl->levels <= RT_BLOOM_MAX_LEVELS, "levels outside 0..8");
    RT_FILM_RULE(std::isfinite(bl->threshold) && bl->threshold >= 0.0, "threshold must be finite and >= 0");
    RT_FILM_RULE(std::isfinite(bl->strength) && bl->strength >= 0.0, "strength must be finite and >= 0");
    RT_FILM_RULE(!(bl->flags & ~RT_BLOOM_NO_TILES), "unknown flag bit");
    RT_FILM_RULE(d_work || bl->levels < 1, "d_work is NULL with levels >= 1");
    const long long npx = (long long)ws * h;
    RT_FILM_RULES(film_strides(e, npx, {sum_stride, out_stride}));
    if (d_work) RT_FILM_RULES(film_strides(e, npx, {work_stride}));
    return film_own(e, {d_out, d_work}, {d_sum}, "d_out and d_work must be buffers of their own");
}

// rt_film_meter and rt_film_meter_solve: their rules in the header's order.
inline Refusal check_film_meter(const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, const void *d_hist)
{
    const char *const e = "rt_film_meter";
    RT_FILM_RULE(d_sum, "d_sum is NULL");
    RT_FILM_RULE(d_hist, "d_hist is NULL");
    RT_FILM_RULES(film_area(e, ws, h));
    RT_FILM_RULE(n >= 1, "n < 1");
    RT_FILM_RULE(sum_stride >= (long long)ws * h, "sum_stride smaller than the frame");
    RT_FILM_RULE(((unsigned long long)(uintptr_t)d_hist & 7) == 0, "d_hist is not 8-byte aligned");
    return film_own(e, {d_hist}, {d_sum}, "d_hist and d_sum must be buffers of their own");
}

inline Refusal check_film_meter_solve(const void *d_hist, const rt_meter *mt, const void *d_state)
{
    const char *const e = "rt_film_meter_solve";
    RT_FILM_RULE(d_hist, "d_hist is NULL");
    RT_FILM_RULE(mt, "mt is NULL");
    RT_FILM_RULE(d_state, "d_state is NULL");
    RT_FILM_RULE(std::isfinite(mt->key) && mt->key > 0.0, "key must be finite and > 0");
    RT_FILM_RULE(mt->percentile >= 0.0 && mt->percentile <= 1.0, "percentile outside 0..1");
    RT_FILM_RULE(std::isfinite(mt->min_exposure) && mt->min_exposure > 0.0, "min_exposure must be finite and > 0");
    RT_FILM_RULE(std::isfinite(mt->max_exposure) && mt->max_exposure > 0.0, "max_exposure must be finite and > 0");
    RT_FILM_RULE(mt->min_exposure <= mt->max_exposure, "min_exposure above max_exposure");
    RT_FILM_RULE(mt->rate > 0.0 && mt->rate <= 1.0, "rate outside (0, 1]");
    RT_FILM_RULE(mt->flags == 0, "flags must be 0");
    RT_FILM_RULE(mt->reserved == 0, "reserved must be 0");
    return film_own(e, {d_state}, {d_hist}, "d_state and d_hist must be buffers of their own");
}

#undef RT_FILM_RULE
#undef RT_FILM_RULES

inline MeterHistArgs meter_hist_args(const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, void *d_hist)
{
    return {(const double *)d_sum, (unsigned long long *)d_hist, sum_stride, (long long)ws * h, (double)n};
}

static_assert(sizeof(rt_meter) == 48, "rt_meter is 48 bytes");

// One launch of rt_film_bloom's plan (rt_bloom.h: bloom_plan): set s of the work planes is planes 3s .. 3s+2 of d_work.
inline BloomArgs bloom_args(const BloomLaunch &l, const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, const rt_bloom *bl, void *d_out,
                            int64_t out_stride, void *d_work, int64_t work_stride)
{
    const auto set = [&](int s) { return s < 0 ? (double *)nullptr : (double *)d_work + (long long)3 * s * work_stride; };
    BloomArgs a;
    std::memset(&a, 0, sizeof a);
    if (l.kind == BLOOM_BRIGHT) { a.src = (const double *)d_sum; a.src_stride = sum_stride; }
    else { a.src = set(l.src); a.src_stride = work_stride; }
    a.dst = set(l.dst); a.dst_stride = work_stride;
    a.out = (double *)d_out; a.out_stride = out_stride;
    a.ws = ws; a.h = h; a.step = l.step;
    a.n = (double)n; a.threshold = bl->threshold;
    a.wl = bl->levels > 0 ? bl->strength / (double)bl->levels : 0.0;
    return a;
}

static_assert(BLOOM_MAX_LEVELS == RT_BLOOM_MAX_LEVELS && BLOOM_NO_TILES == RT_BLOOM_NO_TILES, "rt_bloom.h restates the header's constants");
static_assert(2 * 3 == RT_BLOOM_WORK_PLANES, "the plan uses two sets of three work planes");

// rt_film_upsample and rt_render_guides_grid: their rules in the header's order (the rule macros once more: these entries were added
// behind bloom's and the meter's arguments).
#define RT_FILM_RULE(ok, ...) do { if (!(ok)) return film_refusal(e, __VA_ARGS__); } while (0)
#define RT_FILM_RULES(call) do { const Refusal r_ = (call); if (r_.code != RT_OK) return r_; } while (0)

// A closed-form grid that places pixels: five finite numbers, px, dy and dz not 0.
inline bool upsample_grid_ok(const double g[5])
{
    for (int i = 0; i < 5; ++i) if (!std::isfinite(g[i])) return false;
    return g[0] != 0.0 && g[2] != 0.0 && g[4] != 0.0;
}

inline Refusal check_film_upsample(const void *d_lo, int64_t lo_stride, int wl, int hl, int64_t n, const void *d_lo_guides, int64_t lo_guide_stride,
                                   const void *d_hi_guides, int64_t hi_guide_stride, int w, int h, const rt_upsample *up, const void *d_out,
                                   int64_t out_stride, const void *d_out_kind)
{
    const char *const e = "rt_film_upsample";
    RT_FILM_RULE(d_lo && d_lo_guides && d_hi_guides && d_out && up, "a buffer or up is NULL");
    RT_FILM_RULE(wl >= 1 && hl >= 1 && (long long)wl * hl <= RT_FILM_MAX_PIXELS, "wl*hl outside 1..RT_FILM_MAX_PIXELS");
    RT_FILM_RULE(w >= 1 && h >= 1 && (long long)w * h <= RT_FILM_MAX_PIXELS, "w*h outside 1..RT_FILM_MAX_PIXELS");
    RT_FILM_RULE(n >= 1, "n < 1");
    RT_FILM_RULES(film_strides(e, (long long)wl * hl, {lo_stride, lo_guide_stride}, "a plane stride is smaller than its frame"));
    RT_FILM_RULES(film_strides(e, (long long)w * h, {hi_guide_stride, out_stride}, "a plane stride is smaller than its frame"));
    RT_FILM_RULE(upsample_grid_ok(up->lo_grid) && upsample_grid_ok(up->hi_grid), "a grid entry is not finite, or a px, dy or dz is 0");
    RT_FILM_RULE(up->normal_cos >= -1.0 && up->normal_cos <= 1.0, "normal_cos outside [-1, 1]");
    RT_FILM_RULE(up->demodulate == 0 || up->demodulate == 1, "demodulate must be 0 or 1");
    RT_FILM_RULE(up->reserved == 0, "reserved must be 0");
    return film_own(e, {d_out, d_out_kind}, {d_lo, d_lo_guides, d_hi_guides}, "d_out and d_out_kind must be buffers of their own");
}

static_assert(sizeof(rt_upsample) == 96, "rt_upsample is 96 bytes");

inline void upsample_args(UpsampleArgs &a, const void *d_lo, int64_t lo_stride, int wl, int hl, int64_t n, const void *d_lo_guides,
                          int64_t lo_guide_stride, const void *d_hi_guides, int64_t hi_guide_stride, int w, int h, const rt_upsample *up,
                          void *d_out, int64_t out_stride, void *d_out_kind)
{
    a.lo = (const double *)d_lo; a.lo_guides = (const float *)d_lo_guides; a.hi_guides = (const float *)d_hi_guides;
    a.out = (double *)d_out; a.kind = (float *)d_out_kind;
    a.lo_stride = lo_stride; a.lo_guide_stride = lo_guide_stride; a.hi_guide_stride = hi_guide_stride; a.out_stride = out_stride;
    a.wl = wl; a.hl = hl; a.w = w; a.h = h; a.n = (double)n;
    a.lo_px = up->lo_grid[0]; a.lo_y0 = up->lo_grid[1]; a.lo_dy = up->lo_grid[2]; a.lo_z0 = up->lo_grid[3]; a.lo_dz = up->lo_grid[4];
    a.hi_px = up->hi_grid[0]; a.hi_y0 = up->hi_grid[1]; a.hi_dy = up->hi_grid[2]; a.hi_z0 = up->hi_grid[3]; a.hi_dz = up->hi_grid[4];
    a.normal_cos = up->normal_cos; a.demod = up->demodulate;
}

// rt_render_guides_grid: rt_set_raygen's rule for the frame, then rt_render_guides' for state, columns, buffer and stride, measured
// against the grid of the call.  The context's own grid is not asked for.
inline Refusal check_guides_grid(bool have_scene, bool have_cam, int w, int h, int x0, int x1, const void *d_guides, int64_t plane_stride)
{
    const char *const e = "rt_render_guides_grid";
    RT_FILM_RULE(d_guides, "d_guides is NULL");
    RT_FILM_RULE(rt_geo_frame_ok(w, h), "frame size out of range (1 <= w <= 2^31 - 8, 1 <= h <= 2^29 - 32, w*h <= 2^31)");
    RT_FILM_RULE(have_scene, "rt_set_scene has not been called", RT_ERR_STATE);
    RT_FILM_RULE(have_cam, "rt_set_camera has not been called", RT_ERR_STATE);
    RT_FILM_RULE(x0 >= 0 && x1 <= w && x0 < x1, "column range must satisfy 0 <= x0 < x1 <= w");
    RT_FILM_RULE(plane_stride >= (int64_t)(x1 - x0) * h, "plane_stride smaller than the slab");
    return {};
}

// The view of such a call: the context's camera and lens under the closed-form grid given.
inline View guides_grid_view(const View &ctx_view, int w, int h, double px, double y0, double dy, double z0, double dz)
{
    View v = ctx_view;
    v.w = w; v.h = h; v.px = px; v.y0 = y0; v.dy = dy; v.z0 = z0; v.dz = dz;
    v.explicit_grid = false; v.have_grid = true;
    return v;
}

#undef RT_FILM_RULE
#undef RT_FILM_RULES

}  // namespace rt
