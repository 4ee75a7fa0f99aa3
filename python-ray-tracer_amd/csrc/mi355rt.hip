// mi355rt.hip — host side of libmi355rt.so: the C ABI of include/mi355rt.h over the gfx950
// render kernel in rt_device.h.  HIP only (no torch, no CPU fallback): without a HIP device
// rt_create fails and nothing renders.  What a call decides before it touches the device lives in
// HIP-free headers: the packed scene (rt_scene.h), the launch arithmetic (rt_geometry.h), the
// launch's kernel (family, shape and twin: its entry in the one table KERNELS below) and order shape (rt_plan.h), the kernels' argument and the entry checks (rt_launch.h), the film entries' checks,
// kernel arguments and ping-pong plans (rt_film_launch.h), the dispatch-order feedback (rt_feedback.h), the per-stream state: cull-table
// sets, scratch buffers, scene readers (rt_streams.h).
#include "../../include/mi355rt.h"
#include "rt_device.h"
#include "rt_bloom.h"
#include "rt_denoise.h"
#include "rt_denoise_var.h"
#include "rt_feedback.h"
#include "rt_film.h"
#include "rt_film_launch.h"
#include "rt_geometry.h"
#include "rt_guides.h"
#include "rt_launch.h"
#include "rt_plan.h"
#include "rt_scene.h"
#include "rt_streams.h"
#include "rt_temporal.h"
#include "rt_upsample.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <array>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#pragma clang fp contract(off)

namespace {

std::string g_create_error;

struct Buf {                          // device memory, owned: freed with the Buf
    void *p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(Buf &&o) noexcept { *this = std::move(o); }
    Buf &operator=(Buf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~Buf() { if (p) (void)hipFree(p); }
};

}  // namespace

#define RT_COUNT_WORDS (4 + 2 * (RT_MAX_DEPTH + 1))   /* ray counters + per bounce {waves, alive lanes} */
#define RT_RENDER_CHUNKS 8   /* upper bound; the pipeline uses ctx->render_chunks of them */

struct rt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    struct Pipeline {                 // rt_render's chunk pipeline (created on first use, completely or not at all)
        hipStream_t stream2 = nullptr, copy_stream = nullptr;
        hipEvent_t chunk_ev[RT_RENDER_CHUNKS] = {};
        hipStream_t chunk_stream[RT_RENDER_CHUNKS] = {};
        template <class F> void streams(F f)
        {
            for (hipStream_t s : {stream2, copy_stream}) if (s) f(s);
            for (hipStream_t s : chunk_stream) if (s) f(s);
        }
        ~Pipeline()
        {
            streams([](hipStream_t s) { (void)hipStreamDestroy(s); });
            for (hipEvent_t e : chunk_ev) if (e) (void)hipEventDestroy(e);
        }
    };
    std::unique_ptr<Pipeline> pipe;
    int chunk_mode = -1;              // -1 = by destination memory type
    int cluster_min = rt::CLUSTER_MIN;            // scenes with more spheres are stored in clusters (MI355RT_CLUSTER_MINS overrides)
    int lanes_primary = 1;            // MI355RT_LANES_PRIMARY=0: the lane-owned traversal from bounce 1 on only (primary rays and their shadow
                                      // rays wave-uniform: +2..3 % since the group level exists)
    rt::PlanKnobs knobs;              // what steers the choice of a launch's kernel and order shape (rt_plan.h)
    int render_chunks = 4;            // MI355RT_CHUNKS overrides (1 = one launch, one copy)
    int log_kernels = 0;              // MI355RT_LOG_KERNELS=1: every render launch names its kernel on stderr (its shape and family number), every rt_render_guides call its table mode
    int remeasure = 24;               // MI355RT_REMEASURE: launches a dispatch order measured under an older camera is kept for before
                                      // the tile costs are measured again (a moving camera; any order renders the same frame)
    struct Slot {                     // rt_render_begin / rt_render_end: a frame in flight to host memory
        hipStream_t stream = nullptr;
        Buf u8, f32;
    } slots[RT_RENDER_SLOTS];
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // The packed scene records live in a ring of device buffers: rt_set_scene fills the NEXT one and launches carry the
    // pointer of the one that was current when they were queued, so frames in flight on any stream keep the scene they
    // were launched with (include/mi355rt.h: rt_render_begin).  A buffer comes up for reuse RT_SCENE_RING scene changes
    // later; the streams that launched with it (rt_streams.h) are synchronised then (by that time they have long finished with it).
    Buf scene[RT_SCENE_RING];
    int scene_cur = 0;
    Buf pixel_loc, u8, f32;
    rt::SceneLayout lay;          // the current scene (rt_scene.h): counts, families' flags, block offsets, plane codes, extent
    Buf texels[RT_SCENE_RING];    // per scene buffer of the ring: {R,G,B, texture id} float32 of the S + P object slots, then {R,G,B,-} of the scene's texels;
                                  // allocated by the first textured (or lit) scene that lands in the slot, grown when one needs more
    bool have_scene = false;
    rt::View view;                // camera, ray grid and lens (rt_launch.h)
    size_t lds_set[rt::ROWS] = {};            // per row of KERNELS: hipFuncAttributeMaxDynamicSharedMemorySize of its kernels
    size_t guides_lds_set = 0;                // ... of the three guides kernels (rt_render_guides)
    unsigned *tile_stats = nullptr;   // caller-owned device buffer or NULL
    // Scheduler feedback (rt_feedback.h has the rules and the slots' host state; the device buffers stay here)
    struct Feedback : rt::FeedbackSlot {
        Buf cost, gtmp, btmp, order[2]; // per-block costs of the measuring launch, order_kernel's scratch, the dispatch orders
    } fbs[RT_FEEDBACK_SLOTS];
    rt::FeedbackBook book;
    rt_ctx() { for (int i = 0; i < RT_FEEDBACK_SLOTS; ++i) book.slot[i] = &fbs[i]; }
    // Every stream the context created (a caller's streams are the caller's).
    template <class F> void own_streams(F f)
    {
        if (stream) f(stream);
        for (Slot &sl : slots) if (sl.stream) f(sl.stream);
        if (pipe) pipe->streams(f);
    }
    // (the device is the current one, and the streams are drained: rt_destroy; the members free their buffers after this)
    ~rt_ctx()
    {
        for (auto &f : fbs)
            for (void *e : rt::release_events(f)) (void)hipEventDestroy((hipEvent_t)e);
        pipe.reset();
        own_streams([](hipStream_t s) { (void)hipStreamDestroy(s); });
        for (hipEvent_t e : {ev0, ev1}) if (e) (void)hipEventDestroy(e);
    }
    rt_stats stats = {};              // host-side launch counters (the ray counters live in `counts`)
    Buf counts;                       // 4 x uint64 on the device: ray counters of RT_FLAG_COUNT_RAYS launches
    int cu_count = 256;
    unsigned long long epoch = 1;     // bumped by every rt_set_*: scene, camera or ray grid changed
    unsigned long long scene_epoch = 1;   // bumped by rt_set_scene only
    // Per launching stream (rt_streams.h): its two cull-table sets, its float64 lattice samples (RT_AA_REFERENCE), its float32 pass
    // frames (rt_film_accumulate), and the scene buffers of the ring it reads.
    rt::StreamBook<Buf> streams;
    std::string err;
};

namespace {

int fail(rt_ctx *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->err = msg; else g_create_error = msg;
    return code;
}

#define RT_HIP(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail((ctx), RT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));    \
    } while (0)

int ensure(rt_ctx *ctx, Buf &b, size_t bytes)
{
    if (bytes <= b.cap) return RT_OK;
    if (b.p) { RT_HIP(ctx, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    RT_HIP(ctx, hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return RT_OK;
}

int refuse(rt_ctx *ctx, const rt::Refusal &r)
{
    if (r.code == RT_OK) return RT_OK;
    return fail(ctx, r.code, r.entry ? std::string(r.entry) + ": " + r.msg : std::string(r.msg));
}

int check_params(rt_ctx *ctx, const rt_params *p, int x0, int x1) { return refuse(ctx, rt::check_params(ctx->have_scene, ctx->view, ctx->lay, p, x0, x1)); }

hipStream_t stream_of(rt_ctx *ctx, void *stream) { return stream ? (hipStream_t)stream : ctx->stream; }

using StreamRecord = rt::StreamBook<Buf>::Record;

// The record of a launching stream (rt_streams.h), with the current scene buffer noted as one it reads (set_scene drains the
// readers before the buffer is rewritten).
int stream_record(rt_ctx *ctx, hipStream_t stream, StreamRecord **out)
{
    const int rc = ctx->streams.record(stream, out);
    if (rc != RT_OK) return fail(ctx, rc, ctx->streams.NO_MEMORY);
    ctx->streams.reads_scene(**out, ctx->scene_cur);
    return RT_OK;
}

// More than the default 48 KiB of dynamic LDS: raised on all of `fns` (nullptr: no such kernel) at once; `set` remembers the size.
int raise_lds(rt_ctx *ctx, const void *const *fns, size_t n, size_t lds, size_t &set)
{
    if (lds <= 48 * 1024 || lds <= set) return RT_OK;
    for (size_t i = 0; i < n; ++i)
        if (fns[i]) RT_HIP(ctx, hipFuncSetAttribute(fns[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    set = lds;
    return RT_OK;
}

using rt::Shape; using rt::SHAPES; using rt::NSHAPES;

// KERNELS[row][i]: the render kernel of shape SHAPES[i] in that row of rt_plan.h's table (row_kernels: a family's kernels, the
// ground-plane twins, their small-scene twins per number of cull groups), or nullptr: the row has none (row_has_kernel).  A plan
// names its entry: KERNELS[plan.row()][plan.index].
template <int ROW, int I>
const void *kernel_at()
{
    constexpr Shape s = SHAPES[I];
    constexpr rt::Row r = rt::row_kernels(ROW);
    if constexpr (rt::row_has_kernel(ROW, s))
        return (const void *)rt::render_kernel<s.aa, s.park, s.wpw, s.count, s.lat, s.mode, r.family, r.ground, r.groups>;
    else
        return nullptr;
}
using KernelRow = std::array<const void *, NSHAPES>;
template <int ROW, int... I>
KernelRow kernel_row(std::integer_sequence<int, I...>)
{
    return {kernel_at<ROW, I>()...};
}
template <int... ROW>
std::array<KernelRow, rt::ROWS> all_kernels(std::integer_sequence<int, ROW...>)
{
    return {{kernel_row<ROW>(std::make_integer_sequence<int, NSHAPES>{})...}};
}
const std::array<KernelRow, rt::ROWS> KERNELS = all_kernels(std::make_integer_sequence<int, rt::ROWS>{});

// One of the stream's own buffers, `bytes` large (rt_streams.h: growing frees the old buffer, behind a synchronise).
int stream_buffer(rt_ctx *ctx, Buf &b, hipStream_t stream, size_t bytes, bool sync)
{
    if (sync) RT_HIP(ctx, hipStreamSynchronize(stream));
    return ensure(ctx, b, bytes);
}

// The cull tables for this launch's scene / camera position / floor: reuse one of the stream's sets or rebuild its older one.
int acquire_tables(rt_ctx *ctx, StreamRecord &sr, const rt::KParams &k, const float **out)
{
    const hipStream_t stream = (hipStream_t)sr.stream;
    const rt::TableKey key = rt::table_key(ctx->scene_epoch, k.anchors, k.floor_anch, k.cam_o);
    const size_t bytes = rt::table_floats(k.S, k.NC, k.anchors, false, true, k.P) * sizeof(float);   // (with the colours)
    const rt::TableDecision d = ctx->streams.tables(sr, key, bytes);
    Buf &b = sr.buf[rt::BUF_TABLES0 + d.set];
    if (d.rebuild) {
        int rc = stream_buffer(ctx, b, stream, d.bytes, d.sync);
        if (rc != RT_OK) return rc;
        hipLaunchKernelGGL(rt::tables_kernel, dim3(1), dim3(rt::TABLE_THREADS), 0, stream, k, (float *)b.p);
        ctx->stats.table_builds++;
        RT_HIP(ctx, hipGetLastError());
        ctx->streams.tables_queued(sr, d.set, key);
    }
    *out = (const float *)b.p;
    return RT_OK;
}

int dispatch(rt_ctx *ctx, const rt_params *p, rt::KParams &k, const rt::LaunchPlan &plan, hipStream_t stream, int nframes, int64_t frame_stride);

// nframes > 1 (rt_render_sequence): that many frames of the current scene and camera, frame f into the outputs +
// f * frame_stride elements — one launch for all of them where the dispatch order is settled.
int launch(rt_ctx *ctx, const rt_params *p, int x0, int x1, void *d_u8, void *d_f32, int64_t plane_stride,
           hipStream_t stream, int nframes = 1, int64_t frame_stride = 0)
{
    const rt::View &v = ctx->view;
    // (RT_AA_REFERENCE on the closed-form grid renders the half-pixel lattice, below: lattice columns [li0, li1))
    long long li0 = 0, li1 = 0;
    const bool lattice = p->aa_mode == RT_AA_REFERENCE && !v.explicit_grid && rt_geo_lattice(v.w, v.h, x0, x1, &li0, &li1) &&
                         !(p->flags & RT_FLAG_AA_PER_PIXEL);
    // the launch's family, kernel and LDS size (rt_plan.h), decided once: every slab and frame of the launch runs the same kernel
    const rt::LaunchPlan plan = rt::plan_launch(ctx->lay, ctx->knobs, v.lens_a, !lattice && p->aa_mode != 0, p->flags, lattice, rt::anchors_of(ctx->lay));
    if (plan.index < 0 || !KERNELS[plan.row()][plan.index])
        return fail(ctx, RT_ERR_STATE, "no render kernel for this launch");   // (unreachable: rt_plan.h, missing_kernels_never_park; a twin is named only where the shape has one)
    StreamRecord *sr = nullptr;                                // the stream's record, looked up once: scene, tables, lattice
    int rc = stream_record(ctx, stream, &sr);
    if (rc != RT_OK) return rc;
    rt::KParams k;
    rt::render_part(k, v, ctx->lay, plan.family, p, (const double *)ctx->scene[ctx->scene_cur].p, (const double *)ctx->pixel_loc.p,
                    (const float *)ctx->texels[ctx->scene_cur].p, ctx->lanes_primary, x0, x1, d_u8, d_f32, plane_stride, ctx->tile_stats);
    rc = acquire_tables(ctx, *sr, k, &k.ftab);
    if (rc != RT_OK) return rc;
    // RT_AA_REFERENCE on the closed-form grid: the reference's nine taps of a pixel are the 3x3 neighbourhood of the
    // pixel's centre on the (2w-1) x (2h-1) half-pixel lattice — the tap between two pixels is 0.5 Pa + 0.5 Pb, bit
    // for bit the same from either side (IEEE addition commutes), and with a separable grid both diagonals of a cell
    // cross in the same point.  So every lattice sample is traced ONCE (4 per pixel instead of 9) by the plain kernel
    // over the lattice "frame", stored as float64 (R,G,B), and a second small kernel sums each pixel's nine samples in
    // the reference's order (kernels.py:53-65, including its G/B swap).  Explicit pixel_loc grids are not separable
    // in general and keep the nine-taps-per-pixel kernel.
    if (lattice) {
        // one lattice buffer per launching stream, so that frames in flight on different streams keep their samples apart
        Buf &lb = sr->buf[rt::BUF_LATTICE];
        const size_t bytes = (size_t)(li1 - li0) * (size_t)(2ll * v.h - 1) * 3 * sizeof(double);
        rc = stream_buffer(ctx, lb, stream, bytes, rt::growth(lb.cap, bytes).sync);
        if (rc != RT_OK) return rc;
        double *lat = (double *)lb.p;
        rt::KParams kl;
        rt::lattice_pair(k, kl, li0, li1, lat);
        const long long npx = (long long)(x1 - x0) * v.h;
        for (int f = 0; f < nframes; ++f) {                    // the stream's one lattice buffer serves the frames in turn
            rc = dispatch(ctx, p, kl, plan, stream, 1, 0);
            if (rc != RT_OK) return rc;
            const rt::KParams kf = rt::frame_params(k, f, frame_stride);
            hipLaunchKernelGGL(rt::aa_resolve_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, stream, kf);
            RT_HIP(ctx, hipGetLastError());
        }
        return RT_OK;
    }
    return dispatch(ctx, p, k, plan, stream, nframes, frame_stride);
}

using Feedback = rt_ctx::Feedback;
static_assert(std::is_convertible<hipStream_t, void *>::value && std::is_convertible<hipEvent_t, void *>::value,
              "rt_feedback.h keeps streams and events as opaque handles");
int feedback_slot(rt_ctx *ctx, const rt::FeedbackKey &key, Feedback **out);
int switch_order(rt_ctx *ctx, Feedback &f);
int launch_one(rt_ctx *ctx, rt::KParams &k, const rt::LaunchPlan &plan, const rt_geo_plan &g, const rt::OrderShape &os,
               Feedback *f, hipStream_t stream, int nframes, int64_t frame_stride);

// One launch of the planned kernel over the tiles k describes, cut into pieces that one dispatch holds and one dispatch order
// serves; each piece finds its feedback slot, switches to a finished order and goes out (launch_one).
int dispatch(rt_ctx *ctx, const rt_params *p, rt::KParams &k, const rt::LaunchPlan &plan, hipStream_t stream, int nframes, int64_t frame_stride)
{
    const int x0 = k.x0, x1 = k.x1;
    // At most RT_GEO_MAX_ITEMS work-items per dispatch (rt_geometry.h): a frame beyond that alone goes out as column slabs
    // (they assemble bit-identically), one dispatch each; a sequence as batches of frames.
    const rt_geo_plan g = rt_geo_plan_of(x0, x1, k.h, plan.shape.wpw, nframes);
    auto frame_of = [&](int fr) { return rt::frame_params(k, fr, frame_stride); };
    if (g.nslabs > 1) {
        for (int fr = 0; fr < nframes; ++fr)
            for (long long s = 0; s < g.nslabs; ++s) {
                rt::KParams kf = rt::slab_params(frame_of(fr), g, s);
                int rc = dispatch(ctx, p, kf, plan, stream, 1, 0);
                if (rc != RT_OK) return rc;
            }
        return RT_OK;
    }
    if (nframes > g.frames_per_dispatch) {                    // (more work-items than one dispatch holds: batches of frames)
        const int fpd = (int)g.frames_per_dispatch;
        for (int fr = 0; fr < nframes; fr += fpd) {
            rt::KParams kf = frame_of(fr);
            int rc = dispatch(ctx, p, kf, plan, stream, std::min(fpd, nframes - fr), frame_stride);
            if (rc != RT_OK) return rc;
        }
        return RT_OK;
    }
    const rt::OrderShape os = rt::order_shape(plan, ctx->knobs, p->flags, g);
    Feedback *f = nullptr;                                     // RT_FLAG_NO_FEEDBACK / one-block launches: no slot
    if (os.feedback) {
        int rc = feedback_slot(ctx, rt::feedback_key(x0, x1, k.h, k.aa, plan.shape.lat, k.depth, k.spp, os.code), &f);
        if (rc == RT_OK) rc = switch_order(ctx, *f);
        if (rc != RT_OK) return rc;
    }
    // A launch of several frames (rt_render_sequence) is ONE launch only in a settled order; until then its frames go
    // through this function one by one (a measuring launch stores the costs of one frame).
    if (nframes > 1 && f && !rt::settled(*f, ctx->epoch, ctx->remeasure)) {
        // the first frame on its own (it measures, if no measurement is in flight), then — rather than rendering more
        // frames singly while the order is being built — wait for the build (a fraction of a millisecond, twice per new
        // geometry) and hand the rest back: at most two single frames before whole batches go out in the settled order
        rt::KParams kf = frame_of(0);
        int rc = dispatch(ctx, p, kf, plan, stream, 1, 0);
        if (rc != RT_OK) return rc;
        if (f->building) RT_HIP(ctx, hipEventSynchronize((hipEvent_t)f->done));
        rt::KParams kr = frame_of(1);
        return dispatch(ctx, p, kr, plan, stream, nframes - 1, frame_stride);
    }
    return launch_one(ctx, k, plan, g, os, f, stream, nframes, frame_stride);
}

// The feedback slot of a launch geometry (rt_feedback.h: the one that holds it, else a free or the least recently used one).
int feedback_slot(rt_ctx *ctx, const rt::FeedbackKey &key, Feedback **out)
{
    bool live = false;
    const int i = ctx->book.find(key, &live);
    if (live) RT_HIP(ctx, hipDeviceSynchronize());             // launches of the evicted geometry may still read its orders (rare: > 8 geometries)
    ctx->book.claim(i, key);
    Feedback *f = &ctx->fbs[i];
    if (!f->done) {
        hipEvent_t ev = nullptr;
        RT_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        f->done = ev;
    }
    *out = f;
    return RT_OK;
}

// The order being built is complete: switch to it, and record the events that fence the old order's readers (rt_feedback.h).
int switch_order(rt_ctx *ctx, Feedback &f)
{
    if (!f.building) return RT_OK;
    const hipError_t q = hipEventQuery((hipEvent_t)f.done);
    if (q != hipSuccess) {
        (void)hipGetLastError();                               // hipErrorNotReady is an answer, not a failure
        return RT_OK;
    }
    for (void *us : rt::switch_order(f)) {
        hipEvent_t ev = (hipEvent_t)rt::take_spare(f);
        if (!ev) RT_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        RT_HIP(ctx, hipEventRecord(ev, (hipStream_t)us));
        rt::add_fence(f, us, ev);
    }
    return RT_OK;
}

// One dispatch of the planned kernel: nframes frames of g.blocks workgroups each, in f's order (os.feedback: f is the geometry's
// slot, else nullptr), measuring the tiles' costs behind it if the order is not settled.
int launch_one(rt_ctx *ctx, rt::KParams &k, const rt::LaunchPlan &plan, const rt_geo_plan &g, const rt::OrderShape &os,
               Feedback *f, hipStream_t stream, int nframes, int64_t frame_stride)
{
    const Shape &sh = plan.shape;
    const KernelRow &kernels = KERNELS[plan.row()];
    const void *fn = kernels[plan.index];                      // (launch() checked it)
    const unsigned grid = (unsigned)g.blocks;
    if (ctx->log_kernels)
        std::fprintf(stderr, "mi355rt: render_kernel<%d, %d, %d, %d, %d, %d, (rt::Family)%d>%s\n", (int)sh.aa, (int)sh.park, sh.wpw, (int)sh.count,
                     (int)sh.lat, sh.mode, (int)plan.family, plan.twin.ground ? " ground" : "");
    if (ctx->log_kernels && plan.twin.groups > 0) std::fprintf(stderr, "mi355rt: cull groups %d\n", plan.twin.groups);
    int rc = raise_lds(ctx, kernels.data(), kernels.size(), plan.lds, ctx->lds_set[plan.row()]);
    if (rc != RT_OK) return rc;
    if (sh.count) {
        if (!ctx->counts.p) {
            rc = ensure(ctx, ctx->counts, RT_COUNT_WORDS * sizeof(unsigned long long));
            if (rc != RT_OK) return rc;
            RT_HIP(ctx, hipMemsetAsync(ctx->counts.p, 0, RT_COUNT_WORDS * sizeof(unsigned long long), stream));
        }
        k.ray_counts = (unsigned long long *)ctx->counts.p;
    }
    const rt::FeedbackLaunch d = f ? rt::decide_launch(*f, stream, ctx->epoch, ctx->remeasure) : rt::FeedbackLaunch{};
    if (d.read >= 0) k.order = (const unsigned *)f->order[d.read].p;
    if (d.measure) {
        const size_t words = (size_t)os.items * sizeof(unsigned);
        rc = ensure(ctx, f->cost, words);
        if (rc == RT_OK) rc = ensure(ctx, f->btmp, words);
        if (rc == RT_OK) rc = ensure(ctx, f->order[0], 2 * words);    // longest-first order, then the tile-order one (order_kernel)
        if (rc == RT_OK) rc = ensure(ctx, f->order[1], 2 * words);
        if (rc == RT_OK) rc = ensure(ctx, f->gtmp, words + sizeof(unsigned));
        if (rc != RT_OK) return rc;
        for (void *ev : d.wait) RT_HIP(ctx, hipStreamWaitEvent(stream, (hipEvent_t)ev, 0));
        k.cost = (unsigned *)f->cost.p;
    }
    rt::dispatch_part(k, nframes, grid, frame_stride, os);
    void *args[] = {(void *)&k};
    RT_HIP(ctx, hipLaunchKernel(fn, dim3(grid * (unsigned)nframes), dim3(64 * sh.wpw), args, plan.lds, stream));
    ctx->stats.launches++;
    ctx->stats.frames += (uint64_t)nframes;
    if (d.settled) ctx->stats.launches_settled++;
    if (d.measure) ctx->stats.launches_measuring++;
    if (d.measure) {
        hipLaunchKernelGGL(rt::order_kernel, dim3(1), dim3(rt::ORDER_THREADS), 0, stream, (const unsigned *)f->cost.p,
                           (unsigned *)f->gtmp.p, (unsigned *)f->btmp.p, (unsigned *)f->order[d.write].p, (int)os.items, os.otiles ? os.gshift + os.wshift : os.gshift,
                           os.otiles ? os.wshift : 0, os.otiles ? k.ntiles : (int)grid);
        RT_HIP(ctx, hipEventRecord((hipEvent_t)f->done, stream));
        rt::order_queued(*f, ctx->epoch);
    }
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

// The writes of a variance filter: `prepare` launches write 0 (it is handed the write and the grid), then one launch of
// denoise_var_kernel per level, ping-pong between d_out and d_work so that the last write ends in d_out.
template <class Prepare>
int variance_filter(rt_ctx *ctx, const rt::DenoiseVarArgs &common, int levels, const rt::FilmPingPong &pp, hipStream_t st, Prepare prepare)
{
    const dim3 grid(rt::denoise_grid((long long)common.ws * common.h, ctx->cu_count));
    for (int k = 0; k <= levels; ++k) {
        const rt::FilmWrite w = rt::film_write(true, levels, k, nullptr, 0, pp);
        if (k == 0) prepare(w, grid);
        else hipLaunchKernelGGL(rt::denoise_var_kernel, grid, dim3(rt::DENOISE_THREADS), 0, st, rt::denoise_var_write(common, w, levels, k));
        RT_HIP(ctx, hipGetLastError());
    }
    return RT_OK;
}

// One launch of a temporal kernel (rt_temporal.h) over the context's full frame; the arguments have been checked and built.
template <class Args>
int temporal_launch(rt_ctx *ctx, void (*kernel)(Args), const Args &a, void *stream)
{
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(kernel, dim3(rt::temporal_grid((long long)ctx->view.w * ctx->view.h, ctx->cu_count)), dim3(rt::TEMPORAL_THREADS), 0,
                       stream_of(ctx, stream), a);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

int rt_device_count(int *count)
{
    if (!count) return RT_ERR_BAD_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; g_create_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e); return RT_ERR_NO_DEVICE; }
    *count = n;
    return RT_OK;
}

int rt_create(rt_ctx **out, int device)
{
    if (!out) return fail(nullptr, RT_ERR_BAD_ARG, "ctx out-pointer is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, RT_ERR_NO_DEVICE, std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    if (device < 0 || device >= n) return fail(nullptr, RT_ERR_NO_DEVICE, "device index out of range");
    rt_ctx *ctx = new (std::nothrow) rt_ctx;
    if (!ctx) return fail(nullptr, RT_ERR_ALLOC, "out of host memory");
    ctx->device = device;
    if (const char *e = std::getenv("MI355RT_LANES_PRIMARY")) ctx->lanes_primary = std::atoi(e);
    if (const char *e = std::getenv("MI355RT_LANES_MINS")) ctx->knobs.lanes_min_spheres = std::atoi(e);
    if (const char *e = std::getenv("MI355RT_CLUSTER_MINS")) ctx->cluster_min = std::max(8, std::atoi(e));
    if (const char *e = std::getenv("MI355RT_CHUNK_MODE")) ctx->chunk_mode = std::atoi(e);
    if (const char *e = std::getenv("MI355RT_ORDER_GROUP")) { const int v = std::atoi(e); if (v >= 0 && v <= 6) ctx->knobs.order_group = v; }
    if (const char *e = std::getenv("MI355RT_REMEASURE")) ctx->remeasure = std::max(0, std::atoi(e));
    if (const char *e = std::getenv("MI355RT_F32_RECORDS")) ctx->knobs.f32_records = std::atoi(e) != 0;
    if (const char *e = std::getenv("MI355RT_WPW2_MAX_IMAGE")) ctx->knobs.wpw2_max_image = (size_t)std::max(0, std::atoi(e));
    if (const char *e = std::getenv("MI355RT_ORDER_TILES")) ctx->knobs.order_tiles = std::atoi(e) != 0;
    if (const char *e = std::getenv("MI355RT_LANES_PARK")) ctx->knobs.lanes_park = std::atoi(e) != 0;
    if (const char *e = std::getenv("MI355RT_GROUND_PLANE")) ctx->knobs.ground_plane = std::atoi(e) != 0;
    if (const char *e = std::getenv("MI355RT_SMALL_SCENE")) ctx->knobs.small_scene = std::atoi(e) != 0;
    if (const char *e = std::getenv("MI355RT_LOG_KERNELS")) ctx->log_kernels = std::atoi(e) != 0;
    if (const char *e = std::getenv("MI355RT_SEQ_ORDER")) ctx->knobs.seq_order = std::atoi(e) != 0 ? 1 : 0;
    if (const char *e = std::getenv("MI355RT_CHUNKS")) { const int v = std::atoi(e); if (v >= 1 && v <= RT_RENDER_CHUNKS) ctx->render_chunks = v; }
    hipError_t s;
    if ((s = hipSetDevice(device)) != hipSuccess || (s = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess ||
        (s = hipEventCreate(&ctx->ev0)) != hipSuccess || (s = hipEventCreate(&ctx->ev1)) != hipSuccess) {
        std::string m = std::string("context setup: ") + hipGetErrorString(s);
        delete ctx;
        return fail(nullptr, RT_ERR_HIP, m);
    }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) ctx->cu_count = cus;
        else (void)hipGetLastError();
    }
    *out = ctx;
    return RT_OK;
}

int rt_destroy(rt_ctx *ctx)
{
    if (!ctx) return RT_OK;
    (void)hipSetDevice(ctx->device);
    ctx->own_streams([](hipStream_t s) { (void)hipStreamSynchronize(s); });
    delete ctx;
    return RT_OK;
}

const char *rt_last_error(const rt_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

// Every rt_set_scene* entry: pack the scene on the host (rt_scene.h), upload it into the next buffer of the ring, and make its
// layout the context's.  A scene that fails validation leaves the context as it was.
static int set_scene(rt_ctx *ctx, const rt::SceneDesc &desc)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    const rt::PackedScene ps = rt::pack_scene(desc, ctx->cluster_min, ctx->knobs.lanes_min_spheres);
    if (ps.status != RT_OK) return fail(ctx, ps.status, ps.error);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = ps.rec.size() * sizeof(double);
    // the next buffer of the ring: launches in flight keep reading the buffers they were queued with.  Whatever
    // launched with THIS buffer did so RT_SCENE_RING scene changes ago; its streams are drained before it is rewritten.
    const int next = (ctx->scene_cur + 1) % RT_SCENE_RING;
    int rc = ctx->streams.drain_scene(next, [ctx](void *st) { RT_HIP(ctx, hipStreamSynchronize((hipStream_t)st)); return (int)RT_OK; });
    if (rc == RT_OK) rc = ensure(ctx, ctx->scene[next], bytes);
    if (rc != RT_OK) return rc;
    if (ps.layout.T > 0 || ps.layout.lit) {                 // (the texture and lighting kernels' texel array)
        rc = ensure(ctx, ctx->texels[next], ps.texels.size() * sizeof(float));
        if (rc != RT_OK) return rc;
        RT_HIP(ctx, hipMemcpyAsync(ctx->texels[next].p, ps.texels.data(), ps.texels.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    }
    RT_HIP(ctx, hipMemcpyAsync(ctx->scene[next].p, ps.rec.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));   // ps is about to go out of scope; other streams may launch at once
    ctx->scene_cur = next;
    ctx->lay = ps.layout;
    ctx->have_scene = true;
    ctx->epoch++;
    ctx->scene_epoch++;
    return RT_OK;
}

// What the entries from rt_set_scene_materials on share.
static rt::SceneDesc scene_desc(const float *spheres, int S, const float *lights, int L, const float *planes, int P, int flags,
                                const double *materials, int M, int ncols, const int32_t *sphere_material, const int32_t *plane_material)
{
    rt::SceneDesc d;
    d.spheres = spheres; d.S = S; d.lights = lights; d.L = L; d.planes = planes; d.P = P; d.flags = flags;
    d.materials = materials; d.M = M; d.ncols = ncols; d.sphere_material = sphere_material; d.plane_material = plane_material;
    return d;
}

// The entries from rt_set_scene_textures on.
static void add_textures(rt::SceneDesc &d, const rt_texture *textures, int T, const int32_t *sphere_texture, const int32_t *plane_texture,
                         const float *texels, int64_t n_texels)
{
    d.textures = textures; d.T = T; d.sphere_texture = sphere_texture; d.plane_texture = plane_texture;
    d.texels = texels; d.n_texels = n_texels;
}

// The entries from rt_set_scene_area_lights on: the radii may be NULL only where there is no light.
static int set_scene_radii(rt_ctx *ctx, rt::SceneDesc &d, const float *light_radius, int shadow_samples)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (d.L > 0 && !light_radius) return fail(ctx, RT_ERR_BAD_ARG, "light_radius is NULL with L > 0");
    static const float none = 0.0f;
    d.light_radius = light_radius ? light_radius : &none;
    d.shadow_samples = shadow_samples;
    return set_scene(ctx, d);
}

int rt_set_scene(rt_ctx *ctx, const float *spheres, int S, const float *lights, int L, const float *planes, int P, int flags)
{
    return set_scene(ctx, scene_desc(spheres, S, lights, L, planes, P, flags, nullptr, 0, 3, nullptr, nullptr));
}

int rt_set_scene_materials(rt_ctx *ctx, const float *spheres, int S, const float *lights, int L, const float *planes, int P, int flags,
                           const double *materials, int M, const int32_t *sphere_material, const int32_t *plane_material)
{
    return set_scene(ctx, scene_desc(spheres, S, lights, L, planes, P, flags, materials, M, 3, sphere_material, plane_material));
}

int rt_set_scene_materials_ex(rt_ctx *ctx, const float *spheres, int S, const float *lights, int L, const float *planes, int P, int flags,
                              const double *materials, int M, int ncols, const int32_t *sphere_material, const int32_t *plane_material)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (ncols != 3 && ncols != 5) return fail(ctx, RT_ERR_BAD_ARG, "ncols must be 3 or 5");
    return set_scene(ctx, scene_desc(spheres, S, lights, L, planes, P, flags, materials, M, ncols, sphere_material, plane_material));
}

int rt_set_scene_materials_scatter(rt_ctx *ctx, const float *spheres, int S, const float *lights, int L, const float *planes, int P,
                                   int flags, const double *materials, int M, int ncols, const int32_t *sphere_material,
                                   const int32_t *plane_material)
{
    return set_scene(ctx, scene_desc(spheres, S, lights, L, planes, P, flags, materials, M, ncols, sphere_material, plane_material));
}

int rt_set_scene_area_lights(rt_ctx *ctx, const float *spheres, int S, const float *lights, int L, const float *planes, int P,
                             int flags, const double *materials, int M, int ncols, const int32_t *sphere_material,
                             const int32_t *plane_material, const float *light_radius, int shadow_samples)
{
    rt::SceneDesc d = scene_desc(spheres, S, lights, L, planes, P, flags, materials, M, ncols, sphere_material, plane_material);
    return set_scene_radii(ctx, d, light_radius, shadow_samples);
}

int rt_set_scene_textures(rt_ctx *ctx, const float *spheres, int S, const float *lights, int L, const float *planes, int P,
                          int flags, const double *materials, int M, int ncols, const int32_t *sphere_material,
                          const int32_t *plane_material, const float *light_radius, int shadow_samples,
                          const rt_texture *textures, int T, const int32_t *sphere_texture, const int32_t *plane_texture,
                          const float *texels, int64_t n_texels)
{
    rt::SceneDesc d = scene_desc(spheres, S, lights, L, planes, P, flags, materials, M, ncols, sphere_material, plane_material);
    add_textures(d, textures, T, sphere_texture, plane_texture, texels, n_texels);
    return set_scene_radii(ctx, d, light_radius, shadow_samples);
}

int rt_set_scene_lighting(rt_ctx *ctx, const float *spheres, int S, const float *lights, int L, const float *planes, int P,
                          int flags, const double *materials, int M, int ncols, const int32_t *sphere_material,
                          const int32_t *plane_material, const float *light_radius, int shadow_samples,
                          const rt_texture *textures, int T, const int32_t *sphere_texture, const int32_t *plane_texture,
                          const float *texels, int64_t n_texels, const float *light_rgb)
{
    rt::SceneDesc d = scene_desc(spheres, S, lights, L, planes, P, flags, materials, M, ncols, sphere_material, plane_material);
    add_textures(d, textures, T, sphere_texture, plane_texture, texels, n_texels);
    d.light_rgb = light_rgb; d.lighting = true;
    return set_scene_radii(ctx, d, light_radius, shadow_samples);
}

int rt_set_scene_sky(rt_ctx *ctx, const float *spheres, int S, const float *lights, int L, const float *planes, int P,
                     int flags, const double *materials, int M, int ncols, const int32_t *sphere_material,
                     const int32_t *plane_material, const float *light_radius, int shadow_samples,
                     const rt_texture *textures, int T, const int32_t *sphere_texture, const int32_t *plane_texture,
                     const float *texels, int64_t n_texels, const float *light_rgb, const double *sky)
{
    rt::SceneDesc d = scene_desc(spheres, S, lights, L, planes, P, flags, materials, M, ncols, sphere_material, plane_material);
    add_textures(d, textures, T, sphere_texture, plane_texture, texels, n_texels);
    d.light_rgb = light_rgb; d.lighting = true; d.sky = sky;
    return set_scene_radii(ctx, d, light_radius, shadow_samples);
}

int rt_set_camera(rt_ctx *ctx, const double origin[3], const double rotation[9])
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!origin || !rotation) return fail(ctx, RT_ERR_BAD_ARG, "NULL camera array");
    // the same camera again (the reference's driver passes it with every launch, main.py:41-47) changes nothing a
    // tile's cost depends on: the measured dispatch order and the cull tables stay valid
    rt::View &v = ctx->view;
    if (v.have_cam && std::memcmp(v.cam_o, origin, sizeof v.cam_o) == 0 &&
        std::memcmp(v.cam_R, rotation, sizeof v.cam_R) == 0) return RT_OK;
    std::memcpy(v.cam_o, origin, sizeof v.cam_o);
    std::memcpy(v.cam_R, rotation, sizeof v.cam_R);
    v.have_cam = true;
    ctx->epoch++;
    return RT_OK;
}

int rt_set_lens(rt_ctx *ctx, double aperture, double focus_distance)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!(std::isfinite(aperture) && aperture >= 0.0)) return fail(ctx, RT_ERR_BAD_ARG, "aperture must be finite and >= 0");
    if (!(std::isfinite(focus_distance) && focus_distance > 0.0))
        return fail(ctx, RT_ERR_BAD_ARG, "focus_distance must be finite and > 0");
    // the same lens again changes nothing (as rt_set_camera), nor does a new focus without an aperture (the pinhole camera
    // ignores it); a new lens starts dispatch-order measuring again
    rt::View &v = ctx->view;
    if (aperture == v.lens_a && (focus_distance == v.lens_f || aperture == 0.0)) { v.lens_f = focus_distance; return RT_OK; }
    v.lens_a = aperture;
    v.lens_f = focus_distance;
    ctx->epoch++;
    return RT_OK;
}

int rt_set_raygen(rt_ctx *ctx, int w, int h, double px, double y0, double dy, double z0, double dz)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!rt_geo_frame_ok(w, h)) return fail(ctx, RT_ERR_BAD_ARG, "frame size out of range (1 <= w <= 2^31 - 8, 1 <= h <= 2^29 - 32, w*h <= 2^31)");
    rt::View &v = ctx->view;
    {
        const double now[5] = {px, y0, dy, z0, dz}, was[5] = {v.px, v.y0, v.dy, v.z0, v.dz};
        if (v.have_grid && !v.explicit_grid && v.w == w && v.h == h && std::memcmp(now, was, sizeof now) == 0)
            return RT_OK;                                       // unchanged: keep the measured dispatch order
    }
    v.w = w; v.h = h; v.px = px; v.y0 = y0; v.dy = dy; v.z0 = z0; v.dz = dz;
    v.explicit_grid = false;
    v.have_grid = true;
    ctx->epoch++;
    return RT_OK;
}

int rt_set_pixel_loc(rt_ctx *ctx, const double *pixel_loc, int w, int h)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!pixel_loc) return fail(ctx, RT_ERR_BAD_ARG, "pixel_loc is NULL");
    if (!rt_geo_frame_ok(w, h)) return fail(ctx, RT_ERR_BAD_ARG, "frame size out of range (1 <= w <= 2^31 - 8, 1 <= h <= 2^29 - 32, w*h <= 2^31)");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)3 * w * h * sizeof(double);
    // one buffer, read by every launch of an explicit grid on any stream: nothing may be in flight while it is rewritten
    if (ctx->pixel_loc.p) RT_HIP(ctx, hipDeviceSynchronize());
    int rc = ensure(ctx, ctx->pixel_loc, bytes);
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipMemcpyAsync(ctx->pixel_loc.p, pixel_loc, bytes, hipMemcpyHostToDevice, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->view.w = w; ctx->view.h = h;
    ctx->view.explicit_grid = true;
    ctx->view.have_grid = true;
    ctx->epoch++;
    return RT_OK;
}

int rt_render_device(rt_ctx *ctx, const rt_params *params, int x0, int x1, void *d_u8, void *d_f32, int64_t plane_stride, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    int rc = check_params(ctx, params, x0, x1);
    if (rc == RT_OK) rc = refuse(ctx, rt::check_device_outputs(ctx->view, params, x0, x1, 1, d_u8, d_f32, plane_stride, 0));
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    return launch(ctx, params, x0, x1, d_u8, d_f32, plane_stride, stream_of(ctx, stream));
}

int rt_render_sequence(rt_ctx *ctx, const rt_params *params, int x0, int x1, int n, void *d_u8, void *d_f32, int64_t plane_stride,
                       int64_t frame_stride, const double *cameras, void *const *streams, int n_streams, int frames_per_launch)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n < 0) return fail(ctx, RT_ERR_BAD_ARG, "rt_render_sequence: negative frame count");
    if (n == 0) return RT_OK;
    if (cameras) {                                            // check_params wants a camera: the first frame's
        int rc0 = rt_set_camera(ctx, cameras, cameras + 3);
        if (rc0 != RT_OK) return rc0;
    }
    int rc = check_params(ctx, params, x0, x1);
    if (rc == RT_OK) rc = refuse(ctx, rt::check_device_outputs(ctx->view, params, x0, x1, n, d_u8, d_f32, plane_stride, frame_stride));
    if (rc != RT_OK) return rc;
    if (n_streams < 0 || (n_streams > 0 && !streams)) return fail(ctx, RT_ERR_BAD_ARG, "rt_render_sequence: n_streams without a stream array");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    auto stream_of = [&](int i) { return (n_streams > 0 && streams[i % n_streams]) ? (hipStream_t)streams[i % n_streams] : ctx->stream; };
    uint8_t *u8 = (uint8_t *)d_u8;
    float *f32 = (float *)d_f32;
    if (cameras) {                                            // an animation: one launch per frame, each with its own camera
        for (int i = 0; i < n; ++i) {
            rc = rt_set_camera(ctx, cameras + 12 * (size_t)i, cameras + 12 * (size_t)i + 3);
            if (rc == RT_OK) rc = launch(ctx, params, x0, x1, u8 ? u8 + (size_t)i * frame_stride : nullptr,
                                         f32 ? f32 + (size_t)i * frame_stride : nullptr, plane_stride, stream_of(i));
            if (rc != RT_OK) return rc;
        }
        return RT_OK;
    }
    const int fpl = frames_per_launch > 0 ? frames_per_launch : 8;
    for (int i = 0, g = 0; i < n; i += fpl, ++g) {
        const int nf = std::min(fpl, n - i);
        rc = launch(ctx, params, x0, x1, u8 ? u8 + (size_t)i * frame_stride : nullptr, f32 ? f32 + (size_t)i * frame_stride : nullptr,
                    plane_stride, stream_of(g), nf, frame_stride);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

// The film: `passes` frames of the unchanged render path (launch(), float32 output, seed + i) into the stream's scratch, a batch of
// them (rt_film_launch.h: film_batch) folded into the float64 sum by one add kernel (with d_sq: into the sum and the sum of squares by
// one add2 kernel).  Everything is queued on `stream`: a batch's renders write the scratch only after the add kernel before them has
// read it.  The arguments have been checked by the entry point.
static int film_queue_passes(rt_ctx *ctx, const rt_params *params, int x0, int x1, int passes, int reset, void *d_sum, int64_t sum_stride,
                             void *d_sq, int64_t sq_stride, void *stream)
{
    int rc = RT_OK;
    const long long npx = (long long)(x1 - x0) * ctx->view.h;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream_of(ctx, stream);
    rt_params p = *params;
    p.flags &= ~(RT_FLAG_U8_RGB | RT_FLAG_U8_HWC);
    const rt::FilmBatch fb = rt::film_batch(npx, passes);
    StreamRecord *sr = nullptr;
    rc = stream_record(ctx, st, &sr);
    if (rc != RT_OK) return rc;
    Buf &scratch = sr->buf[rt::BUF_FILM];
    rc = stream_buffer(ctx, scratch, st, fb.batch * fb.pass_bytes, rt::growth(scratch.cap, fb.batch * fb.pass_bytes).sync);
    if (rc != RT_OK) return rc;
    float *const frames = (float *)scratch.p;
    const dim3 grid(rt::film_grid((npx + 3) >> 2, ctx->cu_count, 3), 3);
    for (int i = 0; i < passes; i += fb.batch) {
        const int nb = std::min(fb.batch, passes - i), first = (reset && i == 0) ? 1 : 0;
        for (int b = 0; b < nb; ++b) {
            p.seed = params->seed + (uint32_t)(i + b);
            rc = launch(ctx, &p, x0, x1, nullptr, frames + (size_t)b * 3 * fb.fplane, fb.fplane, st);
            if (rc != RT_OK) return rc;
        }
        if (d_sq) hipLaunchKernelGGL(rt::film_add2_kernel, grid, dim3(rt::FILM_THREADS), 0, st,
                                     rt::film_add2_args(d_sum, sum_stride, d_sq, sq_stride, frames, fb.fplane, npx, nb, first));
        else hipLaunchKernelGGL(rt::film_add_kernel, grid, dim3(rt::FILM_THREADS), 0, st, rt::film_add_args(d_sum, sum_stride, frames, fb.fplane, npx, nb, first));
        RT_HIP(ctx, hipGetLastError());
    }
    return RT_OK;
}

int rt_film_accumulate(rt_ctx *ctx, const rt_params *params, int x0, int x1, int passes, int reset, void *d_sum, int64_t sum_stride,
                       void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    int rc = refuse(ctx, rt::check_film_accumulate("rt_film_accumulate", ctx->have_scene, ctx->view, ctx->lay, params, x0, x1, passes, d_sum, sum_stride,
                                                   false, nullptr, 0));
    if (rc != RT_OK) return rc;
    return film_queue_passes(ctx, params, x0, x1, passes, reset, d_sum, sum_stride, nullptr, 0, stream);
}

// rt_film_accumulate with the sum of squares beside the sum (rt_film.h: film_add2_kernel): the same passes, seeds, scratch and batches.
int rt_film_accumulate_moments(rt_ctx *ctx, const rt_params *params, int x0, int x1, int passes, int reset, void *d_sum, int64_t sum_stride,
                               void *d_sq, int64_t sq_stride, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    int rc = refuse(ctx, rt::check_film_accumulate("rt_film_accumulate_moments", ctx->have_scene, ctx->view, ctx->lay, params, x0, x1, passes, d_sum,
                                                   sum_stride, true, d_sq, sq_stride));
    if (rc != RT_OK) return rc;
    return film_queue_passes(ctx, params, x0, x1, passes, reset, d_sum, sum_stride, d_sq, sq_stride, stream);
}

int rt_film_resolve(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, const rt_film_tone *tone,
                    void *d_u8, void *d_f32, int64_t out_stride, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    int rc = refuse(ctx, rt::check_film_resolve(d_sum, sum_stride, ws, h, n, tone, d_u8, d_f32, out_stride));
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const rt::FilmResolveArgs a = rt::film_resolve_args(d_sum, sum_stride, ws, h, n, tone, d_u8, d_f32, out_stride);
    hipLaunchKernelGGL(rt::film_resolve_kernel, dim3(rt::film_grid((a.npx + 3) >> 2, ctx->cu_count, 1)), dim3(rt::FILM_THREADS), 0,
                       stream_of(ctx, stream), a);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

// The first-hit guides: one launch of the guides kernel (rt_guides.h) per dispatch the slab needs, in plain tile order.  Scene,
// camera and grid travel by value as in a render launch (rt_launch.h: frame_part); the cull tables are the stream's own
// (acquire_tables), built for rays that start at the camera and go no further than the first hit: no lens, depth 0.
static int guides_launch(rt_ctx *ctx, const rt::View &v, int x0, int x1, void *d_guides, int64_t plane_stride, void *stream)
{
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream_of(ctx, stream);
    StreamRecord *sr = nullptr;
    int rc = stream_record(ctx, st, &sr);
    if (rc != RT_OK) return rc;
    rt::KParams k;
    rt::guides_part(k, v, ctx->lay, (const double *)ctx->scene[ctx->scene_cur].p, (const double *)ctx->pixel_loc.p,
                    (const float *)ctx->texels[ctx->scene_cur].p, ctx->lanes_primary, x0, x1, d_guides, plane_stride);
    const rt::GuidesPlan plan = rt::plan_guides(ctx->lay, ctx->knobs, k.anchors);
    if (ctx->log_kernels) std::fprintf(stderr, "mi355rt: guides_kernel<%d>\n", plan.mode);
    rc = acquire_tables(ctx, *sr, k, &k.ftab);
    if (rc != RT_OK) return rc;
    const void *fn = plan.mode == 2 ? (const void *)rt::guides_kernel<2> : (plan.mode == 1 ? (const void *)rt::guides_kernel<1> : (const void *)rt::guides_kernel<0>);
    const void *const all[] = {(const void *)rt::guides_kernel<0>, (const void *)rt::guides_kernel<1>, (const void *)rt::guides_kernel<2>};
    rc = raise_lds(ctx, all, 3, plan.lds, ctx->guides_lds_set);
    if (rc != RT_OK) return rc;
    rt::div_magic((unsigned)k.tiles_y, k.tiles_y_magic, k.tiles_y_shift);
    // at most RT_GEO_MAX_ITEMS work-items per dispatch: a slab beyond that goes out as narrower column slabs
    const rt_geo_plan g = rt_geo_plan_of(x0, x1, v.h, rt::GUIDE_WPW, 1);
    for (long long s = 0; s < g.nslabs; ++s) {
        rt::KParams ks = rt::slab_params(k, g, s);
        int tex = ctx->lay.T > 0 ? 1 : 0;
        void *args[] = {(void *)&ks, (void *)&tex};
        const unsigned blocks = (unsigned)((ks.ntiles + rt::GUIDE_WPW - 1) / rt::GUIDE_WPW);
        RT_HIP(ctx, hipLaunchKernel(fn, dim3(blocks), dim3(64 * rt::GUIDE_WPW), args, plan.lds, st));
    }
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

int rt_render_guides(rt_ctx *ctx, int x0, int x1, void *d_guides, int64_t plane_stride, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!d_guides) return fail(ctx, RT_ERR_BAD_ARG, "rt_render_guides: d_guides is NULL");
    const rt::View &v = ctx->view;
    int rc = refuse(ctx, rt::check_state(ctx->have_scene, v));
    if (rc == RT_OK) rc = refuse(ctx, rt::check_columns(v, x0, x1));
    if (rc != RT_OK) return rc;
    if (plane_stride < (int64_t)(x1 - x0) * v.h) return fail(ctx, RT_ERR_BAD_ARG, "rt_render_guides: plane_stride smaller than the slab");
    return guides_launch(ctx, v, x0, x1, d_guides, plane_stride, stream);
}

// rt_render_guides on the grid of the call: a copy of the view with that grid goes through the same launch routine; ctx->view and
// the epoch stay, so the render launches keep their measured dispatch orders.
int rt_render_guides_grid(rt_ctx *ctx, int w, int h, double px, double y0, double dy, double z0, double dz, int x0, int x1, void *d_guides,
                          int64_t plane_stride, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    int rc = refuse(ctx, rt::check_guides_grid(ctx->have_scene, ctx->view.have_cam, w, h, x0, x1, d_guides, plane_stride));
    if (rc != RT_OK) return rc;
    return guides_launch(ctx, rt::guides_grid_view(ctx->view, w, h, px, y0, dy, z0, dz), x0, x1, d_guides, plane_stride, stream);
}

// The film's filter: one launch of the denoise kernel (rt_denoise.h) per level, ping-pong between d_out and d_work so that the last
// level writes d_out (rt_film_launch.h: film_write); levels == 0 is one launch that writes the mean.
int rt_film_denoise(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, const void *d_guides, int64_t guide_stride,
                    const rt_denoise *dn, void *d_out, int64_t out_stride, void *d_work, int64_t work_stride, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    int nsq = -1;
    int rc = refuse(ctx, rt::check_film_denoise(d_sum, sum_stride, ws, h, n, d_guides, guide_stride, dn, d_out, out_stride, d_work, work_stride, nsq));
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream_of(ctx, stream);
    const rt::FilmPingPong pp = {d_out, out_stride, d_work, work_stride};
    const dim3 grid(rt::denoise_grid((long long)ws * h, ctx->cu_count));
    for (int i = 0; i < (dn->levels ? dn->levels : 1); ++i) {
        const rt::FilmWrite w = rt::film_write(false, dn->levels, i, d_sum, sum_stride, pp);
        hipLaunchKernelGGL(rt::denoise_kernel, grid, dim3(rt::DENOISE_THREADS), 0, st, rt::denoise_args(w, d_guides, guide_stride, ws, h, n, dn, nsq, i));
        RT_HIP(ctx, hipGetLastError());
    }
    return RT_OK;
}

// The variance-guided filter: a prepare launch (rt_denoise_var.h: the mean and the variance of the mean from sum and sum of squares)
// and one launch per level; levels == 0 is the prepare launch alone, without demodulation.
int rt_film_denoise_variance(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, const void *d_sq, int64_t sq_stride, int ws, int h, int64_t n,
                             const void *d_guides, int64_t guide_stride, const rt_denoise_variance *dv, void *d_out, int64_t out_stride,
                             void *d_work, int64_t work_stride, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    int nsq = -1;
    int rc = refuse(ctx, rt::check_film_denoise_variance(d_sum, sum_stride, d_sq, sq_stride, ws, h, n, d_guides, guide_stride, dv, d_out, out_stride,
                                                         d_work, work_stride, nsq));
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream_of(ctx, stream);
    rt::DenoiseVarArgs a = rt::denoise_var_common(d_guides, guide_stride, ws, h, dv, nsq);
    rt::denoise_var_inputs(a, d_sum, sum_stride, d_sq, sq_stride, n, dv->levels);
    return variance_filter(ctx, a, dv->levels, {d_out, out_stride, d_work, work_stride}, st, [&](const rt::FilmWrite &w, dim3 grid) {
        hipLaunchKernelGGL(rt::denoise_var_prepare_kernel, grid, dim3(rt::DENOISE_THREADS), 0, st, rt::denoise_var_write(a, w, dv->levels, 0));
    });
}

// The film through a camera move: one launch of the temporal kernel (rt_temporal.h) over the full frame of the current camera and
// closed-form grid, which travel by value with the previous camera.
int rt_film_temporal(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, int64_t n, const void *d_guides, int64_t guide_stride,
                     const void *d_hist, int64_t hist_stride, const void *d_hist_len, const void *d_hist_guides, int64_t hist_guide_stride,
                     const rt_temporal *tp, void *d_out, int64_t out_stride, void *d_out_len, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    const rt::View &v = ctx->view;
    int rc = refuse(ctx, rt::check_film_temporal("rt_film_temporal", v, d_sum, sum_stride, n, d_guides, guide_stride, d_hist, hist_stride, d_hist_len,
                                                 d_hist_guides, hist_guide_stride, tp, d_out, out_stride, d_out_len));
    if (rc != RT_OK) return rc;
    rt::TemporalArgs a;
    rt::temporal_args(a, v, d_sum, sum_stride, n, d_guides, guide_stride, d_hist, hist_stride, d_hist_len, d_hist_guides, hist_guide_stride, tp, d_out,
                      out_stride, d_out_len);
    return temporal_launch(ctx, rt::temporal_kernel, a, stream);
}

// rt_film_temporal with the second moment beside the mean: one launch of temporal_moments_kernel (rt_temporal.h).
int rt_film_temporal_moments(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, const void *d_sq, int64_t sq_stride, int64_t n,
                             const void *d_guides, int64_t guide_stride, const void *d_hist, int64_t hist_stride, const void *d_hist_sq,
                             int64_t hist_sq_stride, const void *d_hist_len, const void *d_hist_guides, int64_t hist_guide_stride,
                             const rt_temporal *tp, void *d_out, int64_t out_stride, void *d_out_sq, int64_t out_sq_stride, void *d_out_len,
                             void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    const rt::View &v = ctx->view;
    int rc = refuse(ctx, rt::check_film_temporal_moments(v, d_sum, sum_stride, d_sq, sq_stride, n, d_guides, guide_stride, d_hist, hist_stride, d_hist_sq,
                                                         hist_sq_stride, d_hist_len, d_hist_guides, hist_guide_stride, tp, d_out, out_stride, d_out_sq,
                                                         out_sq_stride, d_out_len));
    if (rc != RT_OK) return rc;
    rt::TemporalMomentsArgs m;
    rt::temporal_args(m.t, v, d_sum, sum_stride, n, d_guides, guide_stride, d_hist, hist_stride, d_hist_len, d_hist_guides, hist_guide_stride, tp, d_out,
                      out_stride, d_out_len);
    rt::temporal_moments_args(m, d_sq, sq_stride, d_hist_sq, hist_sq_stride, d_out_sq, out_sq_stride);
    return temporal_launch(ctx, rt::temporal_moments_kernel, m, stream);
}

// The variance-guided filter on a temporal mean: the prepare launch takes each pixel's variance from its own moments or, where its
// history is shorter than spatial_below, from its object's neighbours (rt_denoise_var.h: denoise_var_prepare_len_kernel); the levels
// are rt_film_denoise_variance's.
int rt_film_denoise_variance_temporal(rt_ctx *ctx, const void *d_mean, int64_t mean_stride, const void *d_msq, int64_t msq_stride,
                                      const void *d_len, int ws, int h, const void *d_guides, int64_t guide_stride,
                                      const rt_denoise_variance *dv, double spatial_below, void *d_out, int64_t out_stride, void *d_work,
                                      int64_t work_stride, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    int nsq = -1;
    int rc = refuse(ctx, rt::check_film_denoise_variance_temporal(d_mean, mean_stride, d_msq, msq_stride, d_len, ws, h, d_guides, guide_stride, dv,
                                                                  spatial_below, d_out, out_stride, d_work, work_stride, nsq));
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream_of(ctx, stream);
    return variance_filter(ctx, rt::denoise_var_common(d_guides, guide_stride, ws, h, dv, nsq), dv->levels, {d_out, out_stride, d_work, work_stride}, st,
                           [&](const rt::FilmWrite &w, dim3 grid) {
        hipLaunchKernelGGL(rt::denoise_var_prepare_len_kernel, grid, dim3(rt::DENOISE_THREADS), 0, st,
                           rt::denoise_var_len_args(w, d_mean, mean_stride, d_msq, msq_stride, d_len, ws, h, d_guides, guide_stride, dv, spatial_below));
    });
}

// Bloom: the launches of rt_bloom.h's plan, one after the other on the stream: the bright pass, then per level two gather kernels or
// one tile kernel (bloom_plan says which, and which work planes each reads and writes).
int rt_film_bloom(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, const rt_bloom *bl, void *d_out,
                  int64_t out_stride, void *d_work, int64_t work_stride, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    int rc = refuse(ctx, rt::check_film_bloom(d_sum, sum_stride, ws, h, n, bl, d_out, out_stride, d_work, work_stride));
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream_of(ctx, stream);
    const rt::BloomPlan plan = rt::bloom_plan(bl->levels, bl->flags);
    const dim3 grid(rt::bloom_grid((long long)ws * h, ctx->cu_count)), tiles(rt::bloom_tile_blocks(ws, h), 3), threads(rt::BLOOM_THREADS);
    for (int k = 0; k < plan.count; ++k) {
        const rt::BloomLaunch &l = plan.l[k];
        const rt::BloomArgs a = rt::bloom_args(l, d_sum, sum_stride, ws, h, n, bl, d_out, out_stride, d_work, work_stride);
        if (l.kind == rt::BLOOM_BRIGHT) hipLaunchKernelGGL(rt::bloom_bright_kernel, grid, threads, 0, st, a);
        else if (l.kind == rt::BLOOM_X) hipLaunchKernelGGL(rt::bloom_x_kernel, grid, threads, 0, st, a);
        else if (l.kind == rt::BLOOM_Y) hipLaunchKernelGGL(rt::bloom_y_kernel, grid, threads, 0, st, a);
        else if (l.step == 1) hipLaunchKernelGGL(rt::bloom_tile_kernel<1>, tiles, threads, 0, st, a);
        else if (l.step == 2) hipLaunchKernelGGL(rt::bloom_tile_kernel<2>, tiles, threads, 0, st, a);
        else hipLaunchKernelGGL(rt::bloom_tile_kernel<4>, tiles, threads, 0, st, a);
        RT_HIP(ctx, hipGetLastError());
    }
    return RT_OK;
}

// Metering (rt_meter.h): the histogram of the film's luminance, the exposure solved from it, and the resolve that multiplies it in.
// Three launches on the caller's stream; nothing is allocated and nothing waits for the device.
int rt_film_meter(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, int reset, void *d_hist, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    int rc = refuse(ctx, rt::check_film_meter(d_sum, sum_stride, ws, h, n, d_hist));
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream_of(ctx, stream);
    const rt::MeterHistArgs a = rt::meter_hist_args(d_sum, sum_stride, ws, h, n, d_hist);
    if (reset) hipLaunchKernelGGL(rt::meter_clear_kernel, dim3(1), dim3(rt::METER_THREADS), 0, st, a.hist);
    hipLaunchKernelGGL(rt::meter_hist_kernel, dim3(rt::meter_grid((a.npx + 3) >> 2, ctx->cu_count)), dim3(rt::METER_THREADS), 0, st, a);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

// Guided upsampling: one launch of the upsample kernel (rt_upsample.h) over the output frame; both grids travel by value.
int rt_film_upsample(rt_ctx *ctx, const void *d_lo, int64_t lo_stride, int wl, int hl, int64_t n, const void *d_lo_guides, int64_t lo_guide_stride,
                     const void *d_hi_guides, int64_t hi_guide_stride, int w, int h, const rt_upsample *up, void *d_out, int64_t out_stride,
                     void *d_out_kind, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    int rc = refuse(ctx, rt::check_film_upsample(d_lo, lo_stride, wl, hl, n, d_lo_guides, lo_guide_stride, d_hi_guides, hi_guide_stride, w, h, up,
                                                 d_out, out_stride, d_out_kind));
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    rt::UpsampleArgs a;
    rt::upsample_args(a, d_lo, lo_stride, wl, hl, n, d_lo_guides, lo_guide_stride, d_hi_guides, hi_guide_stride, w, h, up, d_out, out_stride,
                      d_out_kind);
    hipLaunchKernelGGL(rt::upsample_kernel, dim3(rt::upsample_grid((long long)w * h, ctx->cu_count)), dim3(rt::UPSAMPLE_THREADS), 0,
                       stream_of(ctx, stream), a);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

int rt_film_meter_solve(rt_ctx *ctx, const void *d_hist, const rt_meter *mt, void *d_state, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    int rc = refuse(ctx, rt::check_film_meter_solve(d_hist, mt, d_state));
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(rt::meter_solve_kernel, dim3(1), dim3(rt::METER_SOLVE_THREADS), 0, stream_of(ctx, stream),
                       (const unsigned long long *)d_hist, *mt, (double *)d_state);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

int rt_film_resolve_metered(rt_ctx *ctx, const void *d_sum, int64_t sum_stride, int ws, int h, int64_t n, const rt_film_tone *tone,
                            const void *d_state, void *d_u8, void *d_f32, int64_t out_stride, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    int rc = refuse(ctx, rt::check_film_resolve_metered(d_sum, sum_stride, ws, h, n, tone, d_state, d_u8, d_f32, out_stride));
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const rt::FilmResolveArgs a = rt::film_resolve_args(d_sum, sum_stride, ws, h, n, tone, d_u8, d_f32, out_stride);
    hipLaunchKernelGGL(rt::film_resolve_metered_kernel, dim3(rt::film_grid((a.npx + 3) >> 2, ctx->cu_count, 1)), dim3(rt::FILM_THREADS), 0,
                       stream_of(ctx, stream), a, (const double *)d_state);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

// The staging planes grown where the frame is larger than any before, one launch into them and one copy per output to host memory,
// all queued on `stream`.
static int render_staged(rt_ctx *ctx, const rt_params *params, int x0, int x1, uint8_t *out_u8, float *out_f32, Buf &u8, Buf &f32,
                         hipStream_t stream)
{
    const size_t npx = (size_t)(x1 - x0) * ctx->view.h;
    int rc = out_u8 ? ensure(ctx, u8, 3 * npx) : RT_OK;
    if (rc == RT_OK && out_f32) rc = ensure(ctx, f32, 3 * npx * sizeof(float));
    if (rc == RT_OK)
        rc = launch(ctx, params, x0, x1, out_u8 ? u8.p : nullptr, out_f32 ? f32.p : nullptr,
                    (params->flags & RT_FLAG_U8_HWC) ? (int64_t)(x1 - x0) : (int64_t)npx, stream);
    if (rc != RT_OK) return rc;
    if (out_u8) RT_HIP(ctx, hipMemcpyAsync(out_u8, u8.p, 3 * npx, hipMemcpyDeviceToHost, stream));
    if (out_f32) RT_HIP(ctx, hipMemcpyAsync(out_f32, f32.p, 3 * npx * sizeof(float), hipMemcpyDeviceToHost, stream));
    return RT_OK;
}

int rt_render(rt_ctx *ctx, const rt_params *params, int x0, int x1, uint8_t *out_u8, float *out_f32)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    int rc = check_params(ctx, params, x0, x1);
    if (rc != RT_OK) return rc;
    if (!out_u8 && !out_f32) return fail(ctx, RT_ERR_BAD_ARG, "both output pointers are NULL");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npx = (size_t)(x1 - x0) * ctx->view.h;
    if (out_u8 && (rc = ensure(ctx, ctx->u8, 3 * npx)) != RT_OK) return rc;      // (the chunks below need the staging planes too)
    if (out_f32 && (rc = ensure(ctx, ctx->f32, 3 * npx * sizeof(float))) != RT_OK) return rc;
    if ((rc = refuse(ctx, rt::check_host_hwc(params, out_f32))) != RT_OK) return rc;
    const bool hwc = (params->flags & RT_FLAG_U8_HWC) != 0;
    // Large planar frames are rendered in RT_RENDER_CHUNKS column chunks, alternately on two streams (consecutive
    // launches overlap), and every chunk's planes start their way to the host (third stream, behind an
    // event) while the following chunks still render: the copy of a 1080p frame costs about as much as rendering it,
    // and this hides all of it but the last chunk's.  (main.py:41-51: launch, then copy_to_host.)
    const long long tiles = rt_geo_tiles(x1 - x0);
    const int NCH = ctx->render_chunks;
    if (hwc || NCH < 2 || npx < (1u << 19) || tiles < 4 * NCH) {
        rc = render_staged(ctx, params, x0, x1, out_u8, out_f32, ctx->u8, ctx->f32, ctx->stream);
        if (rc != RT_OK) return rc;
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return RT_OK;
    }
    // Page-locked destinations (rt_host_alloc): every chunk on its own stream (descending priority) with its copy queued
    // behind it in the same stream — no cross-stream event between kernel and copy (measured 0.213 ms per 1080p uint8
    // frame against 0.222).  Pageable destinations: the runtime stages those copies on the calling thread, so the
    // chunks alternate on two streams and the copies wait on a third behind events (0.23 ms; in-stream: 0.37).
    // MI355RT_CHUNK_MODE=0/1 forces one scheme.
    bool instream = false;
    {
        hipPointerAttribute_t at;
        void *probe = out_u8 ? (void *)out_u8 : (void *)out_f32;
        if (hipPointerGetAttributes(&at, probe) == hipSuccess) instream = (at.type == hipMemoryTypeHost);
        else (void)hipGetLastError();                           // plain malloc memory: "invalid value", not an error here
        if (ctx->chunk_mode >= 0) instream = ctx->chunk_mode == 1;
    }
    if (!ctx->pipe) {                                          // (a set-up that fails half-way is released here, and tried again by the next call)
        std::unique_ptr<rt_ctx::Pipeline> pl(new (std::nothrow) rt_ctx::Pipeline);
        if (!pl) return fail(ctx, RT_ERR_ALLOC, "out of host memory");
        RT_HIP(ctx, hipStreamCreateWithFlags(&pl->stream2, hipStreamNonBlocking));
        RT_HIP(ctx, hipStreamCreateWithFlags(&pl->copy_stream, hipStreamNonBlocking));
        for (auto &e : pl->chunk_ev) RT_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        int lo = 0, hi = 0;
        RT_HIP(ctx, hipDeviceGetStreamPriorityRange(&lo, &hi));   // lo = least urgent (numerically largest)
        for (int c = 0; c < RT_RENDER_CHUNKS; ++c)
            RT_HIP(ctx, hipStreamCreateWithPriority(&pl->chunk_stream[c], hipStreamNonBlocking, std::min(lo, hi + c)));
        ctx->pipe = std::move(pl);
    }
    rt_ctx::Pipeline &pl = *ctx->pipe;
    int cx[RT_RENDER_CHUNKS + 1];
    // the first and the last chunk are half as wide as the others: the copies start sooner, and the one copy that
    // nothing overlaps (the last chunk's) is short
    for (int c = 0; c <= NCH; ++c) cx[c] = (int)rt_geo_chunk_x(x0, x1, NCH, c);
    // a chunk's three planes = one 2-D copy (3 rows, pitch = plane) while the pitch stays within RT_GEO_MAX_PITCH, else
    // three copies, plane by plane
    auto copy_chunk = [&](size_t off, size_t n, hipStream_t s) -> int {
        if (out_u8) {
            if (rt_geo_copy_2d((long long)npx, 1))
                RT_HIP(ctx, hipMemcpy2DAsync(out_u8 + off, npx, (uint8_t *)ctx->u8.p + off, npx, n, 3, hipMemcpyDeviceToHost, s));
            else
                for (size_t c = 0; c < 3; ++c)
                    RT_HIP(ctx, hipMemcpyAsync(out_u8 + c * npx + off, (uint8_t *)ctx->u8.p + c * npx + off, n, hipMemcpyDeviceToHost, s));
        }
        if (out_f32) {
            if (rt_geo_copy_2d((long long)npx, sizeof(float)))
                RT_HIP(ctx, hipMemcpy2DAsync(out_f32 + off, npx * sizeof(float), (float *)ctx->f32.p + off, npx * sizeof(float),
                                             n * sizeof(float), 3, hipMemcpyDeviceToHost, s));
            else
                for (size_t c = 0; c < 3; ++c)
                    RT_HIP(ctx, hipMemcpyAsync(out_f32 + c * npx + off, (float *)ctx->f32.p + c * npx + off, n * sizeof(float),
                                               hipMemcpyDeviceToHost, s));
        }
        return RT_OK;
    };
    unsigned *const tile_stats = ctx->tile_stats;
    const int tiles_y = (ctx->view.h + rt::TILE - 1) / rt::TILE;
    for (int c = 0; c < NCH; ++c) {
        hipStream_t s = instream ? pl.chunk_stream[c] : ((c & 1) ? pl.stream2 : ctx->stream);
        const size_t off = (size_t)(cx[c] - x0) * ctx->view.h, n = (size_t)(cx[c + 1] - cx[c]) * ctx->view.h;
        // rt_set_tile_stats: a chunk records from its own first tile column on (chunk edges are multiples of the tile size)
        if (tile_stats) ctx->tile_stats = tile_stats + (size_t)((cx[c] - x0) / rt::TILE) * tiles_y;
        rc = launch(ctx, params, cx[c], cx[c + 1], out_u8 ? (uint8_t *)ctx->u8.p + off : nullptr,
                    out_f32 ? (float *)ctx->f32.p + off : nullptr, (int64_t)npx, s);
        ctx->tile_stats = tile_stats;
        if (rc != RT_OK) return rc;
        if (instream) {
            if ((rc = copy_chunk(off, n, s)) != RT_OK) return rc;
        } else RT_HIP(ctx, hipEventRecord(pl.chunk_ev[c], s));
    }
    if (instream) {
        for (int c = 0; c < NCH; ++c) RT_HIP(ctx, hipStreamSynchronize(pl.chunk_stream[c]));
        return RT_OK;
    }
    for (int c = 0; c < NCH; ++c) {
        const size_t off = (size_t)(cx[c] - x0) * ctx->view.h, n = (size_t)(cx[c + 1] - cx[c]) * ctx->view.h;
        RT_HIP(ctx, hipStreamWaitEvent(pl.copy_stream, pl.chunk_ev[c], 0));
        if ((rc = copy_chunk(off, n, pl.copy_stream)) != RT_OK) return rc;
    }
    RT_HIP(ctx, hipStreamSynchronize(pl.copy_stream));
    return RT_OK;
}

int rt_render_begin(rt_ctx *ctx, const rt_params *params, int x0, int x1, uint8_t *out_u8, float *out_f32, int slot)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    int rc = check_params(ctx, params, x0, x1);
    if (rc != RT_OK) return rc;
    if (slot < 0 || slot >= RT_RENDER_SLOTS) return fail(ctx, RT_ERR_BAD_ARG, "rt_render_begin: slot outside 0..RT_RENDER_SLOTS-1");
    if (!out_u8 && !out_f32) return fail(ctx, RT_ERR_BAD_ARG, "both output pointers are NULL");
    if ((rc = refuse(ctx, rt::check_host_hwc(params, out_f32))) != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    rt_ctx::Slot &sl = ctx->slots[slot];
    if (!sl.stream) RT_HIP(ctx, hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
    // One launch and one copy per output, queued on the slot's stream: the frame before this one in the same slot is
    // ahead of it in that stream (its staging planes are free by the time this launch writes them), the frames of the
    // other slots render and travel beside it.  The staging planes grow on the first frame of a larger size only
    // (hipFree waits for the device).
    return render_staged(ctx, params, x0, x1, out_u8, out_f32, sl.u8, sl.f32, sl.stream);
}

int rt_render_end(rt_ctx *ctx, int slot)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (slot < 0 || slot >= RT_RENDER_SLOTS) return fail(ctx, RT_ERR_BAD_ARG, "rt_render_end: slot outside 0..RT_RENDER_SLOTS-1");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->slots[slot].stream) RT_HIP(ctx, hipStreamSynchronize(ctx->slots[slot].stream));
    return RT_OK;
}

int rt_host_alloc(rt_ctx *ctx, size_t bytes, void **hptr)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!hptr || bytes == 0) return fail(ctx, RT_ERR_BAD_ARG, "rt_host_alloc: NULL out-pointer or zero size");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipHostMalloc(hptr, bytes, hipHostMallocDefault));
    return RT_OK;
}

int rt_host_free(rt_ctx *ctx, void *hptr)
{
    if (!hptr) return RT_OK;
    if (ctx) RT_HIP(ctx, hipSetDevice(ctx->device));           // ctx == NULL: the memory outlived its context (allowed)
    RT_HIP(ctx, hipHostFree(hptr));
    return RT_OK;
}

int rt_malloc(rt_ctx *ctx, size_t bytes, void **dptr)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!dptr || bytes == 0) return fail(ctx, RT_ERR_BAD_ARG, "rt_malloc: NULL out-pointer or zero size");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipMalloc(dptr, bytes));
    return RT_OK;
}

int rt_free(rt_ctx *ctx, void *dptr)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!dptr) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RT_HIP(ctx, hipFree(dptr));
    return RT_OK;
}

int rt_memcpy_h2d(rt_ctx *ctx, void *dst_device, const void *src_host, size_t bytes)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!dst_device || !src_host) return fail(ctx, RT_ERR_BAD_ARG, "rt_memcpy_h2d: NULL pointer");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipMemcpyAsync(dst_device, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_memcpy_d2h(rt_ctx *ctx, void *dst_host, const void *src_device, size_t bytes)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!dst_host || !src_device) return fail(ctx, RT_ERR_BAD_ARG, "rt_memcpy_d2h: NULL pointer");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipMemcpyAsync(dst_host, src_device, bytes, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_sync(rt_ctx *ctx)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_stream_create(rt_ctx *ctx, void **stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!stream) return fail(ctx, RT_ERR_BAD_ARG, "stream out-pointer is NULL");
    *stream = nullptr;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = nullptr;
    RT_HIP(ctx, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void *)s;
    return RT_OK;
}

// The context remembers streams that launched on it (owner / readers of the dispatch order, rt_feedback.h; the stream's record,
// rt_streams.h) so that it can fence them later: drop every reference to `stream` once its queued work is complete.
static int forget_stream(rt_ctx *ctx, hipStream_t stream)
{
    RT_HIP(ctx, hipStreamSynchronize(stream));
    ctx->book.forget(stream);                                   // (its work is complete: nothing of it reads an order any more)
    ctx->streams.forget(stream);                                // (its table sets and scratch buffers go with its record: ~Buf)
    return RT_OK;
}

int rt_stream_destroy(rt_ctx *ctx, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!stream) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    int rc = forget_stream(ctx, (hipStream_t)stream);
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipStreamDestroy((hipStream_t)stream));
    return RT_OK;
}

int rt_stream_forget(rt_ctx *ctx, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!stream) return RT_OK;
    if ((hipStream_t)stream == ctx->stream) return fail(ctx, RT_ERR_BAD_ARG, "rt_stream_forget: the context's own stream");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    return forget_stream(ctx, (hipStream_t)stream);
}

int rt_stream_sync(rt_ctx *ctx, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipStreamSynchronize(stream_of(ctx, stream)));
    return RT_OK;
}

int rt_timer_begin(rt_ctx *ctx, void *stream)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipEventRecord(ctx->ev0, stream_of(ctx, stream)));
    return RT_OK;
}

int rt_timer_end(rt_ctx *ctx, void *stream, float *ms)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!ms) return fail(ctx, RT_ERR_BAD_ARG, "ms is NULL");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipEventRecord(ctx->ev1, stream_of(ctx, stream)));
    RT_HIP(ctx, hipEventSynchronize(ctx->ev1));
    RT_HIP(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return RT_OK;
}

int rt_set_tile_stats(rt_ctx *ctx, void *d_cycles)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    ctx->tile_stats = (unsigned *)d_cycles;
    return RT_OK;
}

int rt_get_stats(rt_ctx *ctx, rt_stats *out)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!out) return fail(ctx, RT_ERR_BAD_ARG, "stats is NULL");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    unsigned long long c[RT_COUNT_WORDS] = {0};
    if (ctx->counts.p) {                                        // counting launches may be in flight on any stream
        RT_HIP(ctx, hipDeviceSynchronize());
        RT_HIP(ctx, hipMemcpy(c, ctx->counts.p, sizeof c, hipMemcpyDeviceToHost));
    }
    *out = ctx->stats;
    out->closest_queries = c[0]; out->shadow_traced = c[1]; out->shadow_skipped = c[2]; out->hits = c[3];
    for (int b = 0; b <= RT_MAX_DEPTH; ++b) { out->bounce_waves[b] = c[4 + 2 * b]; out->bounce_lanes[b] = c[5 + 2 * b]; }
    return RT_OK;
}

int rt_reset_stats(rt_ctx *ctx)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->counts.p) {
        RT_HIP(ctx, hipDeviceSynchronize());
        RT_HIP(ctx, hipMemset(ctx->counts.p, 0, RT_COUNT_WORDS * sizeof(unsigned long long)));
    }
    ctx->stats = rt_stats{};
    return RT_OK;
}

int rt_get_kernel_info(rt_ctx *ctx, rt_kernel_info *info)
{
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!info) return fail(ctx, RT_ERR_BAD_ARG, "info is NULL");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipFuncAttributes a;
    // the headline kernel, in the twin that the current scene's plain launches run (rt_plan.h: twin_of); without a scene the generic one
    constexpr Shape headline{false, true, 2, false, false, 0};
    constexpr rt::Family plain = rt::Family::PLAIN;
    const rt::Twin twin = ctx->have_scene ? rt::twin_of(ctx->lay, ctx->knobs, plain, headline, 0, rt::anchors_of(ctx->lay)) : rt::Twin{false, 0};
    static_assert(rt::has_small_kernel(plain, headline), "the headline shape has a kernel in every row it can be asked for in");
    const void *fn = KERNELS[rt::row_of(plain, twin)][rt::shape_index(headline)];
    RT_HIP(ctx, hipFuncGetAttributes(&a, fn));
    hipDeviceProp_t prop;
    RT_HIP(ctx, hipGetDeviceProperties(&prop, ctx->device));
    std::memset(info, 0, sizeof *info);
    info->vgprs = a.numRegs;
    info->lds_static = (int32_t)a.sharedSizeBytes;
    info->max_threads = a.maxThreadsPerBlock;
    info->wave_size = prop.warpSize;
    info->cu_count = prop.multiProcessorCount;
    info->clock_khz = prop.clockRate;
    return RT_OK;
}

}  // extern "C"
