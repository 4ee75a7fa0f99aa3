/* The library's dispatch-order feedback rules (python-ray-tracer_amd/csrc/rt_feedback.h) without HIP, driven as mi355rt.hip's dispatch()
 * and launch_one() drive them, over a fake runtime; in the replay also the cull-table cache of rt_streams.h, as acquire_tables() drives it.  Built with AddressSanitizer and UndefinedBehaviorSanitizer (leak detection on)
 * and run by tests/test_algorithms.py.
 *
 *   feedback_check replay SCRIPT OUT   runs the step script tests/algo/feedback_trace_cases.py writes (the scene and the cameras, then
 *                                      per context its MI355RT_REMEASURE and its steps), synchronising the launching stream after every
 *                                      launch, and writes one line "measured settled tables_built" (0/1 each) per step to OUT.  The
 *                                      keys come from the scene's layout (rt_scene.h), plan_launch and order_shape (rt_plan.h),
 *                                      rt_geo_plan_of and rt_geo_lattice (rt_geometry.h), as launch() and dispatch() build them; the
 *                                      cull tables' key from the launch's KParams (rt_launch.h: render_part), as launch() fills it.
 *   feedback_check walk [SEED]         a random walk of WALK_STEPS = 100000 steps for each MI355RT_REMEASURE of 0, 2 and 24: 12
 *                                      geometries over the 8 slots, 4 streams; launches with and without feedback, epoch bumps,
 *                                      completion of a prefix of a stream's queue (so a switch comes late, early or never),
 *                                      rt_stream_forget, a device synchronise.  After every step:
 *      (a) when a measurement that writes order[b] of a slot is queued, every launch queued earlier that reads that order[b]
 *          happens-before it on the measuring stream;
 *      (b) a launch reads only a buffer whose order kernel the host has observed complete;
 *      (c) no measurement is queued while the slot's previous one may still run (one cost buffer);
 *      (d) a key is in at most one slot, and a live slot is evicted only behind a device synchronise;
 *      (e) at the end, after release_events, every event ever created has been released exactly once.
 *   It prints how often each transition was taken and fails if one never was.
 *
 * The fake runtime: a stream is a pair of counters (queued, completed); an event is (stream, queued count at its record), complete
 * once the stream has completed that far, and lives on the heap, so that a lost or twice-released one is a sanitizer report.
 * Happens-before is a vector clock per stream, advanced by same-stream order, by "stream waits event", by an event or a stream
 * the host has observed complete, and by a device synchronise. */
#include "../../python-ray-tracer_amd/csrc/rt_feedback.h"
#include "../../python-ray-tracer_amd/csrc/rt_launch.h"
#include "../../python-ray-tracer_amd/csrc/rt_plan.h"
#include "../../python-ray-tracer_amd/csrc/rt_streams.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "step %ld: ", g_step); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

static long g_step = 0;
static const int WALK_STEPS = 100000;

typedef std::vector<long> Clock;                      /* per stream: how many of its operations happen-before */
static void join(Clock &a, const Clock &b) { for (size_t i = 0; i < a.size(); ++i) if (b[i] > a[i]) a[i] = b[i]; }

struct Stream {
    int id = 0;
    long queued = 0, completed = 0;
    Clock clock;                                      /* what happens-before the next operation queued here */
    std::vector<Clock> deps;                          /* deps[i]: what operation i + 1 waits for */
};

struct Event {
    int stream = -1;                                  /* -1: never recorded (complete, and waiting for it waits for nothing) */
    long at = 0;
    Clock clock;
};

struct Fake {
    std::vector<Stream> streams;
    Clock host;                                       /* what the host has observed complete */
    std::set<Event *> events;
    long created = 0, released = 0;

    explicit Fake(int n) : streams((size_t)n), host((size_t)n, 0)
    {
        for (int i = 0; i < n; ++i) { streams[(size_t)i].id = i; streams[(size_t)i].clock.assign((size_t)n, 0); }
    }
    Stream &of(void *h) { return *(Stream *)h; }
    void *handle(int i) { return &streams[(size_t)i]; }

    long queue(Stream &s)                             /* an operation goes into the stream's queue */
    {
        join(s.clock, host);                          /* (what the host has seen complete is before anything queued later) */
        s.deps.push_back(s.clock);
        s.clock[(size_t)s.id] = ++s.queued;
        return s.queued;
    }
    bool before(const Stream &s, int t, long op) const   /* operation `op` of stream t happens-before the next one queued on s */
    {
        return std::max(s.clock[(size_t)t], host[(size_t)t]) >= op;
    }
    Event *create() { Event *e = new Event; events.insert(e); ++created; return e; }
    void release(Event *e)
    {
        CHECK(events.erase(e) == 1, "an event released twice, or one the runtime never made");
        ++released;
        delete e;
    }
    void record(Event *e, Stream &s)
    {
        CHECK(events.count(e) == 1, "record of a released event");
        e->stream = s.id; e->at = s.queued; e->clock = s.clock; join(e->clock, host);
    }
    void wait(Stream &s, Event *e)
    {
        CHECK(events.count(e) == 1, "wait for a released event");
        if (e->stream >= 0) join(s.clock, e->clock);
    }
    bool query(Event *e)                              /* hipEventQuery: a complete event is observed by the host */
    {
        CHECK(events.count(e) == 1, "query of a released event");
        if (e->stream >= 0 && streams[(size_t)e->stream].completed < e->at) return false;
        if (e->stream >= 0) join(host, e->clock);
        return true;
    }
    void finish(Stream &s, long upto)                 /* the device completes the stream's operations up to `upto`, and what they wait for */
    {
        while (s.completed < upto) {
            const Clock &d = s.deps[(size_t)s.completed];
            for (size_t t = 0; t < streams.size(); ++t)
                if ((int)t != s.id && streams[t].completed < d[t]) finish(streams[t], d[t]);
            ++s.completed;
        }
    }
    void sync(Stream &s)                              /* hipStreamSynchronize */
    {
        finish(s, s.queued);
        join(host, s.clock);
    }
    void sync_device()
    {
        for (Stream &s : streams) sync(s);
    }
    bool idle() const
    {
        for (const Stream &s : streams) if (s.completed != s.queued || host[(size_t)s.id] != s.queued) return false;
        return true;
    }
};

/* One context as mi355rt.hip keeps it, and what the checks remember about its slots' device buffers. */
struct Op { int stream; long op; };
struct Context {
    Fake &fk;
    rt::FeedbackSlot slots[RT_FEEDBACK_SLOTS];
    rt::FeedbackBook book;
    unsigned long long epoch = 1, scene_epoch = 1;
    int remeasure;
    struct TableBuf { size_t cap = 0; };              /* (the replay keeps no device memory: streams_check.cpp does) */
    rt::StreamBook<TableBuf> streams;
    std::vector<Op> readers[RT_FEEDBACK_SLOTS][2];    /* launches that read order[b] */
    Op writer[RT_FEEDBACK_SLOTS][2];                  /* the last order kernel that wrote order[b] (op 0: none) */
    Op last_order[RT_FEEDBACK_SLOTS];                 /* the slot's last order kernel: the reader of its cost buffer */
    long switches = 0, fenced = 0, evictions = 0, forgets = 0, measured = 0, settled = 0;

    Context(Fake &f, int rm) : fk(f), remeasure(rm)
    {
        for (int i = 0; i < RT_FEEDBACK_SLOTS; ++i) { book.slot[i] = &slots[i]; forget_buffers(i); }
    }
    void forget_buffers(int i)
    {
        for (int b = 0; b < 2; ++b) { readers[i][b].clear(); writer[i][b] = Op{0, 0}; }
        last_order[i] = Op{0, 0};
    }

    /* dispatch() and launch_one() for one dispatch of one frame; key = nullptr: a launch without feedback */
    rt::FeedbackLaunch launch(void *stream, const rt::FeedbackKey *key)
    {
        Stream &s = fk.of(stream);
        rt::FeedbackSlot *f = nullptr;
        int i = -1;
        if (key) {
            bool live = false;
            i = book.find(*key, &live);
            if (live) { fk.sync_device(); ++evictions; }
            if (!(slots[i].key == *key)) {                                          /* (d) */
                CHECK(!slots[i].key.valid || fk.idle(), "a live slot evicted without a device synchronise");
                forget_buffers(i);
            }
            f = &book.claim(i, *key);
            if (!f->done) f->done = fk.create();
            if (f->building && fk.query((Event *)f->done)) {                        /* switch_order */
                ++switches;
                for (void *us : rt::switch_order(*f)) {
                    Event *ev = (Event *)rt::take_spare(*f);
                    if (!ev) ev = fk.create();
                    fk.record(ev, fk.of(us));
                    rt::add_fence(*f, us, ev);
                }
            }
        }
        const rt::FeedbackLaunch d = f ? rt::decide_launch(*f, stream, epoch, remeasure) : rt::FeedbackLaunch{};
        if (d.read >= 0) {                                                          /* (b) */
            const Op w = writer[i][d.read];
            CHECK(w.op > 0 && fk.host[(size_t)w.stream] >= w.op, "a launch reads an order the host has not seen complete");
        }
        if (d.measure) {
            CHECK(d.write == (d.read ^ 1) || d.read < 0, "a measurement writes the order its launch reads");
            for (void *ev : d.wait) fk.wait(s, (Event *)ev);
            if (!d.wait.empty()) ++fenced;
            const Op lo = last_order[i];                                            /* (c) */
            CHECK(lo.op == 0 || fk.before(s, lo.stream, lo.op), "a measurement queued while the previous one may still run");
        }
        const long op = fk.queue(s);                                                /* the render kernel */
        if (d.read >= 0) {
            std::vector<Op> &rd = readers[i][d.read];
            if (rd.size() >= 64) {                                                  /* (those the host has seen complete are before everything) */
                size_t keep = 0;
                for (const Op &r : rd) if (fk.host[(size_t)r.stream] < r.op) rd[keep++] = r;
                rd.resize(keep);
            }
            rd.push_back(Op{s.id, op});
        }
        if (d.measure) {
            for (const Op &r : readers[i][d.write])                                 /* (a) */
                CHECK(fk.before(s, r.stream, r.op), "an order kernel overwrites an order that launch %ld of stream %d may still read", r.op, r.stream);
            readers[i][d.write].clear();
            const long ok = fk.queue(s);                                            /* the order kernel */
            writer[i][d.write] = last_order[i] = Op{s.id, ok};
            fk.record((Event *)f->done, s);
            rt::order_queued(*f, epoch);
            ++measured;
        }
        if (d.settled) ++settled;
        for (int a = 0; a < RT_FEEDBACK_SLOTS; ++a)                                 /* (d) */
            for (int b = a + 1; b < RT_FEEDBACK_SLOTS; ++b) CHECK(!(slots[a].key == slots[b].key), "a key in two slots");
        return d;
    }
    /* acquire_tables() for a launch with these kernel arguments: whether it builds a table set */
    bool tables(void *stream, const rt::KParams &k)
    {
        rt::StreamBook<TableBuf>::Record *sr = nullptr;
        CHECK(streams.record(stream, &sr) == RT_OK, "out of host memory");
        const rt::TableKey key = rt::table_key(scene_epoch, k.anchors, k.floor_anch, k.cam_o);
        const rt::TableDecision d = streams.tables(*sr, key, rt::table_floats(k.S, k.NC, k.anchors, false, true, k.P) * sizeof(float));
        if (!d.rebuild) return false;
        if (d.sync) fk.sync(fk.of(stream));
        TableBuf &b = sr->buf[rt::BUF_TABLES0 + d.set];
        if (b.cap < d.bytes) b.cap = d.bytes;
        fk.queue(fk.of(stream));                                                    /* the tables kernel */
        streams.tables_queued(*sr, d.set, key);
        return true;
    }
    void forget(void *stream)                         /* forget_stream() */
    {
        fk.sync(fk.of(stream));
        streams.forget(stream);
        bool pending = false;
        for (const rt::FeedbackSlot &f : slots)
            for (const auto &e : f.fence) pending |= e.first == stream;
        forgets += pending;
        book.forget(stream);
        for (const rt::FeedbackSlot &f : slots) {
            for (const auto &e : f.fence) CHECK(e.first != stream, "a forgotten stream is still fenced");
            for (void *u : f.users) CHECK(u != stream, "a forgotten stream is still a user");
        }
    }
    void destroy()                                    /* rt_destroy() */
    {
        for (rt::FeedbackSlot &f : slots) {
            for (void *e : rt::release_events(f)) fk.release((Event *)e);
            CHECK(f.fence.empty() && f.spare.empty() && !f.done, "release_events left an event in the slot");
        }
    }
};

static int walk(unsigned seed)
{
    long total[4] = {0, 0, 0, 0};
    for (int remeasure : {0, 2, 24}) {
        std::mt19937 rng(seed + (unsigned)remeasure);
        auto rnd = [&](int n) { return (int)(rng() % (unsigned)n); };
        Fake fk(4);
        Context ctx(fk, remeasure);
        rt::FeedbackKey keys[12];
        for (int g = 0; g < 12; ++g) keys[g] = rt::feedback_key(8 * g, 8 * g + 40, 128, RT_AA_NONE, false, 3, 0, 2);
        int hot = 0;
        for (g_step = 0; g_step < WALK_STEPS; ++g_step) {
            if (rnd(300) == 0) hot = rnd(12);
            const int r = rnd(100);
            void *stream = fk.handle(rnd(4));
            if (r < 62) {
                const int g = rnd(10) < 7 ? (hot + rnd(3)) % 12 : rnd(12);
                ctx.launch(stream, rnd(10) == 0 ? nullptr : &keys[g]);
            } else if (r < 70) {
                ctx.epoch++;
            } else if (r < 92) {
                Stream &s = fk.of(stream);
                if (s.completed < s.queued) fk.finish(s, s.completed + 1 + rnd((int)(s.queued - s.completed)));
            } else if (r < 98) {
                if (stream != fk.handle(0)) ctx.forget(stream);                     /* (rt_stream_forget refuses the context's own) */
            } else {
                fk.sync_device();
            }
            for (const Stream &s : fk.streams) CHECK(s.completed <= s.queued, "the fake completed what was never queued");
        }
        ctx.destroy();
        CHECK(fk.events.empty() && fk.created == fk.released, "%ld events created, %ld released", fk.created, fk.released);   /* (e) */
        std::printf("remeasure=%d launches_measuring=%ld launches_settled=%ld switch=%ld fenced_measure=%ld live_eviction=%ld forget_with_fence=%ld events=%ld\n",
                    remeasure, ctx.measured, ctx.settled, ctx.switches, ctx.fenced, ctx.evictions, ctx.forgets, fk.created);
        total[0] += ctx.switches; total[1] += ctx.fenced; total[2] += ctx.evictions; total[3] += ctx.forgets;
        if (!ctx.switches || !ctx.fenced || !ctx.evictions || !ctx.forgets) {
            std::fprintf(stderr, "remeasure %d: a transition was never taken\n", remeasure);
            return 1;
        }
    }
    std::printf("steps=%d switch=%ld fenced_measure=%ld live_eviction=%ld forget_with_fence=%ld ok\n", 3 * WALK_STEPS, total[0], total[1], total[2], total[3]);
    return 0;
}

/* The replay: launch() and dispatch() of mi355rt.hip down to the key, for launches of one frame that one dispatch holds. */
static int replay(const char *script, const char *out_path)
{
    FILE *fi = std::fopen(script, "r"), *fo = std::fopen(out_path, "w");
    if (!fi || !fo) return 2;
    int S = 0, L = 0, P = 0;
    if (std::fscanf(fi, " scene %d %d %d", &S, &L, &P) != 3) return 2;
    std::vector<float> spheres((size_t)(7 * S)), lights((size_t)(3 * L)), planes((size_t)(9 * P));
    for (std::vector<float> *a : {&spheres, &lights, &planes})
        for (float &v : *a) { double d; if (std::fscanf(fi, "%lf", &d) != 1) return 2; v = (float)d; }
    rt::SceneDesc desc;
    desc.spheres = spheres.data(); desc.S = S; desc.lights = lights.data(); desc.L = L; desc.planes = planes.data(); desc.P = P;
    const rt::PlanKnobs knobs;
    const rt::PackedScene ps = rt::pack_scene(desc, rt::CLUSTER_MIN, knobs.lanes_min_spheres);
    if (ps.status != RT_OK) { std::fprintf(stderr, "pack_scene: %s\n", ps.error.c_str()); return 1; }
    const rt::SceneLayout &lay = ps.layout;
    int ncam = 0;
    if (std::fscanf(fi, " cameras %d", &ncam) != 1 || ncam < 1) return 2;
    std::vector<double> cameras((size_t)(3 * ncam));                             /* rt_set_camera's origins, as float64 */
    for (double &v : cameras) if (std::fscanf(fi, "%lf", &v) != 1) return 2;

    Fake *fk = nullptr;
    Context *ctx = nullptr;
    int w = 0, h = 0, cam = -1;
    char word[32];
    long steps = 0;
    auto close = [&]() {
        if (!ctx) return;
        ctx->destroy();
        CHECK(fk->events.empty() && fk->created == fk->released, "%ld events created, %ld released", fk->created, fk->released);
        delete ctx; delete fk;
        ctx = nullptr; fk = nullptr;
    };
    for (g_step = 0; std::fscanf(fi, "%31s", word) == 1; ++g_step) {
        const std::string kind = word;
        int measured = 0, settled = 0, built = 0;
        if (kind == "ctx") {                                                      /* rt_create under MI355RT_REMEASURE */
            int rm;
            if (std::fscanf(fi, "%d", &rm) != 1) return 2;
            close();
            fk = new Fake(3);
            ctx = new Context(*fk, rm);
            w = h = 0; cam = -1;
            --g_step;
            continue;
        }
        if (!ctx) return 2;
        if (kind == "scene") {                                                    /* rt_set_scene: always a new epoch */
            ctx->epoch++;
            ctx->scene_epoch++;
        } else if (kind == "camera") {                                            /* rt_set_camera: the same camera again changes nothing */
            int c;
            if (std::fscanf(fi, "%d", &c) != 1 || c < 0 || c >= ncam) return 2;
            if (c != cam) ctx->epoch++;
            cam = c;
        } else if (kind == "grid") {                                              /* rt_set_raygen: nor does the same grid */
            int gw, gh;
            if (std::fscanf(fi, "%d %d", &gw, &gh) != 2 || !rt_geo_frame_ok(gw, gh)) return 2;
            if (gw != w || gh != h) ctx->epoch++;
            w = gw; h = gh;
        } else if (kind == "forget") {
            int s;
            if (std::fscanf(fi, "%d", &s) != 1 || s < 1 || s > 2) return 2;
            ctx->forget(fk->handle(s));
        } else if (kind == "launch") {
            int s, x0, x1, depth, aa, spp, flags;
            if (std::fscanf(fi, "%d %d %d %d %d %d %d", &s, &x0, &x1, &depth, &aa, &spp, &flags) != 7) return 2;
            if (s < 0 || s > 2 || x0 < 0 || x1 > w || x0 >= x1 || cam < 0) return 2;
            long long l0 = 0, l1 = 0;
            const bool lattice = aa == RT_AA_REFERENCE && rt_geo_lattice(w, h, x0, x1, &l0, &l1) && !(flags & RT_FLAG_AA_PER_PIXEL);
            const rt::LaunchPlan plan = rt::plan_launch(lay, knobs, 0.0, !lattice && aa != 0, flags, lattice, rt::anchors_of(lay));
            rt::View v;                                                           /* (the tables' key takes the camera's position only) */
            v.w = w; v.h = h; v.have_cam = v.have_grid = true;
            std::memcpy(v.cam_o, &cameras[(size_t)(3 * cam)], sizeof v.cam_o);
            rt_params p;
            std::memset(&p, 0, sizeof p);
            p.depth = depth; p.aa_mode = aa; p.spp = spp; p.flags = flags;
            rt::KParams k;
            rt::render_part(k, v, lay, plan.family, &p, nullptr, nullptr, nullptr, 1, x0, x1, nullptr, nullptr, 0, nullptr);
            built = ctx->tables(fk->handle(s), k);
            const int kx0 = lattice ? (int)l0 : x0, kx1 = lattice ? (int)l1 : x1, kh = lattice ? 2 * h - 1 : h, kaa = lattice ? 0 : aa;
            const rt_geo_plan g = rt_geo_plan_of(kx0, kx1, kh, plan.shape.wpw, 1);
            if (g.nslabs != 1) return 2;
            const rt::OrderShape os = rt::order_shape(plan, knobs, flags, g);
            const rt::FeedbackKey key = rt::feedback_key(kx0, kx1, kh, kaa, plan.shape.lat, depth, spp, os.code);
            const rt::FeedbackLaunch d = ctx->launch(fk->handle(s), os.feedback ? &key : nullptr);
            fk->sync(fk->of(fk->handle(s)));
            measured = d.measure; settled = d.settled;
        } else {
            std::fprintf(stderr, "unknown step %s\n", word);
            return 2;
        }
        std::fprintf(fo, "%d %d %d\n", measured, settled, built);
        ++steps;
    }
    close();
    if (std::fclose(fo) != 0) return 2;
    std::fclose(fi);
    std::printf("steps=%ld ok\n", steps);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "replay")) return replay(argv[2], argv[3]);
    if ((argc == 2 || argc == 3) && !std::strcmp(argv[1], "walk")) return walk(argc == 3 ? (unsigned)std::strtoul(argv[2], nullptr, 10) : 1u);
    return 2;
}
