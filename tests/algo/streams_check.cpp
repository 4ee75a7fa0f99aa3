/* The library's per-stream state (python-ray-tracer_amd/csrc/rt_streams.h) without HIP, driven as mi355rt.hip's launch(),
 * acquire_tables(), stream_buffer(), set_scene(), forget_stream() and rt_destroy() drive it, over a fake runtime.  Built with
 * AddressSanitizer and UndefinedBehaviorSanitizer (leak detection on) and run by tests/test_algorithms.py.
 *
 *   streams_check [SEED]   a random walk of WALK_STEPS = 100000 steps for each of 1, 3 and 6 camera positions: launches on 4 streams
 *                          (the context's own and three of the caller's) with keys drawn from the scene epochs, the cameras, two
 *                          anchor counts and two floors, and table sizes that change with the scene; lattice and film requests whose
 *                          sizes grow and shrink; scene changes round the ring; completion of a prefix of a stream's queue;
 *                          rt_stream_forget; teardown and a fresh context.  After every step:
 *      (a) a hit names a set that was built for exactly that key on that stream, and a rebuild takes an invalid set before a
 *          valid one and the less recently used of two valid ones;
 *      (b) a buffer is freed or regrown only when everything queued on its stream that could read it has completed;
 *      (c) a scene-ring buffer is rewritten only when every launch that reads it has completed (its stream was synchronised
 *          since, or forgotten);
 *      (d) after forget, nothing of the stream remains: no record, no buffer;
 *      (e) at teardown every buffer and stream ever made has been released exactly once.
 *   It prints how often each transition was taken and fails if one never was.
 *
 * The fake runtime: a stream is a queued counter and a completed counter, on the heap; a buffer is a heap object that remembers its
 * stream and the last operation queued there that reads or writes it, so a lost, twice-freed or early-freed one is a report. */
#include "../../python-ray-tracer_amd/csrc/rt_streams.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <utility>

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "step %ld: ", g_step); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

static long g_step = 0;
static const int WALK_STEPS = 100000;

struct Stream { long queued = 0, completed = 0; };
struct Mem { size_t bytes = 0; Stream *stream = nullptr; long last_op = 0; };   /* stream == nullptr: the scene ring's */

struct Fake {
    std::set<Stream *> streams;
    std::set<Mem *> mems;
    long made = 0, released = 0;

    Stream *stream_create() { Stream *s = new Stream; streams.insert(s); ++made; return s; }
    void stream_destroy(Stream *s)
    {
        CHECK(streams.erase(s) == 1, "a stream destroyed twice, or one the runtime never made");
        CHECK(s->completed == s->queued, "a stream destroyed before it was drained");
        ++released;
        delete s;
    }
    void sync(Stream *s) { CHECK(streams.count(s) == 1, "synchronise of a destroyed stream"); s->completed = s->queued; }
    long queue(Stream *s) { CHECK(streams.count(s) == 1, "launch on a destroyed stream"); return ++s->queued; }
    Mem *alloc(size_t bytes, Stream *s) { Mem *m = new Mem; m->bytes = bytes; m->stream = s; mems.insert(m); ++made; return m; }
    void free(Mem *m)
    {
        CHECK(mems.erase(m) == 1, "a buffer freed twice, or one the runtime never made");
        CHECK(!m->stream || streams.count(m->stream) == 0 || m->stream->completed >= m->last_op,            /* (b); (a destroyed stream was drained) */
              "a buffer freed while operation %ld of its stream may still use it", m->last_op);
        ++released;
        delete m;
    }
};
static Fake *g_fake = nullptr;

struct Buf {                                          /* mi355rt.hip's Buf over the fake */
    Mem *p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(Buf &&o) noexcept { *this = std::move(o); }
    Buf &operator=(Buf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~Buf() { if (p) g_fake->free(p); }
};

static void ensure(Buf &b, size_t bytes, Stream *s)
{
    if (bytes <= b.cap) return;
    if (b.p) { g_fake->free(b.p); b.p = nullptr; b.cap = 0; }
    b.p = g_fake->alloc(bytes, s);
    b.cap = bytes;
}

struct Counts { long hit = 0, rebuild_invalid = 0, rebuild_older = 0, grow_sync = 0, drain = 0, forget_bufs = 0, teardowns = 0; };

/* One context as mi355rt.hip keeps it, and what the checks remember on their own. */
struct Context {
    typedef rt::StreamBook<Buf> Book;
    Fake &fk;
    Counts &n;
    Stream *own;
    Book streams;
    Buf scene[RT_SCENE_RING];
    int scene_cur = 0;
    unsigned long long scene_epoch = 1;
    struct Built { bool valid = false; rt::TableKey key; long used = 0; };
    std::map<std::pair<Stream *, int>, Built> built;  /* what the tables kernels wrote, per stream and set */
    std::map<Stream *, long> scene_reader[RT_SCENE_RING];   /* per ring buffer: the last launch of each stream that reads it */
    long uses = 0;

    Context(Fake &f, Counts &c) : fk(f), n(c), own(f.stream_create()) { set_scene(64); }
    ~Context() { fk.stream_destroy(own); }            /* ~rt_ctx: the members free their buffers after this */

    Book::Record &record(Stream *s)                   /* stream_record() */
    {
        Book::Record *sr = nullptr;
        CHECK(streams.record(s, &sr) == RT_OK, "out of host memory");
        Book::reads_scene(*sr, scene_cur);
        return *sr;
    }
    void stream_buffer(Buf &b, Stream *s, size_t bytes, bool sync)
    {
        if (sync) { fk.sync(s); ++n.grow_sync; }
        ensure(b, bytes, s);
    }
    void launch(Stream *s, const rt::TableKey &key, size_t bytes)   /* launch() and acquire_tables() */
    {
        Book::Record &sr = record(s);
        const bool valid[2] = {sr.sets[0].valid, sr.sets[1].valid};
        const rt::TableDecision d = streams.tables(sr, key, bytes);
        Built &b = built[std::make_pair(s, d.set)];
        Buf &tb = sr.buf[rt::BUF_TABLES0 + d.set];
        if (d.rebuild) {
            const Built &other = built[std::make_pair(s, d.set ^ 1)];
            CHECK(!(other.valid && other.key == key), "a rebuild although the stream's other set holds the key");
            CHECK(valid[d.set] == b.valid && valid[d.set ^ 1] == other.valid, "the header's valid flags are not what was built");
            if (b.valid) {                                                          /* (a) */
                CHECK(other.valid, "a valid set rebuilt while the other is invalid");
                CHECK(b.used < other.used, "the more recently used set rebuilt");
                ++n.rebuild_older;
            } else ++n.rebuild_invalid;
            CHECK(!sr.sets[d.set].valid, "the set to rebuild is still valid");
            b.valid = false;
            CHECK(d.bytes == (bytes ? bytes : 16), "a table buffer of %zu bytes for tables of %zu", d.bytes, bytes);
            CHECK(d.sync == (tb.cap > 0 && tb.cap < d.bytes), "the synchronise does not follow the growth rule");
            stream_buffer(tb, s, d.bytes, d.sync);
            tb.p->last_op = fk.queue(s);                                            /* the tables kernel */
            streams.tables_queued(sr, d.set, key);
            b.valid = true; b.key = key;
        } else {
            CHECK(b.valid && b.key == key, "a hit on a set that was not built for this key on this stream");   /* (a) */
            ++n.hit;
        }
        b.used = ++uses;
        CHECK(tb.p && tb.cap >= (bytes ? bytes : 16), "the tables' buffer is too small");
        const long op = fk.queue(s);                                                /* the render kernel */
        tb.p->last_op = op;
        scene_reader[scene_cur][s] = op;
    }
    void scratch(Stream *s, int which, size_t bytes)  /* the lattice of launch(), the frames of rt_film_accumulate */
    {
        Book::Record &sr = record(s);
        Buf &b = sr.buf[which];
        stream_buffer(b, s, bytes, rt::growth(b.cap, bytes).sync);
        CHECK(b.p && b.cap >= bytes, "a scratch buffer smaller than asked for");
        b.p->last_op = fk.queue(s);
        scene_reader[scene_cur][s] = b.p->last_op;
    }
    void set_scene(size_t bytes)                      /* set_scene() */
    {
        const int next = (scene_cur + 1) % RT_SCENE_RING;
        bool drained = false;
        streams.drain_scene(next, [&](void *st) { fk.sync((Stream *)st); drained = true; return (int)RT_OK; });
        n.drain += drained;
        for (const auto &r : scene_reader[next])                                    /* (c) */
            CHECK(fk.streams.count(r.first) == 1 && r.first->completed >= r.second, "a scene buffer rewritten under launch %ld of a stream", r.second);
        scene_reader[next].clear();
        for (const Book::Record &r : streams.records) CHECK(!(r.scenes & (1u << next)), "a drained stream is still a reader");
        ensure(scene[next], bytes, nullptr);
        fk.queue(own);                                                              /* the upload */
        fk.sync(own);
        scene_cur = next;
        ++scene_epoch;
    }
    void forget(Stream *s)                            /* forget_stream() */
    {
        fk.sync(s);
        {
            const Book::Record gone = streams.forget(s);
            bool bufs = false;
            for (const Buf &b : gone.buf) bufs |= b.p != nullptr;
            n.forget_bufs += bufs;
        }
        for (const Book::Record &r : streams.records) CHECK(r.stream != s, "a forgotten stream still has a record");   /* (d) */
        for (const Mem *m : fk.mems) CHECK(m->stream != s, "a forgotten stream still has a buffer");
        for (int set = 0; set < 2; ++set) built.erase(std::make_pair(s, set));
        for (auto &rd : scene_reader) rd.erase(s);                                  /* (its launches are complete) */
    }
};

static int walk(unsigned seed)
{
    Counts total;
    for (int ncam : {1, 3, 6}) {
        std::mt19937 rng(seed + (unsigned)ncam);
        auto rnd = [&](int n) { return (int)(rng() % (unsigned)n); };
        Fake fk;
        g_fake = &fk;
        Counts n;
        Context *ctx = new Context(fk, n);
        Stream *callers[3] = {fk.stream_create(), fk.stream_create(), fk.stream_create()};
        size_t scene_bytes = 64;
        int hot_cam = 0;
        for (g_step = 0; g_step < WALK_STEPS; ++g_step) {
            const int r = rnd(1000), si = rnd(4);
            Stream *s = si ? callers[si - 1] : ctx->own;
            if (rnd(40) == 0) hot_cam = rnd(ncam);
            if (r < 500) {
                const int cam = rnd(4) ? hot_cam : rnd(ncam), anchors = rnd(8) ? 1 : 2;
                const double o[3] = {0.25 * cam, cam ? -0.0 : 0.0, 1.0};
                const rt::TableKey key = rt::table_key(ctx->scene_epoch, anchors, rnd(8) ? 0.5f : 0.125f, o);
                ctx->launch(s, key, scene_bytes / 8 * (size_t)anchors);
            } else if (r < 620) {
                ctx->scratch(s, rnd(2) ? rt::BUF_LATTICE : rt::BUF_FILM, (size_t)(1 + rnd(6)) * 1000);
            } else if (r < 650) {
                scene_bytes = (size_t)rnd(5) * 96;                                  /* (0: a scene without spheres has 16-byte tables) */
                ctx->set_scene(scene_bytes + 8);
            } else if (r < 960) {
                if (s->completed < s->queued) s->completed += 1 + rnd((int)(s->queued - s->completed));
            } else if (r < 999) {
                if (si) ctx->forget(s);                                             /* (rt_stream_forget refuses the context's own) */
            } else {
                /* teardown: the caller closes or synchronises its streams, rt_destroy drains the context's own and deletes it */
                for (Stream *&c : callers) {
                    if (rnd(2)) { ctx->forget(c); fk.stream_destroy(c); c = fk.stream_create(); }   /* rt_stream_destroy */
                    else fk.sync(c);
                }
                fk.sync(ctx->own);
                delete ctx;
                CHECK(fk.mems.empty() && fk.streams.size() == 3, "teardown left %zu buffers and %zu streams", fk.mems.size(), fk.streams.size() - 3);   /* (e) */
                ++n.teardowns;
                ctx = new Context(fk, n);
                scene_bytes = 64;
            }
            for (const Stream *t : fk.streams) CHECK(t->completed <= t->queued, "the fake completed what was never queued");
        }
        for (Stream *c : callers) { fk.sync(c); }
        fk.sync(ctx->own);
        delete ctx;
        for (Stream *c : callers) fk.stream_destroy(c);
        CHECK(fk.mems.empty() && fk.streams.empty() && fk.made == fk.released, "%ld buffers and streams made, %ld released", fk.made, fk.released);   /* (e) */
        std::printf("cameras=%d hit=%ld rebuild_invalid=%ld rebuild_older=%ld grow_behind_sync=%ld scene_drain=%ld forget_with_buffers=%ld teardown=%ld made=%ld\n",
                    ncam, n.hit, n.rebuild_invalid, n.rebuild_older, n.grow_sync, n.drain, n.forget_bufs, n.teardowns, fk.made);
        if (!n.hit || !n.rebuild_invalid || !n.rebuild_older || !n.grow_sync || !n.drain || !n.forget_bufs || !n.teardowns) {
            std::fprintf(stderr, "%d cameras: a transition was never taken\n", ncam);
            return 1;
        }
        total.hit += n.hit; total.rebuild_invalid += n.rebuild_invalid; total.rebuild_older += n.rebuild_older; total.grow_sync += n.grow_sync;
        total.drain += n.drain; total.forget_bufs += n.forget_bufs; total.teardowns += n.teardowns;
        g_fake = nullptr;
    }
    std::printf("steps=%d hit=%ld rebuild_invalid=%ld rebuild_older=%ld grow_behind_sync=%ld scene_drain=%ld forget_with_buffers=%ld teardown=%ld ok\n",
                3 * WALK_STEPS, total.hit, total.rebuild_invalid, total.rebuild_older, total.grow_sync, total.drain, total.forget_bufs, total.teardowns);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 2) return 2;
    return walk(argc == 2 ? (unsigned)std::strtoul(argv[1], nullptr, 10) : 1u);
}
