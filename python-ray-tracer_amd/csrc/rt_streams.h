// rt_streams.h — what the context knows about each stream that has launched on it, in one record per stream: the host state of
// the stream's two cull-table sets, its growable device buffers (two table buffers, the lattice samples of RT_AA_REFERENCE, the
// film's pass frames) and the scene-ring slots it has launched with.  The header finds or adds a record, decides which table set a
// launch reads or rebuilds, says when a buffer must grow and whether the stream is synchronised first, and takes a record out when
// its stream is forgotten.
// HIP-free, like rt_feedback.h and for the same reason: a pure state machine on the host.  Streams are opaque handles; the
// header decides and keeps the books, mi355rt.hip makes the HIP calls the decisions name.  The buffers are of the caller's type B
// (a `cap` member: the bytes it holds, 0: none) and are the caller's to allocate; a record owns them, so what leaves the book is
// freed by B's destructor.  tests/algo/streams_check.cpp drives the header with a fake runtime under AddressSanitizer and UBSan
// on a random walk, and tests/algo/feedback_check.cpp replays a recorded call sequence: the table builds must be the recorded ones.
//
// The float32 cull tables (rt::tables_kernel) of the last (scene, camera position, floor) combinations are kept PER STREAM: a
// set is built on the stream of the launch that needs it and read only by launches of that stream, so rebuilding a
// stream's older set is ordered behind its readers by the stream itself — no events, no cross-stream waits.  (Round 2
// shared three sets among the streams behind events; with a camera that moves every frame the events made every
// stream wait for the others' newest launches: frames of different streams no longer overlapped, +45 %.)  Frames
// of a static camera on n streams build n identical sets once (a few microseconds each).
#pragma once
#include "../../include/mi355rt.h"

#include <cstddef>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#define RT_SCENE_RING 4   /* the packed scenes live in a ring of this many device buffers (at most 32: StreamRecord::scenes) */

namespace rt {

// A stream's growable buffers: the table sets' (TABLES0 + i is set i's), then one per feature that needs scratch of its own.
enum StreamBuf { BUF_TABLES0 = 0, BUF_TABLES1 = 1, BUF_LATTICE = 2, BUF_FILM = 3, STREAM_BUFS = 4 };

// What a table set was built for: the scene, the anchors, the floor and the camera position (bitwise: -0.0 is not 0.0).
struct TableKey {
    unsigned long long scene_epoch = 0;
    int anchors = -1;
    float floor_anch = 0.0f;
    double cam[3] = {0, 0, 0};
    bool operator==(const TableKey &o) const
    {
        return scene_epoch == o.scene_epoch && anchors == o.anchors && floor_anch == o.floor_anch && std::memcmp(cam, o.cam, sizeof cam) == 0;
    }
};

inline TableKey table_key(unsigned long long scene_epoch, int anchors, float floor_anch, const double cam[3])
{
    TableKey k;
    k.scene_epoch = scene_epoch; k.anchors = anchors; k.floor_anch = floor_anch;
    std::memcpy(k.cam, cam, sizeof k.cam);
    return k;
}

struct TableSet {
    bool valid = false;
    TableKey key;
    unsigned long long stamp = 0;     // last use (the stream's less recently used set is rebuilt)
};

// A buffer of `cap` bytes is asked for `bytes`: growing frees the old buffer, which the stream's queued work may still read, so
// the stream is synchronised first (a buffer that does not exist yet has no reader).
struct Growth { bool grow = false, sync = false; };
inline Growth growth(size_t cap, size_t bytes)
{
    Growth g;
    g.grow = cap < bytes;
    g.sync = g.grow && cap > 0;
    return g;
}

template <class B>
struct StreamRecord {
    void *stream = nullptr;
    TableSet sets[2];
    B buf[STREAM_BUFS];
    unsigned scenes = 0;              // bit i: the stream has launched with scene-ring buffer i since that was last rewritten
};

// What a launch does about its cull tables: it reads set `set`; rebuild: after the tables kernel has written it, behind a
// synchronise of the stream if `sync`, into buf[BUF_TABLES0 + set] of at least `bytes`.
struct TableDecision {
    int set = 0;
    bool rebuild = false, sync = false;
    size_t bytes = 0;
};

template <class B>
struct StreamBook {
    typedef StreamRecord<B> Record;
    std::vector<Record> records;
    unsigned long long stamp = 0;     // one counter for all streams' table sets

    // The stream's record, added if this is its first call: RT_OK, or RT_ERR_ALLOC (rt_last_error: NO_MEMORY).  The pointer
    // holds until the next call for another stream.
    static constexpr const char *NO_MEMORY = "out of host memory";
    int record(void *stream, Record **out)
    {
        for (Record &r : records)
            if (r.stream == stream) { *out = &r; return RT_OK; }
        try { records.emplace_back(); } catch (const std::bad_alloc &) { return RT_ERR_ALLOC; }
        records.back().stream = stream;
        *out = &records.back();
        return RT_OK;
    }

    // The cull tables for a launch's key, `bytes` large: a set built for exactly this key, else the stream's less recently used
    // set is rebuilt, an invalid one first.  That set is invalid from here until tables_queued: an allocation that fails in
    // between leaves it so.
    TableDecision tables(Record &r, const TableKey &key, size_t bytes)
    {
        TableDecision d;
        TableSet *victim = &r.sets[0];
        for (TableSet &t : r.sets) {
            if (t.valid && t.key == key) {
                t.stamp = ++stamp;
                d.set = (int)(&t - r.sets);
                return d;
            }
            if ((!t.valid && victim->valid) || (t.valid == victim->valid && t.stamp < victim->stamp)) victim = &t;
        }
        victim->valid = false;
        d.set = (int)(victim - r.sets);
        d.rebuild = true;
        d.bytes = bytes ? bytes : 16;
        d.sync = growth(r.buf[BUF_TABLES0 + d.set].cap, d.bytes).sync;
        return d;
    }

    // The tables kernel that tables() asked for is queued on the record's stream.
    void tables_queued(Record &r, int set, const TableKey &key)
    {
        TableSet &t = r.sets[set];
        t.key = key;
        t.valid = true;
        t.stamp = ++stamp;
    }

    // A launch on the record's stream reads scene-ring buffer `slot`.
    static void reads_scene(Record &r, int slot) { r.scenes |= 1u << slot; }

    // Scene-ring buffer `slot` is about to be rewritten: sync(stream) (RT_OK, or the caller's error, which ends the walk) for
    // every stream that has launched with it; a stream that was synchronised reads it no more.
    template <class F>
    int drain_scene(int slot, F sync)
    {
        for (Record &r : records)
            if (r.scenes & (1u << slot)) {
                const int rc = sync(r.stream);
                if (rc != RT_OK) return rc;
                r.scenes &= ~(1u << slot);
            }
        return RT_OK;
    }

    // The stream's queued work is complete (the caller has waited for it): its record leaves the book, and its buffers go with
    // it, for the caller to free (B's destructor, when the returned record goes out of scope).
    Record forget(void *stream)
    {
        Record gone;
        for (size_t i = 0; i < records.size(); ++i)
            if (records[i].stream == stream) {
                gone = std::move(records[i]);
                records.erase(records.begin() + (long)i);
                break;
            }
        return gone;
    }
};

}  // namespace rt
