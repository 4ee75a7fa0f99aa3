// rt_feedback.h — the rules of the scheduler feedback, the dispatch orders a launch geometry's launches measure and reuse: which
// of a geometry's two order buffers a launch reads, when a launch measures, when the context switches to the order that was
// built, which streams a measurement must be fenced against, when an order counts as settled, and which of the context's
// RT_FEEDBACK_SLOTS slots a new geometry takes.
// HIP-free, like rt_plan.h and for the same reason: a pure state machine on the host.  Streams and events are opaque handles;
// the header decides and keeps the books, mi355rt.hip makes the HIP calls the decisions name (and keeps the slots' device
// buffers).  tests/algo/feedback_check.cpp drives it with a fake runtime under AddressSanitizer and UBSan: a recorded call
// sequence must give the recorded decisions, and on a random walk over streams no measurement may overwrite an order that a
// launch in flight still reads.
//
// Scheduler feedback: a MEASURING launch stores its tile blocks' costs; a small kernel behind it (same stream) turns
// them into a dispatch order (rt::order_kernel).  The order lives in two buffers: launches dispatch in order[cur]
// while a measuring launch's order kernel writes order[cur ^ 1]; the context switches to the new one when a later
// launch (on any stream) finds the order kernel's event complete — so no stream ever waits for another stream's
// measuring launch (round 2: the other streams' first launch in a new order waited for it, and a measuring launch
// waited for everything the other streams had queued; with a camera that moves every frame that was a pipeline
// bubble per measurement).  The buffer a measurement overwrites was last read by launches queued before the previous
// switch; events recorded on their streams AT that switch (complete long before they are waited on) fence them.
#pragma once
#include "../../include/mi355rt.h"

#include <algorithm>
#include <utility>
#include <vector>

#define RT_FEEDBACK_SLOTS 8

namespace rt {

// The launch geometry a slot's orders were built for (valid = false: none).
struct FeedbackKey {
    bool valid = false;
    int x0 = 0, x1 = 0, h = 0, aa = 0, depth = 0, spp = 0, wpw = 0;
    bool operator==(const FeedbackKey &o) const
    {
        return valid && o.valid && x0 == o.x0 && x1 == o.x1 && h == o.h && aa == o.aa && depth == o.depth &&
               spp == o.spp && wpw == o.wpw;
    }
};

// The key of one dispatch: columns [x0, x1) of a frame h high, the launch's AA mode (a lattice launch is a mode of its own),
// depth, the samples of a stochastic launch, and what of the kernel's shape an order depends on (rt_plan.h: OrderShape::code).
inline FeedbackKey feedback_key(int x0, int x1, int h, int aa_mode, bool lattice, int depth, int spp, int order_code)
{
    FeedbackKey k;
    k.valid = true; k.x0 = x0; k.x1 = x1; k.h = h; k.aa = lattice ? 3 : aa_mode; k.depth = depth;
    k.spp = (aa_mode == RT_AA_STOCHASTIC) ? spp : 0; k.wpw = order_code;
    return k;
}

// The host state of one slot.  Written by the functions below only.
struct FeedbackSlot {
    FeedbackKey key;
    int cur = 0;
    bool have = false;            // order[cur] holds a complete order
    bool building = false;        // a measuring launch and its order kernel are in flight, writing order[cur ^ 1]
    unsigned long long epoch = 0; // context epoch the costs behind order[cur] were measured under
    unsigned long long build_epoch = 0;   // ... behind the order being built
    int builds = 0;               // consecutive orders built under `epoch`
    int since = 0;                // launches that used the order under a LATER epoch (moving camera) since the last measurement
    void *done = nullptr;         // event recorded behind every order kernel (the caller creates it)
    std::vector<void *> users;                        // streams that launched in order[cur] since the last switch
    std::vector<std::pair<void *, void *>> fence;     // (stream, event) recorded at the last switch: what may still read order[cur ^ 1]
    std::vector<void *> spare;                        // events to record again
    unsigned long long stamp = 0; // last use (the least recently used geometry is replaced)
};

// An order built for this launch geometry is a valid permutation whatever has happened to scene and camera since: only
// how well it balances the end of the launch depends on them.
//  * Nothing that decides a tile's cost has changed since the order was rebuilt twice (once from plain tile order, once
//    from longest-first order): the costs are the same again, so launches neither measure nor rebuild — they dispatch
//    in that order, on any stream.
//  * Something has changed (rt_set_* bumped the epoch — a moving camera does so with every frame): launches still
//    dispatch in the order there is, and only every `remeasure`-th of them measures its tiles again (under that order)
//    and rebuilds.  Round 2 measured and rebuilt with every frame of a moving camera: +11 us per frame.
inline bool settled(const FeedbackSlot &f, unsigned long long ctx_epoch, int remeasure)
{
    return f.have && (f.epoch == ctx_epoch ? f.builds >= 2 : f.since < remeasure);
}

// The fence's events (all of them, or those of one stream) have been waited for, or guard nothing any more: they are free to be
// recorded again.
inline void retire_fence(FeedbackSlot &f, const void *of = nullptr)
{
    size_t keep = 0;
    for (auto &e : f.fence)
        if (!of || e.first == of) f.spare.push_back(e.second);
        else f.fence[keep++] = e;
    f.fence.resize(keep);
}

// The caller has found `done` complete while the slot was building: switch to the order that was built.  Launches queued so
// far on the streams that used the old order may still read it: the caller records an event on each stream this returns
// (take_spare's, else a new one) and files it with add_fence; the measurement after next waits for them before it overwrites
// that buffer.
inline std::vector<void *> switch_order(FeedbackSlot &f)
{
    f.cur ^= 1;
    f.have = true;
    f.building = false;
    f.builds = (f.build_epoch == f.epoch) ? f.builds + 1 : 1;
    f.epoch = f.build_epoch;
    retire_fence(f);
    std::vector<void *> users;
    users.swap(f.users);
    return users;
}

inline void *take_spare(FeedbackSlot &f)
{
    if (f.spare.empty()) return nullptr;
    void *ev = f.spare.back();
    f.spare.pop_back();
    return ev;
}

inline void add_fence(FeedbackSlot &f, void *stream, void *event) { f.fence.emplace_back(stream, event); }

// What one dispatch does with its geometry's orders.  The default is the launch without feedback (RT_FLAG_NO_FEEDBACK, one
// block): plain tile order, no measuring, no slot.
struct FeedbackLaunch {
    bool settled = false;         // the order is settled: neither measured nor rebuilt
    bool measure = false;         // the launch stores its tiles' costs, and an order kernel behind it writes order[write]
    int read = -1;                // the launch dispatches in order[read] (-1: plain tile order)
    int write = -1;
    std::vector<void *> wait;     // measure: events the launching stream waits for before the launch (other streams' fence)
};

// One dispatch on `stream` in the slot's geometry, decided before it is queued.  One measurement is in flight at a time (one
// cost buffer).  The fence stays in place until order_queued: a launch that fails in between has lost no event.
inline FeedbackLaunch decide_launch(FeedbackSlot &f, void *stream, unsigned long long ctx_epoch, int remeasure)
{
    FeedbackLaunch d;
    d.settled = settled(f, ctx_epoch, remeasure);
    d.measure = !d.settled && !f.building;
    if (d.settled && f.epoch != ctx_epoch) f.since++;
    if (f.have) {
        d.read = f.cur;
        if (std::find(f.users.begin(), f.users.end(), stream) == f.users.end()) f.users.push_back(stream);
    }
    if (d.measure) {
        d.write = f.cur ^ 1;
        for (auto &e : f.fence)                                    // (recorded at the last switch: complete long ago)
            if (e.first != stream) d.wait.push_back(e.second);
    }
    return d;
}

// The measuring launch decide_launch asked for, its order kernel and `done` behind it are queued.
inline void order_queued(FeedbackSlot &f, unsigned long long ctx_epoch)
{
    retire_fence(f);
    f.building = true;
    f.build_epoch = ctx_epoch;
    f.since = 0;
}

// Every event of the slot, for the caller to destroy; the slot keeps none.
inline std::vector<void *> release_events(FeedbackSlot &f)
{
    retire_fence(f);
    std::vector<void *> ev;
    ev.swap(f.spare);
    if (f.done) ev.push_back(f.done);
    f.done = nullptr;
    return ev;
}

// The context's slots, one per launch geometry in use: slabs, chunks and AA modes do not evict each other.  The slots
// themselves live with their device buffers, at the caller's (slot[i] points to them).
struct FeedbackBook {
    FeedbackSlot *slot[RT_FEEDBACK_SLOTS] = {};
    unsigned long long stamp = 0;

    // The slot of a launch geometry: the one that holds it, else a free slot, else the least recently used geometry's.
    // *live: the slot holds another geometry, whose launches may still read its orders (rare: more than RT_FEEDBACK_SLOTS
    // geometries) — the caller synchronises the device before it claims the slot.
    int find(const FeedbackKey &key, bool *live) const
    {
        *live = false;
        int sel = 0;
        for (int i = 0; i < RT_FEEDBACK_SLOTS; ++i) {
            const FeedbackSlot &c = *slot[i], &s = *slot[sel];
            if (c.key == key) return i;
            if ((!c.key.valid && s.key.valid) || (c.key.valid == s.key.valid && c.stamp < s.stamp)) sel = i;
        }
        *live = slot[sel]->key.valid;
        return sel;
    }

    // Slot i, found for this key, is in use now: a slot that held another geometry (or none) starts empty.
    FeedbackSlot &claim(int i, const FeedbackKey &key)
    {
        FeedbackSlot &f = *slot[i];
        if (!(f.key == key)) {
            retire_fence(f);
            f.users.clear();
            f.have = f.building = false; f.builds = 0; f.since = 0; f.cur = 0;
            f.key = key;
        }
        f.stamp = ++stamp;
        return f;
    }

    // The stream's queued work is complete (the caller has waited for it): nothing of it reads an order any more.
    void forget(void *stream)
    {
        for (FeedbackSlot *f : slot) {
            retire_fence(*f, stream);
            f->users.erase(std::remove(f->users.begin(), f->users.end(), stream), f->users.end());
        }
    }
};

}  // namespace rt
