// pipe_schedule.h — the schedule of the pipelined frames (engine.hip render_pipelined) as
// host-only code: which frame group starts when, in which ring slot and with which seed, how
// large the ring is, when a render continues the previous one and what is dropped when it does
// not.  No HIP types, no device pointers, no environment: the engine asks one decision at a
// time and turns each answer into launches; tests/test_pipe_schedule_host.py walks the same
// decisions without a device.
//
// Pipelined frames.  The batch's path state is one slot of a ring of K slots.  A frame
// runs max_depth phases -- phase b: trace (b = 0: the camera rays, else the shadow +
// extension rays its bounce-(b-1) shade spawned) then the bounce-b shade -- and one
// iteration advances every frame in flight by one phase with one flags partition over the
// ring, ONE persistent traversal launch (the listed shadow and extension rays of all frames,
// plus the camera rays of a frame started in that iteration) and ONE shade launch (each path
// at its own bounce).  A render runs the iterations its own frame still needs and then
// accumulates it, so the frame is complete when the call's work has run, as PTPass::OnRun
// requires (pt_pass.cpp:51-56); the other frames in flight belong to the renders that continue
// this one (random_seed + spp each, same camera, scene, tiling, spp and depth), and are
// dropped when the next render does not continue it.  Frames are started in the last
// run + 1 iterations of a render (run = renders in a row that continued the previous
// one), so a continued sequence reaches one iteration per render after K renders, and
// a render that is never continued (a moving camera) pays only for one frame's first
// phase ahead.  Renders that collect counters, depths above 63 (the 6-bit flags tags) and
// PUPIL_AHEAD=0 run with K = 1: one frame at a time, D iterations.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace pupil {

// the PUPIL_* knobs of the schedule (engine.hip read_knobs), per engine
struct PipeKnobs {
    // 1 = single-spp renders or the hint pipeline, 2 = every render, 0 = off (PUPIL_AHEAD)
    int ahead_mode = 1;
    uint32_t limit = 0;  // PUPIL_PIPE: most slots (0 = max_depth)
    // PUPIL_PIPE_GB: most HBM bytes for the ring's path state; default a quarter of the
    // device memory free when the engine was created (config 4 needs 9.5 GB, config 5 19 GB
    // of a 288 GB MI355X), so a drop-in pass leaves the rest of a shared device to others
    double budget = 0.0;
    // PUPIL_PIPE_PATHS: a ring needs no more slots than it takes to put this many paths in
    // flight.  Frames ahead pay off by filling the launch tails of small launches; past
    // ~64 M paths per launch the tail is amortised and a larger ring only spreads the
    // traversal's path-state accesses (config 5, 133 M paths per frame: 2288 Mrays/s with
    // one slot, 2208 / 2195 / 2155 / 2093 with 2 / 3 / 4 / 6, profiles/r03_pipe_sweep_config5.txt)
    double paths = 64e6;
    // PUPIL_PIPE_GROUP_PATHS: renders of fewer paths batch G = ceil(this / paths) frames per slot
    double group_paths = 4e6;
    // PUPIL_PIPE_GROUP_MAX: frames per group at most.  The latency bound is the group's paths
    // (PUPIL_PIPE_GROUP_PATHS, 4 M: two 1080p frames), so the heaviest OnRun carries the same
    // work at any tile share (profiles/r06_shard_probe_onrun.txt); 2 caps it at N = 1 sizes too
    uint32_t group_max = 64;
    bool group_all = false;  // PUPIL_PIPE_GROUP_ALL=1: batched renders (spp > 1) group frames too
    bool split = true;       // PUPIL_PIPE_SPLIT=0: whole iterations only (A/B)
    uint32_t ramp = 1;       // PUPIL_PIPE_RAMP: groups one render may start ahead (0 = no limit)
    // renders that start no frame ahead (a moving camera) with at most this many paths run as one
    // persistent launch per frame (pt_frame.hip); PUPIL_FRAME_PATHS, 0 = never.  Moving-camera
    // OnRuns at 1080p (r05 shard probe): one rank of 8 (260 k paths) 7.40 vs 8.47 ms per 8 OnRuns
    // in one launch vs the stage pipeline, one of 4 (518 k) 12.86 vs 10.56, one GPU 39.7 vs 22.8
    double frame_paths = 4e5;
};

// a group of `frames` consecutive frames (seeds seed, seed + spp, ...) in one ring slot
struct PipeFrame {
    uint32_t slot, seed, phases;  // phases = bounces traced + shaded so far (complete at max_depth)
    bool aov_scratch;             // AOVs wait in the slot's scratch until each frame's render
    uint32_t frames, consumed;    // frames in the group; accumulated (rendered) so far
};

// the trace half of an iteration, as its shade half needs it: with frame-group pacing the
// trace half runs at the end of one render and the shade half at the start of the next
struct HalfIter {
    bool had, inject;  // groups were in flight; a group was started
    PipeFrame nf;      // the group started (inject)
    uint32_t nfp;      // its paths
};

// what the schedule takes from one render
struct PipeRender {
    uint32_t spp, seed, depth;
    bool hint;   // PUPIL_HINT_CONTINUE
    bool stats;  // the render collects counters
    size_t paths;
    uint32_t local_pixels;
    uint32_t tiling[5];  // w, h, tile size, rank, world
};

// the ring a render asks for
struct PipePlan {
    PipeRender r;
    bool may_pipe, speculate;
    bool continues;  // the render continues the last one, whose frames in flight are the ones it needs
    uint32_t K, G;   // ring slots, frames per slot
    // a render that starts no frame ahead has none in flight either (speculation is off only
    // right after a reset) and works on slot 0, frame 0: the ring is allocated for frames ahead
    // only once a render speculates, so a camera moving every OnRun runs on the path-state
    // footprint of PUPIL_AHEAD=0.  K and G stay as computed: the pipeline key does not change
    // when speculation starts
    size_t ring_paths() const { return speculate ? (size_t)K * G * r.paths : r.paths; }
    // AOV scratch holds the AOVs of frames shaded ahead of their render (7 floats per local pixel
    // and frame): needed only once a render speculates (frames in flight imply an earlier
    // speculating render allocated it), so a moving camera keeps the footprint of PUPIL_AHEAD=0
    size_t aov_floats() const { return speculate && K * G > 1 ? (size_t)K * G * 7 * r.local_pixels : 0; }
    // after the ring's allocation failed: a smaller ring, down to no frames ahead; false = none
    bool shrink() {
        if (!speculate || K * G <= 1) return false;
        if (K > 1) K = K > 2 ? K / 2 : 1;
        else G = G > 2 ? G / 2 : 1;
        return true;
    }
};

struct PipeRange {
    size_t off, len;  // in paths (= bytes of the flags and bin arrays)
};

struct PipeCommit {
    bool reset;                      // the frames in flight were dropped
    std::vector<PipeRange> dropped;  // their ring ranges: the flags / bin bytes to clear
};

// the list a shade launch walks when it shades from the traced lists
enum class PipeList { All, Next, NextRange };

struct PipeTrace : HalfIter {
    uint32_t samples;      // of the new group per pixel (primary interleave)
    uint32_t base;         // first path of the new group's slot
    uint32_t read_tag;     // (had) the flags tag the last shade wrote
    uint32_t ring_extent;  // (had) the flags partition scans the slots in use: [0, end of the last group)
    bool check_exit;       // (had) read the list lengths back: nothing listed = stop after this half
};

struct PipeShade {
    uint32_t ring_extent, write_tag;
    PipeList list;
    uint32_t max_count;          // paths the launch may list
    uint32_t range_base, range_n;  // the group started in the trace half
    uint32_t range_seed;
    bool aov_scratch;    // its AOVs wait in the scratch, from frame aov_index on
    uint32_t aov_index;
    bool clear_flags;    // depths above 63, K = 1: tags would alias
};

struct PipeFinish {
    uint32_t slot;      // of the group whose next frame this render accumulates
    size_t offset;      // of that frame in the slot, in paths
    bool aov_scratch;   // its AOVs are in the scratch, frame aov_index
    uint32_t aov_index;
    bool trace_ahead;   // run the trace half of the next render's iteration now (trace_ahead())
};

struct PipeState {
    std::vector<PipeFrame> groups;  // in flight, oldest first
    HalfIter half{};
    bool half_pending = false;  // half's shade half is due at the start of the next render
    uint32_t run = 0;           // consecutive renders that continued the previous one
    uint32_t slots = 0;         // K of the ring in use
    size_t np = 0;              // paths per frame
    size_t cap = 0;             // paths per ring slot (G frames)
    uint32_t key[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // w, h, tile size, rank, world, spp, depth, local pixels, G
    uint32_t next_seed = 0;     // random_seed of the render that would continue the last one
    uint32_t gen = 0;           // iterations so far (flags tags)
    bool valid = false;         // nothing the frames in flight depend on changed since the last render
    // the render being scheduled (commit)
    PipeRender r{};
    uint32_t K = 1, G = 1;
    bool speculate = false;
    // depths above 64: every 16 iterations the host reads the list lengths back and stops
    // once no path is left (all of them missed, were absorbed or were terminated by RR)
    bool early_exit = false;
    // a render that starts on an empty pipeline (the first speculating render after a reset: it
    // traces its own frame from the camera rays) starts at most PUPIL_PIPE_RAMP groups ahead;
    // the renders after it fill the ring as before (one group more per iteration they run)
    uint32_t ahead_started = 0;
    bool fresh_start = false;
    uint64_t started = 0;  // camera rays of the groups this render started

    // camera, geometry, emitters or materials changed: the next render does not continue
    void invalidate() { valid = false; }
    // the ring's memory was released
    void ring_lost() {
        groups.clear();
        half_pending = false;
        valid = false;
    }
    // frames started ahead of the next render (in groups: not yet accumulated)
    uint32_t frames_in_flight() const {
        uint32_t n = 0;
        for (const PipeFrame &g : groups) n += g.frames - g.consumed;
        return n;
    }

    PipePlan plan(const PipeKnobs &kn, const PipeRender &rr) const {
        PipePlan p{};
        p.r = rr;
        const uint32_t D = rr.depth;
        const size_t paths = rr.paths;
        p.may_pipe = kn.ahead_mode != 0 && (kn.ahead_mode == 2 || rr.spp == 1 || rr.hint) && !rr.stats && D >= 2 &&
                     D <= 63;  // the 6-bit flags tags of a slot stay unambiguous for 63 iterations
        // frames ahead are started only once a continuation is likely: the caller said so
        // (PUPIL_HINT_CONTINUE), or the last render was continued too.  A render after a change
        // (a camera moving every OnRun) then traces nothing it may discard.
        const bool cont_seed = valid && next_seed == rr.seed;
        p.speculate = rr.hint || kn.ahead_mode == 2 || (cont_seed && run >= 1);
        uint32_t k = 1, g = 1;
        if (p.may_pipe) {
            // frame groups: 1-spp renders (the OnRun cadence) smaller than PUPIL_PIPE_GROUP_PATHS
            // (one rank's tiles, small films) batch G consecutive frames per ring slot, so each
            // traversal launch carries enough rays to amortise its tail; the renders whose frame an
            // earlier render already completed only accumulate it.  Batched renders (spp > 1, the
            // bench's progressive steps) keep one frame per slot (PUPIL_PIPE_GROUP_ALL=1: group them too)
            if (rr.spp == 1 || kn.group_all)
                g = (uint32_t)std::min((double)kn.group_max, std::max(1.0, std::ceil(kn.group_paths / (double)paths)));
            k = kn.limit ? std::min(kn.limit, D) : D;
            constexpr double kPathBytes = 8 * 16 + 2 + 4 + 8 + 1;  // PathState + bins + nxsh + partition scratch
            k = std::min<uint32_t>(k, (uint32_t)std::max(1.0, std::floor(kn.budget / ((double)g * paths * kPathBytes))));
            k = std::min<uint32_t>(k, (uint32_t)std::max(1.0, std::ceil(kn.paths / ((double)g * paths))));
            while (k * g > 1 && (uint64_t)k * g * paths >= (1ull << 31)) {
                if (g > 1) g--;
                else k--;
            }
        }
        p.K = k;
        p.G = g;
        uint32_t want[9];
        fill_key(want, rr, g);
        // this render continues the last one (OnRun cadence: the next seed, nothing changed);
        // frames in flight, if any, are then exactly the ones it and its successors need
        p.continues = cont_seed && k == slots && paths == np && std::memcmp(want, key, sizeof(key)) == 0 &&
                      (groups.empty() || groups.front().seed + groups.front().consumed * rr.spp == rr.seed);
        return p;
    }

    // The plan as allocated (shrunk, if the allocation failed); grew: the ring or the AOV scratch
    // was reallocated, which loses the frames in flight.  A reset caused only by growing (the
    // render continues the last one) keeps the run count, so the render after the first
    // speculating one speculates as well
    PipeCommit commit(const PipePlan &p, bool grew) {
        PipeCommit c;
        c.reset = !p.continues || grew;
        if (c.reset) {
            // the dropped frames' flags / bins bytes are cleared (every other byte of the ring is
            // clear: a completed frame's accumulate clears its own)
            for (const PipeFrame &g : groups) c.dropped.push_back({(size_t)g.slot * cap, (size_t)g.frames * np});
            groups.clear();
            half_pending = false;  // an iteration split over the last render and this one is dropped
            run = p.continues ? run + 1 : 0;
            slots = p.K;
            np = p.r.paths;
            cap = (size_t)p.G * p.r.paths;
            fill_key(key, p.r, p.G);
        } else {
            run++;
        }
        valid = true;
        r = p.r;
        K = p.K;
        G = p.G;
        speculate = p.speculate;
        early_exit = r.depth > 64 && K == 1;
        ahead_started = 0;
        fresh_start = false;
        started = 0;
        return c;
    }

    // a render that starts nothing ahead and needs no frame in flight, small enough (one rank's
    // tiles, small films): the whole frame in one persistent launch (pt_frame.hip), no
    // per-bounce traversal drain, shade launch or partition
    bool one_launch_frame(const PipeKnobs &kn) const {
        return kn.frame_paths > 0.0 && !r.stats && !speculate && groups.empty() && (double)np <= kn.frame_paths;
    }
    void one_launch_frame_done() {
        next_seed = r.seed + r.spp;
        started = np;
    }

    // iterations this render needs: none when an earlier render completed its frame
    uint32_t iterations() const { return groups.empty() ? r.depth : r.depth - groups.front().phases; }

    // One iteration in two halves: (a) start a frame group if due, list the rays the previous
    // shade spawned and trace them (with the new group's camera rays); (b) partition by
    // material, shade.  Frame-group pacing runs (a) at the end of the render before the one
    // that needs the iteration (trace_ahead), (b) at that render's start.
    PipeTrace trace_half(const PipeKnobs &kn, uint32_t it, uint32_t L) { return trace_half(kn, it, L, run); }

    PipeShade shade_half() {
        const HalfIter &h = half;
        half_pending = false;
        PipeShade s{};
        s.ring_extent = ring_end();
        s.write_tag = (gen + 1u) % 63u + 1u;
        s.list = h.had ? (h.inject ? PipeList::NextRange : PipeList::Next) : PipeList::All;
        uint64_t live = 0;
        for (const PipeFrame &g : groups) live += (uint64_t)g.frames * np;
        s.max_count = (uint32_t)std::min<uint64_t>(s.ring_extent, live);
        s.range_base = (uint32_t)(h.nf.slot * cap);
        s.range_n = h.inject ? h.nfp : 0u;
        s.range_seed = h.nf.seed;
        s.aov_scratch = h.inject && h.nf.aov_scratch;  // AOVs of frames ahead wait in their slot's scratch
        s.aov_index = h.nf.slot * G;
        s.clear_flags = r.depth > 63;
        gen++;
        for (PipeFrame &g : groups) g.phases++;
        return s;
    }

    // this render's frame is complete: accumulate it; the group's slot is free once all its
    // frames are accumulated.  L: the iterations the render ran
    PipeFinish finish(const PipeKnobs &kn, uint32_t L) {
        PipeFrame &g = groups.front();
        PipeFinish f{g.slot, (size_t)g.consumed * np, g.aov_scratch, g.slot * G + g.consumed, false};
        if (++g.consumed == g.frames) groups.erase(groups.begin());
        // Frame-group pacing (r06): the render that displays a group's last frame, and would
        // otherwise do no traversal, runs the trace half of the iteration the next render needs;
        // that render starts with the shade half.  With G = 2 the traversal and the shade of every
        // iteration land in different OnRuns (~0.8 / 0.2 of an iteration) instead of one OnRun
        // doing all of it and the next none.  Speculative like the frames ahead: a reset drops it.
        f.trace_ahead = kn.split && speculate && G > 1 && L == 0 && !groups.empty() && groups.front().phases < r.depth;
        next_seed = r.seed + r.spp;
        return f;
    }
    PipeTrace trace_ahead(const PipeKnobs &kn) { return trace_half(kn, 0, r.depth - groups.front().phases, run + 1); }
    // the launches of trace_ahead ran (false: stopped early, nothing to shade)
    void half_ran(bool ok) { half_pending = ok; }

private:
    static void fill_key(uint32_t k[9], const PipeRender &rr, uint32_t g) {
        std::memcpy(k, rr.tiling, sizeof(rr.tiling));
        k[5] = rr.spp, k[6] = rr.depth, k[7] = rr.local_pixels, k[8] = g;
    }
    uint32_t ring_end() const {
        size_t e = 0;
        for (const PipeFrame &g : groups) e = std::max(e, (size_t)g.slot * cap + (size_t)g.frames * np);
        return (uint32_t)e;
    }
    PipeTrace trace_half(const PipeKnobs &kn, uint32_t it, uint32_t L, uint32_t run_) {
        PipeTrace t{};
        t.had = !groups.empty();
        // start a frame group: this render's own on an empty pipeline (one frame unless
        // speculating), else the next one ahead in the last run + 1 iterations while a slot is free
        if (!t.had) fresh_start = true;
        t.inject = !t.had || (speculate && groups.size() < K && it + run_ + 1 >= L &&
                              (kn.ramp == 0 || !fresh_start || ahead_started < kn.ramp));
        if (t.inject && t.had) ahead_started++;
        // a group started on an empty pipeline (the render's own frame: after a reset, the first
        // speculating render) holds one frame when the ramp is limited, so that render traces
        // its own frame and at most PUPIL_PIPE_RAMP groups' first bounces, not G frames' worth
        // (r06 pacing: the heaviest OnRun after the camera stops)
        t.nf = PipeFrame{0u, r.seed, 0u, false, speculate && (t.had || kn.ramp == 0) ? G : 1u, 0u};
        if (t.inject && t.had) {
            t.nf.slot = (groups.back().slot + 1) % K;
            t.nf.seed = groups.back().seed + groups.back().frames * r.spp;
        }
        t.nf.aov_scratch = t.had || t.nf.frames > 1;  // AOVs wait in the slot's scratch until the frame's render
        t.nfp = (uint32_t)(t.nf.frames * np);
        t.samples = t.nf.frames * r.spp;
        t.base = (uint32_t)(t.nf.slot * cap);
        if (t.inject) started += t.nfp;
        if (t.had) {
            t.read_tag = gen % 63u + 1u;
            t.ring_extent = ring_end();
            t.check_exit = early_exit && it % 16 == 0;
        }
        if (t.inject) groups.push_back(t.nf);  // the group is in flight from here (ring_end covers it)
        half = t;
        return t;
    }
};

}  // namespace pupil
