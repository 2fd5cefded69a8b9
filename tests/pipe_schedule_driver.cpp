// Walks host/pipe_schedule.h exactly as engine.hip render_pipelined does -- plan, allocate
// (retrying on OOM), commit, then "ask, launch" -- with prints in place of the launches.
// stdin, one event per line:
//   knobs  ahead limit budget paths group_paths group_max group_all split ramp frame_paths
//   render spp seed hint depth paths local_pixels
//   invalidate            (a camera / scene update before the next render)
//   key rank              (the tiling changes)
//   fail n                (the next n ring allocations fail)
// stdout: one line per decision (tests/test_pipe_schedule_host.py reads them).
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "host/pipe_schedule.h"

using namespace pupil;

int main() {
    PipeKnobs kn;
    PipeState st;
    size_t cap = 0, aov_cap = 0;  // the engine's allocations: ring paths, AOV scratch floats
    uint32_t rank = 0, fails = 0;
    auto alloc = [&](size_t n) {  // ensure_state: releases the ring, then allocates
        st.ring_lost();
        cap = 0;
        if (fails) return fails--, false;
        cap = n;
        return true;
    };
    auto trace = [&](const PipeTrace &t, uint32_t it) {
        std::printf("trace it=%u had=%d inject=%d slot=%u seed=%u frames=%u aov=%d paths=%u samples=%u base=%u rtag=%u extent=%u check=%d\n",
                    it, t.had, t.inject, t.nf.slot, t.nf.seed, t.nf.frames, t.nf.aov_scratch, t.nfp, t.samples, t.base,
                    t.read_tag, t.ring_extent, t.check_exit);
    };
    auto shade = [&](const PipeShade &h) {
        std::printf("shade extent=%u wtag=%u list=%d max=%u base=%u n=%u seed=%u aov=%d idx=%u clear=%d\n", h.ring_extent,
                    h.write_tag, (int)h.list, h.max_count, h.range_base, h.range_n, h.range_seed, h.aov_scratch, h.aov_index,
                    h.clear_flags);
    };
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string ev;
        if (!(in >> ev)) continue;
        if (ev == "knobs") {
            int group_all = 0, split = 1;
            in >> kn.ahead_mode >> kn.limit >> kn.budget >> kn.paths >> kn.group_paths >> kn.group_max >> group_all >>
                split >> kn.ramp >> kn.frame_paths;
            kn.group_all = group_all, kn.split = split;
        } else if (ev == "invalidate") {
            st.invalidate();
        } else if (ev == "key") {
            in >> rank;
        } else if (ev == "fail") {
            in >> fails;
        } else if (ev == "render") {
            PipeRender r{};
            int hint = 0;
            in >> r.spp >> r.seed >> hint >> r.depth >> r.paths >> r.local_pixels;
            r.hint = hint;
            const uint32_t tiling[5] = {48, 32, 16, rank, 4};
            std::memcpy(r.tiling, tiling, sizeof(tiling));
            std::printf("render spp=%u seed=%u hint=%d depth=%u paths=%zu\n", r.spp, r.seed, hint, r.depth, r.paths);
            PipePlan plan = st.plan(kn, r);
            std::printf("plan may_pipe=%d speculate=%d continues=%d K=%u G=%u need=%zu\n", plan.may_pipe, plan.speculate,
                        plan.continues, plan.K, plan.G, plan.ring_paths());
            bool grew = false, ok = true;
            if (plan.ring_paths() > cap) {
                grew = true;
                ok = alloc(plan.ring_paths());
                while (!ok && plan.shrink()) {
                    std::printf("shrink K=%u G=%u need=%zu\n", plan.K, plan.G, plan.ring_paths());
                    ok = alloc(plan.ring_paths());
                }
            }
            if (!ok) {
                std::printf("oom\n");
                continue;
            }
            if (plan.aov_floats() > aov_cap) grew = true, aov_cap = plan.aov_floats();
            const PipeCommit c = st.commit(plan, grew);
            std::printf("commit reset=%d run=%u K=%u G=%u cap=%zu aov_cap=%zu\n", c.reset, st.run, st.K, st.G, cap, aov_cap);
            for (const PipeRange &d : c.dropped) std::printf("drop off=%zu len=%zu\n", d.off, d.len);
            std::printf("shortcut %d\n", st.one_launch_frame(kn));
            if (st.one_launch_frame(kn)) {
                st.one_launch_frame_done();
            } else {
                if (st.half_pending) shade(st.shade_half());
                const uint32_t L = st.iterations();
                std::printf("iters L=%u\n", L);
                for (uint32_t it = 0; it < L; it++) {
                    trace(st.trace_half(kn, it, L), it);
                    shade(st.shade_half());
                }
                const PipeFinish f = st.finish(kn, L);
                std::printf("finish slot=%u offset=%zu aov=%d idx=%u ahead=%d\n", f.slot, f.offset, f.aov_scratch, f.aov_index,
                            f.trace_ahead);
                if (f.trace_ahead) {
                    trace(st.trace_ahead(kn), 0);
                    st.half_ran(true);
                }
            }
            std::printf("state slots=%u in_flight=%u run=%u pending=%d started=%llu groups=", st.slots, st.frames_in_flight(),
                        st.run, st.half_pending, (unsigned long long)st.started);
            for (const PipeFrame &g : st.groups)
                std::printf("%u:%u:%u:%u:%u,", g.slot, g.seed, g.phases, g.frames, g.consumed);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "unknown event %s\n", ev.c_str());
            return 2;
        }
    }
    return 0;
}
