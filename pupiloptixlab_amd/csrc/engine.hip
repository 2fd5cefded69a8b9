// engine.hip — host side of the HIP path tracer and the C ABI (include/pupil_pt.h).
//
// pupil_pt_create  = PTPass::SetScene + World::GetIASHandle + SBT build
//                    (example/path_tracer/pt_pass.cpp:107-209): scene arrays are
//                    copied to engine-owned HBM, materials get the host
//                    precompute of optix_material.cpp:87-119, the LBVH replaces
//                    the GAS/IAS.
// pupil_pt_render  = spp x PTPass::OnRun (pt_pass.cpp:39-57) as one wavefront batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host/emitter_weight.h"
#include "host/instance_record.h"
#include "host/pipe_schedule.h"
#include "host/prim_tables.h"
#include "host/scoped_buffer.h"
#include "pt_accel.h"

namespace {

thread_local std::string g_last_error;

// most event pairs pending at once: a PUPIL_STATS_TRACE_TIMING sequence that is never
// read folds its pairs into sums at this count, a deep timed render stops recording
constexpr uint32_t kMaxPairs = 4096;

using namespace pupil;

// a device array of the engine's, or the scratch of one call: freed with its holder on every path
template <typename T>
using ScratchBuf = ScopedBuffer<T, HipDevice>;
using Event = ScopedHandle<hipEvent_t, HipDevice>;

// src[0 .. count) into a fresh allocation of b
template <typename T>
hipError_t upload(ScratchBuf<T> &b, const T *src, size_t count) {
    hipError_t e = b.alloc(count);
    if (e == hipSuccess && count) e = hipMemcpy(b.get(), src, sizeof(T) * count, hipMemcpyHostToDevice);
    return e;
}

// the arrays of PathState and Queues that are sized by the ring's paths (ensure_state)
struct Ring {
    ScratchBuf<float4> ray_o, ray_d, hit, thr, rad, sh_d, sh_c;
    ScratchBuf<uint4> misc;
    ScratchBuf<uint8_t> mbin, sflags;
    ScratchBuf<uint32_t> bins, nxsh, hist;
};

// what is sized by the instance count, which drop_stale resets whole: the flow pass's previous
// transforms and snapshot table, the device move's staging block, and their host staging copies
struct InstanceScratch {
    ScratchBuf<float> flow_prev, move_stage;
    ScratchBuf<const float *> flow_verts;
    std::vector<float> h_flow_prev, h_move_stage;
    std::vector<const float *> h_flow_verts;
    std::vector<uint32_t> h_move_ids;
    std::vector<uint8_t> h_move_seen;
};

// material bin of a material type (0 is the miss bin, 8 holds every unknown type)
uint32_t material_bin(uint32_t type) { return type >= 1u && type <= 7u ? type : 8u; }

}  // namespace

namespace Pupil {
void set_last_error(const std::string &m) { g_last_error = m; }
}  // namespace Pupil

int pupil::fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

struct pupil_pt {
    // the stream is declared first, so it is destroyed last: every member below frees its device
    // memory and events before it goes
    ScopedHandle<hipStream_t, HipDevice> own_stream;
    int device = 0;
    DeviceScene sc{};
    SceneAccel accel;
    bool primary_interleave = true;  // primary extend dequeues pixel-major (PUPIL_PRIMARY_ORDER)
    bool shade_list = false;  // shade walks the traced list instead of a material partition (PUPIL_SHADE_LIST)
    // list shading: a fresh batch's generate stores only its camera rays, and its bounce-0 shade
    // derives throughput, radiance and RNG (PUPIL_FRESH_SHADE=0: generate stores them all)
    bool fresh_shade = true;
    bool fresh() const { return fresh_shade && shade_list; }
    uint32_t width = 0, height = 0, max_depth = 1;
    // Pipelined frames (render_pipelined, PUPIL_PIPE): the path state is a ring of K slots of one
    // batch each, and consecutive renders that continue each other keep up to K frames in
    // flight.  The schedule, its knobs and its state: host/pipe_schedule.h
    PipeKnobs knobs;
    PipeState pipe;
    bool ring_fresh = true;           // the ring was (re)allocated: its flags bytes are not yet cleared
    uint32_t bin_mask = 0;            // material bins of the scene's instances + the miss bin (partition)
    uint64_t frame_launches = 0;      // renders run as one persistent launch (pt_frame.hip)
    uint64_t ring_bytes = 0;          // path state + queues + AOV scratch allocated now
    ScratchBuf<float> aov_scratch;    // K slots x 7 floats per local pixel
    size_t aov_cap = 0;
    hipStream_t last_stream = nullptr;  // of the last render (NULL = the default stream)
    bool rendered = false;
    // path state / queues (grown on demand)
    size_t cap = 0;
    Ring ring;
    PathState ps{};  // the pointers of `ring`
    Queues q{};      // the pointers of `ring`, q_counts and q_work
    ScratchBuf<uint32_t> q_counts, q_work;
    ScratchBuf<int> ovf;
    uint32_t ovf_threads = 0;
    // pixel map cache
    ScratchBuf<uint32_t> pixel_map;
    uint32_t pm_key[5] = {0, 0, 0, 0, 0};
    uint32_t pm_count = 0;
    // stats
    ScratchBuf<unsigned long long> trace_counters;  // [0] nodes [1] prims
    // device running totals of the extension and shadow rays listed by the flags partitions
    // ([0..1]); the first partition of a render copies them to [2..3] before adding, so the
    // render's own counts are [0..1] - [2..3] without a per-render clear (snap_taken)
    ScratchBuf<unsigned long long> ray_cum;
    bool snap_taken = false;
    // Terminal-ray cull (pt_shade.h terminal_ray_culled; PUPIL_TERMINAL_CULL=0 turns it off,
    // PUPIL_TERMINAL_CULL_K sets the cap on the set).  d_cull: the scan's count, then the set
    // DeviceScene::cull_set points at.  cull_cum: the sharded running total of culled rays, then
    // its copy from the start of the last render, so that render's own count is the difference
    // (cull_counted: some render has run with a set, the copies are being made)
    bool cull_on = true;
    uint32_t cull_k = 8;
    ScratchBuf<uint32_t> d_cull;
    ScratchBuf<unsigned long long> cull_cum;
    bool cull_counted = false;
    uint32_t cull_scanned = 0;  // entries of d_cull the last scan left, sorted (0: no scan holds for the records as they are)
    bool cull_last = false;  // the last counted work was a render (a ray query culls nothing)
    // any-hit rays (shadow rays, any-hit queries) sort a node's children by overlap instead of by
    // distance (pt_traverse.h visit4); PUPIL_SHADOW_ORDER=0: near to far, as before (A/B)
    uint32_t any_overlap = 1;
    uint64_t primary_cum = 0;                      // host running total of camera rays
    uint32_t last_paths = 0, last_iters = 0;
    uint64_t last_primary = 0;
    bool last_stats = false;
    std::vector<Event> trace_events;       // pairs
    std::vector<uint8_t> pair_kind;        // per pair: 0 extend, 1 shadow / mixed traversal, 2 shade, 3 one-launch frame
    // ev_begin / ev_end bracket renders that collect counters or stage times only (each event
    // leaves a few us of stream gap); ev_sync orders another stream after the last render
    Event ev_begin, ev_end, ev_sync;
    bool last_timed = false;  // the last render recorded ev_begin / ev_end
    uint32_t trace_pairs = 0;
    bool pairs_keep = false;  // the pairs of PUPIL_STATS_TRACE_TIMING renders accumulate until read
    // pairs of a PUPIL_STATS_TRACE_TIMING sequence folded into sums once kMaxPairs are pending
    double kept_ms[4] = {0.0, 0.0, 0.0, 0.0};
    uint64_t kept_n[4] = {0, 0, 0, 0};
    // PUPIL_TRACE_TAIL: per-wave start / drained / exit times of each traversal launch of a stats render
    ScratchBuf<unsigned long long> tail_buf;
    uint32_t tail_waves = 0, tail_launches = 0;
    pupil_pt_counters totals{};
    // the instance table, its host mirror and the primitive -> instance tables: their one owner
    // (host/scene_tables.h), and the two names most readers use
    EngineTables tables;
    std::vector<DevInstance> &h_insts() { return tables.cur().mirror; }
    const std::vector<DevInstance> &h_insts() const { return tables.cur().mirror; }
    DevInstance *d_insts() const { return tables.cur().insts.get(); }
    // the materials' one owner (host/material_tables.h); the successful pupil_pt_update_materials /
    // _update_texture_device calls and the host clock around the last one
    EngineMaterials materials;
    uint64_t mat_updates = 0;
    double mat_ms = 0.0;
    // the emitter state's one owner (host/emitter_tables.h); the successful pupil_pt_update_env_* calls
    // and device-side rebuilds, and the host clock around the last one
    EngineEmitters emitters;
    uint64_t env_updates = 0, emit_refreshes = 0;
    double env_ms = 0.0, emit_ms = 0.0;
    // emitter tables rebuilt at a new size (device-side mode: an emissive mesh replaced, the emissive
    // set changed): the successful calls, the last one's triangle and sphere emitters and host clock
    uint64_t emit_resizes = 0;
    uint32_t emit_resize_areas = 0;
    double emit_resize_ms = 0.0;
    // vertex updates (pupil_pt_update_shape_vertices): each shape's engine-owned device arrays
    // and the event that orders a caller's stream before a device-to-device copy (vertices, texels)
    std::vector<ShapeDev> shapes;
    Event ev_verts;
    // flow pass scratch (pupil_pt_motion_vectors), sized on first use: the ray list (2 float4
    // per pixel), the hit list, the previous instance transforms and their host staging copy
    // (per_inst); ev_flow: the upload of that copy has run (the next call may overwrite it)
    ScratchBuf<float4> flow_rays, flow_hits;
    InstanceScratch per_inst;
    Event ev_flow;
    // vertex snapshots (ShapeDev::prev) as the flow pass reads them: per instance the snapshot of
    // its shape or null, uploaded by the first flow pass after the set of snapshots changed
    // (flow_verts_stale; staged like flow_prev, under ev_flow); ev_snap: the last snapshot copy
    // on the engine's stream, which every flow pass waits for while snapshots are held
    uint32_t snapshots = 0;
    bool flow_verts_stale = false;
    Event ev_snap;
    // ray queries (pupil_pt_query_rays / _query_camera).  query_hits: the compact hits of a call that
    // wants resolved outputs but not the hits themselves; grown geometrically, never shrunk
    // (query_cap rays, query_grows growths; the first build of query_slot counts as one).
    // query_slot: flat BVH only, global primitive id -> record slot for the resolve kernel,
    // rebuilt from the records by the first such query after they moved (query_slot_valid is
    // cleared with the cull set's scan).  ev_q0 / ev_q1 bracket the last query on its stream
    ScratchBuf<float4> query_hits;
    size_t query_cap = 0;
    ScratchBuf<uint32_t> query_slot;
    bool query_slot_valid = false;
    uint64_t queries = 0, query_rays = 0, query_grows = 0;
    Event ev_q0, ev_q1;
    // radiance along rays (pupil_pt_radiance_rays): a path state, queues and identity id list of
    // its own, carved from one block (rad_block) of rad_cap paths, which grows geometrically up to
    // rad_chunk (PUPIL_RADIANCE_CHUNK, read at create) and never shrinks.  rad_cum: its own device
    // totals -- the kCullShards sharded counters of the extension rays its terminal-ray cull
    // resolved, each on its own 128-B line as in cull_cum, then (kRadTotals) the extension [0] and
    // shadow [1] rays its flags partitions listed.
    // ev_r0 / ev_r1 bracket the last call on its stream
    size_t rad_chunk = (size_t)1 << 24;
    size_t rad_cap = 0;
    ScratchBuf<char> rad_block;
    PathState rad_ps{};
    Queues rad_q{};
    uint32_t *rad_ids = nullptr;
    static constexpr uint32_t kRadTotals = kCullShards * kCullStride;  // words of rad_cum before the two totals
    ScratchBuf<unsigned long long> rad_cum;
    uint64_t rad_calls = 0, rad_rays = 0, rad_grows = 0;
    Event ev_r0, ev_r1;
    // instances from device memory (pupil_pt_update_instances_device).  per_inst.move_stage: kMoveHeader
    // floats whose first word counts the skipped ids (a running total the kernel adds to), then
    // kMoveStageFloats per list entry (pt_kernels.h MoveInstancesJob), sized for every instance on
    // the first call; the host's copies of the id list and of the block; the totals since create
    // and what the last call launched, synchronised and took
    static constexpr uint32_t kMoveHeader = 8;
    uint64_t inst_dev_updates = 0, inst_dev_moved = 0, inst_dev_skipped = 0;
    uint32_t inst_dev_launches = 0, inst_dev_syncs = 0;
    double inst_dev_ms = 0.0;
    // meshes replaced in place (pupil_pt_replace_shape_mesh): the successful calls and the host
    // clock around the last one
    uint64_t replacements = 0;
    double replace_ms = 0.0;
    // instance tables replaced as a whole (pupil_pt_set_instances): the successful calls, what the
    // last one built and the host clock around it
    uint64_t inst_sets = 0;
    uint32_t inst_set_blas_builds = 0, inst_set_whole = 0;
    double inst_set_ms = 0.0;

    void point_at_ring() {  // ps and q name the arrays `ring` holds now, or none
        ps = PathState{ring.ray_o.get(), ring.ray_d.get(), ring.hit.get(),  ring.thr.get(),  ring.rad.get(),
                       ring.misc.get(),  ring.sh_d.get(),  ring.sh_c.get(), ring.mbin.get(), ring.sflags.get()};
        q.bins = ring.bins.get(), q.nxsh = ring.nxsh.get(), q.hist = ring.hist.get();
    }
    void release_state() {
        ring_bytes = 0;
        ring_fresh = true;
        ring = Ring{};
        point_at_ring();
        cap = 0;
        pipe.ring_lost();
    }
    ~pupil_pt() {
        (void)hipSetDevice(device);  // before any member is destroyed
        accel.free();
    }
};

namespace {

int ensure_state(pupil_pt *pt, size_t n) {
    if (n <= pt->cap) return PUPIL_OK;
    pt->release_state();
    Ring &r = pt->ring;
    hipError_t e = hipSuccess;
    auto take = [&e](auto &b, size_t count) {  // nothing more once one has failed
        if (e == hipSuccess) e = b.alloc(count);
    };
    for (auto *b : {&r.ray_o, &r.ray_d, &r.hit, &r.thr, &r.rad, &r.sh_d, &r.sh_c}) take(*b, n);
    take(r.misc, n), take(r.mbin, n), take(r.sflags, n), take(r.bins, n), take(r.nxsh, 2 * n);
    take(r.hist, partition_hist_entries((uint32_t)n));
    if (e != hipSuccess) pt->release_state();  // a ring that cannot be allocated whole is freed
    HIP_TRY(e);
    pt->point_at_ring();
    pt->q.capacity = (uint32_t)n;
    pt->cap = n;
    pt->ring_bytes = n * (8 * 16 + 2 + 4 + 8) + sizeof(uint32_t) * (size_t)partition_hist_entries((uint32_t)n);
    return PUPIL_OK;
}

// the engine's own stream waits for everything enqueued so far on the stream of the last
// render (which itself waited for the renders before it on other streams)
hipError_t order_after_renders(pupil_pt *pt) {
    if (!pt->rendered || pt->last_stream == pt->own_stream) return hipSuccess;
    hipError_t e = hipEventRecord(pt->ev_sync, pt->last_stream);
    return e == hipSuccess ? hipStreamWaitEvent(pt->own_stream, pt->ev_sync, 0) : e;
}

// the engine's own stream waits for the work enqueued so far on the caller's stream, whose device
// memory a call is about to read; no device-wide sync
hipError_t order_after_caller(pupil_pt *pt, void *hip_stream) {
    hipError_t e = hipEventRecord(pt->ev_verts, (hipStream_t)hip_stream);
    return e == hipSuccess ? hipStreamWaitEvent(pt->own_stream, pt->ev_verts, 0) : e;
}

// Local pixel list of a rank: tiles t with t % world == rank, row-major tile
// order, row-major pixels inside a tile (clipped at the image border).

uint32_t local_pixels(uint32_t w, uint32_t h, uint32_t ts, uint32_t rank, uint32_t world, uint32_t *out) {
    if (world <= 1) {
        if (out)
            for (uint32_t i = 0; i < w * h; i++) out[i] = i;
        return w * h;
    }
    const uint32_t tx = (w + ts - 1) / ts, ty = (h + ts - 1) / ts;
    uint32_t n = 0;
    for (uint32_t t = rank; t < tx * ty; t += world) {
        const uint32_t bx = (t % tx) * ts, by = (t / tx) * ts;
        for (uint32_t y = by; y < by + ts && y < h; y++)
            for (uint32_t x = bx; x < bx + ts && x < w; x++) {
                if (out) out[n] = y * w + x;
                n++;
            }
    }
    return n;
}

// The device pixel map of a tiling (key = w, h, tile size, rank, world), cached per tiling;
// map = null (identity) for tile_world = 1.
int local_pixel_map(pupil_pt *pt, const uint32_t key[5], const uint32_t **map, uint32_t *num_local) {
    *map = nullptr;
    *num_local = pt->width * pt->height;
    if (key[4] <= 1) return PUPIL_OK;
    if (!pt->pixel_map.get() || std::memcmp(key, pt->pm_key, sizeof(pt->pm_key)) != 0) {
        const uint32_t n = local_pixels(pt->width, pt->height, key[2], key[3], key[4], nullptr);
        std::vector<uint32_t> host(n ? n : 1);
        local_pixels(pt->width, pt->height, key[2], key[3], key[4], host.data());
        HIP_TRY(upload(pt->pixel_map, host.data(), host.size()));
        std::memcpy(pt->pm_key, key, sizeof(pt->pm_key));
        pt->pm_count = n;
    }
    *map = pt->pixel_map.get();
    *num_local = pt->pm_count;
    return PUPIL_OK;
}

// inverse of a row-major 4x4 in double (Gauss-Jordan, partial pivoting); false = singular
bool invert4(const float *m, double *inv) {
    double a[4][8];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            a[r][c] = (double)m[4 * r + c];
            a[r][4 + c] = r == c ? 1.0 : 0.0;
        }
    for (int c = 0; c < 4; c++) {
        int piv = c;
        for (int r = c + 1; r < 4; r++)
            if (std::fabs(a[r][c]) > std::fabs(a[piv][c])) piv = r;
        if (!(std::fabs(a[piv][c]) > 0.0)) return false;
        if (piv != c) std::swap_ranges(a[piv], a[piv] + 8, a[c]);
        const double s = 1.0 / a[c][c];
        for (int k = 0; k < 8; k++) a[c][k] *= s;
        for (int r = 0; r < 4; r++) {
            if (r == c) continue;
            const double f = a[r][c];
            for (int k = 0; k < 8; k++) a[r][k] -= f * a[c][k];
        }
    }
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) inv[4 * r + c] = a[r][4 + c];
    return true;
}

// ------------------------------------------------------------------ frame schedules
// Shared state of one pupil_pt_render call.
struct RenderCtx {
    pupil_pt *pt;
    hipStream_t s;
    bool stats, timing;
    TraceStats ts_dev;
    const uint32_t *key;  // w, h, tile size, rank, world
    bool tail = false;
    bool trace_only = false;  // PUPIL_STATS_TRACE_TIMING: traversal launches only
    uint32_t pair = 0;
    bool open = false;
    const TraceStats *tsp() const { return stats ? &ts_dev : nullptr; }
    // stage events only on request: each hipEventRecord between two kernels costs
    // ~6 us of stream gap (9 per 1-spp render at D = 4)
    uint32_t pair_cap = 0;  // events created for this render
    void ev0(uint8_t kind) {
        open = timing && !(trace_only && kind == 2) && pair < pair_cap;
        if (!open) return;
        pt->pair_kind[pair] = kind;
        (void)hipEventRecord(pt->trace_events[2 * pair], s);
    }
    void ev1() {
        if (!open) return;
        (void)hipEventRecord(pt->trace_events[2 * pair + 1], s);
        pair++;
        open = false;
    }
    void tail_slot() {  // wave-time slice of the next traversal launch (PUPIL_TRACE_TAIL)
        if (tail && pt->tail_launches < kMaxDepth + 1)
            ts_dev.wave_times = pt->tail_buf.get() + (size_t)pt->tail_launches++ * pt->tail_waves * 4;
        else
            ts_dev.wave_times = nullptr;
    }
    // path state of ring slot h: every array offset by h * paths
    PathState view(uint32_t h, size_t paths, size_t extra = 0) const {
        PathState v = pt->ps;
        const size_t o = (size_t)h * paths + extra;
        v.ray_o += o, v.ray_d += o, v.hit += o, v.thr += o, v.rad += o, v.misc += o;
        v.sh_d += o, v.sh_c += o, v.mbin += o, v.sflags += o;
        return v;
    }
};

// Pipelined frames: the launches.  host/pipe_schedule.h decides what a render does -- the ring it
// needs, whether it continues the last render, which frame group starts in which iteration --
// and this function allocates, clears and launches what it is told.  Per path, every operation
// and its order are those of the reference's per-pixel loop (main.cu:84-193): output is
// bit-identical to the oracle whatever the schedule.
int render_pipelined(RenderCtx &cx, const FrameParams &fp, const pupil_pt_launch *launch) {
    pupil_pt *pt = cx.pt;
    hipStream_t s = cx.s;
    PipeState &st = pt->pipe;
    const PipeKnobs &kn = pt->knobs;
    const uint32_t nl = fp.num_local;
    const PipeRender r{fp.spp, launch->random_seed, fp.max_depth, (launch->hints & PUPIL_HINT_CONTINUE) != 0, cx.stats,
                       fp.num_paths, nl, {cx.key[0], cx.key[1], cx.key[2], cx.key[3], cx.key[4]}};
    PipePlan plan = st.plan(kn, r);
    bool grew = false;
    if (plan.ring_paths() > pt->cap) {  // growing the ring loses its contents
        grew = true;
        int rc = ensure_state(pt, plan.ring_paths());
        while (rc == PUPIL_ERR_OOM && plan.shrink()) rc = ensure_state(pt, plan.ring_paths());
        if (rc) return rc;
    }
    if (plan.aov_floats() > pt->aov_cap) {
        grew = true;
        pt->aov_cap = 0;
        HIP_TRY(pt->aov_scratch.alloc(plan.aov_floats()));
        pt->aov_cap = plan.aov_floats();
    }
    const PathState ring = pt->ps;
    const PipeCommit commit = st.commit(plan, grew);
    for (const PipeRange &d : commit.dropped) {
        if (d.off + d.len > pt->cap) continue;
        HIP_TRY(hipMemsetAsync(ring.sflags + d.off, 0, d.len, s));
        if (!pt->shade_list) HIP_TRY(hipMemsetAsync(ring.mbin + d.off, 0xFF, d.len, s));
    }
    if (commit.reset && pt->ring_fresh) {  // a new allocation: everything
        HIP_TRY(hipMemsetAsync(ring.sflags, 0, pt->cap, s));
        if (!pt->shade_list) HIP_TRY(hipMemsetAsync(ring.mbin, 0xFF, pt->cap, s));
        pt->ring_fresh = false;
    }
    Queues &q = pt->q;
    const uint32_t interleave0 = pt->primary_interleave;
    if (st.one_launch_frame(kn) && frame_kernel_supported(pt->sc)) {
        // this render's extension / shadow rays = the growth of the running totals from here
        HIP_TRY(hipMemcpyAsync(pt->ray_cum.get() + 2, pt->ray_cum.get(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
        pt->snap_taken = true;
        FrameParams fs = fp;
        fs.group = 1;
        cx.ev0(3);  // traversal and shading in one kernel: timed apart from trace_ms (frame_ms)
        launch_frame(pt->sc, fs, ring, pt->q.work + kWorkFrame, pt->ray_cum.get(), pt->ovf.get(), pt->ovf_threads,
                     interleave0 && fp.spp > 1 ? fp.spp : 0u, s);
        cx.ev1();
        launch_accumulate(fp, ring, nullptr, true, s);
        st.one_launch_frame_done();
        pt->last_iters = fp.max_depth;
        pt->last_primary = st.started;
        pt->primary_cum += st.started;
        pt->frame_launches++;
        return PUPIL_OK;
    }
    // AOV scratch of frame `index` of the ring (slot-major): 7 floats per local pixel
    auto scratch = [&](uint32_t index) { return pt->aov_scratch.get() + (size_t)index * 7 * nl; };
    pt->snap_taken = false;
    // 1 = an early-exit check found nothing left to trace or shade: the frame is complete
    auto trace = [&](const PipeTrace &t) -> int {
        const uint32_t interleave = interleave0 && t.samples > 1 ? t.samples : 0u;
        if (t.inject) {
            FrameParams fg = fp;
            fg.seed0 = t.nf.seed;
            fg.num_paths = t.nfp;
            launch_generate(pt->sc, fg, cx.view(t.nf.slot, st.cap), s, !pt->fresh());
        }
        if (t.had) {
            // the rays the previous iteration's shade spawned, over the slots in use, in
            // increasing path id: next (bit 0) and shadow (bit 1) lists -> q.nxsh
            launch_partition(ring.sflags, t.ring_extent, 2, kPartFlags, t.read_tag, q.nxsh, q.hist, q.counts + kCntNext,
                             q.counts + kStartNext, nullptr, nullptr, s, pt->ray_cum.get(),
                             pt->snap_taken ? nullptr : pt->ray_cum.get() + 2);
            pt->snap_taken = true;
            if (t.check_exit) {
                uint32_t c[2] = {1, 1};
                HIP_TRY(hipMemcpyAsync(c, q.counts + kCntNext, sizeof(c), hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                if (c[0] == 0 && c[1] == 0) return 1;
            }
            cx.ev0(1);
            cx.tail_slot();
            if (t.inject)  // + the new group's camera rays, dequeued first in every chunk (pixel-major)
                launch_trace_mixed(pt->sc, ring, q, pt->ovf.get(), pt->ovf_threads, cx.tsp(), s, t.nfp, 0u, t.base, interleave, nl,
                                   pt->any_overlap);
            else
                launch_trace_mixed(pt->sc, ring, q, pt->ovf.get(), pt->ovf_threads, cx.tsp(), s, 0u, 0u, 0u, 0u, 0u, pt->any_overlap);
            cx.ev1();
        } else {
            cx.ev0(0);
            cx.tail_slot();
            launch_extend(pt->sc, cx.view(t.nf.slot, st.cap), q, nullptr, nullptr, t.nfp, pt->ovf.get(), pt->ovf_threads,
                          cx.tsp(), s, interleave, nl);
            cx.ev1();
        }
        return 0;
    };
    auto shade = [&](const PipeShade &h) -> int {
        if (!pt->shade_list)  // material bins of every path traced in this iteration -> q.bins
            launch_partition(ring.mbin, h.ring_extent, kPartMaxBins, kPartExclusive, 0u, q.bins, q.hist, q.counts,
                             q.counts + kStartBins, q.counts + kScratch, nullptr, s, nullptr, nullptr, pt->bin_mask);
        FrameParams fs = fp;
        fs.group = st.G;  // AOV frame of a sample: its group frame (samples per ring slot = G spp)
        if (h.aov_scratch) {
            fs.albedo = scratch(h.aov_index);
            fs.normal = fs.albedo + 3 * (size_t)nl;
            fs.test = fs.albedo + 6 * (size_t)nl;
            fs.aov_local = 1;
            fs.aov_frame_stride = (uint32_t)(7 * nl);
        }
        if (h.clear_flags) HIP_TRY(hipMemsetAsync(ring.sflags, 0, h.ring_extent, s));
        constexpr ShadeList kLists[] = {kShadeAll, kShadeNext, kShadeNextRange};
        const ShadeList list = pt->shade_list ? kLists[(int)h.list] : kShadeBins;
        cx.ev0(2);
        launch_shade(pt->sc, fs, ring, q, h.write_tag, s, list, h.range_base, h.range_n, h.max_count, pt->fresh(),
                     h.range_seed);
        cx.ev1();
        return 0;
    };
    // the shade half of an iteration whose trace half the previous render ran (a reset dropped
    // it with the frames it belonged to)
    if (st.half_pending)
        if (const int rc = shade(st.shade_half())) return rc;
    const uint32_t L = st.iterations();
    for (uint32_t it = 0; it < L; it++) {
        const int rc = trace(st.trace_half(kn, it, L));
        if (rc == 1) break;  // depth > 64: nothing left
        if (rc) return rc;
        if (const int rs = shade(st.shade_half())) return rs;
    }
    // (the accumulate clears the frame's flags bytes: no stale tag is ever listed again)
    const PipeFinish fin = st.finish(kn, L);
    launch_accumulate(fp, cx.view(fin.slot, st.cap, fin.offset), fin.aov_scratch ? scratch(fin.aov_index) : nullptr, true, s);
    if (fin.trace_ahead) {
        const int rc = trace(st.trace_ahead(kn));
        if (rc < 0) return rc;
        st.half_ran(rc == 0);
    }
    pt->last_iters = L;
    pt->last_primary = st.started;
    pt->primary_cum += st.started;
    return PUPIL_OK;
}

// ------------------------------------------------------------------ pupil_pt_create, step by step
// (each returns an ABI code; create frees the engine when one fails)

// shapes: validated, their arrays copied to engine-owned HBM
int upload_shapes(pupil_pt *pt, const pupil_scene_desc *scene) {
    std::vector<ShapeDev> &shapes = pt->shapes;
    shapes = std::vector<ShapeDev>(scene->num_shapes);
    for (uint32_t s = 0; s < scene->num_shapes; s++) {
        const pupil_shape &sh = scene->shapes[s];
        shapes[s].kind = sh.kind;
        shapes[s].num_vertices = sh.num_vertices;
        shapes[s].num_faces = sh.num_faces;
        if (sh.kind == PUPIL_SHAPE_MESH) {
            if (!sh.positions || !sh.indices || sh.num_faces == 0)
                return fail(PUPIL_ERR_INVALID, "mesh without positions/indices");
            for (size_t i = 0; i < 3 * (size_t)sh.num_faces; i++)
                if (sh.indices[i] >= sh.num_vertices) return fail(PUPIL_ERR_INVALID, "index out of range");
            if (upload(shapes[s].pos, sh.positions, 3 * (size_t)sh.num_vertices) ||
                (sh.normals && upload(shapes[s].nrm, sh.normals, 3 * (size_t)sh.num_vertices)) ||
                (sh.texcoords && upload(shapes[s].tex, sh.texcoords, 2 * (size_t)sh.num_vertices)) ||
                upload(shapes[s].idx, sh.indices, 3 * (size_t)sh.num_faces))
                return fail(PUPIL_ERR_OOM, "mesh upload failed");
        } else if (sh.kind != PUPIL_SHAPE_SPHERE) {
            return fail(PUPIL_ERR_INVALID, "unknown shape kind");
        }
    }
    return PUPIL_OK;
}

// The scene's instances, validated, as the first generation of the tables -- staged and adopted
// as an update's are (host/scene_tables.h), the records by fill_instance_record.
int upload_tables(pupil_pt *pt, const pupil_scene_desc *scene) {
    const std::vector<DevMaterial> &mats = pt->materials.mirror();
    const uint32_t n = scene->num_instances;
    // an instance's emitter range lies within the triangle and sphere emitters: the delta lights
    // behind them belong to no primitive
    uint32_t true_areas = 0;
    if (scene->area_emitters)
        for (uint32_t e = 0; e < scene->num_area_emitters; e++) {
            const uint32_t t = scene->area_emitters[e].type;
            true_areas += t >= PUPIL_EMITTER_POINT && t <= PUPIL_EMITTER_DIRECTIONAL ? 0u : 1u;
        }
    std::vector<uint32_t> counts(n);
    for (uint32_t i = 0; i < n; i++) {
        const pupil_instance &src = scene->instances[i];
        if (src.shape >= scene->num_shapes) return fail(PUPIL_ERR_INVALID, "instance shape out of range");
        if (src.material >= mats.size()) return fail(PUPIL_ERR_INVALID, "instance material out of range");
        const pupil_shape &sh = scene->shapes[src.shape];
        counts[i] = sh.kind == PUPIL_SHAPE_SPHERE ? 1u : sh.num_faces;
        if (src.emitter_offset >= 0 && (size_t)src.emitter_offset + counts[i] > true_areas)
            return fail(PUPIL_ERR_INVALID, "emitter offset out of range");
    }
    hipStream_t s = pt->own_stream;
    EngineTables::Generation gen;
    // the flattened BVH's limit: SceneAccel::build, which chooses the mode
    if (const int rc = EngineTables::stage(counts.data(), n, false, s, gen)) return drained(s, rc);
    for (uint32_t i = 0; i < n; i++) {
        const pupil_instance &src = scene->instances[i];
        const ShapeDev &sd = pt->shapes[src.shape];
        const InstShape shape{scene->shapes[src.shape].kind, counts[i], sd.pos.get(), sd.nrm.get(), sd.tex.get(), sd.idx.get()};
        const InstBinding bind{src.shape,          src.material, src.flip_normals, src.flip_tex_coords,
                               src.emitter_offset, 0u,           material_bin(mats[src.material].type)};
        fill_instance_record(gen.mirror[i], shape, bind, gen.first[i], src.to_world, src.to_object, false);
    }
    HIP_TRY_DRAINED(s, hipGetLastError());
    HIP_TRY_DRAINED(s, hipMemcpyAsync(gen.insts.get(), gen.mirror.data(), sizeof(DevInstance) * n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    pt->tables.adopt(std::move(gen), pt->sc, pt->totals);
    return PUPIL_OK;
}

// What the shading schedule takes from the instances' material bins: one bin in the whole scene
// and the material partition orders nothing (shade_list: auto; PUPIL_SHADE_LIST=bins / =list
// force), single_bin names it, bin_mask the bins a path can land in.  At create, and again when
// pupil_pt_update_materials moved an instance to another bin
void derive_bins(pupil_pt *pt) {
    DeviceScene &sc = pt->sc;
    const bool was_list = pt->shade_list;
    const uint32_t was_single = sc.single_bin;
    uint32_t bins = 0;
    for (const DevInstance &d : pt->h_insts()) bins |= 1u << d.bin;
    pt->shade_list = (bins & (bins - 1u)) == 0u;
    if (const char *sl = std::getenv("PUPIL_SHADE_LIST")) {
        if (std::strcmp(sl, "bins") == 0) pt->shade_list = false;
        if (std::strcmp(sl, "list") == 0) pt->shade_list = true;
    }
    sc.single_bin = pt->shade_list && bins && (bins & (bins - 1u)) == 0u ? (uint32_t)__builtin_ctz(bins) : 0u;
    pt->bin_mask = bins | 1u;  // the material bins a traced path can land in, and the miss bin
    // the ring's bin bytes are 0xFF for untraced paths only while the bins schedule keeps them so:
    // after a change the next render clears the whole ring, as after an allocation
    if (pt->shade_list != was_list || sc.single_bin != was_single) pt->ring_fresh = true;
}

// the PUPIL_* knobs of the render schedule and their defaults; after the structure is built (the
// ring budget is what is free then)
void read_knobs(pupil_pt *pt) {
    DeviceScene &sc = pt->sc;
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, pt->device);
    sc.num_cus = (uint32_t)std::max(1, cus);
    // persistent BVH4 kernels: refill once 16 lanes are idle (r02 re-tune on the SAH tree:
    // 16 / 12 beat 20 / 24 by ~0.7 % at N = 1 and the 8-way shard)
    sc.trace_refill = 16;
    if (const char *r = std::getenv("PUPIL_REFILL")) sc.trace_refill = (uint32_t)std::min(64, std::max(1, std::atoi(r)));
    if (const char *po = std::getenv("PUPIL_PRIMARY_ORDER")) pt->primary_interleave = std::strcmp(po, "path") != 0;
    derive_bins(pt);
    if (const char *fr = std::getenv("PUPIL_FRESH_SHADE")) pt->fresh_shade = std::atoi(fr) != 0;
    if (const char *tc = std::getenv("PUPIL_TERMINAL_CULL")) pt->cull_on = std::atoi(tc) != 0;
    if (const char *g = std::getenv("PUPIL_SHADOW_ORDER")) pt->any_overlap = std::atoi(g) != 0 ? 1u : 0u;
    if (const char *tk = std::getenv("PUPIL_TERMINAL_CULL_K"))
        pt->cull_k = (uint32_t)std::min((int)kCullSetMax, std::max(1, std::atoi(tk)));
    if (const char *a = std::getenv("PUPIL_AHEAD")) pt->knobs.ahead_mode = std::min(2, std::max(0, std::atoi(a)));
    if (const char *k = std::getenv("PUPIL_PIPE")) pt->knobs.limit = (uint32_t)std::min(63, std::max(0, std::atoi(k)));
    {  // ring budget: a quarter of the device memory free now (after the scene and its BVH)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
        pt->knobs.budget = 0.25 * (double)free_b;
    }
    if (const char *g = std::getenv("PUPIL_PIPE_GB")) pt->knobs.budget = std::max(0.0, std::atof(g)) * 1e9;
    if (const char *g = std::getenv("PUPIL_PIPE_PATHS")) pt->knobs.paths = std::max(1.0, std::atof(g));
    if (const char *g = std::getenv("PUPIL_PIPE_GROUP_PATHS")) pt->knobs.group_paths = std::max(1.0, std::atof(g));
    if (const char *g = std::getenv("PUPIL_PIPE_GROUP_MAX")) pt->knobs.group_max = (uint32_t)std::min(64, std::max(1, std::atoi(g)));
    if (const char *g = std::getenv("PUPIL_PIPE_GROUP_ALL")) pt->knobs.group_all = std::atoi(g) != 0;
    if (const char *g = std::getenv("PUPIL_PIPE_SPLIT")) pt->knobs.split = std::atoi(g) != 0;
    if (const char *g = std::getenv("PUPIL_PIPE_RAMP")) pt->knobs.ramp = (uint32_t)std::max(0, std::atoi(g));
    if (const char *g = std::getenv("PUPIL_FRAME_PATHS")) pt->knobs.frame_paths = std::max(0.0, std::atof(g));
    // most paths of one chunk of pupil_pt_radiance_rays, which bounds its scratch (at least a wave)
    if (const char *g = std::getenv("PUPIL_RADIANCE_CHUNK"))
        pt->rad_chunk = (size_t)std::min(2147483647.0, std::max(64.0, std::atof(g)));
    sc.shade_max_blocks = kShadeMaxBlocks;
    if (const char *g = std::getenv("PUPIL_SHADE_MAX_BLOCKS"))
        sc.shade_max_blocks = (uint32_t)std::min(1 << 20, std::max(64, std::atoi(g)));
    sc.trace_node_min = 8;  // node phase ends below 8 active lanes (7 waves: 8 and 12 beat 4 by 1.5 %; 2 is slower)
    if (const char *r = std::getenv("PUPIL_NODE_MIN")) sc.trace_node_min = (uint32_t)std::min(64, std::max(1, std::atoi(r)));
}

// traversal overflow stacks, counters, events
int alloc_workspace(pupil_pt *pt) {
    pt->ovf_threads = trace_grid_blocks() * (uint32_t)kTraceBlock;
    if (pt->ovf.alloc((size_t)pt->ovf_threads * kStackOvf) || pt->trace_counters.alloc(32) || pt->ray_cum.alloc(4) ||
        pt->q_counts.alloc(kCountSlots) || pt->q_work.alloc(kWorkSlots) || pt->d_cull.alloc(1 + kCullSetMax) ||
        pt->cull_cum.alloc(2 * kCullShards * kCullStride) || pt->rad_cum.alloc(pupil_pt::kRadTotals + 2))
        return fail(PUPIL_ERR_OOM, "workspace allocation failed");
    pt->q.counts = pt->q_counts.get(), pt->q.work = pt->q_work.get();
    if (hipMemset(pt->q.work, 0, kWorkSlots * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(pt->rad_cum.get(), 0, (pupil_pt::kRadTotals + 2) * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(pt->cull_cum.get(), 0, 2 * kCullShards * kCullStride * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(pt->ray_cum.get(), 0, 4 * sizeof(unsigned long long)) != hipSuccess)
        return fail(PUPIL_ERR_HIP, "workspace clear failed");
    if (hipEventCreate(pt->ev_begin.put()) != hipSuccess || hipEventCreate(pt->ev_end.put()) != hipSuccess ||
        hipEventCreateWithFlags(pt->ev_sync.put(), hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(pt->ev_verts.put(), hipEventDisableTiming) != hipSuccess)
        return fail(PUPIL_ERR_HIP, "event creation failed");
    return PUPIL_OK;
}

// Drops what a change of the records or of the tables has outdated; its next user scans or
// allocates anew.  Always (the records moved): the cull set's scan and the content of the query
// slot map, which name record slots.  tables (the swap of an update that resized them): the slot
// map itself, sized by the primitive count, and the vertex snapshot of the shape that was
// `replaced`, sized by its old vertex count -- the flow pass sees none.  instances: the instance
// count changed too, which sized the flow scratch and the device move's staging block.
void drop_stale(pupil_pt *pt, bool tables = false, bool instances = false, const ShapeDev *replaced = nullptr) {
    pt->cull_scanned = 0;
    pt->query_slot_valid = false;
    if (!tables) return;
    pt->query_slot.reset();
    if (replaced && replaced->prev_valid) {  // the snapshot itself goes with the replaced value
        pt->snapshots--;
        pt->flow_verts_stale = true;
    }
    if (!instances) return;
    pt->per_inst = InstanceScratch{};
    pt->flow_verts_stale = true;
}

// ------------------------------------------------------------------ terminal-ray cull set
// DeviceScene::cull_set from the structure and the tables as they are now: the record slots of
// every primitive of an instance that carries emitters, found by a scan of the traversal's own
// world-space records (a refit keeps them, a rebuild moves them) and sorted.  Called whenever the
// structure, an instance, the materials or the emitter tables change, on the engine's stream,
// which the caller has ordered after the renders; returns when the set is written.
// records_changed = false (material and emitter-table updates, which move no record and change no
// instance's emitter range): only whether the scene may have a set is decided anew, and the last
// scan is reused while it holds -- no pass over the records, no synchronisation.  No set (every
// extension ray is traced, as before the cull existed) when the knob is off, the scene has an env
// emitter (a terminal miss adds radiance), the traversal reads object-space records (two-level
// object mode) or the emissive primitives number more than the cap (emissive meshes).  An
// emitter of zero radiance stays in the set: its hit still multiplies the path's throughput by
// that zero (inf * 0), which only the shade itself restates.  The delta lights of the emitter
// table play no part: the count below is of primitives, taken from the instances, and a point,
// spot or directional light is none -- no ray hits it, so it adds nothing to a terminal ray's
// shade.  A scene lit by delta lights alone therefore has no set (and traces every ray).
int derive_cull_set(pupil_pt *pt, bool records_changed = true) {
    DeviceScene &sc = pt->sc;
    sc.cull_set = pt->d_cull.get() + 1;
    sc.cull_n = 0;
    if (records_changed) drop_stale(pt);
    if (!pt->cull_on || sc.has_env || !sc.prims || (sc.two_level && !sc.tl_world)) return PUPIL_OK;
    uint64_t emissive = 0;  // primitives: a mesh instance's faces, a sphere
    for (size_t i = 0; i < pt->h_insts().size(); i++) {
        const DevInstance &d = pt->h_insts()[i];
        if (d.emitter_offset < 0) continue;
        emissive += d.kind == PUPIL_SHAPE_MESH ? pt->shapes[pt->accel.inst_shape[i]].num_faces : 1u;
    }
    if (emissive == 0 || emissive > pt->cull_k) return PUPIL_OK;
    if (pt->cull_scanned == emissive) {  // the records have not moved since the scan
        sc.cull_n = pt->cull_scanned;
        return PUPIL_OK;
    }
    uint32_t found[1 + kCullSetMax] = {};
    HIP_TRY(hipMemsetAsync(pt->d_cull.get(), 0, sizeof(found), pt->own_stream));
    launch_cull_scan(sc.prims, pt->accel.world_record_slots(), pt->d_insts(), (uint32_t)pt->h_insts().size(), pt->d_cull.get(),
                     kCullSetMax, pt->own_stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(found, pt->d_cull.get(), sizeof(found), hipMemcpyDeviceToHost, pt->own_stream));
    HIP_TRY(hipStreamSynchronize(pt->own_stream));
    pt->accel.counts.launches++, pt->accel.counts.syncs++;  // pupil_pt_instances_device_info
    if (found[0] != emissive) return PUPIL_OK;  // the records do not show what the tables say: no set
    std::sort(found + 1, found + 1 + found[0]);
    HIP_TRY(hipMemcpyAsync(pt->d_cull.get(), found, sizeof(found), hipMemcpyHostToDevice, pt->own_stream));
    HIP_TRY(hipStreamSynchronize(pt->own_stream));
    pt->accel.counts.syncs++;
    sc.cull_n = pt->cull_scanned = found[0];
    return PUPIL_OK;
}

// ------------------------------------------------------------------ device-side emitter table
// What pupil_pt_enable_device_emitters takes from a scene: it must describe the engine's
// instances and emitter ranges, and gives each emissive instance's select weight.  Fills
// emit_inst (per emitter) and inst_weight (per instance); changes nothing of the engine.
int device_emitter_tables(const pupil_pt *pt, const pupil_scene_desc *scene, std::vector<uint32_t> &emit_inst,
                          std::vector<float> &inst_weight) {
    // ne: the triangle and sphere emitters, which the ranges must cover; the delta lights behind
    // them (the rebuild leaves them as they are) must be the engine's, type for type
    const uint32_t ni = (uint32_t)pt->h_insts().size(), ne = pt->emitters.cur().num_true_areas;
    if (scene->num_instances != ni) return fail(PUPIL_ERR_INVALID, "the scene's instance count is not the engine's");
    if (scene->num_area_emitters != pt->sc.num_areas)
        return fail(PUPIL_ERR_INVALID, "the scene's area emitter count is not the engine's");
    if ((ni && !scene->instances) || (pt->sc.num_areas && !scene->area_emitters))
        return fail(PUPIL_ERR_INVALID, "missing scene array");
    for (uint32_t e = 0; e < pt->sc.num_areas; e++) {
        const uint32_t t = scene->area_emitters[e].type;
        const bool delta = t >= PUPIL_EMITTER_POINT && t <= PUPIL_EMITTER_DIRECTIONAL;
        if (delta != (e >= ne) || (delta && t != pt->emitters.cur().types[e]))
            return fail(PUPIL_ERR_INVALID, "the scene's delta lights are not the engine's");
    }
    emit_inst.assign(ne, 0u);
    inst_weight.assign(ni, 0.f);
    uint32_t next = 0;  // emitter ranges follow each other in instance order (World::Build)
    for (uint32_t i = 0; i < ni; i++) {
        const DevInstance &d = pt->h_insts()[i];
        if (scene->instances[i].emitter_offset != d.emitter_offset)
            return fail(PUPIL_ERR_INVALID, "an instance's emitter_offset is not the engine's");
        if (d.emitter_offset < 0) continue;
        const uint32_t range = d.kind == PUPIL_SHAPE_MESH ? pt->shapes[pt->accel.inst_shape[i]].num_faces : 1u;
        if ((uint32_t)d.emitter_offset != next || range > ne - next)
            return fail(PUPIL_ERR_INVALID, "an emissive instance's emitter range is not its face count");
        inst_weight[i] = Pupil::world::GetWeight(scene->area_emitters[next].radiance);
        for (uint32_t k = 0; k < range; k++) emit_inst[next + k] = i;
        next += range;
    }
    if (next != ne) return fail(PUPIL_ERR_INVALID, "the emitter ranges do not cover the emitter table");
    return PUPIL_OK;
}

// validates `scene` against the engine, then stages the bookkeeping aside (synchronous copies into
// fresh arrays) and adopts it; after a refusal or failure the bookkeeping and the mode are what they were
int device_emitter_setup(pupil_pt *pt, const pupil_scene_desc *scene) {
    std::vector<uint32_t> emit_inst;
    std::vector<float> inst_weight;
    if (const int rc = device_emitter_tables(pt, scene, emit_inst, inst_weight)) return rc;
    // sized for the whole table: the select scratch and the CDF chain span the delta lights too
    EngineEmitters::Bookkeeping staged;
    staged.enabled = pt->emitters.book().enabled;
    const int rc = EngineEmitters::Bookkeeping::stage(std::move(emit_inst), std::move(inst_weight), pt->sc.num_areas, staged);
    if (!rc) pt->emitters.book() = std::move(staged);
    return rc;
}

// the rebuild (pt_emitters.hip) on the engine's stream, which the caller has ordered after the
// renders; returns when the table is written
int rebuild_emitters(pupil_pt *pt) {
    const auto t0 = std::chrono::steady_clock::now();
    EmitterJob job{};
    const EngineEmitters::Generation &g = pt->emitters.cur();
    const EngineEmitters::Bookkeeping &book = pt->emitters.book();
    job.areas = g.areas.get();
    job.cdf = g.cdf.get();
    job.guide = g.guide.get();
    job.guide_bits = g.guide_bits;
    job.count = g.num_true_areas;
    job.total = pt->sc.num_areas;
    job.emitter_num = pt->sc.num_areas + (pt->sc.has_env ? 1u : 0u);
    job.instances = pt->d_insts();
    job.emit_inst = book.emit_inst.get();
    job.inst_weight = book.inst_weight.get();
    job.weight = book.weight.get();
    job.select = book.select.get();
    job.sum = book.sum.get();
    const uint32_t launches = launch_emitter_rebuild(job, pt->own_stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(pt->own_stream));
    // the stages launch_emitter_rebuild ran (four and the guide's; over delta lights alone, two and the
    // guide's; an empty table, none), one synchronisation: pupil_pt_instances_device_info
    pt->accel.counts.launches += launches;
    pt->accel.counts.syncs++;
    pt->emit_refreshes++;
    pt->emit_ms = ms_since(t0);
    return derive_cull_set(pt, false);
}

// pupil_pt_update_emitters replaced the table: the device-side mode stays on when the new scene
// still describes the engine's emitter ranges (its radiance weights are taken anew), else it goes
// off and pupil_last_error says so; the update itself has succeeded either way
int keep_device_emitters(pupil_pt *pt, const pupil_scene_desc *scene) {
    if (!pt->emitters.book().enabled) return PUPIL_OK;
    if (device_emitter_setup(pt, scene) != PUPIL_OK) {
        pt->emitters.book().enabled = false;
        g_last_error = "device-side emitter table switched off: " + g_last_error;
    }
    return PUPIL_OK;
}

// A staged, resized emitter table (EmitterTables::stage_resize) filled on the stream from `insts`,
// the staged instance table it belongs to, which the stream has filled: k_emit_fill writes the
// records and emit_inst, the five stages everything derived.  Returns once the stream has passed
// them, so a failure shows before anything is swapped.  Nothing the engine reads is touched.
int fill_resized_emitters(pupil_pt *pt, const EngineEmitters::Resize &r, const DevInstance *insts, hipStream_t s) {
    const EngineEmitters::Generation &g = r.gen;
    const uint32_t total = (uint32_t)g.types.size();
    launch_emitter_fill({g.areas.get(), r.book.emit_inst.get(), g.num_true_areas, r.sources.get(), r.num_sources, insts}, s);
    EmitterJob job{};
    job.areas = g.areas.get();
    job.cdf = g.cdf.get();
    job.guide = g.guide.get();
    job.guide_bits = g.guide_bits;
    job.count = g.num_true_areas;
    job.total = total;
    job.emitter_num = total + (g.env.get() ? 1u : 0u);
    job.instances = insts;
    job.emit_inst = r.book.emit_inst.get();
    job.inst_weight = r.book.inst_weight.get();
    job.weight = r.book.weight.get();
    job.select = r.book.select.get();
    job.sum = r.book.sum.get();
    const uint32_t launches = launch_emitter_rebuild(job, s) + (g.num_true_areas ? 1u : 0u);
    HIP_TRY_DRAINED(s, hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    pt->accel.counts.launches += launches;
    pt->accel.counts.syncs++;
    return PUPIL_OK;
}

// the swap of a resize and its counters; t0: the start of the call that resized
void adopt_resized_emitters(pupil_pt *pt, EngineEmitters::Resize &&r, std::chrono::steady_clock::time_point t0) {
    pt->emit_resize_areas = r.gen.num_true_areas;
    pt->emitters.adopt_resize(std::move(r), pt->sc);
    pt->emit_resizes++;
    pt->emit_resize_ms = ms_since(t0);
    // a resize is a rebuild too: pupil_pt_device_emitters_info counts it where pupil_pt_set_instances
    // counts its refresh, i.e. when the table holds a triangle or sphere emitter
    if (pt->emit_resize_areas) {
        pt->emit_refreshes++;
        pt->emit_ms = pt->emit_resize_ms;
    }
}

// The emissive instances of the table pupil_pt_set_instances_emitters is given, from the scene that
// describes it: validates the emitter ranges and the table's shape against the engine (header) and
// fills one source per emissive instance; counts: the new instances' primitive counts.
int scene_emitter_sources(const pupil_pt *pt, const pupil_scene_desc *scene, const std::vector<uint32_t> &counts,
                          std::vector<EmitterSource> &sources, uint32_t &true_areas) {
    if (scene->num_area_emitters && !scene->area_emitters) return fail(PUPIL_ERR_INVALID, "missing emitter array");
    std::vector<uint32_t> types;
    if (const int rc = emitter_table_shape(scene, types, true_areas)) return rc;
    const bool env = scene->env && scene->env->type != PUPIL_EMITTER_NONE;
    if (env != (pt->emitters.cur().env.get() != nullptr))
        return fail(PUPIL_ERR_INVALID, "the scene's env emitter is not the engine's: change it with pupil_pt_update_emitters");
    uint32_t next = 0;  // emitter ranges follow each other in instance order (World::Build)
    for (uint32_t i = 0; i < scene->num_instances; i++) {
        const pupil_instance &in = scene->instances[i];
        if (in.emitter_offset < 0) continue;
        const bool sphere = pt->shapes[in.shape].kind == PUPIL_SHAPE_SPHERE;
        if ((uint32_t)in.emitter_offset != next || counts[i] > true_areas - next)
            return fail(PUPIL_ERR_INVALID, "an emissive instance's emitter range is not its face count, in instance order");
        for (uint32_t k = 0; k < counts[i]; k++)
            if (types[next + k] != (sphere ? PUPIL_EMITTER_SPHERE : PUPIL_EMITTER_TRI_AREA))
                return fail(PUPIL_ERR_INVALID, "an emissive instance's emitter range is not its face count, in instance order");
        EmitterSource s;
        s.inst = i, s.offset = next, s.range = counts[i];
        s.type = sphere ? PUPIL_EMITTER_SPHERE : PUPIL_EMITTER_TRI_AREA;
        s.radiance = scene->area_emitters[next].radiance;
        if (s.radiance.type == PUPIL_TEX_BITMAP && (!s.radiance.rgba || !s.radiance.width || !s.radiance.height))
            return fail(PUPIL_ERR_INVALID, "bitmap texture without texels");
        s.weight = Pupil::world::GetWeight(s.radiance);
        sources.push_back(s);
        next += counts[i];
    }
    if (next != true_areas) return fail(PUPIL_ERR_INVALID, "the emitter ranges and the delta lights do not make up the emitter table");
    return PUPIL_OK;
}

}  // namespace

extern "C" {

const char *pupil_last_error(void) { return g_last_error.c_str(); }
int pupil_abi_version(void) { return 7; }

int pupil_pt_local_pixels(uint32_t width, uint32_t height, uint32_t tile_size, uint32_t tile_rank, uint32_t tile_world,
                          uint32_t *out_pixels, uint32_t *inout_count) {
    if (!inout_count || width == 0 || height == 0) return fail(PUPIL_ERR_INVALID, "bad arguments");
    if (tile_world > 1 && (tile_size == 0 || tile_rank >= tile_world)) return fail(PUPIL_ERR_INVALID, "bad tiling");
    const uint32_t n = local_pixels(width, height, tile_size, tile_rank, tile_world, nullptr);
    if (out_pixels) {
        if (*inout_count < n) return fail(PUPIL_ERR_INVALID, "output too small");
        local_pixels(width, height, tile_size, tile_rank, tile_world, out_pixels);
    }
    *inout_count = n;
    return PUPIL_OK;
}

int pupil_pt_create(const pupil_scene_desc *scene, int device, pupil_pt **out) {
    if (!scene || !out) return fail(PUPIL_ERR_INVALID, "null argument");
    *out = nullptr;
    if (scene->width == 0 || scene->height == 0) return fail(PUPIL_ERR_INVALID, "empty film");
    if (scene->num_instances == 0) return fail(PUPIL_ERR_INVALID, "scene has no instances");
    if (scene->env && scene->env->type == PUPIL_EMITTER_ENV_MAP &&
        !env_map_size_ok(scene->env->radiance.width, scene->env->radiance.height))
        return fail(PUPIL_ERR_INVALID, "env map smaller than 2 x 2 texels");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(PUPIL_ERR_HIP, "no HIP device");
    if (device < 0 || device >= ndev) return fail(PUPIL_ERR_INVALID, "bad device index");
    HIP_TRY(hipSetDevice(device));
    auto pt = new pupil_pt();
    pt->device = device;
    pt->width = scene->width;
    pt->height = scene->height;
    pt->max_depth = scene->max_depth ? scene->max_depth : 1;
    std::memcpy(pt->sc.camera.s2c, scene->sample_to_camera, sizeof(pt->sc.camera.s2c));
    std::memcpy(pt->sc.camera.c2w, scene->camera_to_world, sizeof(pt->sc.camera.c2w));
    int rc = hipStreamCreateWithFlags(pt->own_stream.put(), hipStreamNonBlocking) == hipSuccess
                 ? PUPIL_OK
                 : fail(PUPIL_ERR_HIP, "stream creation failed");
    if (!rc) rc = upload_shapes(pt, scene);
    if (!rc) rc = pt->materials.create(scene->materials, scene->num_materials, pt->sc);
    if (!rc) rc = upload_tables(pt, scene);
    if (!rc) rc = pt->emitters.update(scene, pt->own_stream, pt->sc);
    if (!rc) rc = pt->accel.build({pt->own_stream, &pt->tables, &pt->materials, &pt->sc, &pt->totals}, scene, pt->shapes);
    if (!rc) read_knobs(pt);
    if (!rc) rc = alloc_workspace(pt);
    if (!rc) rc = pt->accel.publish();
    if (!rc) rc = derive_cull_set(pt);
    if (rc) {
        delete pt;
        return rc;
    }
    pt->totals.build_ms = pt->accel.ms;
    *out = pt;
    return PUPIL_OK;
}

int pupil_pt_set_camera(pupil_pt *pt, const float sample_to_camera[16], const float camera_to_world[16]) {
    if (!pt || !sample_to_camera || !camera_to_world) return fail(PUPIL_ERR_INVALID, "null argument");
    if (std::memcmp(pt->sc.camera.s2c, sample_to_camera, sizeof(pt->sc.camera.s2c)) != 0 ||
        std::memcmp(pt->sc.camera.c2w, camera_to_world, sizeof(pt->sc.camera.c2w)) != 0)
        pt->pipe.invalidate();  // frames in flight were started with the old view
    std::memcpy(pt->sc.camera.s2c, sample_to_camera, sizeof(pt->sc.camera.s2c));
    std::memcpy(pt->sc.camera.c2w, camera_to_world, sizeof(pt->sc.camera.c2w));
    return PUPIL_OK;
}

// RenderInstanceUpdate (ias_manager.cpp:116-151) for a set of instances: their new
// transforms, then ONE refit of the acceleration structure over all of them (the
// reference marks its IAS dirty per event and refits once in the next OnRun through
// GetIASHandle(2, true), pt_pass.cpp:46, ias_manager.cpp:199-211).  Flattened BVH: the
// moved instances' records get their new world vertices and every BVH4 node is refitted
// bottom up; two-level: their world records / BLAS copies and the TLAS boxes are
// refitted.  The render after it equals a render of a freshly created engine.  Ordered
// on the engine's stream after every render enqueued so far (no device-wide sync: other
// streams of the process keep running); returns once the structure is updated.
// Emitters follow with pupil_pt_update_emitters.
// With visibility_mask: IASManager::UpdateInstance (ias_manager.cpp:187-197), which copies
// RenderObject::visibility_mask into OptixInstance::visibilityMask next to the transform.  A
// hidden instance ((mask & 0xFF) == 0; every optixTrace passes 255) is the same refit with "no
// geometry" as the new geometry: its records get NaN vertices, which no ray hits and no box
// includes, and keep their id words, so showing it again restores them (bvh_refit.hip
// k_refit_records; accel_two_level.hip k_world_records / rebuild_tlas).  The rebuild paths
// (PUPIL_FLAT_UPDATE / PUPIL_TL_UPDATE = rebuild, the depth-overflow fallback, a tree without a
// level order) build over all the geometry and then apply the masks the same way.  The emitter
// table is not touched (world/world.cpp:45-54 resets it on RenderInstanceTransform only).
int pupil_pt_update_instances_masked(pupil_pt *pt, uint32_t n, const uint32_t *ids, const float *to_world,
                                     const float *to_object, const uint32_t *visibility_mask) {
    if (!pt || (n && (!ids || (!to_world && !visibility_mask) || !to_world != !to_object)))
        return fail(PUPIL_ERR_INVALID, "null argument");
    for (uint32_t k = 0; k < n; k++)
        if (ids[k] >= pt->h_insts().size()) return fail(PUPIL_ERR_INVALID, "instance index out of range");
    if (n == 0) return PUPIL_OK;
    HIP_TRY(hipSetDevice(pt->device));
    HIP_TRY(order_after_renders(pt));  // no render may still read the old tables
    pt->pipe.invalidate();          // frames in flight were traced against the old geometry
    pt->accel.counts = SceneAccel::Counts{};  // pupil_debug_update_counts
    std::vector<uint32_t> changed;
    bool emitters_moved = false;  // device-side emitter table: a transform of an emissive instance
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t id = ids[k];
        DevInstance &d = pt->h_insts()[id];
        if (to_world) {
            emitters_moved = emitters_moved || d.emitter_offset >= 0;
            std::memcpy(d.to_world, to_world + 12 * (size_t)k, sizeof(d.to_world));
            std::memcpy(d.to_object, to_object + 12 * (size_t)k, sizeof(d.to_object));
            if (pt->accel.two_level) refresh_instance_margins(d);  // they depend on the transform
        }
        if (visibility_mask) d.hidden = (visibility_mask[k] & 0xFFu) == 0u ? 1u : 0u;
        if (std::find(changed.begin(), changed.end(), id) == changed.end()) changed.push_back(id);
    }
    // the device copies (pt_scene.h device_instance: a hidden sphere's to_object is NaN there);
    // `staged` outlives the copies (the structure update synchronises the stream)
    std::vector<DevInstance> staged;
    staged.reserve(changed.size());
    for (uint32_t id : changed) {
        staged.push_back(device_instance(pt->h_insts()[id]));
        HIP_TRY(hipMemcpyAsync(pt->d_insts() + id, &staged.back(), sizeof(DevInstance), hipMemcpyHostToDevice,
                               pt->own_stream));
    }
    pt->accel.refits++;  // once the tables have changed, before the structure follows: a failed update counts
    if (const int rc = pt->accel.update_instances(changed)) return rc;
    pt->totals.build_ms = pt->accel.ms;
    if (const int rc = derive_cull_set(pt)) return rc;  // a rebuild moves the records
    if (pt->emitters.book().enabled && emitters_moved) return rebuild_emitters(pt);
    return PUPIL_OK;
}

// Geometry-AS update (OPTIX_BUILD_OPERATION_UPDATE next to the instance-AS update above): the
// vertices of one mesh shape are replaced and every structure derived from them follows in
// place (SceneAccel::update_shape), or, with PUPIL_VERTS_REBUILD, is built anew.
int pupil_pt_update_shape_vertices(pupil_pt *pt, uint32_t shape, const float *positions, const float *normals,
                                   uint32_t flags, void *hip_stream) {
    if (!pt || !positions) return fail(PUPIL_ERR_INVALID, "null argument");
    if (shape >= pt->shapes.size()) return fail(PUPIL_ERR_INVALID, "shape index out of range");
    const ShapeDev &sd = pt->shapes[shape];
    if (sd.kind != PUPIL_SHAPE_MESH) return fail(PUPIL_ERR_INVALID, "shape is not a mesh");
    if (normals && !sd.nrm.get()) return fail(PUPIL_ERR_INVALID, "the shape was created without normals");
    if (flags & ~(PUPIL_VERTS_DEVICE | PUPIL_VERTS_REBUILD)) return fail(PUPIL_ERR_INVALID, "unknown flags");
    const bool device = (flags & PUPIL_VERTS_DEVICE) != 0u, rebuild = (flags & PUPIL_VERTS_REBUILD) != 0u;
    std::vector<uint32_t> changed;
    bool emissive = false;
    for (uint32_t i = 0; i < (uint32_t)pt->h_insts().size(); i++)
        if (pt->accel.inst_shape[i] == shape && pt->h_insts()[i].kind == PUPIL_SHAPE_MESH) {
            changed.push_back(i);
            emissive = emissive || pt->h_insts()[i].emitter_offset >= 0;
        }
    if (device && emissive && !pt->emitters.book().enabled)
        return fail(PUPIL_ERR_UNSUPPORTED, "device vertices of an emissive shape: the emitter table needs the host path");
    HIP_TRY(hipSetDevice(pt->device));
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(order_after_renders(pt));  // no render may still read the old vertices
    pt->pipe.invalidate();          // frames in flight were traced against the old geometry
    const size_t bytes = sizeof(float) * 3 * (size_t)sd.num_vertices;
    if (device) HIP_TRY(order_after_caller(pt, hip_stream));
    const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIP_TRY(hipMemcpyAsync(sd.pos.get(), positions, bytes, kind, pt->own_stream));
    if (normals) HIP_TRY(hipMemcpyAsync(sd.nrm.get(), normals, bytes, kind, pt->own_stream));
    // From here the shape's arrays hold the new vertices.  After a failure below the structure
    // still bounds the OLD vertices, and the engine must not render until an update of this shape
    // succeeds (the header says so).
    if (changed.empty()) {  // no instance shows the shape: only its arrays change
        HIP_TRY(hipStreamSynchronize(pt->own_stream));
    } else {
        if (const int rc = pt->accel.update_shape(shape, changed, rebuild)) return rc;
        pt->totals.build_ms = ms_since(t0);
    }
    pt->accel.refits++;  // only once the structure has followed: a failed update does not count
    if (const int rc = derive_cull_set(pt)) return rc;  // a rebuild moves the records
    if (pt->emitters.book().enabled && emissive) return rebuild_emitters(pt);
    return PUPIL_OK;
}

// The "previous" vertices of the flow pass (pt_flow.hip): a device-to-device copy of the shape's
// own array on the engine's stream, after every render and flow pass enqueued so far (an earlier
// flow pass may still read the snapshot this one overwrites) and before the vertex update that
// follows on the same stream.  Nothing a render reads changes: no refit, no frames dropped.
int pupil_pt_snapshot_shape_vertices(pupil_pt *pt, uint32_t shape) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (shape >= pt->shapes.size()) return fail(PUPIL_ERR_INVALID, "shape index out of range");
    ShapeDev &sd = pt->shapes[shape];
    if (sd.kind != PUPIL_SHAPE_MESH) return fail(PUPIL_ERR_INVALID, "shape is not a mesh");
    HIP_TRY(hipSetDevice(pt->device));
    if (!pt->ev_snap) HIP_TRY(hipEventCreateWithFlags(pt->ev_snap.put(), hipEventDisableTiming));
    if (!sd.prev.get() && sd.prev.alloc(3 * (size_t)sd.num_vertices) != hipSuccess)
        return fail(PUPIL_ERR_OOM, "vertex snapshot allocation failed");
    HIP_TRY(order_after_renders(pt));
    HIP_TRY(hipMemcpyAsync(sd.prev.get(), sd.pos.get(), sizeof(float) * 3 * (size_t)sd.num_vertices, hipMemcpyDeviceToDevice,
                           pt->own_stream));
    HIP_TRY(hipEventRecord(pt->ev_snap, pt->own_stream));
    if (!sd.prev_valid) {
        sd.prev_valid = true;
        pt->snapshots++;
        pt->flow_verts_stale = true;
    }
    return PUPIL_OK;
}

int pupil_pt_clear_vertex_snapshots(pupil_pt *pt) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    for (ShapeDev &sd : pt->shapes) sd.prev_valid = false;
    pt->snapshots = 0;  // the flow pass reads no table; the next snapshot uploads a new one
    return PUPIL_OK;
}

// New topology for one mesh shape (header: the contract).  Three phases.  Aside: a generation of
// the tables is staged (host/scene_tables.h) and the new shape arrays and its instance table are
// filled on the engine's stream (pt_replace.hip) while everything the engine reads stays as it
// is.  Build: SceneAccel::replace_shape rebuilds the whole structure over the staged tables and
// swaps it in, or leaves the old one.  Swap: the staged generation is adopted -- the old arrays
// are freed, the stream has passed every render that read them -- and whatever was sized or
// indexed by the old primitive count is dropped (drop_stale).
int pupil_pt_replace_shape_mesh(pupil_pt *pt, uint32_t shape, const pupil_shape *mesh, uint32_t flags, void *hip_stream) {
    if (!pt || !mesh || !mesh->positions || !mesh->indices) return fail(PUPIL_ERR_INVALID, "null argument");
    if (flags & ~PUPIL_VERTS_DEVICE) return fail(PUPIL_ERR_INVALID, "unknown flags");
    if (shape >= pt->shapes.size()) return fail(PUPIL_ERR_INVALID, "shape index out of range");
    ShapeDev &sd = pt->shapes[shape];
    if (sd.kind != PUPIL_SHAPE_MESH || mesh->kind != PUPIL_SHAPE_MESH) return fail(PUPIL_ERR_INVALID, "shape is not a mesh");
    if (mesh->num_faces == 0 || mesh->num_vertices == 0) return fail(PUPIL_ERR_INVALID, "mesh without faces or vertices");
    const bool device = (flags & PUPIL_VERTS_DEVICE) != 0u;
    const size_t nv = mesh->num_vertices, nf = mesh->num_faces;
    const uint32_t ni = (uint32_t)pt->h_insts().size();
    std::vector<uint32_t> counts(ni);
    bool used = false, emissive = false;
    for (uint32_t i = 0; i < ni; i++) {
        const DevInstance &d = pt->h_insts()[i];
        const bool shows = d.kind == PUPIL_SHAPE_MESH && pt->accel.inst_shape[i] == shape;
        if (shows && d.emitter_offset >= 0) {
            if (!pt->emitters.book().enabled)
                return fail(PUPIL_ERR_UNSUPPORTED, "an instance of the shape is emissive: its emitter range would change");
            emissive = true;
        }
        used = used || shows;
        counts[i] = shows ? mesh->num_faces : d.kind == PUPIL_SHAPE_MESH ? pt->shapes[pt->accel.inst_shape[i]].num_faces : 1u;
    }
    // device-side emitter table: the emitter ranges anew in instance order, as World::Build assigns
    // them; each emissive instance keeps its radiance (the record at its old offset) and select weight
    std::vector<EmitterSource> sources;
    std::vector<int32_t> offsets;
    if (emissive) {
        offsets.assign(ni, -1);
        uint64_t next = 0;
        for (uint32_t i = 0; i < ni; i++) {
            const DevInstance &d = pt->h_insts()[i];
            if (d.emitter_offset < 0) continue;
            EmitterSource src;
            src.inst = i, src.offset = (uint32_t)next, src.range = counts[i];
            src.type = d.kind == PUPIL_SHAPE_SPHERE ? PUPIL_EMITTER_SPHERE : PUPIL_EMITTER_TRI_AREA;
            src.weight = pt->emitters.book().h_inst_weight[i];
            src.kept = d.emitter_offset;
            sources.push_back(src);
            offsets[i] = (int32_t)next;
            next += counts[i];
        }
        if (next + (pt->sc.num_areas - pt->emitters.cur().num_true_areas) > 0x7FFFFFFFull)
            return fail(PUPIL_ERR_UNSUPPORTED, "more than 2^31 emitters");
    }
    if (!device)
        for (size_t i = 0; i < 3 * nf; i++)
            if (mesh->indices[i] >= mesh->num_vertices) return fail(PUPIL_ERR_INVALID, "index out of range");
    HIP_TRY(hipSetDevice(pt->device));
    const auto t0 = std::chrono::steady_clock::now();
    pt->accel.counts = SceneAccel::Counts{};
    hipStream_t s = pt->own_stream;
    // ---- aside: nothing below is read by the engine until the swap.  The tables first: their
    // limits refuse the call before anything is allocated; from there a failure lets the stream pass
    EngineTables::Generation gen;
    if (const int rc = EngineTables::stage(counts.data(), ni, !pt->accel.two_level, s, gen)) return drained(s, rc);
    ShapeDev fresh;  // the new shape: swapped in on success, else it goes with the call, once the stream has passed
    fresh.num_vertices = mesh->num_vertices, fresh.num_faces = mesh->num_faces;
    ScratchBuf<uint32_t> idx_max;
    if (fresh.pos.alloc(3 * nv) || (mesh->normals && fresh.nrm.alloc(3 * nv)) || (mesh->texcoords && fresh.tex.alloc(2 * nv)) ||
        fresh.idx.alloc(3 * nf) || idx_max.alloc(1))
        return drained(s, fail(PUPIL_ERR_OOM, "mesh replacement: allocation failed"));
    if (device) HIP_TRY_DRAINED(s, order_after_caller(pt, hip_stream));
    const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    float *const pos = fresh.pos.get(), *const nrm = fresh.nrm.get(), *const tex = fresh.tex.get();
    uint32_t *const idx = fresh.idx.get();
    HIP_TRY_DRAINED(s, hipMemcpyAsync(idx, mesh->indices, sizeof(uint32_t) * 3 * nf, kind, s));
    if (device) {  // the index check of the host path, as a reduction: 4 bytes come back
        uint32_t largest = 0;
        HIP_TRY_DRAINED(s, hipMemsetAsync(idx_max.get(), 0, sizeof(uint32_t), s));
        launch_index_max(idx, 3 * nf, idx_max.get(), s);
        HIP_TRY_DRAINED(s, hipGetLastError());
        HIP_TRY_DRAINED(s, hipMemcpyAsync(&largest, idx_max.get(), sizeof(largest), hipMemcpyDeviceToHost, s));
        HIP_TRY_DRAINED(s, hipStreamSynchronize(s));
        pt->accel.counts.launches++, pt->accel.counts.syncs++;
        if (largest >= mesh->num_vertices) return fail(PUPIL_ERR_INVALID, "index out of range");
    }
    HIP_TRY_DRAINED(s, hipMemcpyAsync(pos, mesh->positions, sizeof(float) * 3 * nv, kind, s));
    if (mesh->normals) HIP_TRY_DRAINED(s, hipMemcpyAsync(nrm, mesh->normals, sizeof(float) * 3 * nv, kind, s));
    if (mesh->texcoords) HIP_TRY_DRAINED(s, hipMemcpyAsync(tex, mesh->texcoords, sizeof(float) * 2 * nv, kind, s));
    // the second instance table: the engine's own, then the prim offsets and the shape's pointers
    HIP_TRY_DRAINED(s, hipMemcpyAsync(gen.insts.get(), pt->d_insts(), sizeof(DevInstance) * ni, hipMemcpyDeviceToDevice, s));
    ScratchBuf<int32_t> d_offsets;  // emissive: every instance's new emitter_offset
    if (emissive) {
        if (d_offsets.alloc(ni)) return drained(s, fail(PUPIL_ERR_OOM, "mesh replacement: allocation failed"));
        HIP_TRY_DRAINED(s, hipMemcpyAsync(d_offsets.get(), offsets.data(), sizeof(int32_t) * ni, hipMemcpyHostToDevice, s));
    }
    const ReplaceMeshJob job{gen.insts.get(), ni, gen.inst_first.get(), sd.pos.get(), pos, nrm, tex, idx, d_offsets.get()};
    launch_patch_instances(job, s);
    HIP_TRY_DRAINED(s, hipGetLastError());
    pt->accel.counts.launches += 2;  // with the tables' fill
    // the emitter table at its new size, aside too, from the patched instance table and the new arrays
    EngineEmitters::Resize resized;
    if (emissive) {
        if (const int rc = pt->emitters.stage_resize(sources, ni, nullptr, 0, true, resized)) return drained(s, rc);
        if (const int rc = fill_resized_emitters(pt, resized, gen.insts.get(), s)) return rc;
    }
    gen.mirror = pt->h_insts();  // the same patch on the host mirror
    for (uint32_t i = 0; i < ni; i++) {
        DevInstance &d = gen.mirror[i];
        d.prim_offset = gen.first[i];
        if (emissive) d.emitter_offset = offsets[i];
        if (d.kind == PUPIL_SHAPE_MESH && pt->accel.inst_shape[i] == shape) {
            d.positions = pos;
            d.normals = nrm;
            d.texcoords = tex;
            d.indices = idx;
        }
    }
    // ---- build: after the renders enqueued so far (the builders share the engine's stream with
    // nothing of theirs, but the swap below frees what they read)
    HIP_TRY_DRAINED(s, order_after_renders(pt));
    if (const int rc = pt->accel.replace_shape(shape, fresh, used, gen)) return drained(s, rc);
    // ---- swap: the structure is published and the stream idle
    pt->pipe.invalidate();  // frames in flight were traced against the old geometry
    drop_stale(pt, true, false, &sd);
    sd = std::move(fresh);  // the old arrays and the old snapshot go with the replaced value
    pt->tables.adopt(std::move(gen), pt->sc, pt->totals);
    if (emissive) adopt_resized_emitters(pt, std::move(resized), t0);
    pt->accel.refits++;
    if (const int rc = derive_cull_set(pt)) return rc;  // the rebuild moved the records
    pt->replacements++;
    pt->replace_ms = pt->totals.build_ms = ms_since(t0);
    return PUPIL_OK;
}

// The instance table as a whole (header: the contract).  The phases of pupil_pt_replace_shape_mesh.
// Aside: the bindings, a per-shape table, inst_first and the transforms go up, k_fill_instances
// (pt_instance_set.hip) writes a second instance table, launch_prim_tables the primitive tables;
// the host mirror is assembled by the same text (host path) or read back in one copy (device
// path; in the two-level modes the structure's instance stage then fills the two-level fields in the
// mirror and uploads the table again, as create does).  Build: SceneAccel::set_instances builds the
// structure over the staged tables and swaps it in, or leaves the old one.  Swap: the staged
// generation is adopted, and whatever was sized by the old instance or primitive count is dropped
// and re-allocated by its next user (drop_stale).
// scene: null, or (pupil_pt_set_instances_emitters) the description the instances are taken from,
// whose emissive set is free: the emitter table is rebuilt at its new size inside the transaction
static int set_instances_impl(pupil_pt *pt, uint32_t n, const pupil_instance *instances, const uint32_t *visibility_mask,
                              const void *to_world_device, uint32_t flags, void *hip_stream, const pupil_scene_desc *scene) {
    if (!pt || !instances) return fail(PUPIL_ERR_INVALID, "null argument");
    if (flags & ~PUPIL_INSTANCES_DEVICE) return fail(PUPIL_ERR_INVALID, "unknown flags");
    const bool device = (flags & PUPIL_INSTANCES_DEVICE) != 0u;
    if (device != (to_world_device != nullptr))
        return fail(PUPIL_ERR_INVALID, device ? "PUPIL_INSTANCES_DEVICE without a device pointer"
                                              : "a device pointer without PUPIL_INSTANCES_DEVICE");
    if ((uintptr_t)to_world_device & 3u) return fail(PUPIL_ERR_INVALID, "device pointer not 4-byte aligned");
    if (n == 0) return fail(PUPIL_ERR_INVALID, "scene has no instances");  // as pupil_pt_create
    const bool two_level = pt->accel.two_level;
    const uint32_t old_n = (uint32_t)pt->h_insts().size();
    // ---- everything that can refuse the call from the host's tables
    std::vector<InstBinding> bind(n);
    std::vector<uint32_t> counts(n), new_shape(n);
    for (uint32_t i = 0; i < n; i++) {
        const pupil_instance &src = instances[i];
        if (src.shape >= pt->shapes.size()) return fail(PUPIL_ERR_INVALID, "instance shape out of range");
        if (src.material >= pt->materials.count()) return fail(PUPIL_ERR_INVALID, "instance material out of range");
        const ShapeDev &sd = pt->shapes[src.shape];
        counts[i] = sd.kind == PUPIL_SHAPE_SPHERE ? 1u : sd.num_faces;
        new_shape[i] = src.shape;
        InstBinding &b = bind[i];
        b.shape = src.shape;
        b.material = src.material;
        b.flip_normals = src.flip_normals;
        b.flip_tex_coords = src.flip_tex_coords;
        b.emitter_offset = src.emitter_offset;
        b.hidden = visibility_mask && (visibility_mask[i] & 0xFFu) == 0u ? 1u : 0u;
        b.bin = material_bin(pt->materials.mirror()[src.material].type);
    }
    // the new entry: the emitter table follows the scene's emissive set
    std::vector<EmitterSource> sources;
    uint32_t true_areas = 0;
    if (scene) {
        if (!pt->emitters.book().enabled)
            return fail(PUPIL_ERR_UNSUPPORTED,
                        "the emitter table is resized on the device: switch the mode on with pupil_pt_enable_device_emitters");
        if (const int rc = scene_emitter_sources(pt, scene, counts, sources, true_areas)) return rc;
    }
    // the old entry: the emitter table stays: the emissive instances are the old ones, in their order
    // (so every emitter range is one create checked against the table)
    std::vector<uint32_t> old_em, new_em;
    bool emitters_moved = false;
    if (!scene) {
        for (uint32_t i = 0; i < old_n; i++)
            if (pt->h_insts()[i].emitter_offset >= 0) old_em.push_back(i);
        for (uint32_t i = 0; i < n; i++)
            if (instances[i].emitter_offset >= 0) new_em.push_back(i);
        if (old_em.size() != new_em.size())
            return fail(PUPIL_ERR_UNSUPPORTED, "emissive instances added or removed: the emitter table would change");
        for (size_t k = 0; k < old_em.size(); k++) {
            const DevInstance &o = pt->h_insts()[old_em[k]];
            const pupil_instance &c = instances[new_em[k]];
            // the same material: its slot, or another slot of the same content
            const std::vector<DevMaterial> &mats = pt->materials.mirror();
            const bool same_material =
                o.material == c.material || std::memcmp(&mats[o.material], &mats[c.material], sizeof(DevMaterial)) == 0;
            if (pt->accel.inst_shape[old_em[k]] != c.shape || !same_material || o.flip_normals != c.flip_normals ||
                o.flip_tex_coords != c.flip_tex_coords || o.emitter_offset != c.emitter_offset)
                return fail(PUPIL_ERR_UNSUPPORTED, "emissive instances reordered or rebound: the emitter table would change");
            if (!device && (std::memcmp(o.to_world, c.to_world, sizeof(o.to_world)) != 0 ||
                            std::memcmp(o.to_object, c.to_object, sizeof(o.to_object)) != 0)) {
                if (!pt->emitters.book().enabled)
                    return fail(PUPIL_ERR_UNSUPPORTED, "an emissive instance moved: the emitter table needs the device-side mode");
                emitters_moved = true;
            }
        }
    }
    std::vector<InstShape> shape_tab(pt->shapes.size());  // the per-shape table
    for (size_t k = 0; k < pt->shapes.size(); k++) {
        const ShapeDev &sd = pt->shapes[k];
        shape_tab[k] = InstShape{sd.kind, sd.num_faces, sd.pos.get(), sd.nrm.get(), sd.tex.get(), sd.idx.get()};
    }
    HIP_TRY(hipSetDevice(pt->device));
    const auto t0 = std::chrono::steady_clock::now();
    pt->accel.counts = SceneAccel::Counts{};
    hipStream_t s = pt->own_stream;
    // ---- aside: nothing below is read by the engine until the swap.  The tables first: their
    // limits refuse the call before anything is allocated; from there a failure lets the stream pass
    EngineTables::Generation gen;
    if (const int rc = EngineTables::stage(counts.data(), n, !two_level, s, gen)) return drained(s, rc);
    ScratchBuf<InstBinding> d_bind;
    ScratchBuf<InstShape> d_shapes;
    ScratchBuf<float> xf;
    if (d_bind.alloc(n) || d_shapes.alloc(shape_tab.size()) || (!device && xf.alloc(24 * (size_t)n)))
        return drained(s, fail(PUPIL_ERR_OOM, "instance table: allocation failed"));
    // the device-side emitter bookkeeping: the emitters' instances under their new indices
    EngineEmitters::Bookkeeping book;
    EngineEmitters::Resize resized;  // the new entry: the table at its new size, with its own bookkeeping
    const bool remap = pt->emitters.book().enabled && !scene;
    if (scene)
        if (const int rc = pt->emitters.stage_resize(sources, n, scene->area_emitters + true_areas,
                                                     scene->num_area_emitters - true_areas, false, resized))
            return drained(s, rc);
    if (remap)
        if (const int rc = pt->emitters.book().restage(old_em, new_em, n, book, "instance table: allocation failed"))
            return drained(s, rc);
    std::vector<float> h_xf;  // host path: n to_world, then n to_object; outlives the copy (the build synchronises)
    if (device) {
        HIP_TRY_DRAINED(s, order_after_caller(pt, hip_stream));
    } else {
        h_xf.resize(24 * (size_t)n);
        for (uint32_t i = 0; i < n; i++) {
            std::memcpy(&h_xf[12 * (size_t)i], instances[i].to_world, sizeof(float) * 12);
            std::memcpy(&h_xf[12 * ((size_t)n + i)], instances[i].to_object, sizeof(float) * 12);
        }
        HIP_TRY_DRAINED(s, hipMemcpyAsync(xf.get(), h_xf.data(), sizeof(float) * h_xf.size(), hipMemcpyHostToDevice, s));
    }
    HIP_TRY_DRAINED(s, hipMemcpyAsync(d_bind.get(), bind.data(), sizeof(InstBinding) * n, hipMemcpyHostToDevice, s));
    HIP_TRY_DRAINED(s, hipMemcpyAsync(d_shapes.get(), shape_tab.data(), sizeof(InstShape) * shape_tab.size(), hipMemcpyHostToDevice, s));
    FillInstancesJob job{};
    job.out = gen.insts.get();
    job.n = n;
    job.shapes = d_shapes.get();
    job.bindings = d_bind.get();
    job.inst_first = gen.inst_first.get();
    job.to_world = device ? (const float *)to_world_device : xf.get();
    job.to_object = device ? nullptr : xf.get() + 12 * (size_t)n;
    launch_fill_instances(job, s);
    HIP_TRY_DRAINED(s, hipGetLastError());
    pt->accel.counts.launches += 2;  // with the tables' fill
    if (scene)  // emissive instances' transforms are read from the new table, on the device
        if (const int rc = fill_resized_emitters(pt, resized, gen.insts.get(), s)) return rc;
    if (device) {  // one contiguous readback
        HIP_TRY_DRAINED(s, hipMemcpyAsync(gen.mirror.data(), gen.insts.get(), sizeof(DevInstance) * n, hipMemcpyDeviceToHost, s));
        HIP_TRY_DRAINED(s, hipStreamSynchronize(s));
        pt->accel.counts.syncs++;
        // the table holds a hidden sphere's device copy: the mirror keeps its real inverse, the same text
        for (DevInstance &d : gen.mirror)
            if (d.hidden && d.kind == PUPIL_SHAPE_SPHERE) invert_affine3x4(d.to_world, d.to_object);
        for (size_t k = 0; k < old_em.size(); k++) {
            const DevInstance &o = pt->h_insts()[old_em[k]], &c = gen.mirror[new_em[k]];
            if (std::memcmp(o.to_world, c.to_world, sizeof(o.to_world)) == 0 &&
                std::memcmp(o.to_object, c.to_object, sizeof(o.to_object)) == 0)
                continue;
            if (!pt->emitters.book().enabled)
                return fail(PUPIL_ERR_UNSUPPORTED, "an emissive instance moved: the emitter table needs the device-side mode");
            emitters_moved = true;
        }
    } else {
        for (uint32_t i = 0; i < n; i++)
            fill_instance_record(gen.mirror[i], shape_tab[bind[i].shape], bind[i], gen.first[i], instances[i].to_world,
                                 instances[i].to_object, false);
    }
    // ---- build: after the renders enqueued so far (the swap below frees what they read)
    HIP_TRY_DRAINED(s, order_after_renders(pt));
    if (const int rc = pt->accel.set_instances(gen, new_shape, pt->shapes)) return drained(s, rc);
    // ---- swap: the structure is published and the stream idle
    pt->pipe.invalidate();  // frames in flight were traced against the old table
    drop_stale(pt, true, true);
    if (scene) adopt_resized_emitters(pt, std::move(resized), t0);
    else pt->emitters.book() = std::move(book);  // switched off: dropped, the next enable sizes its bookkeeping anew
    pt->tables.adopt(std::move(gen), pt->sc, pt->totals);
    pt->accel.refits++;
    derive_bins(pt);
    if (const int rc = derive_cull_set(pt)) return rc;  // the build moved the records
    if (pt->emitters.book().enabled && !old_em.empty())
        if (const int rc = rebuild_emitters(pt)) return rc;
    pt->inst_sets++;
    pt->inst_set_blas_builds = pt->accel.last_blas_builds;
    pt->inst_set_whole = pt->accel.last_whole_rebuild;
    pt->inst_set_ms = pt->totals.build_ms = ms_since(t0);
    return PUPIL_OK;
}

int pupil_pt_set_instances(pupil_pt *pt, uint32_t n, const pupil_instance *instances, const uint32_t *visibility_mask,
                           const void *to_world_device, uint32_t flags, void *hip_stream) {
    return set_instances_impl(pt, n, instances, visibility_mask, to_world_device, flags, hip_stream, nullptr);
}

// pupil_pt_set_instances with the instance list of `scene` and a free emissive set (header: the
// contract): the phases above, with the emitter table staged at its new size beside the instance
// table (EmitterTables::stage_resize), filled on the device from the staged instance table
// (pt_emitters.hip) and adopted in the same swap.
int pupil_pt_set_instances_emitters(pupil_pt *pt, const pupil_scene_desc *scene, const uint32_t *visibility_mask,
                                    const void *to_world_device, uint32_t flags, void *hip_stream) {
    if (!pt || !scene || !scene->instances) return fail(PUPIL_ERR_INVALID, "null argument");
    return set_instances_impl(pt, scene->num_instances, scene->instances, visibility_mask, to_world_device, flags, hip_stream,
                              scene);
}

int pupil_pt_emitter_table_info(pupil_pt *pt, uint32_t *emitters, uint32_t *true_areas, uint32_t *has_env) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (emitters) *emitters = pt->sc.num_areas;
    if (true_areas) *true_areas = pt->emitters.cur().num_true_areas;
    if (has_env) *has_env = pt->emitters.cur().env.get() ? 1u : 0u;
    return PUPIL_OK;
}

int pupil_pt_emitter_resize_info(pupil_pt *pt, uint64_t *resizes, uint32_t *last_true_areas, double *last_ms) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (resizes) *resizes = pt->emit_resizes;
    if (last_true_areas) *last_true_areas = pt->emit_resize_areas;
    if (last_ms) *last_ms = pt->emit_resize_ms;
    return PUPIL_OK;
}

int pupil_pt_set_instances_info(pupil_pt *pt, uint64_t *calls, uint32_t *last_blas_builds, uint32_t *last_whole_rebuild,
                                double *last_ms) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (calls) *calls = pt->inst_sets;
    if (last_blas_builds) *last_blas_builds = pt->inst_set_blas_builds;
    if (last_whole_rebuild) *last_whole_rebuild = pt->inst_set_whole;
    if (last_ms) *last_ms = pt->inst_set_ms;
    return PUPIL_OK;
}

int pupil_debug_read_prim_tables(pupil_pt *pt, uint32_t *num_prims, uint32_t *guide_shift, uint32_t *guide_entries,
                                 uint32_t *prim_inst, uint32_t *inst_first, uint32_t *inst_guide) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    const DeviceScene &sc = pt->sc;
    const uint32_t entries = sc.num_prims ? ((sc.num_prims - 1u) >> sc.inst_guide_shift) + 2u : 2u;
    if (num_prims) *num_prims = sc.num_prims;
    if (guide_shift) *guide_shift = sc.inst_guide_shift;
    if (guide_entries) *guide_entries = entries;
    HIP_TRY(hipSetDevice(pt->device));
    HIP_TRY(hipStreamSynchronize(pt->own_stream));
    if (prim_inst && sc.num_prims)
        HIP_TRY(hipMemcpy(prim_inst, sc.prim_inst, sizeof(uint32_t) * sc.num_prims, hipMemcpyDeviceToHost));
    if (inst_first)
        HIP_TRY(hipMemcpy(inst_first, sc.inst_first, sizeof(uint32_t) * ((size_t)sc.num_instances + 1), hipMemcpyDeviceToHost));
    if (inst_guide) HIP_TRY(hipMemcpy(inst_guide, sc.inst_guide, sizeof(uint32_t) * entries, hipMemcpyDeviceToHost));
    return PUPIL_OK;
}

int pupil_pt_replace_info(pupil_pt *pt, uint64_t *replacements, double *last_ms) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (replacements) *replacements = pt->replacements;
    if (last_ms) *last_ms = pt->replace_ms;
    return PUPIL_OK;
}

int pupil_pt_update_instances(pupil_pt *pt, uint32_t n, const uint32_t *ids, const float *to_world,
                              const float *to_object) {
    if (!pt || (n && (!ids || !to_world || !to_object))) return fail(PUPIL_ERR_INVALID, "null argument");
    return pupil_pt_update_instances_masked(pt, n, ids, to_world, to_object, nullptr);
}

int pupil_pt_update_instance(pupil_pt *pt, uint32_t instance, const float to_world[12], const float to_object[12]) {
    if (!pt || !to_world || !to_object) return fail(PUPIL_ERR_INVALID, "null argument");
    return pupil_pt_update_instances(pt, 1, &instance, to_world, to_object);
}

// The same update with ids and matrices in device memory (header: the contract).  The ids come
// back first (4n bytes) so that everything that can refuse the call runs before anything changes
// and the host knows which mirror entries follow; then one kernel writes the instance table
// (pt_instances.hip), the structure's own kernels follow on the id list it left on the device
// (SceneAccel::move_*), and one staging block brings the host mirror up to date.
int pupil_pt_update_instances_device(pupil_pt *pt, uint32_t n, const uint32_t *ids_device, const void *to_world_device,
                                     const void *to_object_device, void *hip_stream) {
    if (!pt || !to_world_device) return fail(PUPIL_ERR_INVALID, "null argument");
    const uint32_t ni = (uint32_t)pt->h_insts().size();
    if (n > ni) return fail(PUPIL_ERR_INVALID, "more list entries than instances");
    for (const void *p : {(const void *)ids_device, to_world_device, to_object_device})
        if ((uintptr_t)p & 3u) return fail(PUPIL_ERR_INVALID, "device pointer not 4-byte aligned");
    if (n == 0) return PUPIL_OK;
    HIP_TRY(hipSetDevice(pt->device));
    const auto t0 = std::chrono::steady_clock::now();
    SceneAccel::Counts &cnt = pt->accel.counts;
    cnt = SceneAccel::Counts{};
    ScratchBuf<float> &move_stage = pt->per_inst.move_stage;
    if (!move_stage.get()) {  // the first call: the staging block (a header line, then one line per instance)
        if (move_stage.alloc(pupil_pt::kMoveHeader + (size_t)kMoveStageFloats * ni) != hipSuccess)
            return fail(PUPIL_ERR_OOM, "instance staging allocation failed");
        HIP_TRY(hipMemset(move_stage.get(), 0, sizeof(float) * pupil_pt::kMoveHeader));  // [0]: the skipped ids, a running total
        const uint32_t so_far = (uint32_t)pt->inst_dev_skipped;  // pupil_pt_set_instances dropped an earlier block
        if (so_far) HIP_TRY(hipMemcpy(move_stage.get(), &so_far, sizeof(so_far), hipMemcpyHostToDevice));
    }
    HIP_TRY(order_after_caller(pt, hip_stream));
    std::vector<uint32_t> &ids = pt->per_inst.h_move_ids;  // the list as the caller gave it
    ids.resize(n);
    if (ids_device) {
        HIP_TRY(hipMemcpyAsync(ids.data(), ids_device, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, pt->own_stream));
        HIP_TRY(hipStreamSynchronize(pt->own_stream));
        cnt.syncs++;
    } else {
        for (uint32_t k = 0; k < n; k++) ids[k] = k;
    }
    std::vector<uint32_t> changed;  // the ids in range, each once
    std::vector<uint8_t> &seen = pt->per_inst.h_move_seen;
    seen.assign(ni, 0);
    bool emissive = false;
    for (uint32_t id : ids) {
        if (id >= ni || seen[id]) continue;
        seen[id] = 1;
        changed.push_back(id);
        emissive = emissive || pt->h_insts()[id].emitter_offset >= 0;
    }
    if (emissive && !pt->emitters.book().enabled)
        return fail(PUPIL_ERR_UNSUPPORTED,
                    "device transforms of an emissive instance: the emitter table needs the host path");
    HIP_TRY(order_after_renders(pt));  // no render may still read the old tables
    pt->pipe.invalidate();          // frames in flight were traced against the old geometry
    MoveInstancesJob job{};
    job.instances = pt->d_insts();
    job.num_instances = ni;
    job.n = n;
    job.ids = ids_device;
    job.to_world = (const float *)to_world_device;
    job.to_object = (const float *)to_object_device;
    job.margins = pt->accel.two_level ? 1u : 0u;
    job.fallback = changed.empty() ? 0u : changed[0];
    job.stage = move_stage.get() + pupil_pt::kMoveHeader;
    job.skipped = reinterpret_cast<uint32_t *>(move_stage.get());
    if (!changed.empty())
        if (const int rc = pt->accel.move_begin(&job.list, &job.moved)) return rc;
    launch_move_instances(job, pt->own_stream);
    HIP_TRY(hipGetLastError());
    cnt.launches++;
    if (!changed.empty()) pt->accel.move_boxes(n, job.stage + kMoveStageBox, kMoveStageFloats);
    // the host mirror: what the device computed, in one copy
    std::vector<float> &st = pt->per_inst.h_move_stage;
    st.resize(pupil_pt::kMoveHeader + (size_t)kMoveStageFloats * n);
    HIP_TRY(hipMemcpyAsync(st.data(), move_stage.get(), sizeof(float) * st.size(), hipMemcpyDeviceToHost, pt->own_stream));
    HIP_TRY(hipStreamSynchronize(pt->own_stream));
    cnt.syncs++;
    uint32_t skipped_total = 0;
    std::memcpy(&skipped_total, st.data(), sizeof(skipped_total));
    const uint64_t skipped_now = skipped_total - (uint32_t)pt->inst_dev_skipped;
    pt->inst_dev_skipped += skipped_now;
    const bool boxes = pt->accel.two_level && pt->accel.tl.world;
    seen.assign(ni, 0);
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t id = ids[k];
        if (id >= ni || seen[id]) continue;  // of a repeated id the first entry is mirrored
        seen[id] = 1;
        const float *e = st.data() + pupil_pt::kMoveHeader + (size_t)kMoveStageFloats * k;
        DevInstance &d = pt->h_insts()[id];
        std::memcpy(d.to_world, e, sizeof(d.to_world));
        std::memcpy(d.to_object, e + 12, sizeof(d.to_object));
        if (pt->accel.two_level) std::memcpy(d.margin, e + 24, sizeof(d.margin));
        if (boxes) {
            std::memcpy(d.wlo, e + kMoveStageBox, sizeof(d.wlo));
            std::memcpy(d.whi, e + kMoveStageBox + 3, sizeof(d.whi));
        }
    }
    if (!changed.empty()) {
        pt->accel.refits++;  // as the host entry: once the tables have changed
        if (const int rc = pt->accel.move_finish(changed, n)) return rc;
        if (const int rc = derive_cull_set(pt)) return rc;  // a rebuild moves the records
        if (pt->emitters.book().enabled && emissive)
            if (const int rc = rebuild_emitters(pt)) return rc;
    }
    pt->inst_dev_updates++;
    pt->inst_dev_moved += changed.size();
    pt->inst_dev_launches = cnt.launches;
    pt->inst_dev_syncs = cnt.syncs;
    pt->inst_dev_ms = pt->totals.build_ms = ms_since(t0);
    if (skipped_now)
        g_last_error = std::to_string(skipped_now) + " of " + std::to_string(n) + " instance ids out of range: skipped";
    return PUPIL_OK;
}

int pupil_pt_get_instance_transforms(pupil_pt *pt, uint32_t first, uint32_t n, float *to_world, float *to_object) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    const size_t ni = pt->h_insts().size();
    if (first > ni || n > ni - first) return fail(PUPIL_ERR_INVALID, "instance range out of bounds");
    for (uint32_t k = 0; k < n; k++) {
        const DevInstance &d = pt->h_insts()[first + k];
        if (to_world) std::memcpy(to_world + 12 * (size_t)k, d.to_world, sizeof(d.to_world));
        if (to_object) std::memcpy(to_object + 12 * (size_t)k, d.to_object, sizeof(d.to_object));
    }
    return PUPIL_OK;
}

int pupil_debug_update_counts(pupil_pt *pt, uint32_t *launches, uint32_t *syncs) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (launches) *launches = pt->accel.counts.launches;
    if (syncs) *syncs = pt->accel.counts.syncs;
    return PUPIL_OK;
}

int pupil_pt_instances_device_info(pupil_pt *pt, uint64_t *updates, uint64_t *instances, uint64_t *skipped,
                                   uint32_t *last_launches, uint32_t *last_syncs, double *last_ms) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (updates) *updates = pt->inst_dev_updates;
    if (instances) *instances = pt->inst_dev_moved;
    if (skipped) *skipped = pt->inst_dev_skipped;
    if (last_launches) *last_launches = pt->inst_dev_launches;
    if (last_syncs) *last_syncs = pt->inst_dev_syncs;
    if (last_ms) *last_ms = pt->inst_dev_ms;
    return PUPIL_OK;
}

// EmitterHelper reset after a transform change (world/world.cpp:45-54): the area
// emitter table, selection CDF and env emitter are replaced by the scene's.  When the
// tables keep their shapes (same emitter count and types, no bitmap radiance to upload, the same
// env) they are rewritten in place on the engine's stream after the renders enqueued so
// far; otherwise new tables are uploaded and the old ones freed.
int pupil_pt_update_emitters(pupil_pt *pt, const pupil_scene_desc *scene) {
    if (!pt || !scene) return fail(PUPIL_ERR_INVALID, "null argument");
    if (scene->num_area_emitters && !scene->area_emitters) return fail(PUPIL_ERR_INVALID, "missing emitter array");
    HIP_TRY(hipSetDevice(pt->device));
    HIP_TRY(order_after_renders(pt));
    pt->pipe.invalidate();
    if (const int rc = pt->emitters.update(scene, pt->own_stream, pt->sc)) return rc;
    if (const int rc = derive_cull_set(pt, false)) return rc;  // the scene may have gained or lost its env emitter
    return keep_device_emitters(pt, scene);
}

int pupil_pt_enable_device_emitters(pupil_pt *pt, const pupil_scene_desc *scene) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (!scene) {
        pt->emitters.book().enabled = false;
        return PUPIL_OK;
    }
    HIP_TRY(hipSetDevice(pt->device));
    // everything that can refuse the scene runs before anything of the engine changes (no render reads the bookkeeping)
    if (const int rc = device_emitter_setup(pt, scene)) return rc;
    HIP_TRY(order_after_renders(pt));  // no render may still read the table
    pt->pipe.invalidate();
    HIP_TRY(hipStreamSynchronize(pt->own_stream));
    if (const int rc = rebuild_emitters(pt)) return rc;
    pt->emitters.book().enabled = true;
    return PUPIL_OK;
}

int pupil_pt_refresh_emitters(pupil_pt *pt) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (!pt->emitters.book().enabled) return fail(PUPIL_ERR_INVALID, "the device-side emitter table is not enabled");
    HIP_TRY(hipSetDevice(pt->device));
    HIP_TRY(order_after_renders(pt));
    pt->pipe.invalidate();  // frames in flight were shaded with the old table
    return rebuild_emitters(pt);
}

int pupil_pt_device_emitters_info(pupil_pt *pt, uint32_t *enabled, uint64_t *refreshes, double *last_ms) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (enabled) *enabled = pt->emitters.book().enabled ? 1u : 0u;
    if (refreshes) *refreshes = pt->emit_refreshes;
    if (last_ms) *last_ms = pt->emit_ms;
    return PUPIL_OK;
}

// Materials replaced in place: convert_material is the host precompute of create, so each named
// material becomes what a fresh engine would hold.  Stage: everything that can refuse the call,
// the fresh texels included (a bitmap slot of an unchanged texel count keeps its allocation), runs
// before anything of the engine changes.  Commit: on the engine's stream after the renders enqueued
// so far, the texels, the changed DevMaterial entries and -- when a type changed -- the bins of the
// instances that use it, the records' bin words and the shading schedule derived from the bins.
// No box or link of the acceleration structure depends on a material: accel_refits stays.
// Returns once the stream has passed the copies, and frees the replaced texels then.
int pupil_pt_update_materials(pupil_pt *pt, uint32_t n, const uint32_t *ids, const pupil_material *materials) {
    if (!pt || (n && (!ids || !materials))) return fail(PUPIL_ERR_INVALID, "null argument");
    if (n == 0) return PUPIL_OK;
    HIP_TRY(hipSetDevice(pt->device));
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = pt->own_stream;
    EngineMaterials::Staged staged_mats;
    if (const int rc = pt->materials.stage(n, ids, materials, staged_mats)) return rc;
    HIP_TRY(order_after_renders(pt));  // no render may still read the old materials
    pt->pipe.invalidate();          // frames in flight were shaded with them
    std::vector<EngineMaterials::Texels> replaced;
    bool type_changed = false;
    if (const int rc = pt->materials.commit(staged_mats, s, replaced, type_changed)) return drained(s, rc);
    std::vector<DevInstance> staged;  // outlives the copies (synchronised below)
    if (type_changed) {
        staged.reserve(pt->h_insts().size());
        for (size_t i = 0; i < pt->h_insts().size(); i++) {
            DevInstance &d = pt->h_insts()[i];
            const uint32_t bin = material_bin(pt->materials.mirror()[d.material].type);
            if (bin == d.bin) continue;
            d.bin = bin;
            staged.push_back(device_instance(d));
            HIP_TRY_DRAINED(s, hipMemcpyAsync(pt->d_insts() + i, &staged.back(), sizeof(DevInstance), hipMemcpyHostToDevice, s));
        }
        if (!staged.empty()) {
            pt->accel.update_bins();
            HIP_TRY_DRAINED(s, hipGetLastError());
            derive_bins(pt);
        }
    }
    HIP_TRY(hipStreamSynchronize(s));
    replaced.clear();  // the stream has passed them
    pt->mat_updates++;
    pt->mat_ms = ms_since(t0);
    return derive_cull_set(pt, false);
}

// The texels of one bitmap slot from device memory, ordered like PUPIL_VERTS_DEVICE: an event on
// the caller's stream, the engine's stream waits for it, then the copy device to device.  A
// plastic's specular_sampling_weight follows on the device (pt_materials.hip) when the slot is
// one of the two it is derived from.
int pupil_pt_update_texture_device(pupil_pt *pt, uint32_t material, uint32_t slot, const void *rgba_device,
                                   uint32_t width, uint32_t height, void *hip_stream) {
    if (!pt || !rgba_device) return fail(PUPIL_ERR_INVALID, "null argument");
    if (material >= pt->materials.count() || slot >= 4u) return fail(PUPIL_ERR_INVALID, "no such material texture");
    const DevMaterial &m = pt->materials.mirror()[material];
    const DevTexture &t = m.tex[slot];
    if (t.type != PUPIL_TEX_BITMAP || !t.data)
        return fail(PUPIL_ERR_INVALID, "the slot holds no bitmap: make it one with pupil_pt_update_materials first");
    if (t.width != width || t.height != height)
        return fail(PUPIL_ERR_INVALID, "the slot's bitmap is " + std::to_string(t.width) + " x " + std::to_string(t.height) +
                                           ": set the size with pupil_pt_update_materials first");
    HIP_TRY(hipSetDevice(pt->device));
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(order_after_renders(pt));  // no render may still read the old texels
    pt->pipe.invalidate();
    HIP_TRY(order_after_caller(pt, hip_stream));
    HIP_TRY(hipMemcpyAsync((void *)t.data, rgba_device, sizeof(float4) * (size_t)width * height, hipMemcpyDeviceToDevice,
                           pt->own_stream));
    const uint32_t diffuse_slot = m.type == PUPIL_MAT_PLASTIC ? 0u : 1u;
    if ((m.type == PUPIL_MAT_PLASTIC || m.type == PUPIL_MAT_ROUGH_PLASTIC) &&
        (slot == diffuse_slot || slot == diffuse_slot + 1u)) {
        launch_specular_weight(pt->materials.device() + material, pt->own_stream);  // the mirror keeps the stale weight
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(pt->own_stream));
    pt->mat_updates++;
    pt->mat_ms = ms_since(t0);
    return PUPIL_OK;
}

int pupil_pt_material_info(pupil_pt *pt, uint64_t *updates, double *last_ms) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (updates) *updates = pt->mat_updates;
    if (last_ms) *last_ms = pt->mat_ms;
    return PUPIL_OK;
}

// The texels of the env map from device memory, ordered like pupil_pt_update_texture_device: an
// event on the caller's stream, the engine's stream waits for it, then the copy device to device
// into the engine's own texels and the two table stages of pt_envmap.hip, which rewrite col_cdf,
// row_cdf and normalization in place.  Everything that can refuse the call, the scratch
// allocation of the first call included, runs before anything of the engine changes.
int pupil_pt_update_env_device(pupil_pt *pt, const void *rgba_device, uint32_t width, uint32_t height,
                               void *hip_stream) {
    if (!pt || !rgba_device) return fail(PUPIL_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(pt->device));
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = pt->emitters.reserve_env_texels(width, height)) return rc;
    HIP_TRY(order_after_renders(pt));  // no render may still read the old texels and tables
    pt->pipe.invalidate();
    HIP_TRY(order_after_caller(pt, hip_stream));
    if (const int rc = pt->emitters.write_env_texels(rgba_device, pt->own_stream)) return rc;
    pt->env_updates++;
    pt->env_ms = ms_since(t0);
    return PUPIL_OK;
}

// scale, to_world and to_local of the device's env emitter: two small copies, no table, no texel
int pupil_pt_update_env_params(pupil_pt *pt, float scale, const float to_world[9], const float to_local[9]) {
    if (!pt || !to_world || !to_local) return fail(PUPIL_ERR_INVALID, "null argument");
    if (const int rc = pt->emitters.env_map_held()) return rc;
    HIP_TRY(hipSetDevice(pt->device));
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(order_after_renders(pt));  // no render may still read the old parameters
    pt->pipe.invalidate();
    if (const int rc = pt->emitters.write_env_params(scale, to_world, to_local, pt->own_stream)) return rc;
    pt->env_updates++;
    pt->env_ms = ms_since(t0);
    return PUPIL_OK;
}

int pupil_pt_env_info(pupil_pt *pt, uint64_t *updates, double *last_ms) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (updates) *updates = pt->env_updates;
    if (last_ms) *last_ms = pt->env_ms;
    return PUPIL_OK;
}

int pupil_pt_render(pupil_pt *pt, const pupil_pt_frame *out, const pupil_pt_launch *launch, void *hip_stream) {
    if (!pt || !out || !launch || !out->accum) return fail(PUPIL_ERR_INVALID, "null argument");
    if (launch->spp == 0) return PUPIL_OK;
    const uint32_t world = launch->tile_world ? launch->tile_world : 1u;
    const uint32_t ts = launch->tile_size ? launch->tile_size : 32u;
    if (launch->tile_rank >= world) return fail(PUPIL_ERR_INVALID, "tile_rank >= tile_world");
    HIP_TRY(hipSetDevice(pt->device));
    // NULL is HIP's default (null) stream, as everywhere in HIP: a caller that renders on
    // it and then reads the output on it (torch's default stream, for one) must see the
    // frame.  (Until r02 NULL selected the engine's own non-blocking stream, so e.g. a
    // gather issued on torch's default stream could read a frame still being rendered.)
    hipStream_t s = (hipStream_t)hip_stream;

    // local pixel map (cached per tiling)
    const uint32_t key[5] = {pt->width, pt->height, ts, launch->tile_rank, world};
    const uint32_t *map = nullptr;
    uint32_t num_local = 0;
    if (const int rc = local_pixel_map(pt, key, &map, &num_local)) return rc;
    if (num_local == 0) return PUPIL_OK;
    const size_t paths = (size_t)num_local * launch->spp;
    if (paths >= (1ull << 31)) return fail(PUPIL_ERR_UNSUPPORTED, "too many paths in one batch");
    const bool stats = (launch->collect_stats & PUPIL_STATS_COUNTERS) != 0;
    const bool timing = (launch->collect_stats & PUPIL_STATS_TIMING) != 0;
    // The reference takes integrator.max_depth unclamped at SetScene (pt_pass.cpp:112-115;
    // only the inspector clamps to 1..128): any depth renders.  Diagnostics sized per
    // bounce (tail buffer) cover the first kMaxDepth launches.
    const uint32_t depth = std::max(1u, launch->max_depth ? launch->max_depth : pt->max_depth);
    if (pt->rendered && s != pt->last_stream) {  // another stream: after everything the last one holds
        HIP_TRY(hipEventRecord(pt->ev_sync, pt->last_stream));
        HIP_TRY(hipStreamWaitEvent(s, pt->ev_sync, 0));
    }

    FrameParams fp{};
    fp.width = pt->width;
    fp.height = pt->height;
    fp.num_local = num_local;
    fp.num_paths = (uint32_t)paths;
    fp.spp = launch->spp;
    fp.seed0 = launch->random_seed;
    fp.cnt0 = launch->sample_cnt;
    fp.accumulate = launch->accumulate;
    fp.max_depth = depth;
    fp.compact = out->compact;
    fp.aov_local = out->compact;
    fp.pixel_map = map;
    fp.accum = (float4 *)out->accum;
    fp.frame = (float4 *)out->frame;
    fp.albedo = (float *)out->albedo;
    fp.normal = (float *)out->normal;
    fp.test = (float *)out->test;
    fp.nee_count = stats ? pt->trace_counters.get() + 16 : nullptr;
    fp.cull_cum = pt->sc.cull_n ? pt->cull_cum.get() : nullptr;
    // the culled-ray totals as they are before this render (pupil_pt_stats: its own count)
    pt->cull_counted = pt->cull_counted || pt->sc.cull_n != 0u;
    if (pt->cull_counted)
        HIP_TRY(hipMemcpyAsync(pt->cull_cum.get() + kCullShards * kCullStride, pt->cull_cum.get(),
                               sizeof(unsigned long long) * kCullShards * kCullStride, hipMemcpyDeviceToDevice, s));

    // PUPIL_STATS_TRACE_TIMING: events around the traversal launches only, summed over
    // every render since pupil_pt_stats last read them (a timed sequence of renders)
    const bool trace_timing = (launch->collect_stats & PUPIL_STATS_TRACE_TIMING) != 0 && !timing;
    RenderCtx cx{pt, s, stats, timing || trace_timing, TraceStats{pt->trace_counters.get()}, key};
    cx.trace_only = trace_timing;
    if (!(trace_timing && pt->pairs_keep)) {  // a new sum
        pt->trace_pairs = 0;
        for (int k = 0; k < 4; k++) pt->kept_ms[k] = 0.0, pt->kept_n[k] = 0;
    }
    if (trace_timing && pt->trace_pairs >= kMaxPairs) {  // a long unread sequence: fold the pending pairs
        HIP_TRY(hipEventSynchronize(pt->trace_events[2 * pt->trace_pairs - 1]));
        for (uint32_t i = 0; i < pt->trace_pairs; i++) {
            float m = 0.f;
            HIP_TRY(hipEventElapsedTime(&m, pt->trace_events[2 * i], pt->trace_events[2 * i + 1]));
            pt->kept_ms[pt->pair_kind[i]] += m;
            pt->kept_n[pt->pair_kind[i]]++;
        }
        pt->trace_pairs = 0;
    }
    cx.pair = trace_timing ? pt->trace_pairs : 0u;
    pt->pairs_keep = trace_timing;
    const bool tail = stats && std::getenv("PUPIL_TRACE_TAIL");
    if (tail && !pt->tail_buf.get()) {
        pt->tail_waves = pt->ovf_threads / 64u;
        if (pt->tail_buf.alloc((size_t)(kMaxDepth + 1) * pt->tail_waves * 4)) return fail(PUPIL_ERR_OOM, "tail buffer");
    }
    if (tail) HIP_TRY(hipMemsetAsync(pt->tail_buf.get(), 0, sizeof(unsigned long long) * (kMaxDepth + 1) * pt->tail_waves * 4, s));
    cx.tail = tail;
    pt->tail_launches = 0;
    // events only when times are asked for: one pair per stage launch (kind 0 primary extend,
    // 1 bounce trace, 2 shade), at most two stage launches per iteration and kMaxPairs in all
    if (cx.timing) {
        const uint64_t pairs_needed = std::min<uint64_t>((uint64_t)cx.pair + 2ull * depth + 1ull, kMaxPairs + 2ull * 64);
        cx.pair_cap = (uint32_t)pairs_needed;
        while (pt->trace_events.size() < 2 * pairs_needed) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            pt->trace_events.emplace_back(e);
        }
        if (pt->pair_kind.size() < pairs_needed) pt->pair_kind.resize(pairs_needed, 0);
    }
    pt->last_timed = stats || timing;
    if (pt->last_timed) HIP_TRY(hipEventRecord(pt->ev_begin, s));
    if (stats) HIP_TRY(hipMemsetAsync(pt->trace_counters.get(), 0, 32 * sizeof(unsigned long long), s));
    const int rc = render_pipelined(cx, fp, launch);
    if (rc) return rc;
    if (pt->last_timed) HIP_TRY(hipEventRecord(pt->ev_end, s));
    HIP_TRY(hipGetLastError());
    pt->trace_pairs = cx.pair;
    pt->last_paths = fp.num_paths;
    pt->last_stats = stats;
    pt->cull_last = true;
    pt->last_stream = s;
    pt->rendered = true;
    return PUPIL_OK;
}

int pupil_pt_stats(pupil_pt *pt, pupil_pt_counters *out) {
    if (!pt || !out) return fail(PUPIL_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(pt->device));
    if (pt->rendered) HIP_TRY(hipStreamSynchronize(pt->last_stream));
    pupil_pt_counters c = pt->totals;
    unsigned long long cum[4] = {0, 0, 0, 0};  // running totals, then their values before the last render
    HIP_TRY(hipMemcpy(cum, pt->ray_cum.get(), sizeof(cum), hipMemcpyDeviceToHost));
    // extension rays the terminal-ray cull resolved: in all, and before the last render
    unsigned long long culled[2] = {0, 0};
    if (pt->cull_counted) {
        std::vector<unsigned long long> shards(2 * kCullShards * kCullStride);
        HIP_TRY(hipMemcpy(shards.data(), pt->cull_cum.get(), sizeof(unsigned long long) * shards.size(), hipMemcpyDeviceToHost));
        for (uint32_t h = 0; h < 2; h++)
            for (uint32_t k = 0; k < kCullShards; k++) culled[h] += shards[(h * kCullShards + k) * kCullStride];
    }
    c.terminal_rays_culled = culled[0];
    // rays resolved: a culled ray was cast by the integrator and is counted like a traced one
    c.rays_traced_total = pt->primary_cum + cum[0] + cum[1] + culled[0];
    c.frames_in_flight = pt->pipe.frames_in_flight();
    c.pipeline_slots = pt->pipe.slots;
    c.tlas_sah_splits = pt->accel.two_level ? pt->accel.tl.sah_splits : 0u;
    c.ring_bytes = pt->ring_bytes + sizeof(float) * (uint64_t)pt->aov_cap;
    c.ring_budget_bytes = (uint64_t)pt->knobs.budget;
    c.accel_refits = pt->accel.refits;
    for (const DevInstance &d : pt->h_insts()) c.hidden_instances += d.hidden ? 1u : 0u;
    c.frame_launches = pt->frame_launches;
    for (int a = 0; a < 3; a++) c.node_bound[a] = pt->sc.node_bound[a];
    if (pt->last_paths) {
        // rays traced by the last render's launches (pipelined renders: of every frame in
        // flight; a render whose only iteration traced camera rays lists none)
        c.primary_rays = pt->last_primary;
        c.path_samples = pt->last_paths;
        const unsigned long long culled_last = pt->cull_last ? culled[0] - culled[1] : 0ull;  // by the last render
        c.extension_rays = (pt->snap_taken ? cum[0] - cum[2] : 0u) + culled_last;
        c.shadow_rays = pt->snap_taken ? cum[1] - cum[3] : 0u;
        float ms = 0.f;
        if (pt->last_timed) HIP_TRY(hipEventElapsedTime(&ms, pt->ev_begin, pt->ev_end));
        c.last_render_ms = ms;
        double kind_ms[4] = {pt->kept_ms[0], pt->kept_ms[1], pt->kept_ms[2], pt->kept_ms[3]};
        uint64_t kind_n[4] = {pt->kept_n[0], pt->kept_n[1], pt->kept_n[2], pt->kept_n[3]};
        for (uint32_t i = 0; i < pt->trace_pairs; i++) {
            float m = 0.f;
            HIP_TRY(hipEventElapsedTime(&m, pt->trace_events[2 * i], pt->trace_events[2 * i + 1]));
            kind_ms[pt->pair_kind[i]] += m;
            kind_n[pt->pair_kind[i]]++;
        }
        pt->pairs_keep = false;  // read: the next PUPIL_STATS_TRACE_TIMING render starts a new sum
        c.trace_ms = kind_ms[0] + kind_ms[1];
        c.trace_launches = kind_n[0] + kind_n[1];
        c.extend_ms = kind_ms[0];
        c.extend_launches = kind_n[0];
        c.shade_ms = kind_ms[2];
        c.frame_ms = kind_ms[3];
        if (pt->last_stats && pt->tail_buf.get() && pt->tail_launches) {  // PUPIL_TRACE_TAIL summary on stderr
            std::vector<unsigned long long> tb((size_t)pt->tail_launches * pt->tail_waves * 4);
            HIP_TRY(hipMemcpy(tb.data(), pt->tail_buf.get(), sizeof(unsigned long long) * tb.size(), hipMemcpyDeviceToHost));
            for (uint32_t l = 0; l < pt->tail_launches; l++) {
                const unsigned long long *w = tb.data() + (size_t)l * pt->tail_waves * 4;
                std::vector<double> st, dr, ex;
                unsigned long long t0 = ~0ull, rays = 0;
                for (uint32_t k = 0; k < pt->tail_waves; k++)
                    if (w[4 * k + 2]) t0 = std::min(t0, w[4 * k]);
                for (uint32_t k = 0; k < pt->tail_waves; k++) {
                    if (!w[4 * k + 2]) continue;
                    st.push_back((double)(w[4 * k] - t0) * 0.01);  // 100 MHz -> us
                    dr.push_back(w[4 * k + 1] ? (double)(w[4 * k + 1] - t0) * 0.01 : -1.0);
                    ex.push_back((double)(w[4 * k + 2] - t0) * 0.01);
                    rays += w[4 * k + 3];
                }
                if (ex.empty()) continue;
                auto pct = [](std::vector<double> v, double q) {
                    std::sort(v.begin(), v.end());
                    return v[std::min(v.size() - 1, (size_t)(q * (double)v.size()))];
                };
                std::fprintf(stderr,
                             "[pupil tail] launch %u: %zu waves, %llu rays; start p50 %.1f max %.1f us; drained "
                             "first %.1f p50 %.1f us; exit p10 %.1f p50 %.1f p90 %.1f p99 %.1f max %.1f us\n",
                             l, ex.size(), rays, pct(st, 0.5), pct(st, 1.0), pct(dr, 0.0), pct(dr, 0.5), pct(ex, 0.1),
                             pct(ex, 0.5), pct(ex, 0.9), pct(ex, 0.99), pct(ex, 1.0));
            }
        }
        if (pt->last_stats) {
            unsigned long long tc[32];
            HIP_TRY(hipMemcpy(tc, pt->trace_counters.get(), sizeof(tc), hipMemcpyDeviceToHost));
            if (std::getenv("PUPIL_TRACE_DIAG") && tc[2]) {  // SIMD efficiency, persistent kernels
                const unsigned long long *d = tc + 2;
                const double visits = (double)std::max(1ull, tc[0] + tc[14]);
                std::fprintf(stderr,
                             "[pupil] traversal: node loop %llu wave-iters, %.1f%% lanes active; leaf loop %llu wave-iters, "
                             "%.1f%% lanes active; %llu refills, %.1f lanes each; node visits %.0f, %.1f%% with no child "
                             "hit, %.1f%% of a popped node already beyond tmax\n",
                             d[0], 100.0 * (double)d[1] / (64.0 * (double)d[0]), d[2],
                             100.0 * (double)d[3] / (64.0 * (double)std::max(1ull, d[2])), d[4],
                             (double)d[5] / (double)std::max(1ull, d[4]), visits, 100.0 * (double)tc[9] / visits,
                             100.0 * (double)tc[8] / visits);
            }
            c.node_loop_iters = tc[2];  // trace4_body dg[0..5]
            c.node_loop_lanes = tc[3];
            c.leaf_loop_iters = tc[4];
            c.leaf_loop_lanes = tc[5];
            c.refills = tc[6];
            c.refill_lanes = tc[7];
            c.node_visits = tc[0] + tc[14];
            c.prim_tests = tc[1] + tc[15];
            c.shadow_rays_reference = tc[16];
            c.unique_node_fetches = tc[18];
            // every ray the integrator handed over, each exactly once: the persistent launches'
            // counters, and the rays the terminal-ray cull took and resolved in its one step
            c.queue_handed = tc[20] + culled_last;
            c.queue_activated = tc[21] + culled_last;
            c.queue_retired = tc[22] + culled_last;
            c.queue_listed = tc[23] + culled_last;
            c.extend_node_visits = tc[0];
            c.extend_prim_tests = tc[1];
            const double rays = (double)(c.primary_rays + c.extension_rays + c.shadow_rays);
            // 32 B ray read + 16 B hit write + 64 B per node + 48 B per primitive
            c.trace_bytes = rays * 48.0 + 64.0 * (double)c.node_visits + 48.0 * (double)c.prim_tests;
            c.extend_bytes = (double)(c.primary_rays + c.extension_rays) * 48.0 + 64.0 * (double)tc[0] +
                             48.0 * (double)tc[1];
        }
    }
    *out = c;
    return PUPIL_OK;
}

int pupil_pt_shadow_info(pupil_pt *pt, uint64_t *occluded_rays, uint64_t *occluded_visits, uint32_t *overlap_order) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(pt->device));
    if (pt->rendered) HIP_TRY(hipStreamSynchronize(pt->last_stream));
    unsigned long long tc[32] = {};
    if (pt->last_stats) HIP_TRY(hipMemcpy(tc, pt->trace_counters.get(), sizeof(tc), hipMemcpyDeviceToHost));
    if (occluded_visits) *occluded_visits = tc[24];
    if (occluded_rays) *occluded_rays = tc[25];
    if (overlap_order) *overlap_order = pt->any_overlap;
    return PUPIL_OK;
}

void pupil_pt_destroy(pupil_pt *pt) { delete pt; }

int pupil_pt_export_bvh4(pupil_pt *pt, uint32_t *num_nodes, void *nodes, uint32_t *num_records, float *records,
                         int32_t *root_link) {
    if (!pt || !num_nodes || !num_records || !root_link) return fail(PUPIL_ERR_INVALID, "null argument");
    if (pt->accel.two_level) return fail(PUPIL_ERR_UNSUPPORTED, "only the flattened BVH4 is exported");
    HIP_TRY(hipSetDevice(pt->device));
    const BvhBuildOutput &bvh = pt->accel.bvh;
    const uint32_t nn = bvh.num_nodes4, nr = bvh.num_records;
    if (nodes || records) {
        if (*num_nodes < nn || *num_records < nr) return fail(PUPIL_ERR_INVALID, "output too small");
        HIP_TRY(hipDeviceSynchronize());
        if (nodes && nn) HIP_TRY(hipMemcpy(nodes, bvh.nodes4, sizeof(Bvh4Node) * nn, hipMemcpyDeviceToHost));
        if (records && nr) {  // record slots as 12 floats each (the 4th float4 of a slot is unused)
            std::vector<float4> h((size_t)kRecF4 * nr);
            HIP_TRY(hipMemcpy(h.data(), bvh.prims, sizeof(float4) * h.size(), hipMemcpyDeviceToHost));
            for (size_t r = 0; r < nr; r++) std::memcpy(records + 12 * r, &h[kRecF4 * r], 3 * sizeof(float4));
        }
    }
    *num_nodes = nn;
    *num_records = nr;
    *root_link = (int32_t)bvh.root_link4;
    return PUPIL_OK;
}

// Read-only: no kernel, no launch order touched; the device synchronise puts it after everything
// enqueued so far, like pupil_pt_export_bvh4.
int pupil_debug_export_world_bvh4(pupil_pt *pt, uint32_t *num_nodes, void *nodes, uint32_t *num_records, float *records,
                                  uint32_t *num_instances, float *inst_boxes, int32_t *root_link, uint32_t *tlas_nodes,
                                  uint32_t *tlas_cap, uint32_t *braid) {
    if (!pt || !num_nodes || !num_records || !num_instances) return fail(PUPIL_ERR_INVALID, "null argument");
    if (!pt->accel.two_level || !pt->accel.tl.world)
        return fail(PUPIL_ERR_UNSUPPORTED, "only the world-mode two-level structure is exported");
    HIP_TRY(hipSetDevice(pt->device));
    const TwoLevelAccel &tl = pt->accel.tl;
    const uint32_t nn = tl.num_wnodes, nr = pt->accel.world_record_slots(), ni = (uint32_t)tl.inst_shape.size();
    if (nodes || records || inst_boxes) {
        if (*num_nodes < nn || *num_records < nr || *num_instances < ni) return fail(PUPIL_ERR_INVALID, "output too small");
        HIP_TRY(hipDeviceSynchronize());
        if (nodes && nn) HIP_TRY(hipMemcpy(nodes, tl.wnodes, sizeof(Bvh4Node) * nn, hipMemcpyDeviceToHost));
        if (records && nr) {  // record slots as 12 floats each (the 4th float4 of a slot is unused)
            std::vector<float4> h((size_t)kRecF4 * nr);
            HIP_TRY(hipMemcpy(h.data(), tl.wprims, sizeof(float4) * h.size(), hipMemcpyDeviceToHost));
            for (size_t r = 0; r < nr; r++) std::memcpy(records + 12 * r, &h[kRecF4 * r], 3 * sizeof(float4));
        }
        if (inst_boxes && ni) HIP_TRY(hipMemcpy(inst_boxes, tl.d_boxes, sizeof(float) * 6 * ni, hipMemcpyDeviceToHost));
    }
    *num_nodes = nn;
    *num_records = nr;
    *num_instances = ni;
    if (root_link) *root_link = (int32_t)tl.root_link4;
    if (tlas_nodes) *tlas_nodes = tl.tlas_nodes;
    if (tlas_cap) *tlas_cap = tl.tlas_cap;
    if (braid) *braid = tl.braid;
    return PUPIL_OK;
}

int pupil_pt_trace_rays(pupil_pt *pt, uint32_t n, const float *rays, float *out, int any_hit) {
    if (!pt || !rays || !out) return fail(PUPIL_ERR_INVALID, "null argument");
    if (n == 0) return PUPIL_OK;
    HIP_TRY(hipSetDevice(pt->device));
    HIP_TRY(hipDeviceSynchronize());  // no render on another stream may still use the shared overflow stacks
    ScratchBuf<float> d_rays, d_out;
    HIP_TRY(upload(d_rays, rays, 8 * (size_t)n));
    HIP_TRY(d_out.alloc(4 * (size_t)n));
    // PUPIL_TRACE_RAYS_STATS: the counter kernels (queue accounting, node visits), read back
    // by pupil_pt_stats like a collect_stats render's
    const bool stats = std::getenv("PUPIL_TRACE_RAYS_STATS") != nullptr;
    TraceStats ts{pt->trace_counters.get()};
    HIP_TRY(hipMemsetAsync(pt->q.work + kWorkRays, 0, kWorkKind * sizeof(uint32_t), pt->own_stream));
    if (stats) HIP_TRY(hipMemsetAsync(pt->trace_counters.get(), 0, 32 * sizeof(unsigned long long), pt->own_stream));
    HIP_TRY(hipEventRecord(pt->ev_begin, pt->own_stream));
    launch_trace_debug(pt->sc, d_rays.get(), d_out.get(), n, any_hit, pt->ovf.get(), pt->ovf_threads, pt->q.work + kWorkRays,
                       pt->own_stream, stats ? &ts : nullptr, pt->any_overlap);
    HIP_TRY(hipEventRecord(pt->ev_end, pt->own_stream));
    HIP_TRY(hipStreamSynchronize(pt->own_stream));
    if (stats) {
        pt->last_paths = n;
        pt->last_iters = 0;
        pt->last_primary = n;
        pt->last_stats = true;
        pt->last_timed = true;
        pt->snap_taken = false;
        pt->cull_last = false;
        pt->trace_pairs = 0;
        for (int k = 0; k < 4; k++) pt->kept_ms[k] = 0.0, pt->kept_n[k] = 0;
        pt->rendered = true;
        pt->last_stream = pt->own_stream;
    }
    HIP_TRY(hipMemcpy(out, d_out.get(), sizeof(float) * 4 * (size_t)n, hipMemcpyDeviceToHost));
    return PUPIL_OK;
}

// Flow AOV (pt_flow.hip): camera rays through the pixel centres, the production traversal,
// the projection of the hits through the previous camera.  Runs on hip_stream, ordered by
// stream events after every render enqueued so far (the traversal's overflow stacks are shared
// with them), and the renders after it order themselves behind it the same way.  Its traversal
// has its own work-counter slot and adds to none of the ray totals pupil_pt_stats reports.
// While shapes hold vertex snapshots the projection also takes the vertex motion off the hit
// point (k_flow_project_deform); with none held the pass is launched as it always was.
int pupil_pt_motion_vectors(pupil_pt *pt, const float prev_sample_to_camera[16], const float prev_camera_to_world[16],
                            const float *prev_to_world, void *out_flow, uint32_t compact, uint32_t tile_size,
                            uint32_t tile_rank, uint32_t tile_world, void *hip_stream) {
    if (!pt || !prev_sample_to_camera || !prev_camera_to_world || !out_flow)
        return fail(PUPIL_ERR_INVALID, "null argument");
    const uint32_t world = tile_world ? tile_world : 1u;
    const uint32_t ts = tile_size ? tile_size : 32u;
    if (tile_rank >= world) return fail(PUPIL_ERR_INVALID, "tile_rank >= tile_world");
    // sample <- world of the previous camera, inverted and multiplied in double
    double c2s[16], w2c[16];
    if (!invert4(prev_sample_to_camera, c2s) || !invert4(prev_camera_to_world, w2c))
        return fail(PUPIL_ERR_INVALID, "singular previous camera matrix");
    FlowJob job{};
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            double v = 0.0;
            for (int k = 0; k < 4; k++) v += c2s[4 * r + k] * w2c[4 * k + c];
            job.world_to_sample[4 * r + c] = (float)v;
        }
    HIP_TRY(hipSetDevice(pt->device));
    hipStream_t s = (hipStream_t)hip_stream;
    const uint32_t key[5] = {pt->width, pt->height, ts, tile_rank, world};
    uint32_t num_local = 0;
    if (const int rc = local_pixel_map(pt, key, &job.pixel_map, &num_local)) return rc;
    if (num_local == 0) return PUPIL_OK;
    if (!pt->flow_hits.get()) {  // first use: lists for the whole image serve every tiling (num_local <= w * h)
        const size_t cap = (size_t)pt->width * pt->height;
        if (!pt->flow_rays.get()) HIP_TRY(pt->flow_rays.alloc(2 * cap));
        HIP_TRY(pt->flow_hits.alloc(cap));
    }
    if (pt->rendered && s != pt->last_stream) {  // another stream: after everything the last one holds
        HIP_TRY(hipEventRecord(pt->ev_sync, pt->last_stream));
        HIP_TRY(hipStreamWaitEvent(s, pt->ev_sync, 0));
    }
    // vertex snapshots held: after the last snapshot copy (the vertex update that followed it has
    // synchronised the engine's stream), with the per-instance table of snapshot arrays
    InstanceScratch &in = pt->per_inst;
    const bool table = pt->snapshots > 0 && pt->flow_verts_stale;
    if (pt->snapshots > 0) HIP_TRY(hipStreamWaitEvent(s, pt->ev_snap, 0));
    if (prev_to_world || table) {
        if (!pt->ev_flow) HIP_TRY(hipEventCreateWithFlags(pt->ev_flow.put(), hipEventDisableTiming));
        else HIP_TRY(hipEventSynchronize(pt->ev_flow));  // the previous upload has left the staging copies
    }
    if (prev_to_world) {
        const size_t nf = 12 * pt->h_insts().size();
        if (!in.flow_prev.get()) HIP_TRY(in.flow_prev.alloc(nf));
        in.h_flow_prev.assign(prev_to_world, prev_to_world + nf);
        if (nf) HIP_TRY(hipMemcpyAsync(in.flow_prev.get(), in.h_flow_prev.data(), sizeof(float) * nf, hipMemcpyHostToDevice, s));
        job.prev_to_world = in.flow_prev.get();
    }
    if (table) {
        const size_t ni = pt->h_insts().size();
        if (!in.flow_verts.get()) HIP_TRY(in.flow_verts.alloc(ni));
        in.h_flow_verts.assign(ni, nullptr);
        for (size_t i = 0; i < ni; i++) {
            const ShapeDev &sd = pt->shapes[pt->accel.inst_shape[i]];
            if (sd.kind == PUPIL_SHAPE_MESH && sd.prev_valid) in.h_flow_verts[i] = sd.prev.get();
        }
        HIP_TRY(hipMemcpyAsync(in.flow_verts.get(), in.h_flow_verts.data(), sizeof(const float *) * ni, hipMemcpyHostToDevice, s));
        pt->flow_verts_stale = false;
    }
    if (prev_to_world || table) HIP_TRY(hipEventRecord(pt->ev_flow, s));
    const float *const *prev_verts = pt->snapshots > 0 ? in.flow_verts.get() : nullptr;
    job.width = pt->width;
    job.height = pt->height;
    job.n = num_local;
    job.compact = compact;
    HIP_TRY(hipMemsetAsync(pt->q.work + kWorkFlow, 0, kWorkKind * sizeof(uint32_t), s));
    launch_flow_rays(pt->sc, pt->width, pt->height, job.pixel_map, num_local, 0.5f, 0.5f, pt->flow_rays.get(), s);
    launch_trace_debug(pt->sc, (const float *)pt->flow_rays.get(), (float *)pt->flow_hits.get(), num_local, 0, pt->ovf.get(),
                       pt->ovf_threads, pt->q.work + kWorkFlow, s);
    launch_flow_project(pt->sc, job, pt->flow_rays.get(), pt->flow_hits.get(), (float2 *)out_flow, s, prev_verts);
    HIP_TRY(hipGetLastError());
    pt->last_stream = s;
    pt->rendered = true;
    return PUPIL_OK;
}

extern "C++" {
namespace {

// what both query entries check of their outputs before anything is enqueued: some array is
// wanted, any hit fills none but the hits, and every pointer is aligned for the accesses the
// kernels make -- 16 B for the hits (k_query_resolve loads a float4; the traversal's own four
// 4-B stores need less), 8 B for the texcoords (one float2 store), 4 B for the rest (the ids
// are dword stores, position and normal one 12-B global_store_dwordx3 each, which needs the
// alignment of its dwords only)
int check_query_outputs(const pupil_ray_hits *out, uint32_t flags) {
    if (!out) return fail(PUPIL_ERR_INVALID, "null argument");
    if (flags & ~(uint32_t)PUPIL_QUERY_ANY_HIT) return fail(PUPIL_ERR_INVALID, "unknown query flag");
    const bool resolved =
        out->instance || out->primitive || out->material || out->position || out->normal || out->texcoord;
    if (!out->hit && !resolved) return fail(PUPIL_ERR_INVALID, "no output array is wanted");
    if ((flags & PUPIL_QUERY_ANY_HIT) && resolved)
        return fail(PUPIL_ERR_INVALID, "an any-hit query fills only the hit array");
    auto misaligned = [](const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) != 0u; };
    if (misaligned(out->hit, 16) || misaligned(out->texcoord, 8) || misaligned(out->instance, 4) ||
        misaligned(out->primitive, 4) || misaligned(out->material, 4) || misaligned(out->position, 4) ||
        misaligned(out->normal, 4))
        return fail(PUPIL_ERR_INVALID, "misaligned output array (hit: 16 B, texcoord: 8 B, the others: 4 B)");
    return PUPIL_OK;
}

// The traversal of n rays and the resolve of their hits, enqueued on s.  Ordered by stream events
// after every render, flow pass and query enqueued so far -- the overflow stacks are shared --
// and what follows orders itself behind it the same way (last_stream).  make_rays (or null):
// enqueues what writes the ray list, after the ordering and inside the timed span.  scatter (or
// null): ray l's outputs go to element scatter[l] (a tiled camera query in the frame's index
// space); the traversal writes hits in ray order, so they pass through the scratch and the resolve
// kernel puts them in place.  A call whose scratch fits allocates nothing and synchronises nothing.
template <typename MakeRays>
int run_query(pupil_pt *pt, uint32_t n, const float4 *rays, uint32_t flags, const pupil_ray_hits *out, hipStream_t s,
              const uint32_t *scatter, MakeRays make_rays) {
    const bool any = (flags & PUPIL_QUERY_ANY_HIT) != 0u;
    const bool geo = out->position || out->normal || out->texcoord;
    const bool resolved = geo || out->instance || out->primitive || out->material;
    if (!pt->ev_q0) {
        HIP_TRY(hipEventCreate(pt->ev_q0.put()));
        HIP_TRY(hipEventCreate(pt->ev_q1.put()));
    }
    float4 *hits = (float4 *)out->hit;
    if (!hits || scatter) {  // resolved outputs without the hits: the engine's scratch holds them
        if (pt->query_cap < n) {
            // the scratch a query still in flight reads is freed only once its stream has passed it
            if (pt->query_hits.get() && pt->rendered) HIP_TRY(hipStreamSynchronize(pt->last_stream));
            const size_t cap = std::max<size_t>(n, 2 * pt->query_cap);
            ScratchBuf<float4> grown;  // the old block outlives the allocation of the new one
            HIP_TRY(grown.alloc(cap));
            pt->query_hits = std::move(grown);
            pt->query_cap = cap;
            pt->query_grows++;
        }
        hits = pt->query_hits.get();
    }
    const bool slots = geo && !pt->sc.two_level;  // reconstruct() names flat records by slot
    if (slots && !pt->query_slot.get()) {
        HIP_TRY(pt->query_slot.alloc(pt->tables.cur().num_prims));
        pt->query_grows++;
    }
    if (pt->rendered && s != pt->last_stream) {  // another stream: after everything the last one holds
        HIP_TRY(hipEventRecord(pt->ev_sync, pt->last_stream));
        HIP_TRY(hipStreamWaitEvent(s, pt->ev_sync, 0));
    }
    HIP_TRY(hipEventRecord(pt->ev_q0, s));
    make_rays();
    HIP_TRY(hipMemsetAsync(pt->q.work + kWorkQuery, 0, kWorkKind * sizeof(uint32_t), s));
    launch_trace_debug(pt->sc, (const float *)rays, (float *)hits, n, any ? 1 : 0, pt->ovf.get(), pt->ovf_threads,
                       pt->q.work + kWorkQuery, s, nullptr, pt->any_overlap);
    if (resolved || scatter) {
        const uint32_t rec_slots = slots ? pt->accel.world_record_slots() : 1u;
        if (slots && !pt->query_slot_valid) {
            launch_query_prim_slots(pt->sc.prims, rec_slots, pt->tables.cur().num_prims, pt->query_slot.get(), s);
            pt->query_slot_valid = true;
        }
        const QueryJob job{rays,
                           hits,
                           n,
                           rec_slots,
                           slots ? pt->query_slot.get() : nullptr,
                           (int32_t *)out->instance,
                           (int32_t *)out->primitive,
                           (int32_t *)out->material,
                           (float *)out->position,
                           (float *)out->normal,
                           (float2 *)out->texcoord,
                           scatter,
                           scatter ? (float4 *)out->hit : nullptr};
        launch_query_resolve(pt->sc, job, s);
    }
    HIP_TRY(hipEventRecord(pt->ev_q1, s));
    HIP_TRY(hipGetLastError());
    pt->queries++;
    pt->query_rays += n;
    pt->last_stream = s;
    pt->rendered = true;
    return PUPIL_OK;
}

}  // namespace
}

// Ray queries from device memory: the production traversal over a caller's ray list, read in
// place, then k_query_resolve (pt_query.hip) for whatever of pupil_ray_hits is wanted.  Its
// traversal has its own work-counter slot (kWorkQuery); it adds to none of the ray totals
// pupil_pt_stats reports and touches neither the accumulation nor the frames in flight.
int pupil_pt_query_rays(pupil_pt *pt, uint32_t n, const void *rays_device, uint32_t flags, const pupil_ray_hits *out,
                        void *hip_stream) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (const int rc = check_query_outputs(out, flags)) return rc;
    if (n >= (1u << 31)) return fail(PUPIL_ERR_INVALID, "too many rays in one query");
    if (n == 0) return PUPIL_OK;
    if (!rays_device) return fail(PUPIL_ERR_INVALID, "null argument");
    // the resolve kernel loads a ray as two float4 (the traversal's scalar loads need 4 B)
    if ((uintptr_t)rays_device & 15u) return fail(PUPIL_ERR_INVALID, "misaligned ray list (16 B)");
    HIP_TRY(hipSetDevice(pt->device));
    return run_query(pt, n, (const float4 *)rays_device, flags, out, (hipStream_t)hip_stream, nullptr, [] {});
}

// The G-buffer form: camera_path's ray at film jitter (jitter_x, jitter_y) through every local
// pixel (k_flow_rays, into the flow pass's ray scratch or rays_out_device), then the same trace
// and resolve; outputs indexed like the frame buffers.
int pupil_pt_query_camera(pupil_pt *pt, float jitter_x, float jitter_y, uint32_t compact, uint32_t tile_size,
                          uint32_t tile_rank, uint32_t tile_world, void *rays_out_device, const pupil_ray_hits *out,
                          void *hip_stream) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (const int rc = check_query_outputs(out, 0u)) return rc;
    if ((uintptr_t)rays_out_device & 15u) return fail(PUPIL_ERR_INVALID, "misaligned ray list (16 B)");
    const uint32_t world = tile_world ? tile_world : 1u;
    const uint32_t ts = tile_size ? tile_size : 32u;
    if (tile_rank >= world) return fail(PUPIL_ERR_INVALID, "tile_rank >= tile_world");
    HIP_TRY(hipSetDevice(pt->device));
    hipStream_t s = (hipStream_t)hip_stream;
    const uint32_t key[5] = {pt->width, pt->height, ts, tile_rank, world};
    const uint32_t *map = nullptr;
    uint32_t num_local = 0;
    if (const int rc = local_pixel_map(pt, key, &map, &num_local)) return rc;
    if (num_local == 0) return PUPIL_OK;
    // a rank's outputs in the frame's index space go to their pixels (the map; null = every pixel)
    const uint32_t *scatter = compact ? nullptr : map;
    float4 *rays = (float4 *)rays_out_device;
    if (!rays) {  // the flow pass's list, sized for the whole image: it serves every tiling
        if (!pt->flow_rays.get()) HIP_TRY(pt->flow_rays.alloc(2 * (size_t)pt->width * pt->height));
        rays = pt->flow_rays.get();
    }
    return run_query(pt, num_local, rays, 0u, out, s, scatter, [&] {
        launch_flow_rays(pt->sc, pt->width, pt->height, map, num_local, jitter_x, jitter_y, rays, s);
    });
}

// queries and rays since create, growths of the engine-owned scratch, and the device time of
// the last query from the events around it (waits for that query); any out pointer may be NULL
int pupil_pt_query_info(pupil_pt *pt, uint64_t *queries, uint64_t *rays, uint64_t *scratch_grows, double *last_ms) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (queries) *queries = pt->queries;
    if (rays) *rays = pt->query_rays;
    if (scratch_grows) *scratch_grows = pt->query_grows;
    if (last_ms) {
        *last_ms = 0.0;
        if (pt->queries) {
            HIP_TRY(hipSetDevice(pt->device));
            HIP_TRY(hipEventSynchronize(pt->ev_q1));
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, pt->ev_q0, pt->ev_q1));
            *last_ms = ms;
        }
    }
    return PUPIL_OK;
}

extern "C++" {
namespace {

// The radiance call's scratch for `need` <= rad_chunk paths: path state, queues and the identity
// id list carved from one block.  Grows geometrically up to rad_chunk and never shrinks; a growth
// waits for the calls in flight (everything later enqueued is ordered behind them on
// last_stream) and fills the id list on s.  A call that fits allocates and synchronises nothing.
int ensure_radiance_state(pupil_pt *pt, size_t need, hipStream_t s) {
    if (need <= pt->rad_cap) return PUPIL_OK;
    if (pt->rad_block.get() && pt->rendered) HIP_TRY(hipStreamSynchronize(pt->last_stream));
    const size_t cap = std::min(pt->rad_chunk, std::max(need, 2 * pt->rad_cap));
    auto up = [](size_t bytes) { return (bytes + 255u) & ~(size_t)255u; };
    const size_t rec = up(16 * cap), byte = up(cap);
    const size_t hist = up(sizeof(uint32_t) * partition_hist_entries((uint32_t)cap));
    const size_t total = 8 * rec + 2 * byte + up(4 * cap) + up(8 * cap) + up(4 * cap) + hist + up(4 * kCountSlots);
    pt->rad_cap = 0;
    HIP_TRY(pt->rad_block.alloc(total));
    char *b = pt->rad_block.get();
    auto take = [&b](size_t bytes) {
        char *p = b;
        b += bytes;
        return (void *)p;
    };
    PathState &ps = pt->rad_ps;
    ps.ray_o = (float4 *)take(rec);
    ps.ray_d = (float4 *)take(rec);
    ps.hit = (float4 *)take(rec);
    ps.thr = (float4 *)take(rec);
    ps.rad = (float4 *)take(rec);
    ps.misc = (uint4 *)take(rec);
    ps.sh_d = (float4 *)take(rec);
    ps.sh_c = (float4 *)take(rec);
    ps.mbin = (uint8_t *)take(byte);
    ps.sflags = (uint8_t *)take(byte);
    Queues &q = pt->rad_q;
    q.bins = (uint32_t *)take(up(4 * cap));
    q.nxsh = (uint32_t *)take(up(8 * cap));
    pt->rad_ids = (uint32_t *)take(up(4 * cap));
    q.hist = (uint32_t *)take(hist);
    q.counts = (uint32_t *)take(up(4 * kCountSlots));
    q.work = pt->q.work + kWorkRadiance;
    q.capacity = (uint32_t)cap;
    pt->rad_cap = cap;
    pt->rad_grows++;
    launch_identity_ids(pt->rad_ids, (uint32_t)cap, s);
    return PUPIL_OK;
}

// One chunk of a radiance call, enqueued on s: samples [s0, s0 + ns) of rays [r0, r0 + nr), ns * nr
// paths in the call's own path state.  Generate, the primary extend in its queue form (origins
// from the path state), then per bounce what render_pipelined runs for one frame without a ring --
// flags partition, mixed traversal, material partition (or list shading), shade -- and the
// accumulate into the caller's arrays at the chunk's offset.  Per path every operation and its
// order are the render's.
int radiance_chunk(pupil_pt *pt, hipStream_t s, const float4 *rays, const uint32_t *stream_ids,
                   const pupil_pt_launch *launch, const pupil_ray_radiance *out, uint32_t depth, uint32_t r0,
                   uint32_t nr, uint32_t s0, uint32_t ns) {
    const PathState &ps = pt->rad_ps;
    const Queues &q = pt->rad_q;
    const uint32_t np = nr * ns;
    // no flags byte of an earlier chunk is listed, no bin byte of one is partitioned (list
    // shading partitions no bin bytes)
    HIP_TRY(hipMemsetAsync(ps.sflags, 0, np, s));
    if (!pt->shade_list) HIP_TRY(hipMemsetAsync(ps.mbin, 0xFF, np, s));
    launch_generate_rays(RayGenJob{rays, stream_ids, r0, nr, np, launch->random_seed + s0}, ps, s);
    FrameParams fp{};
    fp.num_local = nr;
    fp.num_paths = np;
    fp.spp = ns;
    fp.seed0 = launch->random_seed + s0;
    fp.cnt0 = launch->sample_cnt + (launch->accumulate ? s0 : 0u);
    fp.accumulate = launch->accumulate;
    fp.max_depth = depth;
    fp.compact = 1;
    fp.aov_local = 1;  // AOVs and radiance are indexed by the ray, from the chunk's first
    fp.group = 1;
    fp.accum = (float4 *)out->radiance + r0;
    fp.albedo = out->albedo ? (float *)out->albedo + 3 * (size_t)r0 : nullptr;
    fp.normal = out->normal ? (float *)out->normal + 3 * (size_t)r0 : nullptr;
    fp.cull_cum = pt->sc.cull_n ? pt->rad_cum.get() : nullptr;
    for (uint32_t b = 0; b < depth; b++) {
        if (b == 0) {
            launch_extend(pt->sc, ps, q, pt->rad_ids, nullptr, np, pt->ovf.get(), pt->ovf_threads, nullptr, s);
        } else {
            // the rays the last shade spawned, in increasing path id: next and shadow lists -> q.nxsh
            launch_partition(ps.sflags, np, 2, kPartFlags, sflag_tag(depth, b - 1), q.nxsh, q.hist, q.counts + kCntNext,
                             q.counts + kStartNext, nullptr, nullptr, s, pt->rad_cum.get() + pupil_pt::kRadTotals, nullptr);
            if (depth > 64 && b % 16 == 0) {  // as a render of such a depth: stop once no path is left
                uint32_t c[2] = {1, 1};
                HIP_TRY(hipMemcpyAsync(c, q.counts + kCntNext, sizeof(c), hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                if (c[0] == 0 && c[1] == 0) break;
            }
            launch_trace_mixed(pt->sc, ps, q, pt->ovf.get(), pt->ovf_threads, nullptr, s, 0u, 0u, 0u, 0u, 0u, pt->any_overlap);
        }
        if (!pt->shade_list)
            launch_partition(ps.mbin, np, kPartMaxBins, kPartExclusive, 0u, q.bins, q.hist, q.counts,
                             q.counts + kStartBins, q.counts + kScratch, nullptr, s, nullptr, nullptr, pt->bin_mask);
        if (depth > 63) HIP_TRY(hipMemsetAsync(ps.sflags, 0, np, s));  // the 6-bit tags would alias
        const ShadeList list = !pt->shade_list ? kShadeBins : (b == 0 ? kShadeAll : kShadeNext);
        launch_shade(pt->sc, fp, ps, q, sflag_tag(depth, b), s, list, 0u, b == 0 ? np : 0u, np);
    }
    launch_accumulate(fp, ps, nullptr, false, s);
    return PUPIL_OK;
}

}  // namespace
}  // extern "C++"

// Path-traced radiance along rays from device memory: every path of __raygen__main with the
// caller's ray as its first, through the wavefront stages over a path state of the call's own
// (its own Queues, work-counter slot kWorkRadiance and ray totals).  Reads the engine's camera
// nowhere, adds to none of the ray totals pupil_pt_stats reports and touches neither a frame's
// accumulation nor the frames in flight of the pipelined ring.
int pupil_pt_radiance_rays(pupil_pt *pt, uint32_t n, const void *rays_device, const uint32_t *stream_ids_device,
                           const pupil_pt_launch *launch, const pupil_ray_radiance *out, void *hip_stream) {
    if (!pt || !launch || !out || !out->radiance) return fail(PUPIL_ERR_INVALID, "null argument");
    if (launch->spp == 0) return fail(PUPIL_ERR_INVALID, "spp = 0");
    if (n >= (1u << 31)) return fail(PUPIL_ERR_INVALID, "too many rays in one call");
    // k_generate_rays loads a ray as two float4, k_accumulate the radiance as one; the AOVs and
    // the ids are read and written by dwords
    if (((uintptr_t)rays_device & 15u) || ((uintptr_t)out->radiance & 15u) || ((uintptr_t)stream_ids_device & 3u) ||
        ((uintptr_t)out->albedo & 3u) || ((uintptr_t)out->normal & 3u))
        return fail(PUPIL_ERR_INVALID, "misaligned pointer (rays, radiance: 16 B, the others: 4 B)");
    if (n == 0) return PUPIL_OK;
    if (!rays_device) return fail(PUPIL_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(pt->device));
    hipStream_t s = (hipStream_t)hip_stream;
    const uint32_t depth = std::max(1u, launch->max_depth ? launch->max_depth : pt->max_depth);
    // chunks of at most rad_chunk paths: `per` rays by `sb` samples (all of them unless spp alone
    // exceeds the chunk; a later range of samples continues the running mean of the earlier ones)
    const uint32_t sb = (uint32_t)std::min<size_t>(launch->spp, pt->rad_chunk);
    const uint32_t per = (uint32_t)std::min<size_t>(n, pt->rad_chunk / sb);
    if (!pt->ev_r0) {
        HIP_TRY(hipEventCreate(pt->ev_r0.put()));
        HIP_TRY(hipEventCreate(pt->ev_r1.put()));
    }
    if (const int rc = ensure_radiance_state(pt, (size_t)sb * per, s)) return rc;
    if (pt->rendered && s != pt->last_stream) {  // another stream: after everything the last one holds
        HIP_TRY(hipEventRecord(pt->ev_sync, pt->last_stream));
        HIP_TRY(hipStreamWaitEvent(s, pt->ev_sync, 0));
    }
    HIP_TRY(hipEventRecord(pt->ev_r0, s));
    // from here work is on s: whatever follows orders itself behind it, also when a chunk fails
    pt->last_stream = s;
    pt->rendered = true;
    for (uint32_t s0 = 0; s0 < launch->spp; s0 += sb)
        for (uint32_t r0 = 0; r0 < n; r0 += per)
            if (const int rc = radiance_chunk(pt, s, (const float4 *)rays_device, stream_ids_device, launch, out, depth,
                                              r0, std::min(per, n - r0), s0, std::min(sb, launch->spp - s0)))
                return rc;
    HIP_TRY(hipEventRecord(pt->ev_r1, s));
    HIP_TRY(hipGetLastError());
    pt->rad_calls++;
    pt->rad_rays += n;
    return PUPIL_OK;
}

// calls and rays since create, the extension and shadow rays their paths cast (device totals of
// the call's own: reading them waits for the last call, as last_ms does), growths of the scratch
// and the device time of the last call from the events around it; any out pointer may be NULL
int pupil_pt_radiance_info(pupil_pt *pt, uint64_t *calls, uint64_t *rays, uint64_t *extension_rays,
                           uint64_t *shadow_rays, uint64_t *scratch_grows, double *last_ms) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (calls) *calls = pt->rad_calls;
    if (rays) *rays = pt->rad_rays;
    if (scratch_grows) *scratch_grows = pt->rad_grows;
    if (extension_rays) *extension_rays = 0;
    if (shadow_rays) *shadow_rays = 0;
    if (last_ms) *last_ms = 0.0;
    if (!pt->rad_calls || !(extension_rays || shadow_rays || last_ms)) return PUPIL_OK;
    HIP_TRY(hipSetDevice(pt->device));
    HIP_TRY(hipEventSynchronize(pt->ev_r1));
    if (extension_rays || shadow_rays) {
        std::vector<unsigned long long> cum(pupil_pt::kRadTotals + 2);
        HIP_TRY(hipMemcpy(cum.data(), pt->rad_cum.get(), sizeof(unsigned long long) * cum.size(), hipMemcpyDeviceToHost));
        unsigned long long culled = 0;  // cast by the integrator and counted like a traced ray
        for (uint32_t k = 0; k < kCullShards; k++) culled += cum[k * kCullStride];
        if (extension_rays) *extension_rays = cum[pupil_pt::kRadTotals] + culled;
        if (shadow_rays) *shadow_rays = cum[pupil_pt::kRadTotals + 1];
    }
    if (last_ms) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, pt->ev_r0, pt->ev_r1));
        *last_ms = ms;
    }
    return PUPIL_OK;
}

int pupil_debug_select_emitter(pupil_pt *pt, uint32_t n, const float *p, int32_t *out) {
    if (!pt || !p || !out) return fail(PUPIL_ERR_INVALID, "null argument");
    if (n == 0) return PUPIL_OK;
    HIP_TRY(hipSetDevice(pt->device));
    HIP_TRY(hipDeviceSynchronize());
    ScratchBuf<float> dp;
    ScratchBuf<int> dout;
    HIP_TRY(upload(dp, p, n));
    HIP_TRY(dout.alloc(n));
    launch_debug_select(pt->sc, dp.get(), dout.get(), n, pt->own_stream);
    HIP_TRY(hipStreamSynchronize(pt->own_stream));
    HIP_TRY(hipMemcpy(out, dout.get(), sizeof(int) * n, hipMemcpyDeviceToHost));
    return PUPIL_OK;
}

int pupil_debug_read_emitters(pupil_pt *pt, uint32_t first, uint32_t n, float *out) {
    if (!pt || (n && !out)) return fail(PUPIL_ERR_INVALID, "null argument");
    if (first > pt->sc.num_areas || n > pt->sc.num_areas - first) return fail(PUPIL_ERR_INVALID, "emitter range out of bounds");
    if (n == 0) return PUPIL_OK;
    HIP_TRY(hipSetDevice(pt->device));
    HIP_TRY(order_after_renders(pt));
    HIP_TRY(hipStreamSynchronize(pt->own_stream));
    std::vector<DevEmitter> areas(n);
    std::vector<float> cdf(n);
    HIP_TRY(hipMemcpy(areas.data(), pt->emitters.cur().areas.get() + first, sizeof(DevEmitter) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cdf.data(), pt->emitters.cur().cdf.get() + first, sizeof(float) * n, hipMemcpyDeviceToHost));
    for (uint32_t e = 0; e < n; e++) {
        const DevEmitter &d = areas[e];
        float *o = out + 24 * (size_t)e;
        o[0] = d.select_probability;
        o[1] = d.area;
        o[2] = cdf[e];
        std::memcpy(o + 3, &d.type, sizeof(float));
        for (int v = 0; v < 3; v++) {
            o[4 + 3 * v] = d.pos[v].x, o[5 + 3 * v] = d.pos[v].y, o[6 + 3 * v] = d.pos[v].z;
            o[13 + 3 * v] = d.nrm[v].x, o[14 + 3 * v] = d.nrm[v].y, o[15 + 3 * v] = d.nrm[v].z;
        }
        if (d.type >= PUPIL_EMITTER_POINT) {  // a delta light: center, color, (cutoff, beam, 0)
            o[4] = d.center.x, o[5] = d.center.y, o[6] = d.center.z;
            o[7] = d.color.x, o[8] = d.color.y, o[9] = d.color.z;
            o[10] = d.pos[0].x, o[11] = d.pos[0].y, o[12] = 0.f;
        }
        o[22] = o[23] = 0.f;
    }
    return PUPIL_OK;
}

int pupil_debug_shade_tables(pupil_pt *pt, uint32_t caps[4], uint32_t *fit) {
    if (caps) shade_table_caps(caps);
    if (fit) {
        if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
        *fit = shade_tables_fit(pt->sc);
    }
    return PUPIL_OK;
}

int pupil_debug_read_emitter_guide(pupil_pt *pt, uint32_t *bits, uint32_t *guide, uint32_t *inout_count) {
    if (!pt || !inout_count) return fail(PUPIL_ERR_INVALID, "null argument");
    const EngineEmitters::Generation &g = pt->emitters.cur();
    const uint32_t count = g.guide.get() ? (1u << g.guide_bits) + 1u : 0u;
    if (bits) *bits = g.guide_bits;
    if (guide && count) {
        if (*inout_count < count) return fail(PUPIL_ERR_INVALID, "output too small");
        HIP_TRY(hipSetDevice(pt->device));
        HIP_TRY(order_after_renders(pt));
        HIP_TRY(hipStreamSynchronize(pt->own_stream));
        HIP_TRY(hipMemcpy(guide, g.guide.get(), sizeof(uint32_t) * count, hipMemcpyDeviceToHost));
    }
    *inout_count = count;
    return PUPIL_OK;
}

extern "C++" {
namespace {
// one probe launch: n inputs of `in_w` floats up, `out_w` floats per input back
template <typename Launch>
int debug_probe(pupil_pt *pt, uint32_t n, const float *in, uint32_t in_w, float *out, uint32_t out_w, Launch launch) {
    HIP_TRY(hipSetDevice(pt->device));
    HIP_TRY(order_after_renders(pt));
    ScratchBuf<float> din, dout;
    HIP_TRY(upload(din, in, (size_t)in_w * n));
    HIP_TRY(dout.alloc((size_t)out_w * n));
    launch(din.get(), dout.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(pt->own_stream));
    HIP_TRY(hipMemcpy(out, dout.get(), sizeof(float) * out_w * n, hipMemcpyDeviceToHost));
    return PUPIL_OK;
}
}  // namespace
}  // extern "C++"

int pupil_debug_env(pupil_pt *pt, uint32_t n, const float *xi_or_dir, const float *pos_nrm, uint32_t mode, float *out) {
    if (!pt || !xi_or_dir || !pos_nrm || !out) return fail(PUPIL_ERR_INVALID, "null argument");
    if (mode > 1u) return fail(PUPIL_ERR_INVALID, "unknown mode");
    if (!pt->emitters.cur().env.get()) return fail(PUPIL_ERR_INVALID, "the scene has no env emitter");
    if (n == 0) return PUPIL_OK;
    if (mode == 0u)  // the CDF searches take random numbers: anything else is not an input of SampleDirect
        for (uint32_t i = 0; i < n; i++)
            if (!(xi_or_dir[3 * i] >= 0.f && xi_or_dir[3 * i] <= 1.f && xi_or_dir[3 * i + 1] >= 0.f && xi_or_dir[3 * i + 1] <= 1.f))
                return fail(PUPIL_ERR_INVALID, "xi outside [0, 1]");
    return debug_probe(pt, n, xi_or_dir, 3, out, 8, [&](const float *din, float *dout) {
        launch_debug_env(pt->sc, din, pos_nrm, mode, dout, n, pt->own_stream);
    });
}

int pupil_debug_emitter_sample(pupil_pt *pt, uint32_t emitter, uint32_t n, const float *xi, const float *pos_nrm,
                               float *out) {
    if (!pt || !xi || !pos_nrm || !out) return fail(PUPIL_ERR_INVALID, "null argument");
    if (emitter > pt->sc.num_areas) return fail(PUPIL_ERR_INVALID, "emitter index beyond the env's");
    const bool env = emitter == pt->sc.num_areas;
    if (env && !pt->emitters.cur().env.get()) return fail(PUPIL_ERR_INVALID, "the scene has no env emitter");
    if (n == 0) return PUPIL_OK;
    for (uint32_t i = 0; i < n; i++)  // the CDF searches take random numbers (pupil_debug_env)
        if (!(xi[3 * i] >= 0.f && xi[3 * i] <= 1.f && xi[3 * i + 1] >= 0.f && xi[3 * i + 1] <= 1.f))
            return fail(PUPIL_ERR_INVALID, "xi outside [0, 1]");
    const DevEmitter *e = env ? pt->emitters.cur().env.get() : pt->emitters.cur().areas.get() + emitter;
    return debug_probe(pt, n, xi, 3, out, 8, [&](const float *din, float *dout) {
        launch_debug_emitter_sample(e, din, pos_nrm, dout, n, pt->own_stream);
    });
}

int pupil_debug_read_env_tables(pupil_pt *pt, uint32_t *width, uint32_t *height, float *col_cdf, float *row_cdf,
                                float *row_weight, float *normalization) {
    if (!pt || !width || !height) return fail(PUPIL_ERR_INVALID, "null argument");
    if (const int rc = pt->emitters.env_map_held()) return rc;
    const DevEmitter &e = pt->emitters.cur().h_env;
    const size_t w = e.map_w, h = e.map_h;
    *width = e.map_w;
    *height = e.map_h;
    if (!col_cdf && !row_cdf && !row_weight && !normalization) return PUPIL_OK;
    HIP_TRY(hipSetDevice(pt->device));
    HIP_TRY(order_after_renders(pt));
    HIP_TRY(hipStreamSynchronize(pt->own_stream));
    if (col_cdf) HIP_TRY(hipMemcpy(col_cdf, e.col_cdf, sizeof(float) * (w + 1) * h, hipMemcpyDeviceToHost));
    if (row_cdf) HIP_TRY(hipMemcpy(row_cdf, e.row_cdf, sizeof(float) * (h + 1), hipMemcpyDeviceToHost));
    if (row_weight) HIP_TRY(hipMemcpy(row_weight, e.row_weight, sizeof(float) * h, hipMemcpyDeviceToHost));
    if (normalization)
        HIP_TRY(hipMemcpy(normalization, &pt->emitters.cur().env.get()->normalization, sizeof(float), hipMemcpyDeviceToHost));
    return PUPIL_OK;
}

int pupil_debug_tex_sample(pupil_pt *pt, uint32_t material, uint32_t slot, uint32_t n, const float *uv, float *out) {
    if (!pt || !uv || !out) return fail(PUPIL_ERR_INVALID, "null argument");
    if (material >= pt->materials.count() || slot >= 4u) return fail(PUPIL_ERR_INVALID, "no such material texture");
    if (n == 0) return PUPIL_OK;
    return debug_probe(pt, n, uv, 2, out, 3, [&](const float *din, float *dout) {
        launch_debug_tex(pt->sc, material, slot, din, dout, n, pt->own_stream);
    });
}

int pupil_debug_read_material(pupil_pt *pt, uint32_t material, uint32_t *type, float out[3]) {
    if (!pt || !type || !out) return fail(PUPIL_ERR_INVALID, "null argument");
    if (material >= pt->materials.count()) return fail(PUPIL_ERR_INVALID, "material index out of range");
    HIP_TRY(hipSetDevice(pt->device));
    HIP_TRY(order_after_renders(pt));
    HIP_TRY(hipStreamSynchronize(pt->own_stream));
    DevMaterial d;
    HIP_TRY(hipMemcpy(&d, pt->materials.device() + material, sizeof(d), hipMemcpyDeviceToHost));
    *type = d.type;
    out[0] = d.eta;
    out[1] = d.int_fdr;
    out[2] = d.specular_sampling_weight;
    return PUPIL_OK;
}

int pupil_debug_fill_tlas_reserve(pupil_pt *pt, float value) {
    if (!pt) return fail(PUPIL_ERR_INVALID, "null argument");
    if (!pt->accel.two_level) return fail(PUPIL_ERR_UNSUPPORTED, "the flattened BVH has no TLAS reserve");
    HIP_TRY(hipSetDevice(pt->device));
    HIP_TRY(order_after_renders(pt));
    const uint64_t lo = pt->accel.tl.tlas_nodes, hi = std::min<uint64_t>(pt->accel.tl.tlas_cap, pt->accel.nodes4_count());
    if (hi > lo) {
        std::vector<float> junk((hi - lo) * (sizeof(Bvh4Node) / sizeof(float)), value);
        HIP_TRY(hipMemcpyAsync((void *)(pt->sc.nodes4 + lo), junk.data(), sizeof(float) * junk.size(),
                               hipMemcpyHostToDevice, pt->own_stream));
        HIP_TRY(hipStreamSynchronize(pt->own_stream));
    }
    if (const int rc = pt->accel.publish()) return rc;
    return derive_cull_set(pt);
}

int pupil_debug_bvh_reinsert(int device, uint32_t n, const float *boxes, uint32_t rounds, double *cost,
                             uint32_t *kept, uint32_t *rejected) {
    if (!boxes || !cost) return fail(PUPIL_ERR_INVALID, "null argument");
    if (n < 2 || rounds > 64u) return fail(PUPIL_ERR_INVALID, "needs n >= 2 boxes and at most 64 rounds");
    HIP_TRY(hipSetDevice(device));
    std::vector<Bvh4Node> nodes;
    std::vector<uint32_t> order;
    ReinsertLog log;
    if (build_bvh4_over_boxes(boxes, n, nodes, order, nullptr, nullptr, (int)rounds, &log) != 0)
        return fail(PUPIL_ERR_HIP, "the box BVH build failed");
    if (log.costs.empty()) return fail(PUPIL_ERR_HIP, "out of device memory for the reinsertion pass");
    for (uint32_t r = 0; r <= rounds; r++) cost[r] = log.costs[std::min<size_t>(r, log.costs.size() - 1)];
    if (kept) *kept = (uint32_t)log.kept;
    if (rejected) *rejected = (uint32_t)log.rejected;
    return PUPIL_OK;
}

int pupil_debug_partition(int device, uint32_t n, uint32_t capacity, const uint8_t *keys, uint32_t nbins,
                          uint32_t mode, uint32_t shift_or_tag, uint32_t bin_mask, const uint64_t *cum_in,
                          uint32_t *out, uint32_t *counts, uint32_t *starts, uint32_t *total, uint32_t *log,
                          uint64_t *cum_out, uint64_t *snap, uint32_t *info) {
    if ((!keys && n > 0) || !out || !counts || !starts) return fail(PUPIL_ERR_INVALID, "null argument");
    if (nbins < 1u || nbins > (uint32_t)kPartMaxBins) return fail(PUPIL_ERR_INVALID, "nbins must be in 1..9");
    if (mode > 1u) return fail(PUPIL_ERR_INVALID, "mode must be 0 (exclusive) or 1 (flags)");
    if (mode == 1u && nbins != 2u) return fail(PUPIL_ERR_INVALID, "the flags mode has two bins");
    if (n > capacity) return fail(PUPIL_ERR_INVALID, "n exceeds the capacity");
    if (capacity > (1u << 28)) return fail(PUPIL_ERR_INVALID, "the capacity exceeds 2^28 paths");
    if (!cum_in && (cum_out || snap)) return fail(PUPIL_ERR_INVALID, "cum_out and snap need cum_in");
    HIP_TRY(hipSetDevice(device));
    constexpr uint32_t kFill = 0xA5A5A5A5u, kGuard = 64;
    const size_t per = mode == 1u ? 2 : 1;  // ids per path the list can hold
    const size_t hist_n = partition_hist_entries(capacity), out_n = per * capacity;
    uint32_t rounds = 0, blocks = 0;
    partition_geometry(n, &rounds, &blocks);
    if ((size_t)nbins * blocks > hist_n) return fail(PUPIL_ERR_INVALID, "the histogram would not fit its scratch");
    // counts, starts, log (kPartMaxBins each) and the total share one small buffer
    constexpr uint32_t kCounts = 0, kStarts = kPartMaxBins, kLog = 2 * kPartMaxBins, kTotal = 3 * kPartMaxBins;
    constexpr uint32_t kSmall = 3 * kPartMaxBins + 1;
    ScratchBuf<uint8_t> d_keys;
    ScratchBuf<uint32_t> d_hist, d_out, d_small;
    ScratchBuf<unsigned long long> d_cum;  // nbins totals, then nbins snapshots
    HIP_TRY(d_keys.alloc(n));
    HIP_TRY(d_hist.alloc(hist_n + kGuard));
    HIP_TRY(d_out.alloc(out_n + kGuard));
    HIP_TRY(d_small.alloc(kSmall));
    HIP_TRY(d_cum.alloc(2 * kPartMaxBins));
    // the engine never clears this scratch between launches: nothing may depend on zeros
    HIP_TRY(hipMemsetD32((hipDeviceptr_t)d_hist.get(), (int)kFill, hist_n + kGuard));
    HIP_TRY(hipMemsetD32((hipDeviceptr_t)d_out.get(), (int)kFill, out_n + kGuard));
    HIP_TRY(hipMemsetD32((hipDeviceptr_t)d_small.get(), (int)kFill, kSmall));
    HIP_TRY(hipMemsetD32((hipDeviceptr_t)d_cum.get(), (int)kFill, 2 * 2 * kPartMaxBins));
    if (n) HIP_TRY(hipMemcpy(d_keys.get(), keys, n, hipMemcpyHostToDevice));
    if (cum_in) HIP_TRY(hipMemcpy(d_cum.get(), cum_in, sizeof(uint64_t) * nbins, hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    launch_partition(d_keys.get(), n, nbins, mode == 1u ? kPartFlags : kPartExclusive, shift_or_tag, d_out.get(),
                     d_hist.get(), d_small.get() + kCounts, d_small.get() + kStarts, d_small.get() + kTotal,
                     d_small.get() + kLog, nullptr, cum_in ? d_cum.get() : nullptr,
                     cum_in && snap ? d_cum.get() + kPartMaxBins : nullptr, bin_mask);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint32_t> h_hist(hist_n + kGuard), h_out(out_n + kGuard);
    uint32_t h_small[kSmall];
    HIP_TRY(hipMemcpy(h_hist.data(), d_hist.get(), sizeof(uint32_t) * h_hist.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_out.data(), d_out.get(), sizeof(uint32_t) * h_out.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_small, d_small.get(), sizeof(h_small), hipMemcpyDeviceToHost));
    if (cum_out) HIP_TRY(hipMemcpy(cum_out, d_cum.get(), sizeof(uint64_t) * nbins, hipMemcpyDeviceToHost));
    if (snap) HIP_TRY(hipMemcpy(snap, d_cum.get() + kPartMaxBins, sizeof(uint64_t) * nbins, hipMemcpyDeviceToHost));
    std::copy(h_out.begin(), h_out.begin() + per * n, out);
    std::copy(h_small + kCounts, h_small + kCounts + nbins, counts);
    std::copy(h_small + kStarts, h_small + kStarts + nbins, starts);
    if (log) std::copy(h_small + kLog, h_small + kLog + nbins, log);
    if (total) *total = h_small[kTotal];
    if (info) {
        const auto untouched = [](const std::vector<uint32_t> &v, size_t from) {
            return std::all_of(v.begin() + from, v.end(), [](uint32_t w) { return w == kFill; });
        };
        info[0] = rounds;
        info[1] = blocks;
        info[2] = (uint32_t)hist_n;
        info[3] = untouched(h_hist, (size_t)nbins * blocks) && untouched(h_out, per * n) ? 1u : 0u;
    }
    return PUPIL_OK;
}

int pupil_debug_math(int device, uint32_t n, const float *x, const float *y2, float *out) {
    if (!x || !y2 || !out) return fail(PUPIL_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(device));
    ScratchBuf<float> dx, dy, dout;
    HIP_TRY(upload(dx, x, n));
    HIP_TRY(upload(dy, y2, n));
    HIP_TRY(dout.alloc(6 * (size_t)n));
    launch_debug_math(dx.get(), dy.get(), dout.get(), n, nullptr);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout.get(), sizeof(float) * 6 * n, hipMemcpyDeviceToHost));
    return PUPIL_OK;
}

}  // extern "C"
