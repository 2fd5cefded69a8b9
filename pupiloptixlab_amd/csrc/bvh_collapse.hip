// bvh_collapse.hip — stage 3 of the BVH builder: the binary tree -> 4-wide quantized nodes.
//   default                      SAH-optimal slot distribution (k_sah_dp, k_collapse_pick_sah),
//                                breadth first; PUPIL_SAH_LEAF lets the SAH keep larger leaves
//   PUPIL_BVH4_COLLAPSE=greedy   greedy surface-area opening (k_collapse_pick), breadth first
//   PUPIL_BVH4_COLLAPSE=parity   binary nodes at even depth (k_depth / k_flag4 / k_emit4); no
//                                level order, so such a tree cannot be refitted
// Subtrees of <= leaf_size primitives become one leaf.  Also here: the 64-bit exclusive scan the
// builder shares (PLOC compaction, the breadth-first numbering, the leaf slots).
#include "bvh_build_detail.h"

#include <algorithm>
#include <utility>

namespace pupil::bvh {

namespace {

// exclusive scan of 64-bit counts: block pass, block-sum pass, add pass
__global__ __launch_bounds__(kScanBlock) void k_scan64_blocks(unsigned long long *data, int n,
                                                            unsigned long long *sums) {
    __shared__ unsigned long long wsum[kScanBlock / 64];
    const int base = blockIdx.x * kScanBlock * kScanItems + threadIdx.x * kScanItems;
    unsigned long long v[kScanItems], tsum = 0;
    for (int k = 0; k < kScanItems; k++) {
        v[k] = base + k < n ? data[base + k] : 0ull;
        tsum += v[k];
    }
    unsigned long long inc = tsum;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = __shfl_up(inc, o);
        if ((int)__lane_id() >= o) inc += u;
    }
    if (__lane_id() == 63) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    if (threadIdx.x < 64) {
        const unsigned long long w = threadIdx.x < kScanBlock / 64 ? wsum[threadIdx.x] : 0ull;
        unsigned long long winc = w;
        for (int o = 1; o < kScanBlock / 64; o <<= 1) {
            const unsigned long long u = __shfl_up(winc, o);
            if ((int)threadIdx.x >= o) winc += u;
        }
        if (threadIdx.x < kScanBlock / 64) wsum[threadIdx.x] = winc - w;
        if (threadIdx.x == kScanBlock / 64 - 1) sums[blockIdx.x] = winc;
    }
    __syncthreads();
    unsigned long long run = wsum[threadIdx.x >> 6] + inc - tsum;
    for (int k = 0; k < kScanItems; k++) {
        if (base + k < n) data[base + k] = run;
        run += v[k];
    }
}

__global__ __launch_bounds__(kScanBlock) void k_scan64_sums(unsigned long long *sums, int nb,
                                                          unsigned long long *total) {
    // nb <= kScanBlock * kScanItems: reuse the block pass on a single block
    __shared__ unsigned long long wsum[kScanBlock / 64];
    const int base = threadIdx.x * kScanItems;
    unsigned long long v[kScanItems], tsum = 0;
    for (int k = 0; k < kScanItems; k++) {
        v[k] = base + k < nb ? sums[base + k] : 0ull;
        tsum += v[k];
    }
    unsigned long long inc = tsum;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = __shfl_up(inc, o);
        if ((int)__lane_id() >= o) inc += u;
    }
    if (__lane_id() == 63) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    if (threadIdx.x < 64) {
        const unsigned long long w = threadIdx.x < kScanBlock / 64 ? wsum[threadIdx.x] : 0ull;
        unsigned long long winc = w;
        for (int o = 1; o < kScanBlock / 64; o <<= 1) {
            const unsigned long long u = __shfl_up(winc, o);
            if ((int)threadIdx.x >= o) winc += u;
        }
        if (threadIdx.x < kScanBlock / 64) wsum[threadIdx.x] = winc - w;
        if (threadIdx.x == kScanBlock / 64 - 1) *total = winc;
    }
    __syncthreads();
    unsigned long long run = wsum[threadIdx.x >> 6] + inc - tsum;
    for (int k = 0; k < kScanItems; k++) {
        if (base + k < nb) sums[base + k] = run;
        run += v[k];
    }
}

__global__ void k_scan64_add(unsigned long long *data, int n, const unsigned long long *sums) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    data[i] += sums[i / (kScanBlock * kScanItems)];
}

// ---------------------------------------------------------------- parity BVH4 collapse
// Binary nodes at even depth become 4-wide nodes whose children are their
// grandchildren (or the child itself where the child is a leaf).
__global__ void k_depth(int n, const int *parent_internal, uint32_t *depth) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n - 1) return;
    uint32_t d = 0;
    for (int p = i; p != 0; p = parent_internal[p]) d++;
    depth[i] = d;
}

__global__ void k_flag4(int n, const int2 *ranges, const uint32_t *depth, uint32_t leaf_size, uint32_t *flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n - 1) return;
    const int2 r = ranges[i];
    flags[i] = ((depth[i] & 1u) == 0u && (uint32_t)(r.y - r.x + 1) > leaf_size) ? 1u : 0u;
}

__global__ void k_emit4(int n, const uint32_t *sorted_vals, const Aabb *prim_boxes, const int2 *children,
                        const int2 *ranges, const Aabb *node_boxes, const uint32_t *flags, const uint32_t *idx4,
                        uint32_t leaf_size, Bvh4Node *nodes4) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n - 1 || !flags[i]) return;
    int link[4];
    Aabb box[4];
    int nk = 0;
    auto add = [&](int c) {
        if (c < 0) {
            link[nk] = make_leaf((uint32_t)~c, 1u);
            box[nk] = prim_boxes[sorted_vals[~c]];
        } else {
            const int2 r = ranges[c];
            const uint32_t cnt = (uint32_t)(r.y - r.x + 1);
            link[nk] = cnt <= leaf_size ? make_leaf((uint32_t)r.x, cnt) : (int)idx4[c];
            box[nk] = node_boxes[c];
        }
        nk++;
    };
    const int2 c = children[i];
    for (int s = 0; s < 2; s++) {
        const int ch = s == 0 ? c.x : c.y;
        bool expand = false;
        if (ch >= 0) {
            const int2 r = ranges[ch];
            expand = (uint32_t)(r.y - r.x + 1) > leaf_size;  // odd-depth internal node: absorb it
        }
        if (expand) {
            const int2 g = children[ch];
            add(g.x);
            add(g.y);
        } else {
            add(ch);
        }
    }
    const Aabb nb = node_boxes[i];
    float clo[3][4], chi[3][4];
    for (int k = 0; k < 4; k++)
        for (int a = 0; a < 3; a++) {
            clo[a][k] = k < nk ? box[k].lo[a] : 0.f;
            chi[a][k] = k < nk ? box[k].hi[a] : 0.f;
        }
    Bvh4Node o;
    uint32_t ex, ey, ez;
    quantize_axis(nb.lo[0], nb.hi[0], clo[0], chi[0], nk, o.ox, ex, o.qlo_x, o.qhi_x);
    quantize_axis(nb.lo[1], nb.hi[1], clo[1], chi[1], nk, o.oy, ey, o.qlo_y, o.qhi_y);
    quantize_axis(nb.lo[2], nb.hi[2], clo[2], chi[2], nk, o.oz, ez, o.qlo_z, o.qhi_z);
    set_scales(o, ex, ey, ez);
    for (int k = 0; k < 4; k++) o.child[k] = k < nk ? link[k] : kEmptyLink;
    nodes4[idx4[i]] = o;
}

// ---------------------------------------------------------------- greedy BVH4 collapse
// Top-down, one level of 4-wide nodes per pass: a 4-wide node starts from its
// binary node's two children and repeatedly opens the child with the largest
// surface area (an internal binary node that is not a leaf-sized subtree) until
// it has four children (the wide-BVH collapse of Wald et al. 2008 / Ylitie et
// al. 2017).  Children that remain internal become the next level's 4-wide
// nodes, numbered breadth-first after a scan of their counts.
constexpr uint32_t kSahLeaf = 1u << 12;  // k_sah_dp decision: the subtree is one leaf
__device__ __forceinline__ bool opens(int c, const int2 *ranges, uint32_t leaf_size, const uint32_t *dec = nullptr) {
    if (c < 0) return false;
    if (dec) return (dec[c] & kSahLeaf) == 0u;
    const int2 r = ranges[c];
    return (uint32_t)(r.y - r.x + 1) > leaf_size;
}

__global__ void k_collapse_pick(int items, const int *item_node, const int2 *children, const int2 *ranges,
                                const Aabb *node_boxes, uint32_t leaf_size, int4 *clist,
                                unsigned long long *inner_count) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= items) return;
    const int b = item_node[t];
    int c[4];
    const int2 ch = children[b];
    c[0] = ch.x;
    c[1] = ch.y;
    int nk = 2;
    while (nk < 4) {
        int best = -1;
        float best_a = -1.f;
        for (int k = 0; k < nk; k++)
            if (opens(c[k], ranges, leaf_size)) {
                const float a = half_area(node_boxes[c[k]]);
                if (a > best_a) {
                    best_a = a;
                    best = k;
                }
            }
        if (best < 0) break;
        const int2 g = children[c[best]];
        c[best] = g.x;
        c[nk++] = g.y;
    }
    unsigned long long inner = 0;
    for (int k = 0; k < nk; k++) inner += opens(c[k], ranges, leaf_size) ? 1ull : 0ull;
    for (int k = nk; k < 4; k++) c[k] = kEmptyLink;
    clist[t] = make_int4(c[0], c[1], c[2], c[3]);
    inner_count[t] = inner;
}

__global__ void k_collapse_emit(int items, int base, int next_base, const int *item_node, const int4 *clist,
                                const unsigned long long *inner_pos, const uint32_t *sorted_vals,
                                const Aabb *prim_boxes, const int2 *ranges, const Aabb *node_boxes,
                                uint32_t leaf_size, int *next_items, Bvh4Node *nodes4, const uint32_t *dec) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= items) return;
    const int4 cl = clist[t];
    const int cc[4] = {cl.x, cl.y, cl.z, cl.w};
    int link[4];
    float clo[3][4], chi[3][4];
    int nk = 0;
    int pos = (int)inner_pos[t];
    for (int k = 0; k < 4; k++) {
        const int c = cc[k];
        if (c == kEmptyLink) break;
        Aabb b;
        if (c < 0) {
            link[nk] = make_leaf((uint32_t)~c, 1u);
            b = prim_boxes[sorted_vals[~c]];
        } else if (!opens(c, ranges, leaf_size, dec)) {
            const int2 r = ranges[c];
            link[nk] = make_leaf((uint32_t)r.x, (uint32_t)(r.y - r.x + 1));
            b = node_boxes[c];
        } else {
            next_items[pos] = c;
            link[nk] = next_base + pos;
            pos++;
            b = node_boxes[c];
        }
        for (int a = 0; a < 3; a++) {
            clo[a][nk] = b.lo[a];
            chi[a][nk] = b.hi[a];
        }
        nk++;
    }
    for (int k = nk; k < 4; k++)
        for (int a = 0; a < 3; a++) clo[a][k] = chi[a][k] = 0.f;
    const Aabb nb = node_boxes[item_node[t]];
    Bvh4Node o;
    uint32_t ex, ey, ez;
    quantize_axis(nb.lo[0], nb.hi[0], clo[0], chi[0], nk, o.ox, ex, o.qlo_x, o.qhi_x);
    quantize_axis(nb.lo[1], nb.hi[1], clo[1], chi[1], nk, o.oy, ey, o.qlo_y, o.qhi_y);
    quantize_axis(nb.lo[2], nb.hi[2], clo[2], chi[2], nk, o.oz, ez, o.qlo_z, o.qhi_z);
    set_scales(o, ex, ey, ez);
    for (int k = 0; k < 4; k++) o.child[k] = k < nk ? link[k] : kEmptyLink;
    nodes4[base + t] = o;
}

// ---------------------------------------------------------------- SAH-optimal BVH4 collapse
// (the default; PUPIL_BVH4_COLLAPSE=greedy keeps the greedy opening) The slot distribution of Ylitie, Karras & Laine 2017,
// section 4, for 4-wide nodes: bottom up over the binary tree, C(n, i) is the least
// cost of the subtree n when it may fill i slots of its parent, with
//   D(n, j)  = min over 0 < k < j of C(left, k) + C(right, j - k)
//   C(n, 1)  = A(n) + D(n, 4)            (n becomes a 4-wide node)
//   C(n, i)  = min(C(n, i - 1), D(n, i)) (n opened into up to i slots)
// Subtrees of at most leaf_size primitives are leaves, as in the greedy collapse, so
// their cost is the same in every distribution and only the surface area of the
// 4-wide nodes is minimised.  dec[n]: bits 0-1 / 2-3 / 4-5 the best k of D(n, 2/3/4),
// bits 8-10 "C(n, i) = C(n, i - 1)" for i = 2, 3, 4.
__global__ void k_sah_parents(int n, const int2 *children, int *parent, int *leaf_parent) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n - 1) return;
    const int2 c = children[b];
    if (c.x >= 0) parent[c.x] = b;
    else leaf_parent[~c.x] = b;
    if (c.y >= 0) parent[c.y] = b;
    else leaf_parent[~c.y] = b;
}

__device__ __forceinline__ float4 sah_cost(int c, const float4 *cost, const uint32_t *sorted_vals,
                                           const Aabb *prim_boxes) {
    if (c < 0) {  // one primitive: a leaf in every distribution
        const float a = half_area(prim_boxes[sorted_vals[~c]]);
        return make_float4(a, a, a, a);
    }
    const uint32_t *w = (const uint32_t *)(cost + c);  // written by another thread: device-coherent loads
    float4 v;
    v.x = __uint_as_float(__hip_atomic_load(w + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    v.y = __uint_as_float(__hip_atomic_load(w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    v.z = __uint_as_float(__hip_atomic_load(w + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    v.w = __uint_as_float(__hip_atomic_load(w + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    return v;
}

// one thread per primitive walks up; the second child to finish computes its parent
__global__ void k_sah_dp(int n, const int *parent, const int *leaf_parent, const int2 *children, const int2 *ranges,
                         const Aabb *node_boxes, const uint32_t *sorted_vals, const Aabb *prim_boxes,
                         uint32_t leaf_size, uint32_t sah_leaf, uint32_t *flags, float4 *cost, uint32_t *dec) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int b = leaf_parent[i];
    while (b >= 0) {
        __threadfence();
        if (atomicAdd(flags + b, 1u) == 0u) return;
        __threadfence();
        const int2 ch = children[b];
        const float4 l4 = sah_cost(ch.x, cost, sorted_vals, prim_boxes);
        const float4 r4 = sah_cost(ch.y, cost, sorted_vals, prim_boxes);
        const float cl[4] = {l4.x, l4.y, l4.z, l4.w}, cr[4] = {r4.x, r4.y, r4.z, r4.w};
        float d[5];
        uint32_t code = 0;
        for (int j = 2; j <= 4; j++) {
            float best = __builtin_huge_valf();
            uint32_t bk = 1;
            for (int k = 1; k < j; k++) {
                const float v = cl[k - 1] + cr[j - k - 1];
                if (v < best) {
                    best = v;
                    bk = (uint32_t)k;
                }
            }
            d[j] = best;
            code |= bk << (2 * (j - 2));
        }
        const int2 r = ranges[b];
        const float a = half_area(node_boxes[b]);
        float c4[4];
        const uint32_t cnt = (uint32_t)(r.y - r.x + 1);
        if (cnt <= leaf_size || (cnt <= sah_leaf && a * (float)cnt <= a + d[4])) {  // one leaf wherever it goes
            c4[0] = c4[1] = c4[2] = c4[3] = a * (float)cnt;
            code |= 7u << 8 | kSahLeaf;
        } else {
            c4[0] = a + d[4];
            for (int s = 2; s <= 4; s++) {
                if (c4[s - 2] <= d[s]) {
                    c4[s - 1] = c4[s - 2];
                    code |= 1u << (8 + s - 2);
                } else {
                    c4[s - 1] = d[s];
                }
            }
        }
        cost[b] = make_float4(c4[0], c4[1], c4[2], c4[3]);
        dec[b] = code;
        b = parent[b];
    }
}

// children of the 4-wide node made from binary node b: D(b, 4) distributed down the
// decisions, a subtree taking one slot (a leaf or the next level's 4-wide node) or
// being opened into the slots it was given
__global__ void k_collapse_pick_sah(int items, const int *item_node, const int2 *children, const int2 *ranges,
                                    const uint32_t *dec, uint32_t leaf_size, int4 *clist,
                                    unsigned long long *inner_count) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= items) return;
    const int b = item_node[t];
    const int2 ch = children[b];
    const uint32_t k4 = (dec[b] >> 4) & 3u;
    int wc[4], wi[4], nw = 0;  // work: (subtree, slots); slots add up to at most 4
    wc[nw] = ch.x, wi[nw++] = (int)k4;
    wc[nw] = ch.y, wi[nw++] = 4 - (int)k4;
    int c[4], nk = 0;
    while (nw > 0) {
        const int x = wc[--nw];
        int s = wi[nw];
        if (!opens(x, ranges, leaf_size, dec) || s <= 1) {
            c[nk++] = x;
            continue;
        }
        const uint32_t dx = dec[x];
        while (s > 1 && ((dx >> (8 + s - 2)) & 1u)) s--;  // C(x, s) = C(x, s - 1)
        if (s == 1) {
            c[nk++] = x;
            continue;
        }
        const int k = (int)((dx >> (2 * (s - 2))) & 3u);
        const int2 g = children[x];
        wc[nw] = g.x, wi[nw++] = k;
        wc[nw] = g.y, wi[nw++] = s - k;
    }
    unsigned long long inner = 0;
    for (int k = 0; k < nk; k++) inner += opens(c[k], ranges, leaf_size, dec) ? 1ull : 0ull;
    for (int k = nk; k < 4; k++) c[k] = kEmptyLink;
    clist[t] = make_int4(c[0], c[1], c[2], c[3]);
    inner_count[t] = inner;
}

// Breadth-first collapse, one level of 4-wide nodes per pass (k_collapse_pick[_sah] /
// k_collapse_emit): the SAH-optimal slot distribution (k_sah_dp) or, for Collapse::Greedy, the
// greedy opening.  The spare words are not used.
hipError_t collapse_levels(const BinaryTree &t, uint32_t leaf_size, const BuildOptions &opts, uint32_t *, uint32_t *,
                           hipStream_t s, Collapsed &out) {
    const int n = t.n;
    const bool sah = opts.collapse == BuildOptions::Collapse::Sah && n >= 2;
    const int cap = n;  // a level never has more 4-wide nodes than binary internal nodes
    hipError_t err = hipSuccess;
    out.nodes4 = scratch<Bvh4Node>(err, (size_t)(n - 1));
    auto items_a_buf = scratch<int>(err, cap);
    auto items_b_buf = scratch<int>(err, cap);
    auto clist = scratch<int4>(err, cap);
    auto cnt = scratch<unsigned long long>(err, cap);
    auto sums = scratch<unsigned long long>(err, scan64_blocks(cap));
    auto total = scratch<unsigned long long>(err, 1);
    DevBuf<int> parent, leaf_parent;
    DevBuf<uint32_t> sflags, dec;
    DevBuf<float4> cost;
    if (sah) {
        parent = scratch<int>(err, n);
        leaf_parent = scratch<int>(err, n);
        sflags = scratch<uint32_t>(err, n);
        cost = scratch<float4>(err, n);
        dec = scratch<uint32_t>(err, n);
        if (!err) err = hipMemsetAsync(parent.get(), 0xFF, sizeof(int) * n, s);  // root: -1
        if (!err) err = hipMemsetAsync(sflags.get(), 0, sizeof(uint32_t) * n, s);
        if (err) return err;
        hipLaunchKernelGGL(k_sah_parents, grid_for(n - 1), dim3(kBlock), 0, s, n, t.children, parent.get(),
                           leaf_parent.get());
        hipLaunchKernelGGL(k_sah_dp, grid_for(n), dim3(kBlock), 0, s, n, parent.get(), leaf_parent.get(), t.children,
                           t.ranges, t.node_boxes, t.prim_order, t.prim_boxes, leaf_size, opts.sah_leaf, sflags.get(),
                           cost.get(), dec.get());
    }
    int *items_a = items_a_buf.get(), *items_b = items_b_buf.get();
    int base = 0, items = 1;
    uint32_t levels = 0;  // breadth first: one iteration per BVH4 level
    out.level_start.clear();
    if (!err) err = hipMemsetAsync(items_a, 0, sizeof(int), s);  // binary root 0
    while (!err && items > 0) {
        out.level_start.push_back((uint32_t)base);
        if (sah)
            hipLaunchKernelGGL(k_collapse_pick_sah, grid_for(items), dim3(kBlock), 0, s, items, items_a, t.children,
                               t.ranges, dec.get(), leaf_size, clist.get(), cnt.get());
        else
            hipLaunchKernelGGL(k_collapse_pick, grid_for(items), dim3(kBlock), 0, s, items, items_a, t.children,
                               t.ranges, t.node_boxes, leaf_size, clist.get(), cnt.get());
        // the scan's capacity guard cannot trigger here: items <= n, and the scratch is sized for n
        err = scan64(cnt.get(), items, sums.get(), total.get(), s);
        if (err) break;
        hipLaunchKernelGGL(k_collapse_emit, grid_for(items), dim3(kBlock), 0, s, items, base, base + items, items_a,
                           clist.get(), cnt.get(), t.prim_order, t.prim_boxes, t.ranges, t.node_boxes, leaf_size,
                           items_b, out.nodes4.get(), sah ? dec.get() : nullptr);
        unsigned long long tot = 0;
        (void)hipMemcpyAsync(&tot, total.get(), sizeof(tot), hipMemcpyDeviceToHost, s);
        err = hipStreamSynchronize(s);
        base += items;
        items = (int)tot;
        levels++;
        if (base + items > n - 1) err = hipErrorUnknown;  // cannot happen
        std::swap(items_a, items_b);
    }
    out.num_nodes4 = (uint32_t)base;
    out.depth4 = levels;
    out.level_start.push_back((uint32_t)base);
    return err;
}

// depth parity -> flags -> compact indices -> nodes.  depth / flags4: the caller's spare words
hipError_t collapse_parity(const BinaryTree &t, uint32_t leaf_size, const BuildOptions &, uint32_t *depth,
                           uint32_t *flags4, hipStream_t s, Collapsed &out) {
    const int n = t.n;
    hipError_t err = hipSuccess;
    auto idx4 = scratch<uint32_t>(err, n);
    if (err) return err;
    hipLaunchKernelGGL(k_depth, grid_for(n - 1), dim3(kBlock), 0, s, n, t.parent_internal, depth);
    hipLaunchKernelGGL(k_flag4, grid_for(n - 1), dim3(kBlock), 0, s, n, t.ranges, depth, leaf_size, flags4);
    uint32_t tail[2] = {0, 0};
    (void)hipMemcpyAsync(idx4.get(), flags4, sizeof(uint32_t) * (n - 1), hipMemcpyDeviceToDevice, s);
    scan32(idx4.get(), (uint32_t)(n - 1), s);
    (void)hipMemcpyAsync(&tail[0], idx4.get() + (n - 2), sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    (void)hipMemcpyAsync(&tail[1], flags4 + (n - 2), sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    err = hipStreamSynchronize(s);
    if (err) return err;
    out.num_nodes4 = tail[0] + tail[1];
    out.nodes4 = scratch<Bvh4Node>(err, out.num_nodes4);
    if (err) return err;
    hipLaunchKernelGGL(k_emit4, grid_for(n - 1), dim3(kBlock), 0, s, n, t.prim_order, t.prim_boxes, t.children,
                       t.ranges, t.node_boxes, flags4, idx4.get(), leaf_size, out.nodes4.get());
    err = hipStreamSynchronize(s);
    if (!err && out.num_nodes4) {
        // depth of the 4-wide tree (the stack-capacity check and the statistics read it): its
        // nodes are the flagged binary nodes, at binary depth 2 j on 4-wide level j + 1
        std::vector<uint32_t> hd((size_t)n - 1), hf((size_t)n - 1);
        err = hipMemcpy(hd.data(), depth, sizeof(uint32_t) * hd.size(), hipMemcpyDeviceToHost);
        if (!err) err = hipMemcpy(hf.data(), flags4, sizeof(uint32_t) * hf.size(), hipMemcpyDeviceToHost);
        for (size_t i = 0; i < hd.size(); i++)
            if (hf[i]) out.depth4 = std::max(out.depth4, hd[i] / 2u + 1u);
    }
    return err;
}

}  // namespace

hipError_t scan64(unsigned long long *data, int n, unsigned long long *sums, unsigned long long *total,
                  hipStream_t s, unsigned long long *host_total) {
    const int nb = scan64_blocks(n);
    if (nb > kScanPer) return hipErrorInvalidValue;  // k_scan64_sums is one block: > 16.7 M items
    hipLaunchKernelGGL(k_scan64_blocks, dim3(nb), dim3(kScanBlock), 0, s, data, n, sums);
    hipLaunchKernelGGL(k_scan64_sums, dim3(1), dim3(kScanBlock), 0, s, sums, nb, total);
    hipLaunchKernelGGL(k_scan64_add, grid_for(n), dim3(kBlock), 0, s, data, n, sums);
    if (!host_total) return hipSuccess;
    return hipMemcpyAsync(host_total, total, sizeof(*host_total), hipMemcpyDeviceToHost, s);
}

hipError_t collapse_bvh4(const BinaryTree &t, uint32_t leaf_size, const BuildOptions &opts, uint32_t *spare_a,
                         uint32_t *spare_b, hipStream_t s, Collapsed &out) {
    const auto stage = opts.collapse == BuildOptions::Collapse::Parity ? collapse_parity : collapse_levels;
    return stage(t, leaf_size, opts, spare_a, spare_b, s, out);
}

}  // namespace pupil::bvh
