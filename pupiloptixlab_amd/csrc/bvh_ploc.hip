// bvh_ploc.hip — stage 2 of the BVH builder: the binary tree over the Morton order.
//   default                  PLOC (k_ploc_*), reinsertion rounds over its tree (bvh_reinsert.hip),
//                            then the export to the arrays below in a new primitive order
//   PUPIL_BVH_BUILDER=lbvh   k_karras (Karras 2012 over the sorted codes, index-augmented) and
//                            k_refit (bottom-up boxes); also the fallback of build_bvh_bounded
// Both leave children / ranges / node boxes / parents with root 0 and contiguous subtrees.
#include "bvh_build_detail.h"

#include <utility>

namespace pupil::bvh {

namespace {

// ---------------------------------------------------------------- Karras 2012
__device__ __forceinline__ int delta(const uint32_t *keys, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    const uint32_t a = keys[i], b = keys[j];
    if (a == b) return 32 + __clz((uint32_t)i ^ (uint32_t)j);
    return __clz(a ^ b);
}

__global__ void k_karras(const uint32_t *keys, int n, int2 *children, int2 *ranges, int *parent_internal,
                         int *parent_leaf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n - 1) return;
    const int d = (delta(keys, n, i, i + 1) - delta(keys, n, i, i - 1)) >= 0 ? 1 : -1;
    const int dmin = delta(keys, n, i, i - d);
    int lmax = 2;
    while (delta(keys, n, i, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int t = lmax >> 1; t >= 1; t >>= 1)
        if (delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = delta(keys, n, i, j);
    int s = 0;
    int t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int gamma = i + s * d + min(d, 0);
    const int first = min(i, j), last = max(i, j);
    // child encoding here: >= 0 internal, < 0 -> leaf ~prim
    const int left = (first == gamma) ? ~gamma : gamma;
    const int right = (last == gamma + 1) ? ~(gamma + 1) : gamma + 1;
    children[i] = make_int2(left, right);
    ranges[i] = make_int2(first, last);
    if (left >= 0) parent_internal[left] = i;
    else parent_leaf[gamma] = i;
    if (right >= 0) parent_internal[right] = i;
    else parent_leaf[gamma + 1] = i;
}

// Bottom-up refit.  The second thread to arrive at a node merges both
// children.  Bounds are published with an agent-scope release before the
// arrival atomic and read after an agent-scope acquire (L1s are per CU and the
// per-XCD L2s are not coherent, MI355X_MICROARCH.md "inter-workgroup visibility").
__global__ void k_refit(int n, const uint32_t *sorted_vals, const Aabb *prim_boxes, const int2 *children,
                        const int *parent_internal, const int *parent_leaf, Aabb *node_boxes, uint32_t *flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int node = parent_leaf[i];
    while (node >= 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const uint32_t prev = __hip_atomic_fetch_add(&flags[node], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == 0u) return;  // first arrival: the sibling finishes the node
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const int2 c = children[node];
        const Aabb a = c.x >= 0 ? node_boxes[c.x] : prim_boxes[sorted_vals[~c.x]];
        const Aabb b = c.y >= 0 ? node_boxes[c.y] : prim_boxes[sorted_vals[~c.y]];
        node_boxes[node] = merge(a, b);
        node = node == 0 ? -1 : parent_internal[node];
    }
}

// ---------------------------------------------------------------- PLOC
// Parallel locally-ordered clustering (Meister & Bittner 2018) over the
// Morton-ordered primitives: each cluster finds its nearest neighbour (smallest
// union surface area, ties to the smaller index) within +-kPlocRadius (32: 2.5 % faster frames than 16 on config 4, 64 no better; profiles/r02_ploc_radius_ab.txt)
// positions, mutual pairs merge, the cluster list is compacted in order, and
// this repeats until one cluster is left.  It yields a tree of markedly lower
// SAH cost than the Karras hierarchy over the same order.  The result is
// converted to the LBVH arrays (children / ranges / parents / node boxes, root
// 0, subtrees contiguous in a new primitive order) so emit and the BVH4
// collapse are shared.  Refs: >= 0 internal node (creation id), < 0 leaf ~pos.
constexpr int kPlocRadius = 32;

__global__ void k_ploc_init(int n, const uint32_t *sorted_vals, const Aabb *prim_boxes, int *ref, Aabb *box) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ref[i] = ~i;
    box[i] = prim_boxes[sorted_vals[i]];
}

__global__ __launch_bounds__(kBlock) void k_ploc_nn(int m, const Aabb *box, int *nn) {
    __shared__ Aabb tile[kBlock + 2 * kPlocRadius];
    const int base = blockIdx.x * kBlock - kPlocRadius;
    for (int t = threadIdx.x; t < kBlock + 2 * kPlocRadius; t += kBlock) {
        const int j = base + t;
        if (j >= 0 && j < m) tile[t] = box[j];
    }
    __syncthreads();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const Aabb bi = tile[threadIdx.x + kPlocRadius];
    float best = __builtin_huge_valf();
    int bj = -1;
    const int j0 = max(0, i - kPlocRadius), j1 = min(m - 1, i + kPlocRadius);
    for (int j = j0; j <= j1; j++) {
        if (j == i) continue;
        const float a = half_area(merge(bi, tile[j - base]));
        if (a < best) {  // ascending j: ties keep the smaller index
            best = a;
            bj = j;
        }
    }
    nn[i] = bj;
}

// per cluster: low word = survives (1), high word = creates a node (1)
__global__ void k_ploc_flags(int m, const int *nn, unsigned long long *flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int j = nn[i];
    const bool mutual = nn[j] == i;
    const unsigned long long keep = (mutual && i > j) ? 0ull : 1ull;
    const unsigned long long make = (mutual && i < j) ? 1ull : 0ull;
    flags[i] = keep | (make << 32);
}

__global__ void k_ploc_compact(int m, const int *ref, const Aabb *box, const int *nn,
                               const unsigned long long *flags, const unsigned long long *pos, int base_id,
                               int *ref_out, Aabb *box_out, int2 *node_child, Aabb *node_box, int *node_count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const unsigned long long f = flags[i];
    if (!(f & 1ull)) return;
    const unsigned long long p = pos[i];
    const int out = (int)(p & 0xFFFFFFFFull);
    if (f >> 32) {
        const int j = nn[i];
        const int id = base_id + (int)(p >> 32);
        const Aabb b = merge(box[i], box[j]);
        const int a = ref[i], c = ref[j];
        node_child[id] = make_int2(a, c);
        node_box[id] = b;
        node_count[id] = (a >= 0 ? node_count[a] : 1) + (c >= 0 ? node_count[c] : 1);
        ref_out[out] = id;
        box_out[out] = b;
    } else {
        ref_out[out] = ref[i];
        box_out[out] = box[i];
    }
}

// creation id -> LBVH arrays (root 0), new primitive order
__global__ void k_ploc_export(int n, const int2 *node_child, const Aabb *node_box, const int *node_count,
                              const int *first, const int *newpos, int2 *children, int2 *ranges, Aabb *node_boxes,
                              int *parent_internal, int *parent_leaf) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n - 1) return;
    const int fid = (n - 2) - id;
    const int2 c = node_child[id];
    const int a = c.x >= 0 ? (n - 2) - c.x : ~newpos[~c.x];
    const int b = c.y >= 0 ? (n - 2) - c.y : ~newpos[~c.y];
    children[fid] = make_int2(a, b);
    ranges[fid] = make_int2(first[id], first[id] + node_count[id] - 1);
    node_boxes[fid] = node_box[id];
    if (a >= 0) parent_internal[a] = fid;
    else parent_leaf[~a] = fid;
    if (b >= 0) parent_internal[b] = fid;
    else parent_leaf[~b] = fid;
}

__global__ void k_ploc_permute(int n, const int *newpos, const uint32_t *vals_in, uint32_t *vals_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    vals_out[newpos[i]] = vals_in[i];
}

// top-down: subtree [first, first + count) of the new primitive order.  The nodes of one
// depth level place their children and queue the internal ones for the next level (any
// binary tree; the queue's order does not matter, first/newpos depend on the topology alone)
__global__ void k_ploc_place(int m, const int *items, const int2 *node_child, const int *node_count, int *first,
                             int *newpos, int *next, int *next_count) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    const int id = items[t];
    const int f = first[id];
    const int2 c = node_child[id];
    const int cl = c.x >= 0 ? node_count[c.x] : 1;
    if (c.x >= 0) first[c.x] = f;
    else newpos[~c.x] = f;
    if (c.y >= 0) first[c.y] = f + cl;
    else newpos[~c.y] = f + cl;
    const int k = (c.x >= 0 ? 1 : 0) + (c.y >= 0 ? 1 : 0);
    if (k) {
        int at = atomicAdd(next_count, k);
        if (c.x >= 0) next[at++] = c.x;
        if (c.y >= 0) next[at] = c.y;
    }
}

// Top-down placement of the creation-id tree, one launch per depth level (after reinsertion the
// creation ids no longer order parents after children): first[] / newpos[] of every node / leaf.
// items_a / items_b: n entries each for the level queues, counter: one int.
hipError_t ploc_place_levels(int n, const int2 *node_child, const int *node_count, int *first, int *newpos,
                             int *items_a, int *items_b, int *counter, hipStream_t s) {
    const int root = n - 2;  // root = last node created
    (void)hipMemsetAsync(first + root, 0, sizeof(int), s);
    hipError_t err = hipMemcpyAsync(items_a, &root, sizeof(int), hipMemcpyHostToDevice, s);
    int level = 1, levels = 0;
    while (!err && level > 0) {
        (void)hipMemsetAsync(counter, 0, sizeof(int), s);
        hipLaunchKernelGGL(k_ploc_place, grid_for(level), dim3(kBlock), 0, s, level, items_a, node_child, node_count,
                           first, newpos, items_b, counter);
        err = hipMemcpyAsync(&level, counter, sizeof(int), hipMemcpyDeviceToHost, s);
        if (!err) err = hipStreamSynchronize(s);
        std::swap(items_a, items_b);
        if (!err && (level < 0 || level > n - 1 || ++levels > n)) err = hipErrorUnknown;  // cannot happen
    }
    return err;
}

// PLOC topology (see the PLOC section) -> LBVH arrays and the new primitive order vals_out;
// opts.reinsert_rounds reinsertion rounds in between
hipError_t build_ploc(int n, const uint32_t *vals_in, uint32_t *vals_out, const Aabb *prim_boxes, int2 *children,
                      int2 *ranges, Aabb *node_boxes, int *parent_internal, int *parent_leaf, hipStream_t s,
                      const BuildOptions &opts, ReinsertLog *log) {
    hipError_t err = hipSuccess;
    auto ref_a_buf = scratch<int>(err, n);
    auto ref_b_buf = scratch<int>(err, n);
    auto nn = scratch<int>(err, n);
    auto node_count = scratch<int>(err, n);
    auto first = scratch<int>(err, n);
    auto newpos = scratch<int>(err, n);
    auto box_a_buf = scratch<Aabb>(err, n);
    auto box_b_buf = scratch<Aabb>(err, n);
    auto node_box = scratch<Aabb>(err, n);
    auto node_child = scratch<int2>(err, n);
    auto flg = scratch<unsigned long long>(err, n);
    auto pos = scratch<unsigned long long>(err, n);
    auto sums = scratch<unsigned long long>(err, scan64_blocks(n));
    auto total = scratch<unsigned long long>(err, 1);
    if (err) return err;
    int *ref_a = ref_a_buf.get(), *ref_b = ref_b_buf.get();
    Aabb *box_a = box_a_buf.get(), *box_b = box_b_buf.get();
    hipLaunchKernelGGL(k_ploc_init, grid_for(n), dim3(kBlock), 0, s, n, vals_in, prim_boxes, ref_a, box_a);
    int m = n, base = 0;
    while (m > 1) {
        hipLaunchKernelGGL(k_ploc_nn, grid_for(m), dim3(kBlock), 0, s, m, box_a, nn.get());
        hipLaunchKernelGGL(k_ploc_flags, grid_for(m), dim3(kBlock), 0, s, m, nn.get(), flg.get());
        (void)hipMemcpyAsync(pos.get(), flg.get(), sizeof(unsigned long long) * m, hipMemcpyDeviceToDevice, s);
        unsigned long long tot = 0;
        err = scan64(pos.get(), m, sums.get(), total.get(), s, &tot);
        if (!err) err = hipStreamSynchronize(s);
        const int m_new = (int)(tot & 0xFFFFFFFFull), merges = (int)(tot >> 32);
        if (!err && (merges <= 0 || m_new != m - merges)) err = hipErrorUnknown;  // cannot happen
        if (err) return err;
        hipLaunchKernelGGL(k_ploc_compact, grid_for(m), dim3(kBlock), 0, s, m, ref_a, box_a, nn.get(), flg.get(),
                           pos.get(), base, ref_b, box_b, node_child.get(), node_box.get(), node_count.get());
        base += merges;
        std::swap(ref_a, ref_b);
        std::swap(box_a, box_b);
        m = m_new;
    }
    err = reinsert_ploc(n, opts, vals_in, prim_boxes, node_child.get(), node_box.get(), node_count.get(), log, s);
    // ref_a / ref_b / nn are free now: the placement's level queues and counter
    if (!err)
        err = ploc_place_levels(n, node_child.get(), node_count.get(), first.get(), newpos.get(), ref_a, ref_b,
                                nn.get(), s);
    if (err) return err;
    hipLaunchKernelGGL(k_ploc_export, grid_for(n - 1), dim3(kBlock), 0, s, n, node_child.get(), node_box.get(),
                       node_count.get(), first.get(), newpos.get(), children, ranges, node_boxes, parent_internal,
                       parent_leaf);
    hipLaunchKernelGGL(k_ploc_permute, grid_for(n), dim3(kBlock), 0, s, n, newpos.get(), vals_in, vals_out);
    return hipStreamSynchronize(s);
}

}  // namespace

hipError_t binary_tree(FrontEnd &fe, int n, const BuildOptions &opts, hipStream_t s, ReinsertLog *log) {
    (void)hipMemsetAsync(fe.parent_internal.get(), 0xFF, sizeof(int) * n, s);
    if (fe.refit_flags.get()) (void)hipMemsetAsync(fe.refit_flags.get(), 0, sizeof(uint32_t) * n, s);
    if (opts.builder == BuildOptions::Builder::Ploc) {
        const hipError_t err =
            build_ploc(n, fe.sorted_vals, fe.spare_vals, fe.boxes.get(), fe.children.get(), fe.ranges.get(),
                       fe.node_boxes.get(), fe.parent_internal.get(), fe.parent_leaf.get(), s, opts, log);
        std::swap(fe.sorted_vals, fe.spare_vals);  // the PLOC primitive order
        return err;
    }
    if (!fe.refit_flags.get()) return hipErrorInvalidValue;  // the Karras refit needs its counters
    hipLaunchKernelGGL(k_karras, grid_for(n - 1), dim3(kBlock), 0, s, fe.sorted_keys, n, fe.children.get(),
                       fe.ranges.get(), fe.parent_internal.get(), fe.parent_leaf.get());
    hipLaunchKernelGGL(k_refit, grid_for(n), dim3(kBlock), 0, s, n, fe.sorted_vals, fe.boxes.get(), fe.children.get(),
                       fe.parent_internal.get(), fe.parent_leaf.get(), fe.node_boxes.get(), fe.refit_flags.get());
    return hipSuccess;
}

}  // namespace pupil::bvh
