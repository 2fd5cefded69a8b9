// bvh_reinsert.hip — parallel reinsertion rounds over the PLOC binary tree (PUPIL_BVH_REINSERT),
// between PLOC's clustering and its export (bvh_ploc.hip build_ploc).
#include "bvh_build_detail.h"

#include <cstdio>

namespace pupil::bvh {

namespace {

// ---------------------------------------------------------------- parallel reinsertion
// Meister & Bittner 2018, "Parallel Reinsertion for Bounding Volume Hierarchy
// Optimization", over the PLOC binary tree (creation ids) before it is exported.  One round:
// every node looks for the position where its subtree, removed and put back as the sibling
// of another node, lowers the tree's surface-area cost the most (k_reins_search); the
// candidates claim the five nodes whose links they rewrite with a 64-bit atomicMax of
// (gain bits, node) and only those owning all five go on (k_reins_resolve); a move whose
// target lies inside another mover's subtree is dropped, since two such moves could close a
// cycle (k_reins_filter); the rest are applied (k_reins_apply) and the boxes and counts
// refitted bottom up (k_reins_refit).  No locks and no waiting: the winners are a function
// of the tree alone.  Nodes are named by one index u: internal creation id < n - 1, leaf at
// Morton position p = n - 1 + p; box[] and parent[] are indexed by u.
constexpr int kReinsStack = 32;    // search stack entries per thread
constexpr int kReinsVisits = 256;  // search visit cap per node

__device__ __forceinline__ int ref_u(int r, int nm1) { return r >= 0 ? r : nm1 + ~r; }
__device__ __forceinline__ int u_ref(int u, int nm1) { return u < nm1 ? u : ~(u - nm1); }

__global__ void k_reins_init(int n, const uint32_t *sorted_vals, const Aabb *prim_boxes, const int2 *node_child,
                             Aabb *box, int *parent) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int nm1 = n - 1;
    if (i < n) box[nm1 + i] = prim_boxes[sorted_vals[i]];
    if (i < nm1) {
        const int2 c = node_child[i];
        parent[ref_u(c.x, nm1)] = i;
        parent[ref_u(c.y, nm1)] = i;
        if (i == n - 2) parent[i] = -1;  // root = last node created
    }
}

__global__ __launch_bounds__(kBlock) void k_reins_search(int n, const int2 *node_child, const Aabb *box,
                                                         const int *parent, int *cand_x, int *cand_pivot,
                                                         float *cand_gain, unsigned long long *claim) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    const int nm1 = n - 1, total = 2 * n - 1;
    if (u >= total) return;
    cand_x[u] = -1;
    const int P = parent[u];
    if (P < 0 || parent[P] < 0) return;  // the root and its children stay: the root keeps its id
    const Aabb bl = box[u];
    const float al = half_area(bl);
    int st_node[kReinsStack];
    float st_ind[kReinsStack];
    float best = 0.f;
    int best_x = -1, best_pivot = -1;
    int visits = 0;
    int pivot = P, from = u;
    float bound = half_area(box[P]);  // area saved so far by taking the subtree out
    Aabb shr;                         // box of `from` once the subtree is out
    bool have_shr = false;
    while (visits < kReinsVisits) {
        const int2 pc = node_child[pivot];
        const int sib = ref_u(pc.x, nm1) == from ? ref_u(pc.y, nm1) : ref_u(pc.x, nm1);
        if (have_shr && from != P) bound += half_area(box[from]) - half_area(shr);
        int sp = 0;
        st_node[sp] = sib;
        st_ind[sp++] = 0.f;
        while (sp > 0 && visits < kReinsVisits) {
            sp--;
            const int x = st_node[sp];
            const float ind = st_ind[sp];
            if (!(bound - ind - al > best)) continue;  // lower bound on the cost below x
            visits++;
            const Aabb bx = box[x];
            const float m = half_area(merge(bx, bl));
            const float g = bound - ind - m;
            if (g > best) {
                best = g;
                best_x = x;
                best_pivot = pivot;
            }
            if (x < nm1) {
                const float cind = ind + (m - half_area(bx));
                if (bound - cind - al > best && sp + 2 <= kReinsStack) {
                    const int2 c = node_child[x];
                    st_node[sp] = ref_u(c.y, nm1);
                    st_ind[sp++] = cind;
                    st_node[sp] = ref_u(c.x, nm1);
                    st_ind[sp++] = cind;
                }
            }
        }
        const Aabb bs = box[sib];
        shr = have_shr ? merge(shr, bs) : bs;
        have_shr = true;
        from = pivot;
        pivot = parent[pivot];
        visits++;
        if (pivot < 0) break;
    }
    if (best_x < 0) return;
    const int2 pc = node_child[P];
    const int S = ref_u(pc.x, nm1) == u ? ref_u(pc.y, nm1) : ref_u(pc.x, nm1);
    if (best_x == S) return;  // the place it has
    cand_x[u] = best_x;
    cand_pivot[u] = best_pivot;
    cand_gain[u] = best;
    // gains are positive floats: their bits order as integers; the node id makes keys unique
    const unsigned long long key = ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)u;
    atomicMax(&claim[u], key);
    atomicMax(&claim[P], key);
    atomicMax(&claim[S], key);
    atomicMax(&claim[best_x], key);
    atomicMax(&claim[parent[best_x]], key);
}

__global__ void k_reins_resolve(int n, const int2 *node_child, const int *parent, const int *cand_x,
                                const float *cand_gain, const unsigned long long *claim, uint8_t *mover) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    const int nm1 = n - 1;
    if (u >= 2 * n - 1) return;
    const int X = cand_x[u];
    bool win = false;
    if (X >= 0) {
        const int P = parent[u];
        const int2 pc = node_child[P];
        const int S = ref_u(pc.x, nm1) == u ? ref_u(pc.y, nm1) : ref_u(pc.x, nm1);
        const unsigned long long key = ((unsigned long long)__float_as_uint(cand_gain[u]) << 32) | (unsigned)u;
        win = claim[u] == key && claim[P] == key && claim[S] == key && claim[X] == key && claim[parent[X]] == key;
    }
    mover[u] = win ? 1 : 0;
}

// moves[k] = (L, slot of P in its parent, slot of X in its parent)
__global__ void k_reins_filter(int n, const int2 *node_child, const int *parent, const int *cand_x,
                               const int *cand_pivot, const uint8_t *mover, int3 *moves, int *num_moves) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    const int nm1 = n - 1;
    if (u >= 2 * n - 1 || !mover[u]) return;
    const int X = cand_x[u], pivot = cand_pivot[u];
    // between the target and the pivot no node may move itself: the pivot and everything
    // above it hold the subtree before and after, so a mover there takes both along
    int a = parent[X];
    for (int k = 0; k < n && a >= 0 && a != pivot; k++) {
        if (mover[a]) return;
        a = parent[a];
    }
    const int P = parent[u], G = parent[P], XP = parent[X];
    const int sg = ref_u(node_child[G].x, nm1) == P ? 0 : 1;
    const int sx = ref_u(node_child[XP].x, nm1) == X ? 0 : 1;
    moves[atomicAdd(num_moves, 1)] = make_int3(u, sg, sx);
}

__global__ void k_reins_apply(int n, int num_moves, const int3 *moves, const int *cand_x, int2 *node_child,
                              int *parent) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int nm1 = n - 1;
    if (k >= num_moves) return;
    const int3 mv = moves[k];
    const int L = mv.x, X = cand_x[L];
    // every link below belongs to a node this move owns (or to one slot of G / XP that no
    // other surviving move rewrites), so the reads of parent[] see the old tree
    const int P = parent[L], G = parent[P], XP = parent[X];
    const int2 pc = node_child[P];
    const int S = ref_u(pc.x, nm1) == L ? ref_u(pc.y, nm1) : ref_u(pc.x, nm1);
    ((int *)&node_child[G])[mv.y] = u_ref(S, nm1);
    ((int *)&node_child[XP])[mv.z] = u_ref(P, nm1);  // XP != P: the target is neither L nor S
    node_child[P] = make_int2(u_ref(X, nm1), u_ref(L, nm1));
    parent[S] = G;
    parent[P] = XP;
    parent[X] = P;
}

// bottom-up boxes and counts from the leaves; the second arrival at a node finishes it
__global__ void k_reins_refit(int n, const int2 *node_child, const int *parent, Aabb *box, int *node_count,
                              uint32_t *flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int nm1 = n - 1;
    if (i >= n) return;
    int node = parent[nm1 + i];
    for (int k = 0; k < n && node >= 0; k++) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const uint32_t prev = __hip_atomic_fetch_add(&flags[node], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == 0u) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const int2 c = node_child[node];
        box[node] = merge(box[ref_u(c.x, nm1)], box[ref_u(c.y, nm1)]);
        node_count[node] = (c.x >= 0 ? node_count[c.x] : 1) + (c.y >= 0 ? node_count[c.y] : 1);
        node = parent[node];
    }
}

// surface-area cost of the binary tree: per-block sums of the internal nodes' half areas,
// in a fixed order (the host adds the blocks in order), so the figure is reproducible
__global__ __launch_bounds__(kBlock) void k_reins_cost(int m, const Aabb *box, double *partial) {
    __shared__ double sh[kBlock];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    sh[threadIdx.x] = i < m ? (double)half_area(box[i]) : 0.0;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

// the pass's working copy of the tree and its per-round arrays, for n leaves
struct ReinsertScratch {
    DevBuf<int2> w_child;
    DevBuf<Aabb> w_box;
    DevBuf<int> w_count, parent, cand_x, cand_pivot;
    DevBuf<float> cand_gain;
    DevBuf<unsigned long long> claim;
    DevBuf<uint8_t> mover;
    DevBuf<int3> moves;
    DevBuf<int> num_moves;
    DevBuf<uint32_t> flags;
    DevBuf<double> partial;
    std::vector<double> host_partial;

    ReinsertScratch(hipError_t &err, int n) {
        const int total = 2 * n - 1, nblk = (n - 1 + kBlock - 1) / kBlock;
        w_child = scratch<int2>(err, n);
        w_box = scratch<Aabb>(err, total);
        w_count = scratch<int>(err, n);
        parent = scratch<int>(err, total);
        cand_x = scratch<int>(err, total);
        cand_pivot = scratch<int>(err, total);
        cand_gain = scratch<float>(err, total);
        claim = scratch<unsigned long long>(err, total);
        mover = scratch<uint8_t>(err, total);
        moves = scratch<int3>(err, total);
        num_moves = scratch<int>(err, 1);
        flags = scratch<uint32_t>(err, n);
        partial = scratch<double>(err, nblk);
        host_partial.resize((size_t)nblk);
    }

    // surface-area cost of the working tree (synchronises)
    hipError_t cost(int n, hipStream_t s, double *out) {
        const int nblk = (int)host_partial.size();
        hipLaunchKernelGGL(k_reins_cost, dim3(nblk), dim3(kBlock), 0, s, n - 1, w_box.get(), partial.get());
        hipError_t e = hipMemcpyAsync(host_partial.data(), partial.get(), sizeof(double) * nblk, hipMemcpyDeviceToHost, s);
        if (!e) e = hipStreamSynchronize(s);
        double c = 0.0;
        for (double v : host_partial) c += v;
        *out = c;
        return e;
    }

    // One round on the working tree: search, resolve, filter, apply, refit.  *after: the cost it
    // leaves; *moved false when no move survived (the tree is untouched and the pass ends).
    hipError_t round(int n, hipStream_t s, bool *moved, double *after) {
        const int total = 2 * n - 1;
        *moved = false;
        hipError_t err = hipMemsetAsync(claim.get(), 0, sizeof(unsigned long long) * total, s);
        if (!err) err = hipMemsetAsync(num_moves.get(), 0, sizeof(int), s);
        if (err) return err;
        hipLaunchKernelGGL(k_reins_search, grid_for(total), dim3(kBlock), 0, s, n, w_child.get(), w_box.get(),
                           parent.get(), cand_x.get(), cand_pivot.get(), cand_gain.get(), claim.get());
        hipLaunchKernelGGL(k_reins_resolve, grid_for(total), dim3(kBlock), 0, s, n, w_child.get(), parent.get(),
                           cand_x.get(), cand_gain.get(), claim.get(), mover.get());
        hipLaunchKernelGGL(k_reins_filter, grid_for(total), dim3(kBlock), 0, s, n, w_child.get(), parent.get(),
                           cand_x.get(), cand_pivot.get(), mover.get(), moves.get(), num_moves.get());
        int nmoves = 0;
        err = hipMemcpyAsync(&nmoves, num_moves.get(), sizeof(int), hipMemcpyDeviceToHost, s);
        if (!err) err = hipStreamSynchronize(s);
        if (err || nmoves <= 0) return err;
        hipLaunchKernelGGL(k_reins_apply, grid_for(nmoves), dim3(kBlock), 0, s, n, nmoves, moves.get(), cand_x.get(),
                           w_child.get(), parent.get());
        err = hipMemsetAsync(flags.get(), 0, sizeof(uint32_t) * n, s);
        if (err) return err;
        hipLaunchKernelGGL(k_reins_refit, grid_for(n), dim3(kBlock), 0, s, n, w_child.get(), parent.get(), w_box.get(),
                           w_count.get(), flags.get());
        *moved = true;
        return cost(n, s, after);
    }
};

}  // namespace

// Up to opts.reinsert_rounds rounds (see the section above) over the creation-id tree
// node_child / node_box / node_count, in place.  A round works on copies and is committed
// only if it did not raise the tree's cost: the gains of one round's moves are computed one
// by one, and moves that refit the same ancestors can in rare cases add up to a loss; such a
// round is thrown away and the pass ends there, as it does after a round without moves.
// log (optional): the cost before the pass and after each committed round, and the rounds
// kept and thrown away.  When the device is out of memory for the scratch arrays the tree
// stays as it is; any other failure is an error.
hipError_t reinsert_ploc(int n, const BuildOptions &opts, const uint32_t *vals_in, const Aabb *prim_boxes,
                         int2 *node_child, Aabb *node_box, int *node_count, ReinsertLog *log, hipStream_t s) {
    const int rounds = opts.reinsert_rounds;
    ReinsertLog env_log;
    const bool print = !log && rounds > 0 && opts.reinsert_log;
    if (print) log = &env_log;
    if (log) *log = ReinsertLog{};
    if (n < 2 || (rounds <= 0 && !log)) return hipSuccess;
    const int nm1 = n - 1;
    hipError_t err = hipSuccess;
    ReinsertScratch w(err, n);
    if (err) {  // out of memory for the pass: the unoptimised tree
        (void)hipGetLastError();
        return err == hipErrorOutOfMemory ? hipSuccess : err;
    }
    double cost = 0.0;
    err = hipMemcpyAsync(w.w_child.get(), node_child, sizeof(int2) * nm1, hipMemcpyDeviceToDevice, s);
    if (!err) err = hipMemcpyAsync(w.w_box.get(), node_box, sizeof(Aabb) * nm1, hipMemcpyDeviceToDevice, s);
    if (!err) err = hipMemcpyAsync(w.w_count.get(), node_count, sizeof(int) * nm1, hipMemcpyDeviceToDevice, s);
    if (!err) {
        hipLaunchKernelGGL(k_reins_init, grid_for(n), dim3(kBlock), 0, s, n, vals_in, prim_boxes, w.w_child.get(),
                           w.w_box.get(), w.parent.get());
        err = w.cost(n, s, &cost);
    }
    if (!err && log) log->costs.push_back(cost);
    for (int r = 0; r < rounds && !err; r++) {
        bool moved = false;
        double after = 0.0;
        err = w.round(n, s, &moved, &after);
        if (err || !moved) break;
        if (after > cost) {  // a round that raised the cost is not committed
            if (log) log->rejected++;
            break;
        }
        err = hipMemcpyAsync(node_child, w.w_child.get(), sizeof(int2) * nm1, hipMemcpyDeviceToDevice, s);
        if (!err) err = hipMemcpyAsync(node_box, w.w_box.get(), sizeof(Aabb) * nm1, hipMemcpyDeviceToDevice, s);
        if (!err) err = hipMemcpyAsync(node_count, w.w_count.get(), sizeof(int) * nm1, hipMemcpyDeviceToDevice, s);
        cost = after;
        if (!err && log) {
            log->costs.push_back(cost);
            log->kept++;
        }
    }
    if (!err) err = hipStreamSynchronize(s);
    if (print && !log->costs.empty())
        std::fprintf(stderr, "reinsert: %d leaves, %d rounds asked, %d kept, %d rejected, cost %.9g -> %.9g\n", n, rounds,
                     log->kept, log->rejected, log->costs.front(), log->costs.back());
    return err;
}

}  // namespace pupil::bvh
