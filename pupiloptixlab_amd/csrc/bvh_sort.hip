// bvh_sort.hip — stage 1 of the BVH builder: the Morton order of n boxes.
//   k_bounds       centroid bounds (wave reduce + ordered-int atomics)
//   k_morton       30-bit Morton code of each centroid
//   radix sort     hand-written stable LSD sort, 8-bit digits, wave-ballot multisplit ranking
//                  (k_sort_hist / k_sort_scan / k_sort_scatter), four passes
#include "bvh_build_detail.h"

#include <utility>

namespace pupil::bvh {

namespace {

__device__ __forceinline__ uint32_t float_to_ordered(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_to_float(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// centroid bounds -> 6 ordered uints (lo xyz as min, hi xyz as max)
__global__ void k_bounds(const Aabb *boxes, uint32_t n, uint32_t *out) {
    float lo[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()};
    float hi[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const Aabb b = boxes[i];
        for (int k = 0; k < 3; k++) {
            const float c = 0.5f * (b.lo[k] + b.hi[k]);
            lo[k] = fminf(lo[k], c);
            hi[k] = fmaxf(hi[k], c);
        }
    }
    for (int k = 0; k < 3; k++) {
        for (int o = 32; o > 0; o >>= 1) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], o));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o));
        }
    }
    if ((threadIdx.x & 63) == 0) {
        for (int k = 0; k < 3; k++) {
            atomicMin(&out[k], float_to_ordered(lo[k]));
            atomicMax(&out[3 + k], float_to_ordered(hi[k]));
        }
    }
}

__device__ __forceinline__ uint32_t expand_bits(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

__global__ void k_morton(const Aabb *boxes, uint32_t n, const uint32_t *bounds, uint32_t *keys, uint32_t *vals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float lo[3], ext[3];
    for (int k = 0; k < 3; k++) {
        lo[k] = ordered_to_float(bounds[k]);
        const float h = ordered_to_float(bounds[3 + k]);
        ext[k] = h - lo[k];
    }
    const Aabb b = boxes[i];
    uint32_t q[3];
    for (int k = 0; k < 3; k++) {
        const float c = 0.5f * (b.lo[k] + b.hi[k]);
        float t = ext[k] > 0.f ? (c - lo[k]) / ext[k] : 0.5f;
        t = fminf(fmaxf(t * 1024.f, 0.f), 1023.f);
        q[k] = (uint32_t)t;
    }
    keys[i] = (expand_bits(q[0]) << 2) | (expand_bits(q[1]) << 1) | expand_bits(q[2]);
    vals[i] = i;
}

// ---------------------------------------------------------------- radix sort
constexpr int kSortItems = 16;
constexpr int kSortTile = kBlock * kSortItems;

__global__ __launch_bounds__(kBlock) void k_sort_hist(const uint32_t *keys, uint32_t n, int shift, uint32_t *hist,
                                                      uint32_t nblocks) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kSortTile;
    for (int j = 0; j < kSortItems; j++) {
        const uint32_t i = base + j * kBlock + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & 0xFFu], 1u);
    }
    __syncthreads();
    hist[threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];  // digit-major
}

// single-block exclusive scan of `count` entries (in place)
__global__ __launch_bounds__(1024) void k_sort_scan(uint32_t *data, uint32_t count) {
    __shared__ uint32_t partial[1024];
    const uint32_t per = (count + 1023) / 1024;
    const uint32_t begin = threadIdx.x * per;
    const uint32_t end = min(begin + per, count);
    uint32_t sum = 0;
    for (uint32_t i = begin; i < end; i++) sum += data[i];
    partial[threadIdx.x] = sum;
    __syncthreads();
    // Hillis-Steele inclusive scan over 1024 partial sums
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const uint32_t v = threadIdx.x >= off ? partial[threadIdx.x - off] : 0u;
        __syncthreads();
        partial[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = threadIdx.x > 0 ? partial[threadIdx.x - 1] : 0u;
    for (uint32_t i = begin; i < end; i++) {
        const uint32_t v = data[i];
        data[i] = run;
        run += v;
    }
}

__global__ __launch_bounds__(kBlock) void k_sort_scatter(const uint32_t *keys_in, const uint32_t *vals_in,
                                                         uint32_t *keys_out, uint32_t *vals_out, uint32_t n, int shift,
                                                         const uint32_t *offsets, uint32_t nblocks) {
    constexpr int kWaves = kBlock / 64;
    __shared__ uint32_t wave_count[kWaves][256];
    __shared__ uint32_t wave_off[kWaves][256];
    __shared__ uint32_t running[256];
    running[threadIdx.x] = offsets[threadIdx.x * nblocks + blockIdx.x];
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const uint32_t base = blockIdx.x * kSortTile;
    for (int j = 0; j < kSortItems; j++) {
        for (int w = 0; w < kWaves; w++) wave_count[w][threadIdx.x] = 0;
        __syncthreads();
        const uint32_t i = base + j * kBlock + threadIdx.x;
        const bool valid = i < n;
        uint32_t key = 0, val = 0, digit = 0;
        if (valid) {
            key = keys_in[i];
            val = vals_in[i];
            digit = (key >> shift) & 0xFFu;
        }
        unsigned long long peers = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            peers &= bit ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & lt);
        if (valid && rank == 0) wave_count[wave][digit] = (uint32_t)__popcll(peers);
        __syncthreads();
        {
            const uint32_t d = threadIdx.x;
            uint32_t r = running[d];
            for (int w = 0; w < kWaves; w++) {
                wave_off[w][d] = r;
                r += wave_count[w][d];
            }
            running[d] = r;
        }
        __syncthreads();
        if (valid) {
            const uint32_t pos = wave_off[wave][digit] + rank;
            keys_out[pos] = key;
            vals_out[pos] = val;
        }
        __syncthreads();
    }
}

}  // namespace

FrontEnd::FrontEnd(hipError_t &err, int n, bool with_refit_flags) {
    const size_t nblocks = (size_t)((n + kSortTile - 1) / kSortTile);
    boxes = scratch<Aabb>(err, n);
    node_boxes = scratch<Aabb>(err, n);
    bounds = scratch<uint32_t>(err, 6);
    keys = scratch<uint32_t>(err, n);
    vals = scratch<uint32_t>(err, n);
    keys2 = scratch<uint32_t>(err, n);
    vals2 = scratch<uint32_t>(err, n);
    hist = scratch<uint32_t>(err, 256 * nblocks);
    if (with_refit_flags) refit_flags = scratch<uint32_t>(err, n);
    children = scratch<int2>(err, n);
    ranges = scratch<int2>(err, n);
    parent_internal = scratch<int>(err, n);
    parent_leaf = scratch<int>(err, n);
}

BinaryTree FrontEnd::tree(int n) const {
    return BinaryTree{n,           sorted_vals,      boxes.get(),          children.get(),
                      ranges.get(), node_boxes.get(), parent_internal.get()};
}

void scan32(uint32_t *data, uint32_t count, hipStream_t s) {
    hipLaunchKernelGGL(k_sort_scan, dim3(1), dim3(1024), 0, s, data, count);
}

void morton_order(FrontEnd &fe, int n, hipStream_t s) {
    const uint32_t g = (uint32_t)((n + kBlock - 1) / kBlock);
    const uint32_t nblocks = (uint32_t)((n + kSortTile - 1) / kSortTile);
    const Aabb *boxes = fe.boxes.get();
    uint32_t *bounds = fe.bounds.get(), *hist = fe.hist.get();
    const uint32_t init[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
    (void)hipMemcpyAsync(bounds, init, sizeof(init), hipMemcpyHostToDevice, s);
    hipLaunchKernelGGL(k_bounds, dim3(min(g, 1024u)), dim3(kBlock), 0, s, boxes, (uint32_t)n, bounds);
    hipLaunchKernelGGL(k_morton, dim3(g), dim3(kBlock), 0, s, boxes, (uint32_t)n, bounds, fe.keys.get(),
                       fe.vals.get());
    uint32_t *ki = fe.keys.get(), *vi = fe.vals.get(), *ko = fe.keys2.get(), *vo = fe.vals2.get();
    for (int shift = 0; shift < 30; shift += 8) {
        hipLaunchKernelGGL(k_sort_hist, dim3(nblocks), dim3(kBlock), 0, s, ki, (uint32_t)n, shift, hist, nblocks);
        scan32(hist, 256u * nblocks, s);
        hipLaunchKernelGGL(k_sort_scatter, dim3(nblocks), dim3(kBlock), 0, s, ki, vi, ko, vo, (uint32_t)n, shift,
                           hist, nblocks);
        std::swap(ki, ko);
        std::swap(vi, vo);
    }
    fe.sorted_keys = ki, fe.sorted_vals = vi, fe.spare_keys = ko, fe.spare_vals = vo;
}

}  // namespace pupil::bvh
