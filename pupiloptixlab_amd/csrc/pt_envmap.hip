// pt_envmap.hip — the env map's CDF tables rebuilt on the device (pupil_pt_update_env_device).
//
// The host derives the tables in host/emitter_tables.h (convert_emitter's env branch, the reference's
// BuildEnvMapCdfTable, world/emitter.cpp:107-149).  The two stages here restate those operations
// in the host's order, so the block col_cdf | row_cdf | row_weight is bit for bit the host's for
// the same texels (the build has -ffp-contract=off on both sides; / is correctly rounded on both):
//   1. k_env_rows     one wave per row of the map: col_cdf of the row, and the row's luminance sum
//                     (col_sum) into scratch
//   2. k_env_columns  one wave: row_cdf from col_sum[y] * row_weight[y], and DevEmitter::normalization
// Both stages are the same scan.  The host adds the values in index order in float, and float
// addition is not associative, so ONE lane chains the adds (no tree, no wave scan): the 64 lanes
// compute a chunk of kEnvStage values in parallel with coalesced loads (luminance of a texel, or
// the product of a row; both are order-independent) and stage them in the LDS, lane 0 reads them
// back four per LDS load, adds, and writes the partial sums to the stage, and all lanes store them
// coalesced as the CDF's raw entries.  Once the total is known every lane divides the entries it
// stored itself (entry 1 + e belongs to lane e % 64 in both passes, so a lane reads back only its
// own stores).  The parallelism is across rows: a 2048 x 1024 map runs 1024 chains at once.
// row_weight is std::sin of the host's libm and depends on the height only: it is read, never
// written.  Nothing else of the DevEmitter is written.
// Precondition, as on the host: texels finite, every row's luminance sum > 0 (else 0 / 0).
#include <hip/hip_runtime.h>

#include "pt_kernels.h"

namespace pupil {
namespace {

static_assert(kEnvStage % 64u == 0u, "a chunk starts at a multiple of 64: lane e % 64 owns entry 1 + e in both passes");

// cdf[0] = 0, cdf[1 + e] = (value(0) + ... + value(e)) / total for e < n - 1, cdf[n] = 1, with the
// sums chained in index order from 0.f; returns the total (every lane).  One wave; n >= 1.
template <typename Value>
__device__ __forceinline__ float chained_cdf(float4 *stage, float *total, uint32_t n, float *cdf, Value value) {
    float *stage_f = reinterpret_cast<float *>(stage);
    const uint32_t lane = threadIdx.x;
    float sum = 0.f;  // lane 0's
    for (uint32_t base = 0; base < n; base += kEnvStage) {
        const uint32_t len = min(kEnvStage, n - base);
        for (uint32_t k = lane; k < len; k += 64u) stage_f[k] = value(base + k);
        __syncthreads();
        if (lane == 0) {
            uint32_t k = 0;
            for (; k + 4 <= len; k += 4) {
                float4 v = stage[k / 4];
                sum = sum + v.x, v.x = sum;
                sum = sum + v.y, v.y = sum;
                sum = sum + v.z, v.z = sum;
                sum = sum + v.w, v.w = sum;
                stage[k / 4] = v;
            }
            for (; k < len; k++) {
                sum = sum + stage_f[k];
                stage_f[k] = sum;
            }
        }
        __syncthreads();
        for (uint32_t k = lane; k < len; k += 64u) cdf[1u + base + k] = stage_f[k];
        __syncthreads();  // the next chunk overwrites the stage
    }
    if (lane == 0) *total = sum;
    __syncthreads();
    const float t = *total;
    if (lane == 0) cdf[0] = 0.f;
    for (uint32_t e = lane; e < n; e += 64u) cdf[1u + e] = e + 1u < n ? cdf[1u + e] / t : 1.f;
    return t;
}

// stage 1: the inner loop of BuildEnvMapCdfTable for row blockIdx.x
__global__ __launch_bounds__(64) void k_env_rows(const float4 *texels, uint32_t w, float *col_cdf, float *col_sum) {
    __shared__ float4 stage[kEnvStage / 4];
    __shared__ float total;
    const uint32_t y = blockIdx.x;
    const float4 *row = texels + (size_t)y * w;
    const float sum = chained_cdf(stage, &total, w, col_cdf + (size_t)y * (w + 1u), [row](uint32_t x) {
        const float4 t = row[x];
        return luminance(v3(t.x, t.y, t.z));
    });
    if (threadIdx.x == 0) col_sum[y] = sum;
}

// stage 2: its outer loop, and the normalization (w and h converted as the host's size_t values are)
__global__ __launch_bounds__(64) void k_env_columns(const float *col_sum, const float *row_weight, uint32_t w, uint32_t h,
                                                    float *row_cdf, DevEmitter *env) {
    __shared__ float4 stage[kEnvStage / 4];
    __shared__ float total;
    const float row_sum = chained_cdf(stage, &total, h, row_cdf,
                                      [col_sum, row_weight](uint32_t y) { return col_sum[y] * row_weight[y]; });
    if (threadIdx.x == 0) env->normalization = 1.f / (row_sum * (2.f * kPi / (float)w) * (kPi / (float)h));
}

}  // namespace

void launch_env_tables(const EnvTablesJob &job, hipStream_t s) {
    if (job.w == 0u || job.h == 0u) return;
    hipLaunchKernelGGL(k_env_rows, dim3(job.h), dim3(64), 0, s, job.texels, job.w, job.col_cdf, job.col_sum);
    hipLaunchKernelGGL(k_env_columns, dim3(1), dim3(64), 0, s, (const float *)job.col_sum, job.row_weight, job.w, job.h,
                       job.row_cdf, job.env);
}

}  // namespace pupil
