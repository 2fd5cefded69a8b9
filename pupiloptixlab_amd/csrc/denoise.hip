// denoise.hip — substitute for the reference's OptiX AI denoiser
// (framework/optix/denoiser.{h,cpp}: Denoiser(mode), Setup(w, h), Execute(data)).
//
// There is no ROCm counterpart of the OptiX denoiser network, so this is an
// edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch 2010):
// five passes of the 5x5 B3-spline kernel h = (1, 4, 6, 4, 1) / 16 at strides
// 1, 2, 4, 8, 16.  Tap q of pixel p is weighted by
//     h(dx) h(dy) exp(-(|t_p - t_q|^2 / s_c^2 + |n_p - n_q|^2 / s_n^2 + |a_p - a_q|^2 / s_a^2))
// where t = log(1 + max(c, 0)) per channel (the colour edge-stopping term on
// log radiance, so HDR edges such as emitters stay sharp while the noise of
// dim regions is averaged), with the colour
// sigma halved every pass (s_c = sigma_color * 2^-pass), the
// normal / albedo terms only when the mode asks for those guides
// (OptixDenoiserOptions::guideAlbedo / guideNormal, denoiser.cpp:46-60).
// Taps outside the image are skipped.
//
// UseTemporal blends the filtered frame with prev_output.  Without a flow image it is the
// fixed blend of a static camera, out = prev + 0.2 (filtered - prev).  With one
// (motion_vector: cur - prev pixel position per pixel, pupil_pt_motion_vectors) the history
// is reprojected: pixel (x, y) fetches prev_output at q = (x, y) - flow with the four
// bilinear taps at floor(q), tap j weighted by
//     w_j = b_j exp(-(|n_p - hn_j|^2 / s_n^2 + |a_p - ha_j|^2 / s_a^2))
// (b_j the bilinear weight, hn / ha the guides of the previous call, the terms present only
// for the guides the mode selects; taps outside the image are skipped).  The history is
// valid when the flow is finite and W = sum w_j > kHistoryMinWeight; then, with the history
// length n = sum w_j len_j / W,
//     alpha = max(0.2, 1 / (n + 1)),  out = hist + alpha (filtered - hist),  len = min(n + 1, 5),
// so a surface that just came into view converges as a running mean before it settles into
// the exponential blend.  Otherwise (disocclusion, a source outside the image, NaN flow)
// out = filtered and len = 1.  The denoiser keeps the previous call's packed guides (swapped
// with the current ones after every execute) and a double-buffered history length.
//
// Layout: the guides are repacked once per call into float4 images (one 16-B
// load per tap), colour ping-pongs between two float4 images; each pass is one
// pixel per lane, 25 taps served by L1/L2 (a 1080p pass moves ~2.5 GB through
// the caches, ~0.1 ms).  The filter is pinned by a float64 numpy restatement in
// tests/test_denoise.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <utility>

#include "../../include/pupil_pt.h"

namespace Pupil {
void set_last_error(const std::string &m);
}

struct pupil_denoiser {
    int device = 0;
    uint32_t mode = PUPIL_DENOISE_USE_ALBEDO | PUPIL_DENOISE_USE_NORMAL;
    uint32_t width = 0, height = 0;
    float sigma_color = 1.f;
    float4 *ping = nullptr, *pong = nullptr, *gn = nullptr, *ga = nullptr;
    // temporal history (allocated by setup for UseTemporal modes only): the packed guides of the
    // previous execute, the history length read by this execute (len[0]) and written by it
    // (len[1]).  hist_guides = the guide bits hn / ha hold, -1 = none; len_valid = len[0] was
    // written since the last setup with a new size / reset_history (a first frame or a
    // reprojecting execute: the fixed blend and the non-temporal modes never write it).  A
    // reprojecting execute uses the history only when both say so.
    float4 *hn = nullptr, *ha = nullptr;
    float *len[2] = {nullptr, nullptr};
    int hist_guides = -1;
    bool len_valid = false;
    void release() {
        void *b[] = {ping, pong, gn, ga, hn, ha, len[0], len[1]};
        for (void *p : b)
            if (p) (void)hipFree(p);
        ping = pong = gn = ga = hn = ha = nullptr;
        len[0] = len[1] = nullptr;
        hist_guides = -1;
        len_valid = false;
    }
};

namespace {

constexpr float kSigmaNormal = 0.35f;
constexpr float kSigmaAlbedo = 0.1f;
constexpr float kTemporalAlpha = 0.2f;
// reprojected history is used when the summed tap weight exceeds this: below it the taps are
// mostly outside the image or on another surface (a bilinear footprint with one matching
// corner tap of weight < 0.05 lies within a quarter pixel of that surface's edge)
constexpr float kHistoryMinWeight = 0.05f;
constexpr int kBlockX = 16, kBlockY = 16;

int fail(int code, const char *msg) {
    Pupil::set_last_error(msg);
    return code;
}

__device__ __forceinline__ float b3(int k) {  // (1, 4, 6, 4, 1) / 16
    return k == 0 ? 0.375f : ((k == 1 || k == -1) ? 0.25f : 0.0625f);
}

__global__ void k_pack_guides(const float *normal, const float *albedo, uint32_t n, float4 *gn, float4 *ga) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (gn) gn[i] = make_float4(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], 0.f);
    if (ga) ga[i] = make_float4(albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2], 0.f);
}

template <bool N, bool A>
__global__ __launch_bounds__(kBlockX *kBlockY) void k_atrous(const float4 *cin, float4 *cout, const float4 *gn,
                                                             const float4 *ga, uint32_t w, uint32_t h, int step,
                                                             float inv_sc2) {
    const int x = blockIdx.x * kBlockX + threadIdx.x;
    const int y = blockIdx.y * kBlockY + threadIdx.y;
    if (x >= (int)w || y >= (int)h) return;
    const size_t i = (size_t)y * w + x;
    const float4 cp = cin[i];
    const float tpx = log1pf(fmaxf(cp.x, 0.f)), tpy = log1pf(fmaxf(cp.y, 0.f)), tpz = log1pf(fmaxf(cp.z, 0.f));
    float4 np = make_float4(0.f, 0.f, 0.f, 0.f), ap = np;
    if (N) np = gn[i];
    if (A) ap = ga[i];
    const float inv_sn2 = 1.f / (kSigmaNormal * kSigmaNormal);
    const float inv_sa2 = 1.f / (kSigmaAlbedo * kSigmaAlbedo);
    float sr = 0.f, sg = 0.f, sb = 0.f, ws = 0.f;
    for (int dy = -2; dy <= 2; dy++) {
        const int yy = y + dy * step;
        if (yy < 0 || yy >= (int)h) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int xx = x + dx * step;
            if (xx < 0 || xx >= (int)w) continue;
            const size_t j = (size_t)yy * w + xx;
            const float4 cq = cin[j];
            const float dr = tpx - log1pf(fmaxf(cq.x, 0.f)), dg = tpy - log1pf(fmaxf(cq.y, 0.f)),
                        db = tpz - log1pf(fmaxf(cq.z, 0.f));
            float e = (dr * dr + dg * dg + db * db) * inv_sc2;
            if (N) {
                const float4 nq = gn[j];
                const float ux = np.x - nq.x, uy = np.y - nq.y, uz = np.z - nq.z;
                e += (ux * ux + uy * uy + uz * uz) * inv_sn2;
            }
            if (A) {
                const float4 aq = ga[j];
                const float ux = ap.x - aq.x, uy = ap.y - aq.y, uz = ap.z - aq.z;
                e += (ux * ux + uy * uy + uz * uz) * inv_sa2;
            }
            const float wgt = b3(dx) * b3(dy) * expf(-e);
            sr += wgt * cq.x;
            sg += wgt * cq.y;
            sb += wgt * cq.z;
            ws += wgt;
        }
    }
    cout[i] = make_float4(sr / ws, sg / ws, sb / ws, cp.w);  // ws >= h(0)^2 > 0 (the centre tap)
}

__global__ void k_temporal(const float4 *filtered, const float4 *prev, float4 *out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 f = filtered[i], p = prev[i];
    out[i] = make_float4(p.x + kTemporalAlpha * (f.x - p.x), p.y + kTemporalAlpha * (f.y - p.y),
                         p.z + kTemporalAlpha * (f.z - p.z), f.w);
}

// UseTemporal with a flow image: reprojected, disocclusion-aware blend (see the file header).
// One pixel per lane; four taps of prev / hn / ha / len_in around (x, y) - flow.
template <bool N, bool A>
__global__ __launch_bounds__(kBlockX *kBlockY) void k_temporal_reproject(
    const float4 *filtered, const float4 *prev, const float2 *flow, const float4 *gn, const float4 *ga,
    const float4 *hn, const float4 *ha, const float *len_in, float *len_out, float4 *out, uint32_t w, uint32_t h) {
    const int x = blockIdx.x * kBlockX + threadIdx.x;
    const int y = blockIdx.y * kBlockY + threadIdx.y;
    if (x >= (int)w || y >= (int)h) return;
    const size_t i = (size_t)y * w + x;
    const float4 f = filtered[i];
    const float2 mv = flow[i];
    float4 np = make_float4(0.f, 0.f, 0.f, 0.f), ap = np;
    if (N) np = gn[i];
    if (A) ap = ga[i];
    const float inv_sn2 = 1.f / (kSigmaNormal * kSigmaNormal);
    const float inv_sa2 = 1.f / (kSigmaAlbedo * kSigmaAlbedo);
    float sr = 0.f, sg = 0.f, sb = 0.f, sl = 0.f, ws = 0.f;
    const float qx = (float)x - mv.x, qy = (float)y - mv.y;
    const float fx = floorf(qx), fy = floorf(qy);
    // NaN / infinite flow fails the comparisons; the range also keeps the int conversion defined
    if (fx >= -1.f && fx < (float)w && fy >= -1.f && fy < (float)h) {
        const int ix = (int)fx, iy = (int)fy;
        const float tx = qx - fx, ty = qy - fy;
        for (int dy = 0; dy <= 1; dy++) {
            const int yy = iy + dy;
            if (yy < 0 || yy >= (int)h) continue;
            for (int dx = 0; dx <= 1; dx++) {
                const int xx = ix + dx;
                if (xx < 0 || xx >= (int)w) continue;
                const size_t j = (size_t)yy * w + xx;
                float e = 0.f;
                if (N) {
                    const float4 nq = hn[j];
                    const float ux = np.x - nq.x, uy = np.y - nq.y, uz = np.z - nq.z;
                    e += (ux * ux + uy * uy + uz * uz) * inv_sn2;
                }
                if (A) {
                    const float4 aq = ha[j];
                    const float ux = ap.x - aq.x, uy = ap.y - aq.y, uz = ap.z - aq.z;
                    e += (ux * ux + uy * uy + uz * uz) * inv_sa2;
                }
                const float wgt = (dx ? tx : 1.f - tx) * (dy ? ty : 1.f - ty) * expf(-e);
                const float4 pq = prev[j];
                sr += wgt * pq.x;
                sg += wgt * pq.y;
                sb += wgt * pq.z;
                sl += wgt * len_in[j];
                ws += wgt;
            }
        }
    }
    if (ws > kHistoryMinWeight) {
        const float hr = sr / ws, hg = sg / ws, hb = sb / ws, n = sl / ws;
        const float alpha = fmaxf(kTemporalAlpha, 1.f / (n + 1.f));
        out[i] = make_float4(hr + alpha * (f.x - hr), hg + alpha * (f.y - hg), hb + alpha * (f.z - hb), f.w);
        len_out[i] = fminf(n + 1.f, 1.f / kTemporalAlpha);
    } else {
        out[i] = f;
        len_out[i] = 1.f;
    }
}

__global__ void k_fill(float *a, float v, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = v;
}

}  // namespace

extern "C" {

int pupil_denoiser_create(int device, uint32_t mode, pupil_denoiser **out) {
    if (!out) return fail(PUPIL_ERR_INVALID, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(PUPIL_ERR_HIP, "no HIP device");
    if (device < 0 || device >= ndev) return fail(PUPIL_ERR_INVALID, "bad device index");
    if (mode & (PUPIL_DENOISE_APPLY_TO_AOV | PUPIL_DENOISE_USE_UPSCALE_2X))
        return fail(PUPIL_ERR_UNSUPPORTED, "ApplyToAOV / UseUpscale2X are not supported by the a-trous denoiser");
    auto d = new pupil_denoiser();
    d->device = device;
    d->mode = mode;
    *out = d;
    return PUPIL_OK;
}

int pupil_denoiser_setup(pupil_denoiser *d, uint32_t mode, uint32_t width, uint32_t height, float sigma_color) {
    if (!d || width == 0 || height == 0) return fail(PUPIL_ERR_INVALID, "bad arguments");
    if (mode & (PUPIL_DENOISE_APPLY_TO_AOV | PUPIL_DENOISE_USE_UPSCALE_2X))
        return fail(PUPIL_ERR_UNSUPPORTED, "ApplyToAOV / UseUpscale2X are not supported by the a-trous denoiser");
    if (hipSetDevice(d->device) != hipSuccess) return fail(PUPIL_ERR_HIP, "hipSetDevice failed");
    d->mode = mode;
    d->sigma_color = sigma_color > 0.f ? sigma_color : 1.f;
    if (width != d->width || height != d->height) {
        d->release();
        const size_t n = (size_t)width * height;
        if (hipMalloc((void **)&d->ping, sizeof(float4) * n) != hipSuccess ||
            hipMalloc((void **)&d->pong, sizeof(float4) * n) != hipSuccess ||
            hipMalloc((void **)&d->gn, sizeof(float4) * n) != hipSuccess ||
            hipMalloc((void **)&d->ga, sizeof(float4) * n) != hipSuccess) {
            d->release();
            d->width = d->height = 0;
            return fail(PUPIL_ERR_OOM, "denoiser workspace allocation failed");
        }
        d->width = width;
        d->height = height;
    }
    // the history buffers, for the modes that can use them (a denoiser that never runs
    // UseTemporal keeps the footprint of ping / pong and the guides)
    if ((mode & PUPIL_DENOISE_USE_TEMPORAL) && !d->hn) {
        const size_t n = (size_t)width * height;
        if (hipMalloc((void **)&d->hn, sizeof(float4) * n) != hipSuccess ||
            hipMalloc((void **)&d->ha, sizeof(float4) * n) != hipSuccess ||
            hipMalloc((void **)&d->len[0], sizeof(float) * n) != hipSuccess ||
            hipMalloc((void **)&d->len[1], sizeof(float) * n) != hipSuccess) {
            d->release();
            d->width = d->height = 0;
            return fail(PUPIL_ERR_OOM, "denoiser history allocation failed");
        }
        d->hist_guides = -1;
        d->len_valid = false;
    }
    return PUPIL_OK;
}

int pupil_denoiser_execute(pupil_denoiser *d, const pupil_denoise_data *data, void *hip_stream) {
    if (!d || !data || !data->input || !data->output) return fail(PUPIL_ERR_INVALID, "null argument");
    if (!d->ping) return fail(PUPIL_ERR_INVALID, "denoiser not set up");
    // reprojected history: UseTemporal with both the previous output and a flow image
    const bool reproject = (d->mode & PUPIL_DENOISE_USE_TEMPORAL) && data->prev_output && data->motion_vector;
    if (reproject && data->output == data->prev_output)
        return fail(PUPIL_ERR_INVALID, "output must not alias prev_output when motion vectors are given");
    const bool use_n = (d->mode & PUPIL_DENOISE_USE_NORMAL) != 0;
    const bool use_a = (d->mode & PUPIL_DENOISE_USE_ALBEDO) != 0;
    if ((use_n && !data->normal) || (use_a && !data->albedo)) return fail(PUPIL_ERR_INVALID, "missing guide buffer");
    if (hipSetDevice(d->device) != hipSuccess) return fail(PUPIL_ERR_HIP, "hipSetDevice failed");
    hipStream_t s = (hipStream_t)hip_stream;
    const uint32_t w = d->width, h = d->height;
    const uint32_t n = w * h;
    if (use_n || use_a)
        hipLaunchKernelGGL(k_pack_guides, dim3((n + 255) / 256), dim3(256), 0, s, (const float *)data->normal,
                           (const float *)data->albedo, n, use_n ? d->gn : nullptr, use_a ? d->ga : nullptr);
    const dim3 grid((w + kBlockX - 1) / kBlockX, (h + kBlockY - 1) / kBlockY), block(kBlockX, kBlockY);
    const float4 *src = (const float4 *)data->input;
    float4 *bufs[2] = {d->ping, d->pong};
    for (int pass = 0; pass < 5; pass++) {
        float4 *dst = bufs[pass & 1];
        const float sc = d->sigma_color * std::ldexp(1.f, -pass);
        const float inv_sc2 = 1.f / (sc * sc);
#define ATROUS(N, A) \
    hipLaunchKernelGGL((k_atrous<N, A>), grid, block, 0, s, src, dst, d->gn, d->ga, w, h, 1 << pass, inv_sc2)
        if (use_n && use_a) ATROUS(true, true);
        else if (use_n) ATROUS(true, false);
        else if (use_a) ATROUS(false, true);
        else ATROUS(false, false);
#undef ATROUS
        src = dst;
    }
    const int guides = (use_n ? PUPIL_DENOISE_USE_NORMAL : 0) | (use_a ? PUPIL_DENOISE_USE_ALBEDO : 0);
    const bool temporal = (d->mode & PUPIL_DENOISE_USE_TEMPORAL) != 0;
    // a reprojecting call without history (no execute has written the history length since the
    // last setup with a new size or reset_history, or the history holds other guides than this
    // call's) is a first frame
    if (reproject && d->len_valid && d->hist_guides == guides) {
#define REPROJECT(N, A)                                                                                           \
    hipLaunchKernelGGL((k_temporal_reproject<N, A>), grid, block, 0, s, src, (const float4 *)data->prev_output,   \
                       (const float2 *)data->motion_vector, d->gn, d->ga, d->hn, d->ha, d->len[0], d->len[1],     \
                       (float4 *)data->output, w, h)
        if (use_n && use_a) REPROJECT(true, true);
        else if (use_n) REPROJECT(true, false);
        else if (use_a) REPROJECT(false, true);
        else REPROJECT(false, false);
#undef REPROJECT
        std::swap(d->len[0], d->len[1]);
    } else if (temporal && data->prev_output && !reproject) {  // fixed blend; the history length stays
        hipLaunchKernelGGL(k_temporal, dim3((n + 255) / 256), dim3(256), 0, s, src, (const float4 *)data->prev_output,
                           (float4 *)data->output, n);
    } else {
        if (hipMemcpyAsync(data->output, src, sizeof(float4) * n, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(PUPIL_ERR_HIP, "output copy failed");
        if (temporal) {  // a first frame starts the history
            hipLaunchKernelGGL(k_fill, dim3((n + 255) / 256), dim3(256), 0, s, d->len[0], 1.f, n);
            d->len_valid = true;
        }
    }
    if (temporal) {  // this call's guides are the next call's history
        std::swap(d->gn, d->hn);
        std::swap(d->ga, d->ha);
        d->hist_guides = guides;
    } else {
        d->hist_guides = -1;  // hn / ha are no longer the previous call's
    }
    if (hipGetLastError() != hipSuccess) return fail(PUPIL_ERR_HIP, "denoiser launch failed");
    return PUPIL_OK;
}

int pupil_denoiser_reset_history(pupil_denoiser *d) {
    if (!d) return fail(PUPIL_ERR_INVALID, "null argument");
    d->hist_guides = -1;
    d->len_valid = false;
    return PUPIL_OK;
}

void pupil_denoiser_destroy(pupil_denoiser *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    d->release();
    delete d;
}

}  // extern "C"
