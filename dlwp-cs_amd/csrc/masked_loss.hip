// Masked 'mse' / 'mae' losses (dlwpcs_loss_masked_fwd_bwd): dlwpcs_loss_fwd_bwd for targets with holes.  The definition is the
// header's (include/dlwpcs.h); this file follows it.
//
// Both kernels are HBM-bound streaming passes.  Stage 1 is elementwise.hip's mse_stage1(_vec)_kernel with three additions: the
// hole test t != t, the select that replaces d by 0 at a hole before loss_elem (common.h) runs, and a uint32 count of the
// non-holes per lane.  Geometry, lane -> element map, fp32 lane sums and the 8-level LDS tree are the plain kernels', so that
// without a hole (and, under DLWPCS_NORM_ALL, on inputs with zeros written at the holes) the sums are the plain kernels' bits.
// Stage 2 (one workgroup, fp64) adds the workgroup sums in loss_stage2_body's order and the counts, and under DLWPCS_NORM_VALID
// leaves gscale in the scratch for masked_dy_kernel, which writes the gradient.  No atomics, no host synchronisation.
//
// Scratch (floats; dlwpcs_loss_scratch_bytes() = 8208): [0, 2 g) the workgroup sums {S0, S1}, [2048, 2048 + g) the workgroup counts
// (uint32), [8192] gscale of DLWPCS_NORM_VALID.  g <= 1024.
#include "common.h"

namespace dlwpcs {

namespace {

constexpr int ML_BLOCKS = 1024;             // stage 1 (the plain kernels' MSE_BLOCKS)
constexpr int ML_DY_BLOCKS = 2048;          // masked_dy_kernel
constexpr int ML_COUNT = 2 * ML_BLOCKS;     // scratch offset (floats) of the workgroup counts
constexpr int ML_COEF = 8 * ML_BLOCKS;      // scratch offset (floats) of gscale

// ---- storage vectors: E elements per lane, fp32 in registers (bf16 is rounded to nearest even once, on store) ------------
struct alignas(16) MH8 { uint4 u; };        // 8 x bf16
struct alignas(16) MF8 { float4 a, b; };    // 8 x fp32
template <typename V> struct MV;
template <> struct MV<float> {
    static constexpr int E = 1;
    static __device__ __forceinline__ void ld(const float *p, float *v) { v[0] = *p; }
    static __device__ __forceinline__ void st(float *p, const float *v) { *p = v[0]; }
};
template <> struct MV<bf16_t> {
    static constexpr int E = 1;
    static __device__ __forceinline__ void ld(const bf16_t *p, float *v) { v[0] = bf2f(*p); }
    static __device__ __forceinline__ void st(bf16_t *p, const float *v) { *p = f2bf(v[0]); }
};
template <> struct MV<MF8> {
    static constexpr int E = 8;
    static __device__ __forceinline__ void ld(const MF8 *p, float *v) {
        const float4 a = p->a, b = p->b;
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    static __device__ __forceinline__ void st(MF8 *p, const float *v) {
        p->a = make_float4(v[0], v[1], v[2], v[3]); p->b = make_float4(v[4], v[5], v[6], v[7]);
    }
};
template <> struct MV<MH8> {
    static constexpr int E = 8;
    static __device__ __forceinline__ void ld(const MH8 *p, float *v) {
        const uint4 q = p->u;
        v[0] = bf_lo(q.x); v[1] = bf_hi(q.x); v[2] = bf_lo(q.y); v[3] = bf_hi(q.y);
        v[4] = bf_lo(q.z); v[5] = bf_hi(q.z); v[6] = bf_lo(q.w); v[7] = bf_hi(q.w);
    }
    static __device__ __forceinline__ void st(MH8 *p, const float *v) {
        p->u = make_uint4(f2bf2(v[0], v[1]), f2bf2(v[2], v[3]), f2bf2(v[4], v[5]), f2bf2(v[6], v[7]));
    }
};

// One item (1 or 8 elements) of either kernel: g[] = the stored gradient, sq / ab / cnt the lane's sums.  W: the field index of the
// first element is divided once and stepped along the item (n < 2^32), as in mse_stage1_vec_kernel.
template <typename YV, typename TV, int LK, bool W>
__device__ __forceinline__ void masked_item(const YV *__restrict__ y, const TV *__restrict__ t, size_t i, float gscale,
                                            const LossField &wf, float *g, float &sq, float &ab, uint32_t &cnt) {
    constexpr int E = MV<YV>::E;
    float yv[E], tv[E];
    MV<YV>::ld(y + i, yv);
    MV<TV>::ld(t + i, tv);
    uint32_t q = 0, r = 0;
    if (W) { const uint32_t e = (uint32_t)i * (uint32_t)E, c = e / wf.div; q = c % wf.per; r = e - c * wf.div; }
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const bool hole = tv[k] != tv[k];
        const float d = hole ? 0.f : yv[k] - tv[k];
        const float gk = loss_elem<LK, W>(d, W ? wf.p[q] : 1.f, gscale, sq, ab);
        g[k] = hole ? 0.f : gk;
        cnt += hole ? 0u : 1u;
        if (W && ++r == wf.div) { r = 0; if (++q == wf.per) q = 0; }
    }
}

template <typename YV, typename TV, int LK, bool W>
__global__ void __launch_bounds__(256) masked_stage1_kernel(const YV *__restrict__ y, const TV *__restrict__ t,
                                                            YV *__restrict__ dy, float *__restrict__ scratch, size_t items,
                                                            float gscale, LossField wf) {
    float sq = 0.f, ab = 0.f;
    uint32_t cnt = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (size_t)gridDim.x * blockDim.x) {
        float g[MV<YV>::E];
        masked_item<YV, TV, LK, W>(y, t, i, gscale, wf, g, sq, ab, cnt);
        if (dy) MV<YV>::st(dy + i, g);
    }
    __shared__ float s_sq[256], s_ab[256];
    __shared__ uint32_t s_cnt[256];
    s_sq[threadIdx.x] = sq; s_ab[threadIdx.x] = ab; s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_sq[threadIdx.x] += s_sq[threadIdx.x + s]; s_ab[threadIdx.x] += s_ab[threadIdx.x + s];
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        scratch[2 * blockIdx.x] = s_sq[0]; scratch[2 * blockIdx.x + 1] = s_ab[0];
        reinterpret_cast<uint32_t *>(scratch + ML_COUNT)[blockIdx.x] = s_cnt[0];
    }
}

// One workgroup: the sums in loss_stage2_body's order (fp64), the counts, the results; valid != 0 (DLWPCS_NORM_VALID): the divisor
// is the count and gscale = gnum / count goes to the scratch for masked_dy_kernel (0 when nothing is valid).
__global__ void __launch_bounds__(256) masked_stage2_kernel(float *__restrict__ scratch, float *__restrict__ loss_out,
                                                            uint32_t *__restrict__ valid_out, int nblocks, float inv_n,
                                                            float weight, float gnum, int valid, int overwrite) {
    __shared__ double s_sq[256], s_ab[256];
    __shared__ uint32_t s_cnt[256];
    const uint32_t *counts = reinterpret_cast<const uint32_t *>(scratch + ML_COUNT);
    double sq = 0.0, ab = 0.0;
    uint32_t cnt = 0;
    for (int i = threadIdx.x; i < nblocks; i += 256) { sq += scratch[2 * i]; ab += scratch[2 * i + 1]; cnt += counts[i]; }
    s_sq[threadIdx.x] = sq; s_ab[threadIdx.x] = ab; s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_sq[threadIdx.x] += s_sq[threadIdx.x + s]; s_ab[threadIdx.x] += s_ab[threadIdx.x + s];
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t count = s_cnt[0];
        float inv = inv_n;
        if (valid) {
            const double c = (double)(float)count;
            inv = (float)(1.0 / c);
            scratch[ML_COEF] = count ? (float)((double)gnum / c) : 0.f;
        }
        float l0 = (float)(s_sq[0] * inv) * weight, l1 = (float)(s_ab[0] * inv);
        if (count == 0) l0 = l1 = 0.f;
        loss_out[0] = overwrite ? l0 : loss_out[0] + l0;
        loss_out[1] = overwrite ? l1 : loss_out[1] + l1;
        if (valid_out) valid_out[0] = count;
    }
}

// DLWPCS_NORM_VALID: dy with the gscale stage 2 left in device memory (the sums loss_elem forms here are dropped)
template <typename YV, typename TV, int LK, bool W>
__global__ void __launch_bounds__(256) masked_dy_kernel(const YV *__restrict__ y, const TV *__restrict__ t, YV *__restrict__ dy,
                                                        size_t items, const float *__restrict__ coef, LossField wf) {
    const float gscale = coef[0];
    float sq = 0.f, ab = 0.f;
    uint32_t cnt = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (size_t)gridDim.x * blockDim.x) {
        float g[MV<YV>::E];
        masked_item<YV, TV, LK, W>(y, t, i, gscale, wf, g, sq, ab, cnt);
        MV<YV>::st(dy + i, g);
    }
}

template <typename YV, typename TV, int LK, bool W>
static void masked_run(const void *y, const void *t, void *dy, float *scratch, size_t items, size_t g, float gscale, bool valid,
                       LossField wf, hipStream_t s) {
    hipLaunchKernelGGL((masked_stage1_kernel<YV, TV, LK, W>), dim3((unsigned)g), dim3(256), 0, s, (const YV *)y, (const TV *)t,
                       valid ? (YV *)nullptr : (YV *)dy, scratch, items, gscale, wf);
}

template <typename YV, typename TV, int LK, bool W>
static void masked_dy_run(const void *y, const void *t, void *dy, float *scratch, size_t items, LossField wf, hipStream_t s) {
    size_t g = (items + 255) / 256;
    if (g > ML_DY_BLOCKS) g = ML_DY_BLOCKS;
    hipLaunchKernelGGL((masked_dy_kernel<YV, TV, LK, W>), dim3((unsigned)g), dim3(256), 0, s, (const YV *)y, (const TV *)t, (YV *)dy,
                       items, (const float *)(scratch + ML_COEF), wf);
}

// stage: 1 = the reduction, 3 = the gradient launch of DLWPCS_NORM_VALID
template <int LK, bool W>
static void masked_dispatch(int stage, int dtype, bool t_f32, bool vec, const void *y, const void *t, void *dy, float *scratch,
                            size_t items, size_t g, float gscale, bool valid, LossField wf, hipStream_t s) {
#define ML_GO(YV, TV) do { if (stage == 1) masked_run<YV, TV, LK, W>(y, t, dy, scratch, items, g, gscale, valid, wf, s); \
                           else masked_dy_run<YV, TV, LK, W>(y, t, dy, scratch, items, wf, s); } while (0)
    if (vec) {
        if (dtype == DLWPCS_BF16 && t_f32) ML_GO(MH8, MF8);
        else if (dtype == DLWPCS_BF16) ML_GO(MH8, MH8);
        else ML_GO(MF8, MF8);
    } else if (dtype == DLWPCS_BF16 && t_f32) ML_GO(bf16_t, float);
    else if (dtype == DLWPCS_BF16) ML_GO(bf16_t, bf16_t);
    else ML_GO(float, float);
#undef ML_GO
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

#define REQUIRE(cond, ...) do { if (!(cond)) return fail(DLWPCS_E_INVALID, __VA_ARGS__); } while (0)

extern "C" int dlwpcs_loss_masked_fwd_bwd(const dlwpcs_loss_desc *L, const void *y, const void *t, int normalize, void *dy,
                                          float *loss_out, uint32_t *valid_out, size_t n, int dtype, void *scratch,
                                          dlwpcs_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    const bool t_f32 = (dtype & DLWPCS_MSE_TARGET_F32) != 0;
    dtype &= ~(DLWPCS_MSE_TARGET_F32 | DLWPCS_MSE_OVERWRITE);
    if (!dtype_ok(dtype)) return fail(DLWPCS_E_UNSUPPORTED, "loss_masked_fwd_bwd: dtype %d not built", dtype);
    REQUIRE(L && y && t && loss_out && scratch && n > 0, "loss_masked_fwd_bwd: bad arguments");
    if (L->kind == DLWPCS_LOSS_ACC)
        return fail(DLWPCS_E_UNSUPPORTED, "loss_masked_fwd_bwd: a masked anomaly-correlation loss is not built");
    REQUIRE(L->kind == DLWPCS_LOSS_MSE || L->kind == DLWPCS_LOSS_MAE, "loss_masked_fwd_bwd: unknown loss kind %d", L->kind);
    REQUIRE(!L->clim, "loss_masked_fwd_bwd: a climatology belongs to the anomaly-correlation loss");
    REQUIRE(normalize == DLWPCS_NORM_ALL || normalize == DLWPCS_NORM_VALID, "loss_masked_fwd_bwd: unknown normalize %d", normalize);
    REQUIRE(!L->weight || (L->weight_div >= 1 && L->weight_period >= 1), "loss_masked_fwd_bwd: weight field needs div, period >= 1");
    REQUIRE(n < (1ull << 32), "loss_masked_fwd_bwd: %zu elements (the count is a uint32: n < 2^32)", n);
    const LossField wf{L->weight, (uint32_t)L->weight_div, (uint32_t)L->weight_period};
    float *scr = (float *)scratch;
    const float weight = L->loss_weight;
    const bool valid = normalize == DLWPCS_NORM_VALID;
    const float gscale = L->kind == DLWPCS_LOSS_MSE ? weight * 2.f / (float)n : weight / (float)n;     // (loss_fwd_bwd_impl's)
    const float gnum = L->kind == DLWPCS_LOSS_MSE ? weight * 2.f : weight;
    const bool al = (((uintptr_t)y | (uintptr_t)t | (uintptr_t)dy) & 31) == 0;
    const bool vec = n % 8 == 0 && al;
    const size_t items = vec ? n / 8 : n;
    size_t g = (items + 255) / 256;
    if (g > ML_BLOCKS) g = ML_BLOCKS;
    const bool W = L->weight != nullptr;
    for (int stage = 1; stage <= 3; stage += 2) {
        if (stage == 3) {
            hipLaunchKernelGGL(masked_stage2_kernel, dim3(1), dim3(256), 0, s, scr, loss_out, valid_out, (int)g, 1.f / (float)n,
                               weight, gnum, valid ? 1 : 0, L->overwrite & 1);
            if (!valid || !dy) break;
        }
        if (L->kind == DLWPCS_LOSS_MSE && !W)
            masked_dispatch<DLWPCS_LOSS_MSE, false>(stage, dtype, t_f32, vec, y, t, dy, scr, items, g, gscale, valid, wf, s);
        else if (L->kind == DLWPCS_LOSS_MSE)
            masked_dispatch<DLWPCS_LOSS_MSE, true>(stage, dtype, t_f32, vec, y, t, dy, scr, items, g, gscale, valid, wf, s);
        else if (!W)
            masked_dispatch<DLWPCS_LOSS_MAE, false>(stage, dtype, t_f32, vec, y, t, dy, scr, items, g, gscale, valid, wf, s);
        else
            masked_dispatch<DLWPCS_LOSS_MAE, true>(stage, dtype, t_f32, vec, y, t, dy, scr, items, g, gscale, valid, wf, s);
    }
    return check_launch("loss_masked_fwd_bwd");
}
