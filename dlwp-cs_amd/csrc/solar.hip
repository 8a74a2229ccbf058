// Top-of-atmosphere insolation computed where it is written (reference DLWP/util.py:306-364, restated in DLWP/util.py): the
// computing twin of the one-variable dlwpcs_batch_gather out of a dense (T, 1, S) insolation array.  Same output addressing,
//     channels_last : out[b][s][c_off + n*c_stride]      channels_first: out[b][c_off + n*c_stride][s]
// with row r = samples[b] + t_off + n*t_stride, but the value comes from two small host-built tables instead of HBM rows:
//     row_tab[r]  = {sin(decl), cos(decl), S0 * dist^-2, day}          (fp64; day holds an fp32 value)
//     cell_tab[s] = {sin(phi), cos(phi), lon / 360}                     (fp64; lon / 360 holds an fp32 value)
//     value       = max(0, scale * (sinphi * sindec - cosphi * cosdec * cos(hour))),   hour = f32(2 pi) * (day + lonfrac)
// The host function forms `hour` in fp32 from a day of up to 366 and takes the cosine of an argument of up to 2300 rad: that
// quantisation is part of its result, so `hour` is formed here with the same two rounded fp32 operations (no contraction, no
// reduction modulo one day first) and handed to the accurate cosf.  The combine runs in fp64 without contraction, is rounded to
// fp32 and only then to the output dtype: the device differs from the host through the cosine alone, and a bf16 output is the
// round-to-nearest-even of the fp32 output, as the gather rounds the stored fp32 array.
//
// Write-bound: one workgroup owns one (b, n) row and a strip of cells, the row's four scalars are uniform loads kept in registers,
// a lane computes 16 B of output (4 fp32 / 8 bf16) and stores it as one vector wherever the destination is contiguous in s
// (channels_first, or channels_last with a single channel).  Channels interleaved with others (the generator's main input) are
// element stores at stride Ctot, like batch_gather_cl_kernel's.
#include "common.h"

namespace dlwpcs {

namespace {

constexpr int SF_THREADS = 256;

struct SolarRow {
    double sindec, cosdec, scale;
    float day;
};

__device__ __forceinline__ SolarRow solar_row(const double *__restrict__ row_tab, int64_t r) {
    const double *p = row_tab + 4 * r;
    SolarRow R;
    R.sindec = p[0];
    R.cosdec = p[1];
    R.scale = p[2];
    R.day = (float)p[3];
    return R;
}

__device__ __forceinline__ float solar_elem(const SolarRow &R, double sinphi, double cosphi, float lonfrac) {
#pragma clang fp contract(off)
    const float hour = __fmul_rn((float)6.283185307179586, __fadd_rn(R.day, lonfrac));
    const double c = (double)cosf(hour);
    // (plain operators: the pragma above governs this block, not the bodies of inlined helpers -- a * b - c would fuse there)
    const double a = sinphi * R.sindec;
    const double b = (cosphi * R.cosdec) * c;
    const double d = a - b;
    const double v = R.scale * d;
    return (float)fmax(v, 0.0);
}

// destination contiguous in s: element (b, n, s) at out[base + b * b_stride + n * n_stride + s].  EV = elements per lane (EV > 1:
// S % EV == 0 and every row start is 16-B aligned -- host).  grid.x = B * n_steps * strips.
template <typename OT, int EV>
__global__ void __launch_bounds__(SF_THREADS) solar_fill_rows_kernel(const double *__restrict__ row_tab,
                                                                     const double *__restrict__ cell_tab, uint32_t S,
                                                                     uint32_t strips, const int32_t *__restrict__ samples,
                                                                     int n_steps, int t_off, int t_stride, OT *__restrict__ out,
                                                                     int64_t base, int64_t b_stride, int64_t n_stride) {
    const uint32_t row = blockIdx.x / strips, strip = blockIdx.x - row * strips;
    const uint32_t b = row / (uint32_t)n_steps, n = row - b * (uint32_t)n_steps;
    const SolarRow R = solar_row(row_tab, (int64_t)samples[b] + t_off + (int64_t)n * t_stride);
    const uint32_t s0 = (strip * SF_THREADS + threadIdx.x) * EV;
    if (s0 >= S) return;
    float v[EV];
#pragma unroll
    for (int k = 0; k < EV; ++k) {
        const double *c = cell_tab + 3 * (size_t)(s0 + k);
        v[k] = solar_elem(R, c[0], c[1], (float)c[2]);
    }
    OT *dst = out + base + (int64_t)b * b_stride + (int64_t)n * n_stride + s0;
    if constexpr (EV == 8) {
        *reinterpret_cast<uint4 *>(dst) = make_uint4(f2bf2(v[0], v[1]), f2bf2(v[2], v[3]), f2bf2(v[4], v[5]), f2bf2(v[6], v[7]));
    } else if constexpr (EV == 4) {
        *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (sizeof(OT) == 2) {
        *dst = f2bf(v[0]);
    } else {
        *dst = v[0];
    }
}

// channels_last with other channels between: out[(b * S + s) * Ctot + c_off + n * c_stride].  A lane keeps its cell's constants and
// walks the n_steps rows.  grid.x = B * strips.
template <typename OT>
__global__ void __launch_bounds__(SF_THREADS) solar_fill_cl_kernel(const double *__restrict__ row_tab,
                                                                   const double *__restrict__ cell_tab, uint32_t S,
                                                                   uint32_t strips, const int32_t *__restrict__ samples,
                                                                   int n_steps, int t_off, int t_stride, OT *__restrict__ out,
                                                                   int Ctot, int c_off, int c_stride) {
    const uint32_t b = blockIdx.x / strips, strip = blockIdx.x - b * strips;
    const uint32_t s = strip * SF_THREADS + threadIdx.x;
    const int64_t t0 = (int64_t)samples[b] + t_off;
    if (s >= S) return;
    const double *c = cell_tab + 3 * (size_t)s;
    const double sinphi = c[0], cosphi = c[1];
    const float lonfrac = (float)c[2];
    OT *dst = out + ((size_t)b * S + s) * Ctot + c_off;
    for (int n = 0; n < n_steps; ++n) {
        const SolarRow R = solar_row(row_tab, t0 + (int64_t)n * t_stride);
        const float v = solar_elem(R, sinphi, cosphi, lonfrac);
        if constexpr (sizeof(OT) == 2) dst[(size_t)n * c_stride] = f2bf(v);
        else dst[(size_t)n * c_stride] = v;
    }
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" int dlwpcs_solar_fill(const double *row_tab, int64_t T, const double *cell_tab, int64_t S,
                                 const int32_t *samples_dev, int B, int n_steps, int t_off, int t_stride, void *out, int Ctot,
                                 int c_off, int c_stride, int channels_last, int dtype, dlwpcs_stream_t stream) {
    if (!dtype_ok(dtype)) return fail(DLWPCS_E_INVALID, "solar_fill: dtype %d is neither DLWPCS_F32 nor DLWPCS_BF16", dtype);
    if (!row_tab || !cell_tab || !samples_dev || !out) return fail(DLWPCS_E_INVALID, "solar_fill: null pointer");
    if (T < 1 || S < 1 || B < 0 || n_steps < 1 || Ctot < 1 || c_off < 0 || c_stride < 0)
        return fail(DLWPCS_E_INVALID, "solar_fill: bad shape T=%lld S=%lld B=%d n_steps=%d Ctot=%d", (long long)T, (long long)S, B,
                    n_steps, Ctot);
    if ((int64_t)c_off + (int64_t)(n_steps - 1) * c_stride + 1 > Ctot)
        return fail(DLWPCS_E_INVALID, "solar_fill: channel window exceeds Ctot=%d", Ctot);
    if (B == 0) return DLWPCS_OK;
    if (S >= (1ll << 31)) return fail(DLWPCS_E_UNSUPPORTED, "solar_fill: %lld cells (< 2^31)", (long long)S);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t S32 = (uint32_t)S;
    const bool bf = dtype == DLWPCS_BF16;
    if (channels_last && !(Ctot == 1 && n_steps == 1)) {
        const int64_t strips = (S + SF_THREADS - 1) / SF_THREADS;
        const int64_t nblk = strips * B;
        if (nblk >= (1ll << 31)) return fail(DLWPCS_E_UNSUPPORTED, "solar_fill: %lld workgroups is too many", (long long)nblk);
        const dim3 grid((unsigned)nblk), blk(SF_THREADS);
        if (bf)
            hipLaunchKernelGGL(solar_fill_cl_kernel<bf16_t>, grid, blk, 0, s, row_tab, cell_tab, S32, (uint32_t)strips, samples_dev,
                               n_steps, t_off, t_stride, (bf16_t *)out, Ctot, c_off, c_stride);
        else
            hipLaunchKernelGGL(solar_fill_cl_kernel<float>, grid, blk, 0, s, row_tab, cell_tab, S32, (uint32_t)strips, samples_dev,
                               n_steps, t_off, t_stride, (float *)out, Ctot, c_off, c_stride);
        return check_launch("solar_fill");
    }
    // contiguous in s: channels_first rows, or a channels_last tensor that has this one channel
    int64_t base, b_stride, n_stride;
    if (channels_last) {
        base = 0; b_stride = S; n_stride = 0;
    } else {
        base = (int64_t)c_off * S; b_stride = (int64_t)Ctot * S; n_stride = (int64_t)c_stride * S;
    }
    const int ev = bf ? 8 : 4;
    const bool vec = S % ev == 0 && ((uintptr_t)out & 15) == 0;
    const int64_t per = (int64_t)SF_THREADS * (vec ? ev : 1);
    const int64_t strips = (S + per - 1) / per;
    const int64_t nblk = strips * B * n_steps;
    if (nblk >= (1ll << 31)) return fail(DLWPCS_E_UNSUPPORTED, "solar_fill: %lld workgroups is too many", (long long)nblk);
    const dim3 grid((unsigned)nblk), blk(SF_THREADS);
#define SOLAR_ROWS(OT, EV)                                                                                                        \
    hipLaunchKernelGGL((solar_fill_rows_kernel<OT, EV>), grid, blk, 0, s, row_tab, cell_tab, S32, (uint32_t)strips, samples_dev,  \
                       n_steps, t_off, t_stride, (OT *)out, base, b_stride, n_stride)
    if (bf) { if (vec) SOLAR_ROWS(bf16_t, 8); else SOLAR_ROWS(bf16_t, 1); }
    else { if (vec) SOLAR_ROWS(float, 4); else SOLAR_ROWS(float, 1); }
#undef SOLAR_ROWS
    return check_launch("solar_fill");
}
