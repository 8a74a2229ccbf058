// Missing values per plane (dlwpcs_missing_count): count[p] = the number of NaN elements (fp32: any payload, either sign, not
// +-inf) or of -32768 codes (int16, the packed series' missing code) among the `plane` elements of plane p of a contiguous
// (n_planes, plane) array.
//
// One streaming pass.  A workgroup owns whole planes (plane p, p + gridDim.x, ...), so every count is written by exactly one
// workgroup, once: no atomics, and `count` need not be zeroed.  The base pointer is aligned only to its element, and a plane
// may start anywhere, so each plane is cut at the 16-byte lines of the ADDRESS: up to 16 B / element - 1 head elements and as
// many tail elements are read one by one (one lane each), everything between as 16-byte vectors, MC_UNROLL of them in flight per
// lane.  A lane's count goes over the wave by shuffles, over the four waves through LDS, in a fixed order (integer sums: the
// order changes no bit anyway).  dlwpcs_fill_missing (below) cuts its array the same way.
#include "common.h"

namespace dlwpcs {

namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_UNROLL = 4;
constexpr int64_t MC_MAX_GRID = 1ll << 20;

__device__ __forceinline__ int is_nan_bits(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ int fill_codes(uint32_t w) { return ((w & 0xffffu) == 0x8000u) + ((w >> 16) == 0x8000u); }

template <typename T> __device__ __forceinline__ int missing_elem(const T *p);
template <> __device__ __forceinline__ int missing_elem<float>(const float *p) { return is_nan_bits(__float_as_uint(*p)); }
template <> __device__ __forceinline__ int missing_elem<short>(const short *p) { return *p == (short)-32768; }

template <typename T> __device__ __forceinline__ int missing_vec(const uint4 &w);
template <> __device__ __forceinline__ int missing_vec<float>(const uint4 &w) {
    return is_nan_bits(w.x) + is_nan_bits(w.y) + is_nan_bits(w.z) + is_nan_bits(w.w);
}
template <> __device__ __forceinline__ int missing_vec<short>(const uint4 &w) {
    return fill_codes(w.x) + fill_codes(w.y) + fill_codes(w.z) + fill_codes(w.w);
}

template <typename T>
__global__ void __launch_bounds__(MC_THREADS) missing_count_kernel(const T *__restrict__ x, int64_t n_planes, int64_t plane,
                                                                   int32_t *__restrict__ count) {
    constexpr int64_t VE = 16 / (int64_t)sizeof(T);     // elements per 16-byte vector
    __shared__ int s_part[MC_THREADS / 64];
    const int tid = (int)threadIdx.x;
    for (int64_t p = blockIdx.x; p < n_planes; p += gridDim.x) {
        const T *base = x + p * plane;
        // elements before the first 16-byte line (all of the plane when it ends before that line)
        int64_t head = (int64_t)((16u - (uint32_t)((uintptr_t)base & 15u)) & 15u) / (int64_t)sizeof(T);
        if (head > plane) head = plane;
        const int64_t nvec = (plane - head) / VE;
        const int64_t tail0 = head + nvec * VE;         // first element after the last whole vector
        int n = 0;
        if (tid < head) n += missing_elem<T>(base + tid);
        if (tail0 + tid < plane) n += missing_elem<T>(base + tail0 + tid);
        const uint4 *v = reinterpret_cast<const uint4 *>(base + head);
        for (int64_t i = tid; i < nvec; i += (int64_t)MC_THREADS * MC_UNROLL) {
            uint4 w[MC_UNROLL];
#pragma unroll
            for (int u = 0; u < MC_UNROLL; ++u) {
                const int64_t iu = i + (int64_t)u * MC_THREADS;
                w[u] = iu < nvec ? v[iu] : make_uint4(0u, 0u, 0u, 0u);     // (zeros are neither NaN nor the fill code)
            }
#pragma unroll
            for (int u = 0; u < MC_UNROLL; ++u) n += missing_vec<T>(w[u]);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
        if ((tid & 63) == 0) s_part[tid >> 6] = n;
        __syncthreads();
        if (tid == 0) {
            int total = 0;
#pragma unroll
            for (int wv = 0; wv < MC_THREADS / 64; ++wv) total += s_part[wv];
            count[p] = total;
        }
        __syncthreads();                                // s_part is reused by the workgroup's next plane
    }
}

// ---- dlwpcs_fill_missing: x[e] = fill[(e / div) % per] where x[e] is NaN, in place ----------------------------------------
// The same cut at the 16-byte lines of the address: head and tail elements one lane each (workgroup 0), everything between as
// 16-byte vectors, MC_UNROLL loads in flight per lane, every vector stored back (an element that is not NaN with its own bits).  The
// field index of a vector's first element is divided once and stepped along the vector (n < 2^32).
constexpr int FM_MAX_GRID = 2048;

struct FillIdx {
    uint32_t div, per, q, r;
    __device__ __forceinline__ FillIdx(uint32_t e, uint32_t d, uint32_t p) : div(d), per(p) {
        const uint32_t c = e / d;
        q = c % p; r = e - c * d;
    }
    __device__ __forceinline__ void step() { if (++r == div) { r = 0; if (++q == per) q = 0; } }
};

__device__ __forceinline__ uint32_t fill_f32(uint32_t u, float f) { return is_nan_bits(u) ? __float_as_uint(f) : u; }
__device__ __forceinline__ uint32_t fill_bf16(uint32_t h, float f) { return (h & 0x7fffu) > 0x7f80u ? (uint32_t)f2bf(f) : h; }

template <typename T> __device__ __forceinline__ void fill_elem(T *p, uint32_t e, const float *fill, uint32_t div, uint32_t per);
template <> __device__ __forceinline__ void fill_elem<float>(float *p, uint32_t e, const float *fill, uint32_t div, uint32_t per) {
    const uint32_t u = __float_as_uint(*p);
    if (is_nan_bits(u)) *p = fill[(e / div) % per];
}
template <> __device__ __forceinline__ void fill_elem<bf16_t>(bf16_t *p, uint32_t e, const float *fill, uint32_t div, uint32_t per) {
    if ((*p & 0x7fffu) > 0x7f80u) *p = f2bf(fill[(e / div) % per]);
}

template <typename T> __device__ __forceinline__ uint32_t fill_word(uint32_t w, const float *fill, FillIdx &ix);
template <> __device__ __forceinline__ uint32_t fill_word<float>(uint32_t w, const float *fill, FillIdx &ix) {
    const uint32_t o = fill_f32(w, fill[ix.q]);
    ix.step();
    return o;
}
template <> __device__ __forceinline__ uint32_t fill_word<bf16_t>(uint32_t w, const float *fill, FillIdx &ix) {
    const uint32_t lo = fill_bf16(w & 0xffffu, fill[ix.q]);
    ix.step();
    const uint32_t hi = fill_bf16(w >> 16, fill[ix.q]);
    ix.step();
    return lo | (hi << 16);
}

template <typename T>
__global__ void __launch_bounds__(MC_THREADS) fill_missing_kernel(T *__restrict__ x, uint32_t n, const float *__restrict__ fill,
                                                                  uint32_t div, uint32_t per) {
    constexpr uint32_t VE = 16 / (uint32_t)sizeof(T);
    uint32_t head = ((16u - (uint32_t)((uintptr_t)x & 15u)) & 15u) / (uint32_t)sizeof(T);
    if (head > n) head = n;
    const uint32_t nvec = (n - head) / VE;
    const uint32_t tail0 = head + nvec * VE;
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x == 0) {
        if (tid < head) fill_elem<T>(x + tid, tid, fill, div, per);
        if (tail0 + tid < n) fill_elem<T>(x + tail0 + tid, tail0 + tid, fill, div, per);      // (no wrap: n < 2^32 - 256, host)
    }
    uint4 *v = reinterpret_cast<uint4 *>(x + head);
    // a lane's MC_UNROLL vectors of one sweep lie a whole grid apart: a launch of fewer than MC_UNROLL grids of vectors still
    // spreads over every workgroup (one vector per lane), a large one keeps MC_UNROLL loads in flight per lane
    const uint64_t lanes = (uint64_t)gridDim.x * MC_THREADS;
    for (uint64_t i0 = (uint64_t)blockIdx.x * MC_THREADS + tid; i0 < nvec; i0 += lanes * MC_UNROLL) {
        uint4 w[MC_UNROLL];
#pragma unroll
        for (int u = 0; u < MC_UNROLL; ++u) {
            const uint64_t iu = i0 + (uint64_t)u * lanes;
            if (iu < nvec) w[u] = v[iu];
        }
#pragma unroll
        for (int u = 0; u < MC_UNROLL; ++u) {
            const uint64_t iu = i0 + (uint64_t)u * lanes;
            if (iu < nvec) {
                FillIdx ix(head + (uint32_t)iu * VE, div, per);
                uint4 o;
                o.x = fill_word<T>(w[u].x, fill, ix); o.y = fill_word<T>(w[u].y, fill, ix);
                o.z = fill_word<T>(w[u].z, fill, ix); o.w = fill_word<T>(w[u].w, fill, ix);
                v[iu] = o;
            }
        }
    }
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" int dlwpcs_missing_count(const void *x, int dtype, int64_t n_planes, int64_t plane, int32_t *count,
                                    dlwpcs_stream_t stream) {
    if (dtype != DLWPCS_F32 && dtype != DLWPCS_I16)
        return fail(DLWPCS_E_INVALID, "missing_count: dtype %d is neither DLWPCS_F32 nor DLWPCS_I16", dtype);
    if (n_planes < 0 || plane < 0)
        return fail(DLWPCS_E_INVALID, "missing_count: negative extent (%lld planes of %lld)", (long long)n_planes, (long long)plane);
    if (plane >= (1ll << 31)) return fail(DLWPCS_E_UNSUPPORTED, "missing_count: a plane of %lld elements (< 2^31)", (long long)plane);
    if (n_planes == 0) return DLWPCS_OK;
    if (!count) return fail(DLWPCS_E_INVALID, "missing_count: null output");
    if (plane > 0 && !x) return fail(DLWPCS_E_INVALID, "missing_count: null source");
    const size_t esz = dtype == DLWPCS_I16 ? 2 : 4;
    if (((uintptr_t)x) & (esz - 1)) return fail(DLWPCS_E_INVALID, "missing_count: x is not aligned to its %zu-byte elements", esz);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(n_planes < MC_MAX_GRID ? n_planes : MC_MAX_GRID)), blk(MC_THREADS);
    if (dtype == DLWPCS_I16)
        hipLaunchKernelGGL(missing_count_kernel<short>, grid, blk, 0, s, (const short *)x, n_planes, plane, count);
    else
        hipLaunchKernelGGL(missing_count_kernel<float>, grid, blk, 0, s, (const float *)x, n_planes, plane, count);
    return check_launch("missing_count");
}

extern "C" int dlwpcs_fill_missing(void *x, int dtype, size_t n, const float *fill, int fill_div, int fill_period,
                                   dlwpcs_stream_t stream) {
    if (!dtype_ok(dtype)) return fail(DLWPCS_E_INVALID, "fill_missing: dtype %d is neither DLWPCS_F32 nor DLWPCS_BF16", dtype);
    if (n >= (1ull << 32) - MC_THREADS) return fail(DLWPCS_E_UNSUPPORTED, "fill_missing: %zu elements (< 2^32 - %d)", n, MC_THREADS);
    if (fill_div < 1 || fill_period < 1) return fail(DLWPCS_E_INVALID, "fill_missing: the fill field needs div, period >= 1");
    if (n == 0) return DLWPCS_OK;
    if (!x || !fill) return fail(DLWPCS_E_INVALID, "fill_missing: null pointer");
    const size_t esz = dtype_size(dtype);
    if (((uintptr_t)x) & (esz - 1)) return fail(DLWPCS_E_INVALID, "fill_missing: x is not aligned to its %zu-byte elements", esz);
    hipStream_t s = (hipStream_t)stream;
    size_t g = (n * esz / 16 + MC_THREADS - 1) / MC_THREADS;
    if (g > FM_MAX_GRID) g = FM_MAX_GRID;
    if (g < 1) g = 1;
    const dim3 grid((unsigned)g), blk(MC_THREADS);
    if (dtype == DLWPCS_BF16)
        hipLaunchKernelGGL(fill_missing_kernel<bf16_t>, grid, blk, 0, s, (bf16_t *)x, (uint32_t)n, fill, (uint32_t)fill_div,
                           (uint32_t)fill_period);
    else
        hipLaunchKernelGGL(fill_missing_kernel<float>, grid, blk, 0, s, (float *)x, (uint32_t)n, fill, (uint32_t)fill_div,
                           (uint32_t)fill_period);
    return check_launch("fill_missing");
}
