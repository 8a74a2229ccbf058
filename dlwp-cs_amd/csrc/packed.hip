// The resident series in 16-bit packed form (the CF / netCDF convention ERA5 is distributed in): x = q * scale[v] + offset[v], q an
// int16 code in [-32767, 32767], code -32768 = missing = NaN.  Four entry points over a contiguous (T, V, S) array:
//   channel_range     {min, max} over the finite elements of every variable and the count of the others (what scale / offset are
//                     formed from on the host)
//   pack_i16          q = clamp(rint((x - offset[v]) / scale[v]), -32767, 32767), non-finite x -> -32768
//   unpack_i16        x = float(q) * scale[v] + offset[v], -32768 -> NaN
//   batch_gather_i16  dlwpcs_batch_gather (elementwise.hip) out of the codes: same addressing, the value decoded on the way
// Every arithmetic step is one rounded fp32 operation (contraction off in the element functions, plain operators as in
// scaling.hip's affine_elem), so numpy's float32 arithmetic reproduces the bits.
//
// All four are HBM-bound.  channel_range: grid = variable x column tile x row slab; a lane owns one 16-B chunk of a row (one
// element off the vector path) and walks the rows of its slab with RG_UNROLL loads in flight; min / max / count per workgroup
// through LDS into one partial, a second launch folds a variable's partials.  min, max and an integer count do not depend on the
// order, so no care is needed for the bits.  pack / unpack: workgroup = (row (t, v), tile of 2048 elements), the row's scale and
// offset are uniform loads; a lane moves 8 elements (32 B of fp32 against 16 B of codes) on the vector path.
// batch_gather_i16: the three forms of the fp32 gather -- a 64-pixel padded LDS tile for any S / channel window, 256 pixels x all
// channels with 16-B loads (8 codes per lane, half a wave per channel row) and 16-B stores when the gathered channels are the whole
// output row, and a channels-first form that needs no transpose.  The LDS tiles hold DECODED fp32 values, so the write-out loops
// are the fp32 gather's.
#include "strided.h"
#include <math.h>

namespace dlwpcs {

namespace {

constexpr int PK_THREADS = 256;
constexpr int PK_CHUNK = 8;                         // elements per lane of pack / unpack / the wide gathers: 16 B of codes
constexpr int PK_TILE = PK_THREADS * PK_CHUNK;
constexpr int RG_UNROLL = 4;                        // rows in flight per lane
constexpr int64_t RG_TARGET_BLOCKS = 1024;          // 256 CUs x 4
constexpr int PK_FILL = -32768;

// ---- element arithmetic ----------------------------------------------------------------------------------------------

__device__ __forceinline__ float decode_elem(int q, float sc, float off) {
#pragma clang fp contract(off)
    const float m = (float)q * sc;                  // (the conversion is exact)
    const float r = m + off;
    return q == PK_FILL ? __uint_as_float(0x7fc00000u) : r;
}

__device__ __forceinline__ int encode_elem(float x, float sc, float off) {
#pragma clang fp contract(off)
    const float d = x - off;
    const float r = d / sc;
    const float q = fminf(fmaxf(rintf(r), -32767.f), 32767.f);
    return __builtin_isfinite(x) ? (int)q : PK_FILL;
}

__device__ __forceinline__ uint32_t pair16(int lo, int hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); }
__device__ __forceinline__ int code_lo(uint32_t w) { return (int)(int16_t)(w & 0xffffu); }
__device__ __forceinline__ int code_hi(uint32_t w) { return (int)w >> 16; }

// the 8 codes of one 16-B load, decoded
__device__ __forceinline__ void decode8(const uint4 &w, float sc, float off, float v[8]) {
    v[0] = decode_elem(code_lo(w.x), sc, off); v[1] = decode_elem(code_hi(w.x), sc, off);
    v[2] = decode_elem(code_lo(w.y), sc, off); v[3] = decode_elem(code_hi(w.y), sc, off);
    v[4] = decode_elem(code_lo(w.z), sc, off); v[5] = decode_elem(code_hi(w.z), sc, off);
    v[6] = decode_elem(code_lo(w.w), sc, off); v[7] = decode_elem(code_hi(w.w), sc, off);
}

template <typename OT>
__device__ __forceinline__ void store_elem(OT *p, float v) {
    if constexpr (sizeof(OT) == 2) *p = f2bf(v);
    else *p = v;
}

// 8 values to 8 consecutive outputs, p 16-B aligned
template <typename OT>
__device__ __forceinline__ void store8(OT *p, const float v[8]) {
    if constexpr (sizeof(OT) == 2) {
        *reinterpret_cast<uint4 *>(p) = make_uint4(f2bf2(v[0], v[1]), f2bf2(v[2], v[3]), f2bf2(v[4], v[5]), f2bf2(v[6], v[7]));
    } else {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4 *>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
}

// ---- channel_range ---------------------------------------------------------------------------------------------------

struct RangeGeom {
    int64_t T, V, S;
    int64_t ncol;                                   // chunks per row
    int64_t tiles;                                  // column tiles of PK_THREADS chunks
    int64_t slabs, rps;                             // row slabs per (variable, tile), rows per slab
    int64_t units;                                  // tiles * slabs: partials per variable
    int64_t nblk;
};

struct RangePart {
    float mn, mx;
    long long bad;
};

void range_plan(int64_t T, int64_t V, int64_t S, bool vec, RangeGeom &G) {
    G.T = T; G.V = V; G.S = S;
    G.ncol = vec ? S / 4 : S;
    G.tiles = (G.ncol + PK_THREADS - 1) / PK_THREADS;
    const int64_t per = V * G.tiles;
    const int64_t want = (RG_TARGET_BLOCKS + per - 1) / per;
    int64_t rps = (T + want - 1) / want;
    rps = (rps + RG_UNROLL - 1) / RG_UNROLL * RG_UNROLL;
    G.rps = rps;
    G.slabs = (T + rps - 1) / rps;
    G.units = G.tiles * G.slabs;
    G.nblk = V * G.units;
}

// the workgroup's {min, max, count}: valid in thread 0
__device__ __forceinline__ void block_range(float &mn, float &mx, long long &bad) {
    __shared__ float s_mn[PK_THREADS], s_mx[PK_THREADS];
    __shared__ long long s_bad[PK_THREADS];
    s_mn[threadIdx.x] = mn; s_mx[threadIdx.x] = mx; s_bad[threadIdx.x] = bad;
    __syncthreads();
    for (int s = PK_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_mn[threadIdx.x] = fminf(s_mn[threadIdx.x], s_mn[threadIdx.x + s]);
            s_mx[threadIdx.x] = fmaxf(s_mx[threadIdx.x], s_mx[threadIdx.x + s]);
            s_bad[threadIdx.x] += s_bad[threadIdx.x + s];
        }
        __syncthreads();
    }
    mn = s_mn[0]; mx = s_mx[0]; bad = s_bad[0];
}

template <bool VEC>
__global__ void __launch_bounds__(PK_THREADS) channel_range_kernel(RangeGeom G, const float *__restrict__ src,
                                                                   RangePart *__restrict__ partial) {
    constexpr int W = VEC ? 4 : 1;
    const int64_t bid = flat_block();
    if (bid >= G.nblk) return;
    const int64_t v = bid / G.units;
    const int64_t rem = bid - v * G.units;
    const int64_t tile = rem / G.slabs, slab = rem - tile * G.slabs;
    const int64_t q = tile * PK_THREADS + threadIdx.x;
    const int64_t j0 = slab * G.rps;
    const int64_t j1 = j0 + G.rps < G.T ? j0 + G.rps : G.T;
    float mn = INFINITY, mx = -INFINITY;
    long long bad = 0;
    if (q < G.ncol) {
        const float *p = src + v * G.S + q * W;
        const int64_t rs = G.V * G.S;
        for (int64_t j = j0; j < j1; j += RG_UNROLL) {
            float x[RG_UNROLL][W];
#pragma unroll
            for (int u = 0; u < RG_UNROLL; ++u)
                if (j + u < j1) {
                    const float *pr = p + (j + u) * rs;
                    if constexpr (VEC) {
                        const float4 t = *reinterpret_cast<const float4 *>(pr);
                        x[u][0] = t.x; x[u][1] = t.y; x[u][2] = t.z; x[u][3] = t.w;
                    } else {
                        x[u][0] = *pr;
                    }
                }
#pragma unroll
            for (int u = 0; u < RG_UNROLL; ++u)
                if (j + u < j1) {
#pragma unroll
                    for (int k = 0; k < W; ++k) {
                        if (__builtin_isfinite(x[u][k])) {
                            mn = fminf(mn, x[u][k]);
                            mx = fmaxf(mx, x[u][k]);
                        } else {
                            ++bad;
                        }
                    }
                }
        }
    }
    block_range(mn, mx, bad);
    if (threadIdx.x == 0) {
        RangePart r;
        r.mn = mn; r.mx = mx; r.bad = bad;
        partial[bid] = r;
    }
}

// one workgroup per variable folds its partials (units = 0: the empty range)
__global__ void __launch_bounds__(PK_THREADS) channel_range_finish_kernel(int64_t units, const RangePart *__restrict__ partial,
                                                                          float *__restrict__ range, int64_t *__restrict__ nonfinite) {
    const int64_t v = blockIdx.x;
    const RangePart *p = partial + v * units;
    float mn = INFINITY, mx = -INFINITY;
    long long bad = 0;
    for (int64_t i = threadIdx.x; i < units; i += PK_THREADS) {
        const RangePart r = p[i];
        mn = fminf(mn, r.mn);
        mx = fmaxf(mx, r.mx);
        bad += r.bad;
    }
    block_range(mn, mx, bad);
    if (threadIdx.x == 0) {
        range[2 * v] = mn;
        range[2 * v + 1] = mx;
        nonfinite[v] = bad;
    }
}

// ---- pack / unpack ---------------------------------------------------------------------------------------------------

// workgroup = (row (t, v), tile of PK_TILE elements).  VEC (S % 8 == 0, both pointers 16-B aligned): a lane owns 8 consecutive
// elements; otherwise 8 elements PK_THREADS apart.
template <bool VEC>
__global__ void __launch_bounds__(PK_THREADS) pack_i16_kernel(int64_t nblk, int64_t tiles, int64_t V, int64_t S,
                                                              const float *__restrict__ src, const float *__restrict__ scale,
                                                              const float *__restrict__ offset, int16_t *__restrict__ dst) {
    const int64_t bid = flat_block();
    if (bid >= nblk) return;
    const int64_t row = bid / tiles, tile = bid - row * tiles;
    const int64_t v = row % V;
    const float sc = scale[v], off = offset[v];
    const float *ps = src + row * S;
    int16_t *pd = dst + row * S;
    if constexpr (VEC) {
        const int64_t e = tile * PK_TILE + (int64_t)threadIdx.x * PK_CHUNK;
        if (e >= S) return;
        const float4 a = *reinterpret_cast<const float4 *>(ps + e);
        const float4 b = *reinterpret_cast<const float4 *>(ps + e + 4);
        uint4 w;
        w.x = pair16(encode_elem(a.x, sc, off), encode_elem(a.y, sc, off));
        w.y = pair16(encode_elem(a.z, sc, off), encode_elem(a.w, sc, off));
        w.z = pair16(encode_elem(b.x, sc, off), encode_elem(b.y, sc, off));
        w.w = pair16(encode_elem(b.z, sc, off), encode_elem(b.w, sc, off));
        *reinterpret_cast<uint4 *>(pd + e) = w;
    } else {
        float x[PK_CHUNK];
#pragma unroll
        for (int k = 0; k < PK_CHUNK; ++k) {
            const int64_t e = tile * PK_TILE + k * PK_THREADS + threadIdx.x;
            if (e < S) x[k] = ps[e];
        }
#pragma unroll
        for (int k = 0; k < PK_CHUNK; ++k) {
            const int64_t e = tile * PK_TILE + k * PK_THREADS + threadIdx.x;
            if (e < S) pd[e] = (int16_t)encode_elem(x[k], sc, off);
        }
    }
}

template <bool VEC>
__global__ void __launch_bounds__(PK_THREADS) unpack_i16_kernel(int64_t nblk, int64_t tiles, int64_t V, int64_t S,
                                                                const int16_t *__restrict__ src, const float *__restrict__ scale,
                                                                const float *__restrict__ offset, float *__restrict__ dst) {
    const int64_t bid = flat_block();
    if (bid >= nblk) return;
    const int64_t row = bid / tiles, tile = bid - row * tiles;
    const int64_t v = row % V;
    const float sc = scale[v], off = offset[v];
    const int16_t *ps = src + row * S;
    float *pd = dst + row * S;
    if constexpr (VEC) {
        const int64_t e = tile * PK_TILE + (int64_t)threadIdx.x * PK_CHUNK;
        if (e >= S) return;
        float x[8];
        decode8(*reinterpret_cast<const uint4 *>(ps + e), sc, off, x);
        store8<float>(pd + e, x);
    } else {
        int q[PK_CHUNK];
#pragma unroll
        for (int k = 0; k < PK_CHUNK; ++k) {
            const int64_t e = tile * PK_TILE + k * PK_THREADS + threadIdx.x;
            if (e < S) q[k] = ps[e];
        }
#pragma unroll
        for (int k = 0; k < PK_CHUNK; ++k) {
            const int64_t e = tile * PK_TILE + k * PK_THREADS + threadIdx.x;
            if (e < S) pd[e] = decode_elem(q[k], sc, off);
        }
    }
}

// ---- batch gather ----------------------------------------------------------------------------------------------------

// any S, any channel window: 64 pixels x all gathered channels through a padded LDS tile (batch_gather_cl_kernel with the decode
// on the way in)
template <typename OT>
__global__ void __launch_bounds__(256) batch_gather_i16_cl_kernel(const int16_t *__restrict__ array, size_t S, int V,
                                                                  const int32_t *__restrict__ samples,
                                                                  const int32_t *__restrict__ var_idx,
                                                                  const float *__restrict__ scale, const float *__restrict__ offset,
                                                                  int nv, int n_steps, int t_off, int t_stride, OT *__restrict__ out,
                                                                  int Ctot, int c_off, int c_stride) {
    extern __shared__ float tile[];                 // [nch][65]
    const int nch = n_steps * nv;
    const size_t s0 = (size_t)blockIdx.x * 64;
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long t0 = (long)samples[b] + t_off;
    for (int cc = w; cc < nch; cc += 4) {
        const int n = cc / nv, j = cc - n * nv;
        const int var = var_idx[j];
        const int16_t *src = array + ((size_t)(t0 + (long)n * t_stride) * V + var) * S;
        tile[cc * 65 + lane] = (s0 + lane < S) ? decode_elem(src[s0 + lane], scale[var], offset[var]) : 0.f;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * nch; idx += 256) {
        const int px = idx / nch, cc = idx - px * nch;
        if (s0 + px >= S) break;
        const int n = cc / nv, j = cc - n * nv;
        store_elem(out + ((size_t)b * S + s0 + px) * Ctot + c_off + n * c_stride + j, tile[cc * 65 + px]);
    }
}

// the gathered channels ARE the output row (c_off = 0, c_stride = nv, Ctot = n_steps * nv), S % 8 == 0, array and out 16-B aligned:
// 256 pixels x all channels per workgroup.  Half a wave loads 512 contiguous bytes of one channel row (16 B = 8 codes per lane), the
// tile's 256 x nch outputs are one contiguous block of `out`, written as 16-B vectors (npx % 8 == 0, so the block is a whole
// number of vectors for either output type).
template <typename OT>
__global__ void __launch_bounds__(256) batch_gather_i16_cl_rows_kernel(const int16_t *__restrict__ array, size_t S, int V,
                                                                       const int32_t *__restrict__ samples,
                                                                       const int32_t *__restrict__ var_idx,
                                                                       const float *__restrict__ scale,
                                                                       const float *__restrict__ offset, int nv, int n_steps,
                                                                       int t_off, int t_stride, OT *__restrict__ out) {
    extern __shared__ float tile[];                 // [nch][257]
    const int nch = n_steps * nv;
    const size_t s0 = (size_t)blockIdx.x * 256;
    const int b = blockIdx.y;
    const int l32 = threadIdx.x & 31, h = threadIdx.x >> 5;         // 8 half-waves
    const long t0 = (long)samples[b] + t_off;
    const int npx = (int)(S - s0 < 256 ? S - s0 : 256);             // (a multiple of 8)
    for (int cc = h; cc < nch; cc += 8) {
        const int n = cc / nv, j = cc - n * nv;
        const int var = var_idx[j];
        const int16_t *src = array + ((size_t)(t0 + (long)n * t_stride) * V + var) * S + s0;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (l32 * 8 < npx) decode8(*reinterpret_cast<const uint4 *>(src + l32 * 8), scale[var], offset[var], v);
        float *t = tile + cc * 257 + l32 * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = v[k];
    }
    __syncthreads();
    constexpr int EV = 16 / (int)sizeof(OT);        // output elements per 16-B store: 8 bf16 / 4 fp32
    const int total = npx * nch;
    OT *dst = out + ((size_t)b * S + s0) * nch;
    for (int e0 = threadIdx.x * EV; e0 < total; e0 += 256 * EV) {
        int px = e0 / nch, cc = e0 - px * nch;
        float v[EV];
#pragma unroll
        for (int k = 0; k < EV; ++k) {
            v[k] = tile[cc * 257 + px];
            if (++cc == nch) { cc = 0; ++px; }
        }
        if constexpr (sizeof(OT) == 2) {
            *reinterpret_cast<uint4 *>(dst + e0) = make_uint4(f2bf2(v[0], v[1]), f2bf2(v[2], v[3]), f2bf2(v[4], v[5]), f2bf2(v[6], v[7]));
        } else {
            *reinterpret_cast<float4 *>(dst + e0) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

// channels_first: source and destination rows are both contiguous in s.  grid = (strips, gathered channel, b).  VEC (S % 8 == 0,
// array and out 16-B aligned): 8 elements per lane.
template <typename OT, bool VEC>
__global__ void __launch_bounds__(256) batch_gather_i16_cf_kernel(const int16_t *__restrict__ array, size_t S, int V,
                                                                  const int32_t *__restrict__ samples,
                                                                  const int32_t *__restrict__ var_idx,
                                                                  const float *__restrict__ scale, const float *__restrict__ offset,
                                                                  int nv, int t_off, int t_stride, OT *__restrict__ out, int Ctot,
                                                                  int c_off, int c_stride) {
    const int cc = blockIdx.y, b = blockIdx.z;
    const int n = cc / nv, j = cc - n * nv;
    const int var = var_idx[j];
    const float sc = scale[var], off = offset[var];
    const int16_t *src = array + ((size_t)((long)samples[b] + t_off + (long)n * t_stride) * V + var) * S;
    OT *dst = out + ((size_t)b * Ctot + c_off + n * c_stride + j) * S;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    if constexpr (VEC) {
        for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < S / 8; c += step) {
            float v[8];
            decode8(*reinterpret_cast<const uint4 *>(src + c * 8), sc, off, v);
            store8<OT>(dst + c * 8, v);
        }
    } else {
        for (size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += step)
            store_elem(dst + s, decode_elem(src[s], sc, off));
    }
}

int check_tvs(const char *what, int64_t T, int64_t V, int64_t S) {
    if (T < 0 || V < 0 || S < 0)
        return fail(DLWPCS_E_INVALID, "%s: negative extent (T=%lld V=%lld S=%lld)", what, (long long)T, (long long)V, (long long)S);
    return DLWPCS_OK;
}

// the launch geometry of pack / unpack: false = too many workgroups
bool rows_plan(int64_t T, int64_t V, int64_t S, int64_t &tiles, int64_t &nblk) {
    tiles = (S + PK_TILE - 1) / PK_TILE;
    if (T * V > MAX_BLOCKS / tiles) return false;
    nblk = T * V * tiles;
    return true;
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" size_t dlwpcs_channel_range_scratch_bytes(int64_t T, int64_t V, int64_t S) {
    if (check_tvs("channel_range", T, V, S) != DLWPCS_OK) return 0;
    if (T == 0 || V == 0 || S == 0) return 0;
    // sized for either load width: the pointer's alignment is not known here
    RangeGeom G;
    range_plan(T, V, S, false, G);
    int64_t cells = G.nblk;
    if (S % 4 == 0) {
        range_plan(T, V, S, true, G);
        if (G.nblk > cells) cells = G.nblk;
    }
    return (size_t)cells * sizeof(RangePart);
}

extern "C" int dlwpcs_channel_range(const float *src, int64_t T, int64_t V, int64_t S, float *range, int64_t *nonfinite,
                                    void *scratch, size_t scratch_bytes, dlwpcs_stream_t stream) {
    int rc = check_tvs("channel_range", T, V, S);
    if (rc != DLWPCS_OK) return rc;
    if (V >= (1ll << 31)) return fail(DLWPCS_E_UNSUPPORTED, "channel_range: %lld variables (< 2^31)", (long long)V);
    if (V == 0) return DLWPCS_OK;
    if (!range || !nonfinite) return fail(DLWPCS_E_INVALID, "channel_range: null output");
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(PK_THREADS);
    if (T == 0 || S == 0) {
        hipLaunchKernelGGL(channel_range_finish_kernel, dim3((unsigned)V), blk, 0, s, (int64_t)0, (const RangePart *)nullptr, range,
                           nonfinite);
        return check_launch("channel_range");
    }
    if (!src) return fail(DLWPCS_E_INVALID, "channel_range: null source");
    const bool vec = S % 4 == 0 && aligned16(src);
    RangeGeom G;
    range_plan(T, V, S, vec, G);
    if (G.nblk > MAX_BLOCKS) return fail(DLWPCS_E_UNSUPPORTED, "channel_range: %lld workgroups is too many", (long long)G.nblk);
    const size_t need = (size_t)G.nblk * sizeof(RangePart);
    if (!scratch || scratch_bytes < need || (((uintptr_t)scratch) & 7))
        return fail(DLWPCS_E_WORKSPACE, "channel_range: scratch of %zu bytes, need %zu (8-byte aligned)", scratch_bytes, need);
    RangePart *partial = (RangePart *)scratch;
    if (vec) hipLaunchKernelGGL(channel_range_kernel<true>, launch_grid(G.nblk), blk, 0, s, G, src, partial);
    else hipLaunchKernelGGL(channel_range_kernel<false>, launch_grid(G.nblk), blk, 0, s, G, src, partial);
    hipLaunchKernelGGL(channel_range_finish_kernel, dim3((unsigned)V), blk, 0, s, G.units, (const RangePart *)partial, range,
                       nonfinite);
    return check_launch("channel_range");
}

extern "C" int dlwpcs_pack_i16(const float *src, int64_t T, int64_t V, int64_t S, const float *scale, const float *offset,
                               int16_t *dst, dlwpcs_stream_t stream) {
    int rc = check_tvs("pack_i16", T, V, S);
    if (rc != DLWPCS_OK) return rc;
    if (T == 0 || V == 0 || S == 0) return DLWPCS_OK;
    if (!src || !scale || !offset || !dst) return fail(DLWPCS_E_INVALID, "pack_i16: null operand");
    int64_t tiles, nblk;
    if (!rows_plan(T, V, S, tiles, nblk)) return fail(DLWPCS_E_UNSUPPORTED, "pack_i16: too many workgroups");
    const dim3 grid = launch_grid(nblk), blk(PK_THREADS);
    if (S % PK_CHUNK == 0 && aligned16(src) && aligned16(dst))
        hipLaunchKernelGGL(pack_i16_kernel<true>, grid, blk, 0, (hipStream_t)stream, nblk, tiles, V, S, src, scale, offset, dst);
    else
        hipLaunchKernelGGL(pack_i16_kernel<false>, grid, blk, 0, (hipStream_t)stream, nblk, tiles, V, S, src, scale, offset, dst);
    return check_launch("pack_i16");
}

extern "C" int dlwpcs_unpack_i16(const int16_t *src, int64_t T, int64_t V, int64_t S, const float *scale, const float *offset,
                                 float *dst, dlwpcs_stream_t stream) {
    int rc = check_tvs("unpack_i16", T, V, S);
    if (rc != DLWPCS_OK) return rc;
    if (T == 0 || V == 0 || S == 0) return DLWPCS_OK;
    if (!src || !scale || !offset || !dst) return fail(DLWPCS_E_INVALID, "unpack_i16: null operand");
    int64_t tiles, nblk;
    if (!rows_plan(T, V, S, tiles, nblk)) return fail(DLWPCS_E_UNSUPPORTED, "unpack_i16: too many workgroups");
    const dim3 grid = launch_grid(nblk), blk(PK_THREADS);
    if (S % PK_CHUNK == 0 && aligned16(src) && aligned16(dst))
        hipLaunchKernelGGL(unpack_i16_kernel<true>, grid, blk, 0, (hipStream_t)stream, nblk, tiles, V, S, src, scale, offset, dst);
    else
        hipLaunchKernelGGL(unpack_i16_kernel<false>, grid, blk, 0, (hipStream_t)stream, nblk, tiles, V, S, src, scale, offset, dst);
    return check_launch("unpack_i16");
}

extern "C" int dlwpcs_batch_gather_i16(const int16_t *array, int64_t T, int V, int64_t S, const float *scale, const float *offset,
                                       const int32_t *samples_dev, int B, const int32_t *var_idx_dev, int nv, int n_steps,
                                       int t_off, int t_stride, void *out, int Ctot, int c_off, int c_stride, int channels_last,
                                       int dtype, dlwpcs_stream_t stream) {
    if (!dtype_ok(dtype)) return fail(DLWPCS_E_INVALID, "batch_gather_i16: dtype %d is neither DLWPCS_F32 nor DLWPCS_BF16", dtype);
    if (!array || !scale || !offset || !samples_dev || !var_idx_dev || !out)
        return fail(DLWPCS_E_INVALID, "batch_gather_i16: null pointer");
    if (!(T >= 1 && V >= 1 && S >= 1 && B >= 0 && nv >= 1 && n_steps >= 1 && Ctot >= 1 && c_off >= 0 && c_stride >= 0))
        return fail(DLWPCS_E_INVALID, "batch_gather_i16: bad shape T=%lld V=%d S=%lld B=%d nv=%d n_steps=%d", (long long)T, V,
                    (long long)S, B, nv, n_steps);
    if (c_off + (n_steps - 1) * c_stride + nv > Ctot)
        return fail(DLWPCS_E_INVALID, "batch_gather_i16: channel window exceeds Ctot=%d", Ctot);
    if (B == 0) return DLWPCS_OK;
    if (B > 65535) return fail(DLWPCS_E_UNSUPPORTED, "batch_gather_i16: batch > 65535");
    hipStream_t s = (hipStream_t)stream;
    const int nch = n_steps * nv;
    const bool bf = dtype == DLWPCS_BF16;
    const bool wide = S % PK_CHUNK == 0 && aligned16(array) && aligned16(out);
    if (channels_last) {
        const size_t lds = (size_t)nch * 65 * sizeof(float);
        if (lds > 64 * 1024) return fail(DLWPCS_E_UNSUPPORTED, "batch_gather_i16: %d gathered channels exceed the LDS tile", nch);
        const size_t lds_rows = (size_t)nch * 257 * sizeof(float);
        if (wide && c_off == 0 && c_stride == nv && Ctot == nch && lds_rows <= 64 * 1024) {
            const dim3 grid_r((unsigned)((S + 255) / 256), (unsigned)B);
            if (bf)
                hipLaunchKernelGGL(batch_gather_i16_cl_rows_kernel<bf16_t>, grid_r, dim3(256), lds_rows, s, array, (size_t)S, V,
                                   samples_dev, var_idx_dev, scale, offset, nv, n_steps, t_off, t_stride, (bf16_t *)out);
            else
                hipLaunchKernelGGL(batch_gather_i16_cl_rows_kernel<float>, grid_r, dim3(256), lds_rows, s, array, (size_t)S, V,
                                   samples_dev, var_idx_dev, scale, offset, nv, n_steps, t_off, t_stride, (float *)out);
            return check_launch("batch_gather_i16");
        }
        const dim3 grid((unsigned)((S + 63) / 64), (unsigned)B);
        if (bf)
            hipLaunchKernelGGL(batch_gather_i16_cl_kernel<bf16_t>, grid, dim3(256), lds, s, array, (size_t)S, V, samples_dev,
                               var_idx_dev, scale, offset, nv, n_steps, t_off, t_stride, (bf16_t *)out, Ctot, c_off, c_stride);
        else
            hipLaunchKernelGGL(batch_gather_i16_cl_kernel<float>, grid, dim3(256), lds, s, array, (size_t)S, V, samples_dev,
                               var_idx_dev, scale, offset, nv, n_steps, t_off, t_stride, (float *)out, Ctot, c_off, c_stride);
        return check_launch("batch_gather_i16");
    }
    if (nch > 65535) return fail(DLWPCS_E_UNSUPPORTED, "batch_gather_i16: too many channels");
    size_t gx = ((wide ? S / PK_CHUNK : S) + 255) / 256;
    if (gx > 64) gx = 64;
    const dim3 grid((unsigned)gx, (unsigned)nch, (unsigned)B);
#define GATHER_CF(OT, VEC)                                                                                                       \
    hipLaunchKernelGGL((batch_gather_i16_cf_kernel<OT, VEC>), grid, dim3(256), 0, s, array, (size_t)S, V, samples_dev, var_idx_dev, \
                       scale, offset, nv, t_off, t_stride, (OT *)out, Ctot, c_off, c_stride)
    if (bf) { if (wide) GATHER_CF(bf16_t, true); else GATHER_CF(bf16_t, false); }
    else { if (wide) GATHER_CF(float, true); else GATHER_CF(float, false); }
#undef GATHER_CF
    return check_launch("batch_gather_i16");
}
