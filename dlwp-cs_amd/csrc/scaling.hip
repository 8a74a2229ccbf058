// Per-variable data scaling (reference DLWP/model/preprocessing.py:645-682, 844-882; Tutorial 4 cell 19): the moments of every
// channel of a resident fp32 array, and the per-channel affine transform in both directions.  Both address the array as
// (R rows, C channels, S inner elements) through dlwpcs_chan_desc, strides in elements.
//
// channel_moments_kernel: grid = channel x column tile x row slab, 256 threads.  A lane owns one chunk of a row (a float4 on the
// vector path, one element otherwise) and walks the rows of its slab with CM_UNROLL loads in flight, so neighbouring lanes read
// neighbouring addresses of one row and the row index is one scalar load per row.  fp64 accumulators in registers (one set per
// vector component), a wave reduction by __shfl_down, LDS across the four waves, one partial triple {n, s1, s2} per workgroup.
// channel_finish_kernel (one workgroup per channel) adds a channel's partials in index order.  The partition -- CM_THREADS columns
// per tile, rows per slab from CM_TARGET_BLOCKS -- is a function of the descriptor and the row count only, and no addition's
// place depends on the grid's timing: the same call gives the same bits.  No atomics.
//
// channel_affine_*: y = x * a[c] + b[c] or (x - b[c]) / a[c] as two rounded fp32 operations (contraction off in the element
// function; the tests compare bits with numpy).  rows: 16-byte loads and stores along a row, the channel uniform per workgroup.
// flat: both sides one channels-last stream, 16-byte loads and stores over it, channel = flat index mod C carried incrementally,
// tables in LDS.  any: one element per lane, lanes along the destination's contiguous dim; with lanes along s a workgroup loops
// over the channels itself, so a channels-last source is fetched from HBM once and re-read from the cache.
#include "strided.h"

namespace dlwpcs {

namespace {

constexpr int CM_THREADS = 256;
constexpr int CM_WAVES = CM_THREADS / 64;
constexpr int CM_UNROLL = 8;                    // rows in flight per lane
constexpr int64_t CM_TARGET_BLOCKS = 512;       // 256 CUs x 2
constexpr int CA_THREADS = 256;
constexpr int CA_UNROLL = 4;                    // 16-byte chunks per lane

// ---- moments ---------------------------------------------------------------------------------------------------------

struct MomGeom {
    int64_t C, NR;                              // channels, selected rows
    int64_t rs, cs, is;                         // source strides
    int64_t ncol;                               // chunks per row
    int64_t tiles;                              // column tiles of CM_THREADS chunks
    int64_t slabs, rps;                         // row slabs per (channel, tile), rows per slab (a multiple of CM_UNROLL)
    int64_t units;                              // tiles * slabs: partials per channel
    int64_t nblk;
};

// the three block sums, in a fixed order: lanes by __shfl_down, then the waves in wave order.  Valid in thread 0.
__device__ __forceinline__ void block_sum3(double v[3]) {
    __shared__ double sh[3][CM_WAVES];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) sh[k][wave] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double t = sh[k][0];
#pragma unroll
            for (int w = 1; w < CM_WAVES; ++w) t += sh[k][w];
            v[k] = t;
        }
    }
}

template <bool VEC, bool SKIP>
__global__ void __launch_bounds__(CM_THREADS) channel_moments_kernel(MomGeom G, const float *__restrict__ src,
                                                                    const int32_t *__restrict__ rows,
                                                                    const double *__restrict__ center,
                                                                    double *__restrict__ partial) {
    constexpr int V = VEC ? 4 : 1;
    const int64_t bid = flat_block();
    if (bid >= G.nblk) return;
    const int64_t c = bid / G.units;
    const int64_t rem = bid - c * G.units;
    const int64_t tile = rem / G.slabs, slab = rem - tile * G.slabs;
    const int64_t q = tile * CM_THREADS + threadIdx.x;
    const double ctr = center ? center[c] : 0.0;
    const int64_t j0 = slab * G.rps;
    const int64_t j1 = j0 + G.rps < G.NR ? j0 + G.rps : G.NR;
    double s1[V], s2[V];
    unsigned long long n = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) { s1[v] = 0.0; s2[v] = 0.0; }
    if (q < G.ncol) {
        const float *p = src + c * G.cs + q * V * G.is;
        for (int64_t j = j0; j < j1; j += CM_UNROLL) {
            float x[CM_UNROLL][V];
#pragma unroll
            for (int u = 0; u < CM_UNROLL; ++u)
                if (j + u < j1) {
                    const int64_t r = rows ? (int64_t)rows[j + u] : j + u;
                    const float *pr = p + r * G.rs;
                    if constexpr (VEC) {
                        const float4 t = *reinterpret_cast<const float4 *>(pr);
                        x[u][0] = t.x; x[u][1] = t.y; x[u][2] = t.z; x[u][3] = t.w;
                    } else {
                        x[u][0] = *pr;
                    }
                }
#pragma unroll
            for (int u = 0; u < CM_UNROLL; ++u)
                if (j + u < j1) {
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        if (SKIP && isnan(x[u][v])) continue;
                        const double d = (double)x[u][v] - ctr;
                        s1[v] += d;
                        s2[v] += d * d;
                        ++n;
                    }
                }
        }
    }
    double t[3];
    t[0] = (double)n;                                       // exact: a workgroup counts far fewer than 2^53 elements
    if constexpr (VEC) {
        t[1] = (s1[0] + s1[1]) + (s1[2] + s1[3]);
        t[2] = (s2[0] + s2[1]) + (s2[2] + s2[3]);
    } else {
        t[1] = s1[0];
        t[2] = s2[0];
    }
    block_sum3(t);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) partial[bid * 3 + k] = t[k];
    }
}

// out[c] = the channel's partials added in index order: thread i takes i, i + 256, ..., then the block sum
__global__ void __launch_bounds__(CM_THREADS) channel_finish_kernel(int64_t units, const double *__restrict__ partial,
                                                                   double *__restrict__ out) {
    const int64_t c = blockIdx.x;
    const double *p = partial + c * units * 3;
    double t[3] = {0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < units; i += CM_THREADS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] += p[i * 3 + k];
    }
    block_sum3(t);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[c * 3 + k] = t[k];
    }
}

int check_desc(const dlwpcs_chan_desc *d, const char *what, bool with_dst) {
    if (!d) return fail(DLWPCS_E_INVALID, "%s: null descriptor", what);
    if (d->R < 0 || d->C < 0 || d->S < 0)
        return fail(DLWPCS_E_INVALID, "%s: negative extent (R=%lld C=%lld S=%lld)", what, (long long)d->R, (long long)d->C, (long long)d->S);
    if (d->row_stride < 0 || d->chan_stride < 0 || d->inner_stride < 0 ||
        (with_dst && (d->dst_row_stride < 0 || d->dst_chan_stride < 0 || d->dst_inner_stride < 0)))
        return fail(DLWPCS_E_INVALID, "%s: negative stride", what);
    return DLWPCS_OK;
}

// a stride over an extent of one is never multiplied by anything but zero
inline bool mult4(int64_t stride, int64_t ext) { return ext <= 1 || stride % 4 == 0; }

bool moments_vec_shape(const dlwpcs_chan_desc *d) {
    return d->inner_stride == 1 && d->S % 4 == 0 && mult4(d->row_stride, d->R) && mult4(d->chan_stride, d->C);
}

void moments_plan(const dlwpcs_chan_desc *d, int64_t nr, bool vec, MomGeom &G) {
    G.C = d->C;
    G.NR = nr;
    G.rs = d->row_stride; G.cs = d->chan_stride; G.is = d->inner_stride;
    G.ncol = vec ? d->S / 4 : d->S;
    G.tiles = (G.ncol + CM_THREADS - 1) / CM_THREADS;
    const int64_t per = G.C * G.tiles;
    int64_t want = (CM_TARGET_BLOCKS + per - 1) / per;
    if (want < 1) want = 1;
    int64_t rps = (nr + want - 1) / want;
    rps = (rps + CM_UNROLL - 1) / CM_UNROLL * CM_UNROLL;
    G.rps = rps;
    G.slabs = (nr + rps - 1) / rps;
    G.units = G.tiles * G.slabs;
    G.nblk = G.C * G.units;
}

// ---- affine ----------------------------------------------------------------------------------------------------------

// (plain operators: the pragma governs the operations written in this block, not the bodies of inlined helpers such as
// __fmul_rn -- the compiler fused those into one fma)
template <int MODE>
__device__ __forceinline__ float affine_elem(float x, float a, float b) {
#pragma clang fp contract(off)
    if constexpr (MODE == DLWPCS_AFFINE_MUL_ADD) {
        const float m = x * a;
        return m + b;
    } else {
        const float s = x - b;
        return s / a;
    }
}

struct AffGeom {
    int64_t R, C, S;
    int64_t srs, scs, sis, drs, dcs, dis;
    int64_t tiles;                              // per row (rows / any), of the whole stream (flat)
    int64_t total;                              // flat: elements of the stream
    int64_t nblk;
};

// both sides contiguous along s: workgroup = (r, c, tile of CA_THREADS * CA_UNROLL chunks)
template <int MODE>
__global__ void __launch_bounds__(CA_THREADS) channel_affine_rows_kernel(AffGeom G, const float *src, const float *__restrict__ a,
                                                                        const float *__restrict__ b, float *dst) {
    const int64_t bid = flat_block();
    if (bid >= G.nblk) return;
    const int64_t rc = bid / G.tiles, tile = bid - rc * G.tiles;
    const int64_t r = rc / G.C, c = rc - r * G.C;
    const float av = a[c], bv = b[c];
    const float *ps = src + r * G.srs + c * G.scs;
    float *pd = dst + r * G.drs + c * G.dcs;
    const int64_t q0 = tile * (CA_THREADS * CA_UNROLL) + threadIdx.x, nq = G.S / 4;
    float4 x[CA_UNROLL];
#pragma unroll
    for (int u = 0; u < CA_UNROLL; ++u) {
        const int64_t q = q0 + u * CA_THREADS;
        if (q < nq) x[u] = *reinterpret_cast<const float4 *>(ps + q * 4);
    }
#pragma unroll
    for (int u = 0; u < CA_UNROLL; ++u) {
        const int64_t q = q0 + u * CA_THREADS;
        if (q < nq) {
            float4 y;
            y.x = affine_elem<MODE>(x[u].x, av, bv);
            y.y = affine_elem<MODE>(x[u].y, av, bv);
            y.z = affine_elem<MODE>(x[u].z, av, bv);
            y.w = affine_elem<MODE>(x[u].w, av, bv);
            *reinterpret_cast<float4 *>(pd + q * 4) = y;
        }
    }
}

// both sides one channels-last stream of G.total elements, channel = index mod C: workgroup = CA_THREADS * CA_UNROLL chunks
template <int MODE>
__global__ void __launch_bounds__(CA_THREADS) channel_affine_flat_kernel(AffGeom G, const float *src, const float *__restrict__ a,
                                                                        const float *__restrict__ b, float *dst) {
    __shared__ float sa[DLWPCS_AFFINE_MAX_CHANNELS], sb[DLWPCS_AFFINE_MAX_CHANNELS];
    const int64_t bid = flat_block();
    if (bid >= G.nblk) return;
    const uint32_t C = (uint32_t)G.C;
    for (uint32_t i = threadIdx.x; i < C; i += CA_THREADS) { sa[i] = a[i]; sb[i] = b[i]; }
    __syncthreads();
    constexpr uint32_t SPAN = CA_THREADS * 4;                       // elements between a lane's chunks
    const int64_t base = bid * (int64_t)(SPAN * CA_UNROLL);
    const uint32_t bm = (uint32_t)(base % (int64_t)C);
    uint32_t m = (bm + threadIdx.x * 4u) % C;                       // channel of the lane's first element
    const uint32_t step = SPAN % C;
    float4 x[CA_UNROLL];
#pragma unroll
    for (int u = 0; u < CA_UNROLL; ++u) {
        const int64_t e = base + (int64_t)u * SPAN + threadIdx.x * 4;
        if (e + 4 <= G.total) x[u] = *reinterpret_cast<const float4 *>(src + e);
    }
#pragma unroll
    for (int u = 0; u < CA_UNROLL; ++u) {
        const int64_t e = base + (int64_t)u * SPAN + threadIdx.x * 4;
        uint32_t ch[4];
        ch[0] = m;
#pragma unroll
        for (int k = 1; k < 4; ++k) ch[k] = ch[k - 1] + 1 == C ? 0 : ch[k - 1] + 1;
        if (e + 4 <= G.total) {
            float4 y;
            y.x = affine_elem<MODE>(x[u].x, sa[ch[0]], sb[ch[0]]);
            y.y = affine_elem<MODE>(x[u].y, sa[ch[1]], sb[ch[1]]);
            y.z = affine_elem<MODE>(x[u].z, sa[ch[2]], sb[ch[2]]);
            y.w = affine_elem<MODE>(x[u].w, sa[ch[3]], sb[ch[3]]);
            *reinterpret_cast<float4 *>(dst + e) = y;
        } else {
            for (int k = 0; k < 4; ++k)                             // the stream's last, partial chunk
                if (e + k < G.total) dst[e + k] = affine_elem<MODE>(src[e + k], sa[ch[k]], sb[ch[k]]);
        }
        m += step;
        if (m >= C) m -= C;
    }
}

// any strides, one element per lane.  CFAST = false: lanes along s, workgroup = (r, tile of s), loops over the channels.
// CFAST = true (destination contiguous along c): lanes along the (s, c) pairs of a row, c fastest; S * C < 2^31 (host).
template <int MODE, bool CFAST>
__global__ void __launch_bounds__(CA_THREADS) channel_affine_any_kernel(AffGeom G, const float *src, const float *__restrict__ a,
                                                                       const float *__restrict__ b, float *dst) {
    const int64_t bid = flat_block();
    if (bid >= G.nblk) return;
    const int64_t r = bid / G.tiles, tile = bid - r * G.tiles;
    const int64_t i = tile * CA_THREADS + threadIdx.x;
    const float *ps = src + r * G.srs;
    float *pd = dst + r * G.drs;
    if constexpr (CFAST) {
        if (i >= G.S * G.C) return;
        const uint32_t s = (uint32_t)i / (uint32_t)G.C, c = (uint32_t)i - s * (uint32_t)G.C;
        pd[c * G.dcs + s * G.dis] = affine_elem<MODE>(ps[c * G.scs + s * G.sis], a[c], b[c]);
    } else {
        if (i >= G.S) return;
        ps += i * G.sis;
        pd += i * G.dis;
        for (int64_t c0 = 0; c0 < G.C; c0 += CA_UNROLL) {
            float x[CA_UNROLL];
#pragma unroll
            for (int u = 0; u < CA_UNROLL; ++u)
                if (c0 + u < G.C) x[u] = ps[(c0 + u) * G.scs];
#pragma unroll
            for (int u = 0; u < CA_UNROLL; ++u)
                if (c0 + u < G.C) pd[(c0 + u) * G.dcs] = affine_elem<MODE>(x[u], a[c0 + u], b[c0 + u]);
        }
    }
}


}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" size_t dlwpcs_channel_moments_scratch_bytes(const dlwpcs_chan_desc *d, int64_t n_rows) {
    if (check_desc(d, "channel_moments", false) != DLWPCS_OK) return 0;
    const int64_t nr = n_rows > 0 ? n_rows : d->R;
    if (nr == 0 || d->C == 0 || d->S == 0) return 0;
    // sized for either load width: the pointer's alignment is not known here
    MomGeom G;
    moments_plan(d, nr, false, G);
    int64_t cells = G.nblk;
    if (moments_vec_shape(d)) {
        moments_plan(d, nr, true, G);
        if (G.nblk > cells) cells = G.nblk;
    }
    return (size_t)cells * 3 * sizeof(double);
}

extern "C" int dlwpcs_channel_moments(const dlwpcs_chan_desc *d, const float *src, const int32_t *rows, int64_t n_rows,
                                      const double *center, int skipna, double *out, void *scratch, size_t scratch_bytes,
                                      dlwpcs_stream_t stream) {
    int rc = check_desc(d, "channel_moments", false);
    if (rc != DLWPCS_OK) return rc;
    if (rows && n_rows < 0) return fail(DLWPCS_E_INVALID, "channel_moments: negative row count");
    if (d->R >= (1ll << 31)) return fail(DLWPCS_E_UNSUPPORTED, "channel_moments: %lld rows (< 2^31)", (long long)d->R);
    if (d->C >= (1ll << 31)) return fail(DLWPCS_E_UNSUPPORTED, "channel_moments: %lld channels (< 2^31)", (long long)d->C);
    if (d->C == 0) return DLWPCS_OK;
    if (!out) return fail(DLWPCS_E_INVALID, "channel_moments: null output");
    hipStream_t s = (hipStream_t)stream;
    const int64_t nr = rows ? n_rows : d->R;
    if (nr == 0 || d->S == 0) {
        if (hipMemsetAsync(out, 0, (size_t)d->C * 3 * sizeof(double), s) != hipSuccess) return check_launch("channel_moments");
        return DLWPCS_OK;
    }
    if (!src) return fail(DLWPCS_E_INVALID, "channel_moments: null source");
    const bool vec = moments_vec_shape(d) && aligned16(src);
    MomGeom G;
    moments_plan(d, nr, vec, G);
    if (G.nblk > MAX_BLOCKS) return fail(DLWPCS_E_UNSUPPORTED, "channel_moments: %lld workgroups is too many", (long long)G.nblk);
    const size_t need = (size_t)G.nblk * 3 * sizeof(double);
    if (!scratch || scratch_bytes < need || (((uintptr_t)scratch) & 7))
        return fail(DLWPCS_E_WORKSPACE, "channel_moments: scratch of %zu bytes, need %zu (8-byte aligned)", scratch_bytes, need);
    double *partial = (double *)scratch;
    const dim3 grid = launch_grid(G.nblk), blk(CM_THREADS);
#define CM_LAUNCH(VEC, SKIP) \
    hipLaunchKernelGGL((channel_moments_kernel<VEC, SKIP>), grid, blk, 0, s, G, src, rows, center, partial)
    if (vec) { if (skipna) CM_LAUNCH(true, true); else CM_LAUNCH(true, false); }
    else { if (skipna) CM_LAUNCH(false, true); else CM_LAUNCH(false, false); }
#undef CM_LAUNCH
    hipLaunchKernelGGL(channel_finish_kernel, dim3((unsigned)G.C), blk, 0, s, G.units, partial, out);
    return check_launch("channel_moments");
}

extern "C" int dlwpcs_channel_affine(const dlwpcs_chan_desc *d, const float *src, const float *a, const float *b, int mode,
                                     float *dst, dlwpcs_stream_t stream) {
    int rc = check_desc(d, "channel_affine", true);
    if (rc != DLWPCS_OK) return rc;
    if (mode != DLWPCS_AFFINE_MUL_ADD && mode != DLWPCS_AFFINE_SUB_DIV) return fail(DLWPCS_E_INVALID, "channel_affine: mode %d", mode);
    if (d->C > DLWPCS_AFFINE_MAX_CHANNELS)
        return fail(DLWPCS_E_UNSUPPORTED, "channel_affine: %lld channels, at most %d are served", (long long)d->C, DLWPCS_AFFINE_MAX_CHANNELS);
    if (d->R == 0 || d->C == 0 || d->S == 0) return DLWPCS_OK;
    if (!src || !a || !b || !dst) return fail(DLWPCS_E_INVALID, "channel_affine: null operand");
    AffGeom G;
    G.R = d->R; G.C = d->C; G.S = d->S;
    G.srs = d->row_stride; G.scs = d->chan_stride; G.sis = d->inner_stride;
    G.drs = d->dst_row_stride; G.dcs = d->dst_chan_stride; G.dis = d->dst_inner_stride;
    G.total = 0;
    const bool al = aligned16(src) && aligned16(dst);
    const bool one_s = d->S == 1, one_c = d->C == 1, one_r = d->R == 1;
    const bool rows_path = al && G.sis == 1 && G.dis == 1 && d->S % 4 == 0 && mult4(G.srs, d->R) &&
                           mult4(G.scs, d->C) && mult4(G.drs, d->R) && mult4(G.dcs, d->C);
    const bool flat_path = !rows_path && al && (one_c || (G.scs == 1 && G.dcs == 1)) && (one_s || (G.sis == d->C && G.dis == d->C)) &&
                           (one_r || (G.srs == d->S * d->C && G.drs == d->S * d->C));
    void (*kernel)(AffGeom, const float *, const float *, const float *, float *);
    const bool mul = mode == DLWPCS_AFFINE_MUL_ADD;
    if (rows_path) {
        const int64_t per = (int64_t)CA_THREADS * CA_UNROLL;
        G.tiles = (d->S / 4 + per - 1) / per;
        G.nblk = d->R * d->C * G.tiles;
        kernel = mul ? channel_affine_rows_kernel<DLWPCS_AFFINE_MUL_ADD> : channel_affine_rows_kernel<DLWPCS_AFFINE_SUB_DIV>;
    } else if (flat_path) {
        const int64_t per = (int64_t)CA_THREADS * CA_UNROLL * 4;
        G.total = d->R * d->C * d->S;
        G.tiles = (G.total + per - 1) / per;
        G.nblk = G.tiles;
        kernel = mul ? channel_affine_flat_kernel<DLWPCS_AFFINE_MUL_ADD> : channel_affine_flat_kernel<DLWPCS_AFFINE_SUB_DIV>;
    } else if (G.dcs == 1 && G.dis != 1 && !one_c) {
        if (d->S * d->C >= (1ll << 31))
            return fail(DLWPCS_E_UNSUPPORTED, "channel_affine: %lld elements per row on the one-element path (< 2^31)",
                        (long long)(d->S * d->C));
        G.tiles = (d->S * d->C + CA_THREADS - 1) / CA_THREADS;
        G.nblk = d->R * G.tiles;
        kernel = mul ? channel_affine_any_kernel<DLWPCS_AFFINE_MUL_ADD, true> : channel_affine_any_kernel<DLWPCS_AFFINE_SUB_DIV, true>;
    } else {
        G.tiles = (d->S + CA_THREADS - 1) / CA_THREADS;
        G.nblk = d->R * G.tiles;
        kernel = mul ? channel_affine_any_kernel<DLWPCS_AFFINE_MUL_ADD, false> : channel_affine_any_kernel<DLWPCS_AFFINE_SUB_DIV, false>;
    }
    if (G.nblk > MAX_BLOCKS) return fail(DLWPCS_E_UNSUPPORTED, "channel_affine: %lld workgroups is too many", (long long)G.nblk);
    hipLaunchKernelGGL(kernel, launch_grid(G.nblk), dim3(CA_THREADS), 0, (hipStream_t)stream, G, src, a, b, dst);
    return check_launch("channel_affine");
}
