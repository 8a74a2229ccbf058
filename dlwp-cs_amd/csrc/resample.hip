// Block-bootstrap means along the row axis (dlwpcs_row_resample): B resamples of the T rows of a row set, each a list of nb blocks
// of L consecutive rows (wrapping) whose starts come from a (B, nb) int32 table, per element the mean of the drawn entries that are
// not NaN.  include/dlwpcs.h states the operations; the ORDER (a block's rows from zero, then the blocks from zero, fp64) is a
// property of the resample, so one lane does all of a (resample, element) and nothing depends on how the work is cut.
//
// Staged form.  A resample reuses the same T rows over and over, so a workgroup copies a tile of W columns x T rows into LDS once
// (coalesced, 16-byte loads where the layout allows) and serves its resamples from there: the series is read from memory once
// instead of B times.  The tile lies at [row][column]: the lanes of a wave read W consecutive dwords of one row, consecutive banks.
// A wave holds 64 / W resamples (W = 64: one, up to 640 rows; W = 32: two, one per half-wave, up to 1280 rows); the block starts are
// uniform over the wave (per half-wave: two scalar loads and a select), as the row index is in group_mean_kernel.  1024 threads:
// the 160 KiB tile allows one workgroup per compute unit, and 4-byte LDS reads want about four waves per SIMD to reach their rate.
// Work items are (column tile, resample range); a fixed number of persistent workgroups strides over them and restages only when
// the column tile changes.  With fewer column tiles than compute units the resamples are cut into ranges so that small K under
// large B still fills the chip; each range then stages its tile again, which the planner prices (rs_plan).
//
// Direct form.  The same loops read the rows from memory: for T beyond the staged cap.  A tile's rows are read B times but a tile
// of 64 columns x T rows stays in L2 for the sizes in question.  No LDS.
//
// No profiler tags: the launch profiler's registry is the convolution family's, as for the other verification kernels.
#include <string.h>
#include "strided.h"

namespace dlwpcs {

namespace {

constexpr int RS_STAGED_THREADS = 1024;
constexpr int RS_DIRECT_THREADS = 256;
constexpr int RS_DIRECT_W = 64;
constexpr int RS_UNROLL = 8;                        // reads of a group, issued back to back
constexpr int RS_STAGE_UNROLL = 4;                  // rows in flight per lane while staging
constexpr int64_t RS_CUS = 256;                     // compute units: placement only, no bit depends on it
constexpr int64_t RS_DIRECT_SLOTS = RS_CUS * 8;     // persistent workgroups of the direct form
constexpr int64_t RS_STAGED_MIN_RANGE = 32;         // resamples of a range at the least: staging a tile costs about 16
constexpr int64_t RS_DIRECT_MIN_RANGE = 4;

struct RsClass { int rows, w; };
constexpr int RS_NCLASS = 2;
constexpr RsClass RS_CLASSES[RS_NCLASS] = {{640, 64}, {1280, 32}};
constexpr int RS_CAP = RS_CLASSES[RS_NCLASS - 1].rows;

struct RsGeom {
    RowsAddr A;                                     // nblk: workgroups of the launch; ncol: chunks per row
    int64_t inner;                                  // elements per row
    int64_t items, splits;                          // work items = column tiles x resample ranges
    int64_t B, per;                                 // resamples, resamples per range
    int64_t nb;
    int32_t T, L, last_len, need;
};

// element e of a row -> element offsets; the geometry counts chunks of V
template <int V>
__device__ __forceinline__ void rs_element_offsets(const RsGeom &G, int64_t e, int64_t &soff, int64_t &ooff) {
    int64_t s, o;
    rows_offsets<V, false>(G.A, e / V, s, o);
    const int v = (int)(e % V);
    soff = s + v;                                   // (V = 4 only where the last dim has stride 1)
    ooff = o + v * G.A.last_out_stride();
}

struct RsLdsColumn {
    const float *col;
    int32_t w;
    __device__ __forceinline__ float get(int32_t r) const { return col[r * w]; }
};

struct RsMemColumn {
    const float *p;
    int64_t rs;
    __device__ __forceinline__ float get(int32_t r) const { return p[(int64_t)r * rs]; }
};

// a start that is out of range reads no row outside the series
__device__ __forceinline__ int32_t rs_start(int32_t s, int32_t T) { return s < 0 ? 0 : (s >= T ? T - 1 : s); }

// s and n never hold -0 (they start at +0 and IEEE sums of +0 give +0), so adding the +0 of a missing entry changes no bit
__device__ __forceinline__ void rs_add(float x, double &s, int32_t &n) {
    const bool ok = !isnan(x);
    s += ok ? (double)x : 0.0;
    n += ok ? 1 : 0;
}

// the block starts of RS_UNROLL consecutive blocks, raw: scalar loads with nothing between them
template <int SUBS>
__device__ __forceinline__ void rs_fetch(const int32_t *__restrict__ sa, const int32_t *__restrict__ sb, int64_t j, int32_t a[RS_UNROLL],
                                         int32_t b[RS_UNROLL]) {
#pragma unroll
    for (int u = 0; u < RS_UNROLL; ++u) {
        a[u] = sa[j + u];
        if constexpr (SUBS == 2) b[u] = sb[j + u];
    }
}

// this lane's start out of the wave's one or two
template <int SUBS>
__device__ __forceinline__ int32_t rs_pick(int32_t a, int32_t b, int sub, int32_t T) {
    int32_t st = rs_start(a, T);
    if constexpr (SUBS == 2) {
        const int32_t s1 = rs_start(b, T);
        st = sub ? s1 : st;
    }
    return st;
}

// row st + i of the series, wrapped: st < T and i < L <= T < 2^31, so the sum fits 32 unsigned bits
__device__ __forceinline__ int32_t rs_wrap(int32_t st, uint32_t i, int32_t T) {
    const uint32_t r = (uint32_t)st + i;
    return (int32_t)(r >= (uint32_t)T ? r - (uint32_t)T : r);
}

// One (resample, element): the total and count of the drawn entries.  sa / sb: the block starts of the wave's resamples (SUBS = 2:
// sub selects the half-wave's own); uniform pointers, so the loads are scalar.  Scalar loads and LDS reads share one counter and
// scalar loads return out of order, so a start that is waited for drains every read in flight: the starts of a whole group are
// fetched before its reads, the group's reads are issued back to back, and the next group's starts are fetched under them.
template <int SUBS, bool L1, class Column>
__device__ __forceinline__ void rs_lane(const RsGeom &G, const Column &c, const int32_t *__restrict__ sa,
                                        const int32_t *__restrict__ sb, int sub, double &tot, int32_t &cnt) {
    const int32_t T = G.T;
    tot = 0.0;
    cnt = 0;
    if constexpr (L1) {
        // blocks of one row: the block sum is +0 + x, and tot + (+0 + x) has the bits of tot + x (tot is never -0)
        const int64_t full = G.nb - G.nb % RS_UNROLL;
        int32_t a[RS_UNROLL], b[RS_UNROLL];
        if (full) rs_fetch<SUBS>(sa, sb, 0, a, b);
        for (int64_t j = 0; j < full; j += RS_UNROLL) {
            float x[RS_UNROLL];
#pragma unroll
            for (int u = 0; u < RS_UNROLL; ++u) x[u] = c.get(rs_pick<SUBS>(a[u], b[u], sub, T));
            if (j + RS_UNROLL < full) rs_fetch<SUBS>(sa, sb, j + RS_UNROLL, a, b);
#pragma unroll
            for (int u = 0; u < RS_UNROLL; ++u) rs_add(x[u], tot, cnt);
        }
        for (int64_t j = full; j < G.nb; ++j) rs_add(c.get(rs_pick<SUBS>(sa[j], SUBS == 2 ? sb[j] : 0, sub, T)), tot, cnt);
    } else {
        int32_t a = sa[0], b = SUBS == 2 ? sb[0] : 0;
        for (int64_t j = 0; j < G.nb; ++j) {
            const int32_t st = rs_pick<SUBS>(a, b, sub, T);
            if (j + 1 < G.nb) {                             // the next block's start, under this block's reads
                a = sa[j + 1];
                if constexpr (SUBS == 2) b = sb[j + 1];
            }
            const uint32_t len = (uint32_t)(j == G.nb - 1 ? G.last_len : G.L);
            double s = 0.0;
            int32_t n = 0;
            uint32_t i = 0;
            for (; i + RS_UNROLL <= len; i += RS_UNROLL) {
                float x[RS_UNROLL];
#pragma unroll
                for (int u = 0; u < RS_UNROLL; ++u) x[u] = c.get(rs_wrap(st, i + u, T));
#pragma unroll
                for (int u = 0; u < RS_UNROLL; ++u) rs_add(x[u], s, n);
            }
            for (; i < len; ++i) rs_add(c.get(rs_wrap(st, i, T)), s, n);
            tot += s;
            cnt += n;
        }
    }
}

__device__ __forceinline__ void rs_store(const RsGeom &G, double tot, int32_t cnt, float *__restrict__ out,
                                         int32_t *__restrict__ count, int64_t off) {
    float r = quiet_nan();
    if (cnt >= G.need) {
        r = (float)(tot / (double)cnt);
        r = r != r ? quiet_nan() : r;
    }
    out[off] = r;
    if (count) count[off] = cnt;
}

// the resamples [b_lo, b_hi) of one tile column, a wave (or half-wave) per resample
template <int SUBS, bool L1, class Column>
__device__ __forceinline__ void rs_range(const RsGeom &G, const Column &c, bool active, int64_t ooff, int wave, int waves, int sub,
                                         int64_t b_lo, int64_t b_hi, const int32_t *__restrict__ starts, float *__restrict__ out,
                                         int32_t *__restrict__ count) {
    for (int64_t b0 = b_lo + (int64_t)wave * SUBS; b0 < b_hi; b0 += (int64_t)waves * SUBS) {
        const int64_t b1 = b0 + 1 < b_hi ? b0 + 1 : b0;         // (the idle half-wave of an odd range reads its neighbour's starts)
        const int64_t b = b0 + sub;
        if (!active) continue;
        double tot;
        int32_t cnt;
        rs_lane<SUBS, L1>(G, c, starts + b0 * G.nb, starts + b1 * G.nb, sub, tot, cnt);
        if (b < b_hi) rs_store(G, tot, cnt, out, count, b * G.A.out_row_stride + ooff);
    }
}

template <int ROWS, int W, bool VEC, bool L1>
__global__ void __launch_bounds__(RS_STAGED_THREADS) resample_staged_kernel(RsGeom G, const float *__restrict__ src,
                                                                            const int32_t *__restrict__ starts,
                                                                            float *__restrict__ out, int32_t *__restrict__ count) {
    constexpr int V = VEC ? 4 : 1;
    constexpr int SUBS = 64 / W;
    constexpr int CH = W / V;                                   // chunks of a tile row
    constexpr int RPP = RS_STAGED_THREADS / CH;                 // rows staged per pass of the workgroup
    __shared__ __align__(16) float s_tile[ROWS * W];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sub = lane / W, c = lane % W;
    const int sc = threadIdx.x % CH, sr = threadIdx.x / CH;     // this thread's chunk and first row while staging
    const int32_t T = G.T < ROWS ? G.T : ROWS;                  // (the plan chose the class: T <= ROWS)
    int64_t staged = -1;
    bool active = false;
    int64_t ooff = 0;
    for (int64_t item = blockIdx.x; item < G.items; item += G.A.nblk) {
        const int64_t ct = item / G.splits, sp = item - ct * G.splits;
        if (ct != staged) {                                     // uniform over the workgroup
            __syncthreads();                                    // the last tile's readers are done
            const int64_t q = ct * CH + sc;
            if (q < G.A.ncol) {
                int64_t soff, o;
                rows_offsets<V, false>(G.A, q, soff, o);
                const float *p = src + soff;
                for (int32_t r = sr; r < T; r += RPP * RS_STAGE_UNROLL) {
                    float x[RS_STAGE_UNROLL][V];
#pragma unroll
                    for (int u = 0; u < RS_STAGE_UNROLL; ++u)
                        if (r + u * RPP < T) load_chunk<V>(p + (int64_t)(r + u * RPP) * G.A.src_row_stride, x[u]);
#pragma unroll
                    for (int u = 0; u < RS_STAGE_UNROLL; ++u)
                        if (r + u * RPP < T) {
                            float *d = s_tile + (r + u * RPP) * W + sc * V;
                            if constexpr (V == 4) *reinterpret_cast<float4 *>(d) = make_float4(x[u][0], x[u][1], x[u][2], x[u][3]);
                            else d[0] = x[u][0];
                        }
                }
            }
            __syncthreads();
            staged = ct;
            const int64_t e = ct * W + c;
            active = e < G.inner;
            if (active) {
                int64_t soff;
                rs_element_offsets<V>(G, e, soff, ooff);
            }
        }
        const int64_t b_lo = sp * G.per;
        const int64_t b_hi = b_lo + G.per < G.B ? b_lo + G.per : G.B;
        const RsLdsColumn col = {s_tile + c, W};
        rs_range<SUBS, L1>(G, col, active, ooff, wave, RS_STAGED_THREADS / 64, sub, b_lo, b_hi, starts, out, count);
    }
}

template <bool L1>
__global__ void __launch_bounds__(RS_DIRECT_THREADS) resample_direct_kernel(RsGeom G, const float *__restrict__ src,
                                                                            const int32_t *__restrict__ starts,
                                                                            float *__restrict__ out, int32_t *__restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t item = blockIdx.x; item < G.items; item += G.A.nblk) {
        const int64_t ct = item / G.splits, sp = item - ct * G.splits;
        const int64_t e = ct * RS_DIRECT_W + lane;
        const bool active = e < G.inner;
        int64_t soff = 0, ooff = 0;
        if (active) rs_element_offsets<1>(G, e, soff, ooff);
        const int64_t b_lo = sp * G.per;
        const int64_t b_hi = b_lo + G.per < G.B ? b_lo + G.per : G.B;
        const RsMemColumn col = {src + soff, G.A.src_row_stride};
        rs_range<1, L1>(G, col, active, ooff, wave, RS_DIRECT_THREADS / 64, 0, b_lo, b_hi, starts, out, count);
    }
}

struct RsPlan {
    RsGeom G;
    int form;                                           // DLWPCS_RESAMPLE_STAGED / _DIRECT
    int cls;                                            // index into RS_CLASSES (staged)
    bool vec;
    int w;
    int64_t tiles;                                      // column tiles
};

int rs_plan(const dlwpcs_rows_desc *d, const void *src, const void *out, int64_t n_rows, int64_t n_resamples, int64_t n_blocks,
            int64_t block_length, int64_t n_draw, int mode, int min_count, int form, int64_t splits, RsPlan &P) {
    RsGeom &G = P.G;
    memset(&G, 0, sizeof(G));
    int rc = rows_addr_init(d, "row_resample", G.A, G.inner);
    if (rc != DLWPCS_OK) return rc;
    if (n_resamples < 0 || n_rows < 0) return fail(DLWPCS_E_INVALID, "row_resample: negative resample / row count");
    if (form < DLWPCS_RESAMPLE_CHOOSE || form > DLWPCS_RESAMPLE_DIRECT) return fail(DLWPCS_E_INVALID, "row_resample: form %d", form);
    if (mode != DLWPCS_RESAMPLE_SKIP && mode != DLWPCS_RESAMPLE_PROPAGATE) return fail(DLWPCS_E_INVALID, "row_resample: mode %d", mode);
    if (splits < 0) return fail(DLWPCS_E_INVALID, "row_resample: %lld resample ranges", (long long)splits);
    P.form = form == DLWPCS_RESAMPLE_DIRECT ? DLWPCS_RESAMPLE_DIRECT : DLWPCS_RESAMPLE_STAGED;
    P.cls = 0;
    P.vec = false;
    P.w = RS_CLASSES[0].w;
    P.tiles = 0;
    if (n_resamples == 0 || G.inner == 0) return DLWPCS_OK;
    if (n_rows < 1 || block_length < 1 || block_length > n_rows)
        return fail(DLWPCS_E_INVALID, "row_resample: block length %lld of %lld rows (1 .. rows)", (long long)block_length, (long long)n_rows);
    if (n_draw < 1 || n_blocks != (n_draw + block_length - 1) / block_length)
        return fail(DLWPCS_E_INVALID, "row_resample: %lld blocks of %lld rows for %lld draws", (long long)n_blocks, (long long)block_length,
                    (long long)n_draw);
    if (n_rows > DLWPCS_RESAMPLE_MAX_ROWS || n_draw > DLWPCS_RESAMPLE_MAX_ROWS || n_resamples > DLWPCS_RESAMPLE_MAX_ROWS)
        return fail(DLWPCS_E_UNSUPPORTED, "row_resample: %lld rows, %lld draws, %lld resamples (each at most 2^31 - 1)", (long long)n_rows,
                    (long long)n_draw, (long long)n_resamples);
    if ((((uintptr_t)src) | ((uintptr_t)out)) & 3) return fail(DLWPCS_E_INVALID, "row_resample: an operand is not aligned to its 4-byte elements");
    if (form == DLWPCS_RESAMPLE_STAGED && n_rows > RS_CAP)
        return fail(DLWPCS_E_UNSUPPORTED, "row_resample: the staged form holds at most %d rows, got %lld", RS_CAP, (long long)n_rows);
    if (form == DLWPCS_RESAMPLE_CHOOSE && n_rows > RS_CAP) P.form = DLWPCS_RESAMPLE_DIRECT;
    G.T = (int32_t)n_rows;
    G.L = (int32_t)block_length;
    G.nb = n_blocks;
    G.last_len = (int32_t)(n_draw - (n_blocks - 1) * block_length);
    G.need = mode == DLWPCS_RESAMPLE_SKIP ? (min_count > 1 ? min_count : 1) : (int32_t)n_draw;
    G.B = n_resamples;
    int64_t slots, min_range;
    if (P.form == DLWPCS_RESAMPLE_STAGED) {
        P.cls = n_rows <= RS_CLASSES[0].rows ? 0 : 1;
        bool ovec;
        rows_vector_ok(d, P.vec, ovec);
        if (P.vec && !aligned16(src)) P.vec = false;
        P.w = RS_CLASSES[P.cls].w;
        slots = RS_CUS;
        min_range = RS_STAGED_MIN_RANGE;
    } else {
        P.w = RS_DIRECT_W;
        slots = RS_DIRECT_SLOTS;
        min_range = RS_DIRECT_MIN_RANGE;
    }
    if (P.vec) G.A.ext[G.A.n_inner - 1] /= 4;
    G.A.ncol = G.inner / (P.vec ? 4 : 1);
    P.tiles = (G.inner + P.w - 1) / P.w;
    G.A.tiles = P.tiles;
    // Resample ranges: only with fewer column tiles than workgroup slots, and no range shorter than min_range resamples, since
    // every range of the staged form stages its tile again.
    int64_t sp = splits;
    if (sp == 0) {
        sp = 1;
        if (P.tiles < slots) {
            sp = (slots + P.tiles - 1) / P.tiles;
            const int64_t most = n_resamples / min_range;
            if (sp > most) sp = most;
            if (sp < 1) sp = 1;
        }
    }
    if (sp > n_resamples) sp = n_resamples;
    G.per = (n_resamples + sp - 1) / sp;
    G.splits = (n_resamples + G.per - 1) / G.per;               // no empty range
    if (P.tiles > MAX_BLOCKS / G.splits) return fail(DLWPCS_E_UNSUPPORTED, "row_resample: %lld x %lld work items is too many",
                                                      (long long)P.tiles, (long long)G.splits);
    G.items = P.tiles * G.splits;
    G.A.nblk = G.items < slots ? G.items : slots;
    return DLWPCS_OK;
}

template <int ROWS, int W>
void rs_launch_staged(const RsPlan &P, const float *src, const int32_t *starts, float *out, int32_t *count, hipStream_t s) {
    const dim3 grid((unsigned)P.G.A.nblk), blk(RS_STAGED_THREADS);      // (at most RS_CUS workgroups: one grid dimension)
    const bool l1 = P.G.L == 1;
    if (P.vec && l1) hipLaunchKernelGGL((resample_staged_kernel<ROWS, W, true, true>), grid, blk, 0, s, P.G, src, starts, out, count);
    else if (P.vec) hipLaunchKernelGGL((resample_staged_kernel<ROWS, W, true, false>), grid, blk, 0, s, P.G, src, starts, out, count);
    else if (l1) hipLaunchKernelGGL((resample_staged_kernel<ROWS, W, false, true>), grid, blk, 0, s, P.G, src, starts, out, count);
    else hipLaunchKernelGGL((resample_staged_kernel<ROWS, W, false, false>), grid, blk, 0, s, P.G, src, starts, out, count);
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" int dlwpcs_row_resample(const dlwpcs_rows_desc *d, const float *src, const int32_t *starts, int64_t n_rows,
                                   int64_t n_resamples, int64_t n_blocks, int64_t block_length, int64_t n_draw, int mode,
                                   int min_count, int form, int64_t splits, float *out, int32_t *count, dlwpcs_stream_t stream) {
    RsPlan P;
    int rc = rs_plan(d, src, out, n_rows, n_resamples, n_blocks, block_length, n_draw, mode, min_count, form, splits, P);
    if (rc != DLWPCS_OK) return rc;
    if (n_resamples == 0 || P.G.inner == 0) return DLWPCS_OK;
    if (!src || !starts || !out) return fail(DLWPCS_E_INVALID, "row_resample: null operand");
    if ((((uintptr_t)starts) | ((uintptr_t)count)) & 3) return fail(DLWPCS_E_INVALID, "row_resample: an operand is not aligned to its 4-byte elements");
    hipStream_t s = (hipStream_t)stream;
    if (P.form == DLWPCS_RESAMPLE_STAGED) {
        if (P.cls == 0) rs_launch_staged<RS_CLASSES[0].rows, RS_CLASSES[0].w>(P, src, starts, out, count, s);
        else rs_launch_staged<RS_CLASSES[1].rows, RS_CLASSES[1].w>(P, src, starts, out, count, s);
    } else {
        const dim3 grid((unsigned)P.G.A.nblk), blk(RS_DIRECT_THREADS);      // (at most RS_DIRECT_SLOTS workgroups)
        if (P.G.L == 1) hipLaunchKernelGGL((resample_direct_kernel<true>), grid, blk, 0, s, P.G, src, starts, out, count);
        else hipLaunchKernelGGL((resample_direct_kernel<false>), grid, blk, 0, s, P.G, src, starts, out, count);
    }
    return check_launch("row_resample");
}

extern "C" int dlwpcs_row_resample_plan_info(const dlwpcs_rows_desc *d, const void *src, int64_t n_rows, int64_t n_resamples,
                                             int64_t n_blocks, int64_t block_length, int64_t n_draw, int form, int64_t splits,
                                             int64_t info[8]) {
    if (!info) return fail(DLWPCS_E_INVALID, "row_resample_plan_info: null info");
    RsPlan P;
    int rc = rs_plan(d, src, nullptr, n_rows, n_resamples, n_blocks, block_length, n_draw, DLWPCS_RESAMPLE_SKIP, 1, form, splits, P);
    if (rc != DLWPCS_OK) return rc;
    const bool any = n_resamples > 0 && P.G.inner > 0;
    if (any && !src) return fail(DLWPCS_E_INVALID, "row_resample: null operand");
    const bool staged = P.form == DLWPCS_RESAMPLE_STAGED;
    info[0] = P.form;
    info[1] = P.w;
    info[2] = RS_CAP;
    info[3] = any ? P.G.A.nblk : 0;
    info[4] = staged ? (int64_t)RS_CLASSES[P.cls].rows * RS_CLASSES[P.cls].w * 4 : 0;
    info[5] = 0;                                            // the block-sum table: not built
    info[6] = P.vec ? 4 : 1;
    info[7] = any ? P.G.splits : 0;
    return DLWPCS_OK;
}
