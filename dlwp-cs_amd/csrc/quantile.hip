// Grouped quantiles along the row axis (dlwpcs_group_quantile): the row set and the CSR of dlwpcs_group_mean, per (group, element)
// the 'linear' quantiles of the members that are not NaN.  One lane owns one (group, element) column and does everything for it:
// nothing crosses lanes, no barrier, no scratch, no atomics, one launch.
//
// Keys.  A value goes to its order-preserving 32-bit key (sign bit flipped for non-negative values, all bits flipped for negative
// ones; -0 first becomes +0), so that unsigned integer order is the order of the values, +-inf included.  Every NaN goes to the
// one key no value has (0xffffffff), which no pass counts: a column read from memory needs no branch around its NaN entries.
//
// Selection.  The order statistic j of a column is found bit by bit from bit 31 down: with the bits above already fixed in a
// prefix, count the keys that agree with the prefix there and have a 0 at this bit; if j is below the count the bit is 0, else it
// is 1 and j drops by the count.  32 passes over the column, each shared by all n_probs order statistics (one prefix and one
// counter per probability, indexed at compile time: classes of 1, 2, 4, 8, 16).  One more pass gives x_(j+1): it is x_(j) when
// more than j + 1 keys are <= it, else the smallest key above it.  No sort, no per-lane arrays, exact.
//
// Staged form: the column lies in LDS, compacted per lane at [slot][lane] (a lane's bank is its lane number whatever slot it is at:
// no conflicts, the layout of ensemble.hip); the group's rows are read from memory once.  Long form: the same passes read the rows
// from memory each time (34 reads of the group); for a once-per-dataset computation over groups no workgroup's LDS holds.
//
// No profiler tags: the launch profiler's registry is the convolution family's (tests/test_conv_coverage_tags.py closes it over the
// convolution case table), as for the other verification kernels.
#include <math.h>
#include "strided.h"

namespace dlwpcs {

namespace {

constexpr int QT_MAXP = DLWPCS_QUANTILE_MAX_PROBS;
constexpr int QT_LONG_THREADS = 256;
constexpr int QT_UNROLL = 4;                        // rows in flight per lane

struct QtClass { int rows, lanes; };
constexpr int QT_NCLASS = 4;
constexpr QtClass QT_CLASSES[QT_NCLASS] = {{64, 256}, {128, 128}, {256, 64}, {640, 64}};

struct QtGeom {
    RowsAddr A;                                     // chunks of one element
    int32_t n_probs;
    int64_t out_prob_stride;
    double p[QT_MAXP];                              // unused slots: 0
};

// element q of a row -> offsets in the source and in the output; every extent fits 31 bits when ncol does: 32-bit index arithmetic
__device__ __forceinline__ void qt_offsets(const QtGeom &G, int64_t q, int64_t &soff, int64_t &ooff) {
    if (G.A.ncol < (1ll << 31)) rows_offsets<1, true>(G.A, q, soff, ooff);
    else rows_offsets<1, false>(G.A, q, soff, ooff);
}

// Every NaN goes to QT_NO_KEY, the key of no value (it would be that of the NaN 0x7fffffff): it sorts behind every member, is
// never counted by a selection pass (it has no 0 bit) and is never selected (an order statistic lies among the n members), so a
// column read from memory needs no branch around its NaN entries.
constexpr uint32_t QT_NO_KEY = 0xffffffffu;
__device__ __forceinline__ uint32_t qt_key(uint32_t u) {
    if (u == 0x80000000u) u = 0u;
    const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return (u & 0x7fffffffu) > 0x7f800000u ? QT_NO_KEY : k;
}
__device__ __forceinline__ float qt_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// a column in LDS: n keys, all members
template <int LANES>
struct QtLdsColumn {
    static constexpr int UNROLL = 8;                // LDS reads in flight per lane
    const uint32_t *col;
    int32_t n;
    __device__ __forceinline__ int32_t size() const { return n; }
    __device__ __forceinline__ uint32_t get(int32_t i) const { return col[i * LANES]; }
};

// a column in memory: the group's rows at this element, NaN entries come as QT_NO_KEY
struct QtMemColumn {
    static constexpr int UNROLL = 16;               // rows in flight per lane: one lane per column, the loads must cover the latency
    const float *p;
    const int32_t *rows;
    int64_t rs;
    int32_t len;
    __device__ __forceinline__ int32_t size() const { return len; }
    __device__ __forceinline__ uint32_t get(int32_t i) const { return qt_key(__float_as_uint(p[(int64_t)rows[i] * rs])); }
};

// the n_probs quantiles of a column of n members, stored at out[q * out_prob_stride + off]
template <int NP, class Column>
__device__ __forceinline__ void qt_select(const QtGeom &G, const Column &c, int32_t n, float *__restrict__ out,
                                          int32_t *__restrict__ count, int64_t off) {
#pragma clang fp contract(off)
    if (count) count[off] = n;
    if (n == 0) {
        for (int q = 0; q < G.n_probs; ++q) out[q * G.out_prob_stride + off] = quiet_nan();
        return;
    }
    const int32_t len = c.size();
    const double nm1 = (double)(n - 1);
    uint32_t prefix[NP];
    int32_t rank[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        prefix[q] = 0u;
        rank[q] = (int32_t)floor(nm1 * G.p[q]);
    }
    for (int bit = 31; bit >= 0; --bit) {
        // a key counts when it agrees with the prefix above this bit and has a 0 here: the prefix has a 0 here too, so that is
        // one shift per key and one compare per probability
        int32_t cnt[NP];
        uint32_t pre[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) { cnt[q] = 0; pre[q] = prefix[q] >> bit; }
#pragma unroll Column::UNROLL
        for (int32_t i = 0; i < len; ++i) {
            const uint32_t ks = c.get(i) >> bit;
#pragma unroll
            for (int q = 0; q < NP; ++q) cnt[q] += ks == pre[q] ? 1 : 0;
        }
#pragma unroll
        for (int q = 0; q < NP; ++q)
            if (rank[q] >= cnt[q]) {
                rank[q] -= cnt[q];
                prefix[q] |= 1u << bit;
            }
    }
    // prefix[q] is the key of x_(j); x_(j+1) from the keys at or below it and the smallest above it
    int32_t cle[NP];
    uint32_t nxt[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) { cle[q] = 0; nxt[q] = 0xffffffffu; }
#pragma unroll Column::UNROLL
    for (int32_t i = 0; i < len; ++i) {
        const uint32_t k = c.get(i);
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const bool le = k <= prefix[q];
            cle[q] += le ? 1 : 0;
            nxt[q] = (!le && k < nxt[q]) ? k : nxt[q];
        }
    }
#pragma unroll
    for (int q = 0; q < NP; ++q)
        if (q < G.n_probs) {
            const double h = nm1 * G.p[q];
            const double j = floor(h);
            const double g = h - j;
            const double xj = (double)qt_value(prefix[q]);
            double v = xj;
            if (g != 0.0) {
                const double xj1 = cle[q] > (int32_t)j + 1 ? xj : (double)qt_value(nxt[q]);
                v = xj + g * (xj1 - xj);
            }
            const float r = (float)v;
            out[q * G.out_prob_stride + off] = r != r ? quiet_nan() : r;
        }
}

template <int ROWS, int LANES, int NP>
__global__ void __launch_bounds__(LANES) quantile_staged_kernel(QtGeom G, const float *__restrict__ src,
                                                                const int32_t *__restrict__ group_start,
                                                                const int32_t *__restrict__ row_index, float *__restrict__ out,
                                                                int32_t *__restrict__ count) {
    __shared__ uint32_t s_keys[ROWS * LANES];
    const int64_t bid = flat_block();
    if (bid >= G.A.nblk) return;
    const int64_t k = bid / G.A.tiles;
    const int64_t e = (bid - k * G.A.tiles) * LANES + threadIdx.x;
    if (e >= G.A.ncol) return;                            // (no barrier anywhere: a column belongs to its lane)
    const int32_t g0 = group_start[k];
    int32_t g1 = group_start[k + 1];
    if (g1 - g0 > ROWS) g1 = g0 + ROWS;                 // (max_group_rows chose the class: rows beyond it are not read)
    int64_t soff, ooff;
    qt_offsets(G, e, soff, ooff);
    const float *p = src + soff;
    uint32_t *col = s_keys + threadIdx.x;               // member i of this lane: col[i * LANES]
    int32_t n = 0;
    for (int32_t j = g0; j < g1; j += QT_UNROLL) {
        uint32_t u[QT_UNROLL];
#pragma unroll
        for (int t = 0; t < QT_UNROLL; ++t)
            u[t] = j + t < g1 ? __float_as_uint(p[(int64_t)row_index[j + t] * G.A.src_row_stride]) : 0x7fc00000u;
#pragma unroll
        for (int t = 0; t < QT_UNROLL; ++t) {
            const uint32_t key = qt_key(u[t]);
            if (key != QT_NO_KEY) {
                col[n * LANES] = key;
                ++n;
            }
        }
    }
    const QtLdsColumn<LANES> c = {col, n};
    qt_select<NP>(G, c, n, out, count, k * G.A.out_row_stride + ooff);
}

template <int NP>
__global__ void __launch_bounds__(QT_LONG_THREADS) quantile_long_kernel(QtGeom G, const float *__restrict__ src,
                                                                        const int32_t *__restrict__ group_start,
                                                                        const int32_t *__restrict__ row_index,
                                                                        float *__restrict__ out, int32_t *__restrict__ count) {
    const int64_t bid = flat_block();
    if (bid >= G.A.nblk) return;
    const int64_t k = bid / G.A.tiles;
    const int64_t e = (bid - k * G.A.tiles) * QT_LONG_THREADS + threadIdx.x;
    if (e >= G.A.ncol) return;
    const int32_t g0 = group_start[k], g1 = group_start[k + 1];
    int64_t soff, ooff;
    qt_offsets(G, e, soff, ooff);
    const QtMemColumn c = {src + soff, row_index + g0, G.A.src_row_stride, g1 - g0};
    int32_t n = 0;
#pragma unroll QtMemColumn::UNROLL
    for (int32_t i = 0; i < c.len; ++i) n += c.get(i) != QT_NO_KEY ? 1 : 0;
    qt_select<NP>(G, c, n, out, count, k * G.A.out_row_stride + ooff);
}

struct QtPlan {
    QtGeom G;
    int cls;                                            // index into QT_CLASSES, QT_NCLASS: the long form
    int np_class;
    int lanes;
    int64_t inner;
};

int qt_plan(const dlwpcs_rows_desc *d, int n_groups, int64_t max_group_rows, int n_probs, QtPlan &P) {
    QtGeom &G = P.G;
    memset(&G, 0, sizeof(G));
    const int rc = rows_addr_init(d, "group_quantile", G.A, P.inner);
    if (rc != DLWPCS_OK) return rc;
    if (n_groups < 0 || max_group_rows < 0) return fail(DLWPCS_E_INVALID, "group_quantile: negative group / row count");
    if (n_probs < 1 || n_probs > QT_MAXP)
        return fail(DLWPCS_E_INVALID, "group_quantile: %d probabilities (1 .. %d)", n_probs, QT_MAXP);
    if (max_group_rows >= (1ll << 31)) return fail(DLWPCS_E_INVALID, "group_quantile: a group of %lld rows", (long long)max_group_rows);
    G.n_probs = n_probs;
    P.cls = QT_NCLASS;
    for (int c = QT_NCLASS - 1; c >= 0; --c)
        if (max_group_rows <= QT_CLASSES[c].rows) P.cls = c;
    P.np_class = n_probs <= 1 ? 1 : n_probs <= 2 ? 2 : n_probs <= 4 ? 4 : n_probs <= 8 ? 8 : 16;
    P.lanes = P.cls < QT_NCLASS ? QT_CLASSES[P.cls].lanes : QT_LONG_THREADS;
    G.A.ncol = P.inner;
    G.A.tiles = (G.A.ncol + P.lanes - 1) / P.lanes;
    G.A.nblk = (int64_t)n_groups * G.A.tiles;
    if (G.A.nblk > MAX_BLOCKS) return fail(DLWPCS_E_INVALID, "group_quantile: %lld workgroups is too many", (long long)G.A.nblk);
    return DLWPCS_OK;
}

template <int NP>
void qt_launch(const QtPlan &P, const float *src, const int32_t *gs, const int32_t *ri, float *out, int32_t *count, hipStream_t s) {
    const dim3 grid = launch_grid(P.G.A.nblk);
    switch (P.cls) {
    case 0: hipLaunchKernelGGL((quantile_staged_kernel<64, 256, NP>), grid, dim3(256), 0, s, P.G, src, gs, ri, out, count); break;
    case 1: hipLaunchKernelGGL((quantile_staged_kernel<128, 128, NP>), grid, dim3(128), 0, s, P.G, src, gs, ri, out, count); break;
    case 2: hipLaunchKernelGGL((quantile_staged_kernel<256, 64, NP>), grid, dim3(64), 0, s, P.G, src, gs, ri, out, count); break;
    case 3: hipLaunchKernelGGL((quantile_staged_kernel<640, 64, NP>), grid, dim3(64), 0, s, P.G, src, gs, ri, out, count); break;
    default: hipLaunchKernelGGL((quantile_long_kernel<NP>), grid, dim3(QT_LONG_THREADS), 0, s, P.G, src, gs, ri, out, count); break;
    }
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" int dlwpcs_group_quantile(const dlwpcs_rows_desc *d, const float *src, const int32_t *group_start, const int32_t *row_index,
                                     int n_groups, int64_t max_group_rows, const double *probs, int n_probs, float *out,
                                     int64_t out_prob_stride, int32_t *count, dlwpcs_stream_t stream) {
    QtPlan P;
    int rc = qt_plan(d, n_groups, max_group_rows, n_probs, P);
    if (rc != DLWPCS_OK) return rc;
    if (!probs) return fail(DLWPCS_E_INVALID, "group_quantile: null probabilities");
    for (int q = 0; q < n_probs; ++q) {
        if (!(probs[q] >= 0.0 && probs[q] <= 1.0))
            return fail(DLWPCS_E_INVALID, "group_quantile: probability %d is %g, outside [0, 1]", q, probs[q]);
        P.G.p[q] = probs[q];
    }
    if (n_groups == 0 || P.inner == 0) return DLWPCS_OK;
    if (!src || !group_start || !row_index || !out) return fail(DLWPCS_E_INVALID, "group_quantile: null operand");
    if ((((uintptr_t)src) | ((uintptr_t)out) | ((uintptr_t)count)) & 3)
        return fail(DLWPCS_E_INVALID, "group_quantile: an operand is not aligned to its 4-byte elements");
    P.G.out_prob_stride = out_prob_stride;
    hipStream_t s = (hipStream_t)stream;
    switch (P.np_class) {
    case 1: qt_launch<1>(P, src, group_start, row_index, out, count, s); break;
    case 2: qt_launch<2>(P, src, group_start, row_index, out, count, s); break;
    case 4: qt_launch<4>(P, src, group_start, row_index, out, count, s); break;
    case 8: qt_launch<8>(P, src, group_start, row_index, out, count, s); break;
    default: qt_launch<16>(P, src, group_start, row_index, out, count, s); break;
    }
    return check_launch("group_quantile");
}

extern "C" int dlwpcs_group_quantile_plan_info(const dlwpcs_rows_desc *d, const void *src, int n_groups, int64_t max_group_rows,
                                               int n_probs, int32_t info[8]) {
    if (!info) return fail(DLWPCS_E_INVALID, "group_quantile_plan_info: null info");
    QtPlan P;
    int rc = qt_plan(d, n_groups, max_group_rows, n_probs, P);
    if (rc != DLWPCS_OK) return rc;
    if (n_groups > 0 && P.inner > 0 && !src) return fail(DLWPCS_E_INVALID, "group_quantile: null operand");
    const bool staged = P.cls < QT_NCLASS;
    const dim3 grid = launch_grid(P.inner > 0 ? P.G.A.nblk : 0);
    info[0] = staged ? 0 : 1;
    info[1] = staged ? QT_CLASSES[P.cls].rows : 0;
    info[2] = P.lanes;
    info[3] = P.np_class;
    info[4] = (int32_t)grid.x;
    info[5] = (int32_t)grid.y;
    info[6] = staged ? QT_CLASSES[P.cls].rows * QT_CLASSES[P.cls].lanes * 4 : 0;
    info[7] = 0;
    return DLWPCS_OK;
}
