// Climatologies (reference DLWP/verify.py:167-214, 426-456): a grouped per-element mean over the rows of an fp32 array, and an
// indexed row gather.  Both address a row through dlwpcs_rows_desc: every inner dim has a stride in the source and in the
// output, lanes run along the last dim.
//
// group_mean_kernel: grid = (group [x slab]) x column tiles, 256 threads; a lane owns one chunk of a row (a float4 on the vector
// path, one element otherwise) and walks the rows of its group in CSR order, so neighbouring lanes read neighbouring addresses of
// the same row and the row index is one scalar load per row.  fp64 sums.  The ORDER is a property of the group, not of the grid:
// rows are cut into slabs of GM_SLAB rows, a slab is summed row by row from zero and the slab sums are added in slab order.
// One launch: the lane loops over the slabs itself.  Two launches (few groups, many rows): launch 1 gives every (group, slab)
// its own workgroups and stores the slab sums, group_finish_kernel adds them -- the same additions in the same order, so the
// two forms give the same bits.  No atomics.
#include <string.h>
#include "strided.h"

namespace dlwpcs {

namespace {

constexpr int GM_THREADS = 256;
constexpr int GM_UNROLL = 4;                    // rows in flight per lane
constexpr int GM_SLAB = DLWPCS_GROUP_SLAB_ROWS;
constexpr int64_t GM_TARGET_BLOCKS = 512;       // 256 CUs x 2: measured, 648 workgroups in one launch already stream at the HBM rate

struct RowsGeom {
    RowsAddr A;
    int32_t out_vec;
    int64_t slabs;                              // slabs per group of the split form
};

// rows [j0, j1) of the CSR added to s / n row by row
template <int V>
__device__ __forceinline__ void slab_sum(const float *__restrict__ src, const int32_t *__restrict__ row_index, int64_t rs,
                                         int64_t j0, int64_t j1, double s[V], int32_t n[V]) {
    for (int64_t j = j0; j < j1; j += GM_UNROLL) {
        float x[GM_UNROLL][V];
#pragma unroll
        for (int u = 0; u < GM_UNROLL; ++u)
            if (j + u < j1) load_chunk<V>(src + (int64_t)row_index[j + u] * rs, x[u]);
#pragma unroll
        for (int u = 0; u < GM_UNROLL; ++u)
            if (j + u < j1) {
#pragma unroll
                for (int v = 0; v < V; ++v)
                    if (!isnan(x[u][v])) { s[v] += (double)x[u][v]; ++n[v]; }
            }
    }
}

template <int V>
__device__ __forceinline__ void finish(const RowsGeom &G, const double tot[V], const int32_t cnt[V], float *__restrict__ out,
                                       int32_t *__restrict__ count, int64_t off) {
    const float nan = quiet_nan();
    float r[V];
#pragma unroll
    for (int v = 0; v < V; ++v) r[v] = cnt[v] ? (float)(tot[v] / (double)cnt[v]) : nan;
    const int64_t st = G.A.last_out_stride();
    store_chunk<V>(out + off, r, G.out_vec != 0, st);
    if (count) {
#pragma unroll
        for (int v = 0; v < V; ++v) count[off + v * st] = cnt[v];
    }
}

template <bool VEC, bool SPLIT>
__global__ void __launch_bounds__(GM_THREADS) group_mean_kernel(RowsGeom G, const float *__restrict__ src,
                                                               const int32_t *__restrict__ group_start,
                                                               const int32_t *__restrict__ row_index, double *__restrict__ psum,
                                                               int32_t *__restrict__ pcnt, float *__restrict__ out,
                                                               int32_t *__restrict__ count) {
    constexpr int V = VEC ? 4 : 1;
    const int64_t bid = flat_block();
    if (bid >= G.A.nblk) return;
    const int64_t unit = bid / G.A.tiles;
    const int64_t q = (bid - unit * G.A.tiles) * GM_THREADS + threadIdx.x;
    if (q >= G.A.ncol) return;
    const int64_t k = SPLIT ? unit / G.slabs : unit;
    const int64_t g0 = group_start[k], g1 = group_start[k + 1];
    int64_t soff, ooff;
    rows_offsets<V, false>(G.A, q, soff, ooff);
    const float *p = src + soff;
    if constexpr (SPLIT) {
        const int64_t slab = unit - k * G.slabs;
        const int64_t j0 = g0 + slab * GM_SLAB;
        if (j0 >= g1) return;                               // launch 2 reads the slabs of the group's own rows only
        double s[V];
        int32_t n[V];
#pragma unroll
        for (int v = 0; v < V; ++v) { s[v] = 0.0; n[v] = 0; }
        slab_sum<V>(p, row_index, G.A.src_row_stride, j0, j0 + GM_SLAB < g1 ? j0 + GM_SLAB : g1, s, n);
        const int64_t at = (unit * G.A.ncol + q) * V;
#pragma unroll
        for (int v = 0; v < V; ++v) { psum[at + v] = s[v]; pcnt[at + v] = n[v]; }
    } else {
        double tot[V];
        int32_t cnt[V];
#pragma unroll
        for (int v = 0; v < V; ++v) { tot[v] = 0.0; cnt[v] = 0; }
        for (int64_t j0 = g0; j0 < g1; j0 += GM_SLAB) {
            double s[V];
#pragma unroll
            for (int v = 0; v < V; ++v) s[v] = 0.0;
            slab_sum<V>(p, row_index, G.A.src_row_stride, j0, j0 + GM_SLAB < g1 ? j0 + GM_SLAB : g1, s, cnt);
#pragma unroll
            for (int v = 0; v < V; ++v) tot[v] += s[v];
        }
        finish<V>(G, tot, cnt, out, count, k * G.A.out_row_stride + ooff);
    }
}

template <bool VEC>
__global__ void __launch_bounds__(GM_THREADS) group_finish_kernel(RowsGeom G, const int32_t *__restrict__ group_start,
                                                                 const double *__restrict__ psum,
                                                                 const int32_t *__restrict__ pcnt, float *__restrict__ out,
                                                                 int32_t *__restrict__ count) {
    constexpr int V = VEC ? 4 : 1;
    const int64_t bid = flat_block();
    if (bid >= G.A.nblk) return;
    const int64_t k = bid / G.A.tiles;
    const int64_t q = (bid - k * G.A.tiles) * GM_THREADS + threadIdx.x;
    if (q >= G.A.ncol) return;
    const int64_t rows = (int64_t)group_start[k + 1] - group_start[k];
    const int64_t nslab = (rows + GM_SLAB - 1) / GM_SLAB;
    int64_t soff, ooff;
    rows_offsets<V, false>(G.A, q, soff, ooff);
    double tot[V];
    int32_t cnt[V];
#pragma unroll
    for (int v = 0; v < V; ++v) { tot[v] = 0.0; cnt[v] = 0; }
    for (int64_t s = 0; s < nslab; ++s) {
        const int64_t at = ((k * G.slabs + s) * G.A.ncol + q) * V;
#pragma unroll
        for (int v = 0; v < V; ++v) { tot[v] += psum[at + v]; cnt[v] += pcnt[at + v]; }
    }
    finish<V>(G, tot, cnt, out, count, k * G.A.out_row_stride + ooff);
}

template <bool VEC>
__global__ void __launch_bounds__(GM_THREADS) rows_gather_kernel(RowsGeom G, const float *__restrict__ src,
                                                                const int32_t *__restrict__ index, float *__restrict__ out) {
    constexpr int V = VEC ? 4 : 1;
    const int64_t bid = flat_block();
    if (bid >= G.A.nblk) return;
    const int64_t i = bid / G.A.tiles;
    const int64_t q = (bid - i * G.A.tiles) * GM_THREADS + threadIdx.x;
    if (q >= G.A.ncol) return;
    int64_t soff, ooff;
    rows_offsets<V, false>(G.A, q, soff, ooff);
    const int32_t r = index[i];
    float x[V];
    if (r >= 0) {
        load_chunk<V>(src + (int64_t)r * G.A.src_row_stride + soff, x);
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v) x[v] = quiet_nan();
    }
    store_chunk<V>(out + i * G.A.out_row_stride + ooff, x, G.out_vec != 0, G.A.last_out_stride());
}

struct RowsPlan {
    RowsGeom G;
    bool vec;
    int64_t inner;                                          // elements per row
};

int make_rows_plan(const dlwpcs_rows_desc *d, const char *what, RowsPlan &P) {
    RowsGeom &G = P.G;
    memset(&G, 0, sizeof(G));
    const int rc = rows_addr_init(d, what, G.A, P.inner);
    if (rc != DLWPCS_OK) return rc;
    // vector path: 16-byte loads along the last dim; every other offset keeps a row chunk on 16 bytes
    bool ovec;
    rows_vector_ok(d, P.vec, ovec);
    G.out_vec = ovec;
    return DLWPCS_OK;
}

// after the pointers are known: settle the load width, then the chunk counts
void settle(RowsPlan &P, const void *src, const void *out) {
    if (P.vec && !aligned16(src)) P.vec = false;
    if (P.G.out_vec && (!P.vec || !aligned16(out))) P.G.out_vec = 0;
    if (P.vec) P.G.A.ext[P.G.A.n_inner - 1] /= 4;
    P.G.A.ncol = P.inner / (P.vec ? 4 : 1);
    P.G.A.tiles = (P.G.A.ncol + GM_THREADS - 1) / GM_THREADS;
}

bool want_split(const RowsPlan &P, int n_groups, int64_t max_group_rows, int split) {
    const int64_t slabs = (max_group_rows + GM_SLAB - 1) / GM_SLAB;
    if (split >= 0) return split != 0;
    const int64_t tiles = (P.inner / (P.vec ? 4 : 1) + GM_THREADS - 1) / GM_THREADS;
    return slabs > 1 && (int64_t)n_groups * tiles < GM_TARGET_BLOCKS;
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" size_t dlwpcs_group_mean_scratch_bytes(const dlwpcs_rows_desc *d, int n_groups, int64_t max_group_rows, int split) {
    RowsPlan P;
    if (make_rows_plan(d, "group_mean", P) != DLWPCS_OK || n_groups < 1 || max_group_rows < 1) return 0;
    // sized for either load width (the pointers' alignment is not known here): elements per row, not chunks
    RowsPlan Q = P;
    Q.vec = false;
    if (!want_split(P, n_groups, max_group_rows, split) && !want_split(Q, n_groups, max_group_rows, split)) return 0;
    const int64_t slabs = (max_group_rows + GM_SLAB - 1) / GM_SLAB;
    return (size_t)((int64_t)n_groups * slabs * P.inner) * (sizeof(double) + sizeof(int32_t));
}

extern "C" int dlwpcs_group_mean(const dlwpcs_rows_desc *d, const float *src, const int32_t *group_start, const int32_t *row_index,
                                 int n_groups, int64_t max_group_rows, int split, float *out, int32_t *count, void *scratch,
                                 size_t scratch_bytes, dlwpcs_stream_t stream) {
    RowsPlan P;
    int rc = make_rows_plan(d, "group_mean", P);
    if (rc != DLWPCS_OK) return rc;
    if (n_groups < 0 || max_group_rows < 0) return fail(DLWPCS_E_INVALID, "group_mean: negative group / row count");
    if (n_groups == 0 || P.inner == 0) return DLWPCS_OK;
    if (!src || !group_start || !row_index || !out) return fail(DLWPCS_E_INVALID, "group_mean: null operand");
    settle(P, src, out);
    RowsGeom &G = P.G;
    G.slabs = (max_group_rows + GM_SLAB - 1) / GM_SLAB;
    if (G.slabs < 1) G.slabs = 1;
    const bool sp = want_split(P, n_groups, max_group_rows, split);
    const int64_t finish_blocks = (int64_t)n_groups * G.A.tiles;
    G.A.nblk = sp ? finish_blocks * G.slabs : finish_blocks;
    if (G.A.nblk > MAX_BLOCKS) return fail(DLWPCS_E_INVALID, "group_mean: %lld workgroups is too many", (long long)G.A.nblk);
    double *psum = nullptr;
    int32_t *pcnt = nullptr;
    if (sp) {
        const size_t cells = (size_t)((int64_t)n_groups * G.slabs * P.inner);
        const size_t need = cells * (sizeof(double) + sizeof(int32_t));
        if (!scratch || scratch_bytes < need || (((uintptr_t)scratch) & 7))
            return fail(DLWPCS_E_INVALID, "group_mean: scratch of %zu bytes, need %zu (8-byte aligned)", scratch_bytes, need);
        psum = (double *)scratch;
        pcnt = (int32_t *)(psum + cells);
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid = launch_grid(G.A.nblk), blk(GM_THREADS);
    if (!sp) {
        if (P.vec) hipLaunchKernelGGL((group_mean_kernel<true, false>), grid, blk, 0, s, G, src, group_start, row_index, psum, pcnt, out, count);
        else hipLaunchKernelGGL((group_mean_kernel<false, false>), grid, blk, 0, s, G, src, group_start, row_index, psum, pcnt, out, count);
        return check_launch("group_mean");
    }
    if (P.vec) hipLaunchKernelGGL((group_mean_kernel<true, true>), grid, blk, 0, s, G, src, group_start, row_index, psum, pcnt, out, count);
    else hipLaunchKernelGGL((group_mean_kernel<false, true>), grid, blk, 0, s, G, src, group_start, row_index, psum, pcnt, out, count);
    G.A.nblk = finish_blocks;
    if (P.vec) hipLaunchKernelGGL((group_finish_kernel<true>), launch_grid(G.A.nblk), blk, 0, s, G, group_start, psum, pcnt, out, count);
    else hipLaunchKernelGGL((group_finish_kernel<false>), launch_grid(G.A.nblk), blk, 0, s, G, group_start, psum, pcnt, out, count);
    return check_launch("group_mean");
}

extern "C" int dlwpcs_rows_gather(const dlwpcs_rows_desc *d, const float *src, const int32_t *index, int64_t n, float *out,
                                  dlwpcs_stream_t stream) {
    RowsPlan P;
    int rc = make_rows_plan(d, "rows_gather", P);
    if (rc != DLWPCS_OK) return rc;
    if (n < 0) return fail(DLWPCS_E_INVALID, "rows_gather: negative row count");
    if (n == 0 || P.inner == 0) return DLWPCS_OK;
    if (!src || !index || !out) return fail(DLWPCS_E_INVALID, "rows_gather: null operand");
    settle(P, src, out);
    RowsGeom &G = P.G;
    G.A.nblk = n * G.A.tiles;
    if (G.A.nblk > MAX_BLOCKS) return fail(DLWPCS_E_INVALID, "rows_gather: %lld workgroups is too many", (long long)G.A.nblk);
    hipStream_t s = (hipStream_t)stream;
    if (P.vec) hipLaunchKernelGGL((rows_gather_kernel<true>), launch_grid(G.A.nblk), dim3(GM_THREADS), 0, s, G, src, index, out);
    else hipLaunchKernelGGL((rows_gather_kernel<false>), launch_grid(G.A.nblk), dim3(GM_THREADS), 0, s, G, src, index, out);
    return check_launch("rows_gather");
}
