// Least-squares fits along the row axis (dlwpcs_time_regression, dlwpcs_time_regression_apply): per element of a dlwpcs_rows_desc
// row set, the coefficients of a (T, K) basis fitted to the rows that are present, by fp64 normal equations in a fixed order
// (include/dlwpcs.h states the operation; the tests compare bits against it).  No atomics, nothing crosses lanes: 256 lanes, a lane
// owns one chunk of a row (a float4 up to term class 8, one element in class 16), grid = column tiles [x slabs], as in
// group_mean_kernel.
//
// The streaming pass (time_regression_kernel): a lane walks its rows once and keeps c[k] = sum b[r,k] x[r,e] and n per element, K
// a compile-time class (1, 2, 4, 8, 16) so that c[] is indexed statically; the basis row is uniform over the workgroup and comes
// through the scalar cache; the next batch of rows is in flight while one is summed.  b and x are fp32, so every product is exact
// in fp64 and fma has the bits of a multiply and an add.  A missing entry enters as b * 0 = +-0: the sums start at +0, a sum of
// doubles is -0 only when both terms are, so adding a zero changes nothing.  split = 1 gives every (tile, slab) its workgroups and
// stores the slab sums, split = 0 lets a lane walk its slabs and stores their sum: either way the sums pass through scratch to
// the finishing launch, so this kernel keeps the registers of a streaming kernel (68 in class 16; with the solves inlined it
// was 256 and one wave per SIMD).
//
// G = sum b[r,i] b[r,j] over the present rows.  A column with no missing row has the G of every other such column:
// time_regression_gram_kernel sums it slab by slab out of LDS, time_regression_factor_kernel adds the slab sums and factorises,
// once per call, into the caller's scratch; a complete column only does the two triangular solves with factors read through the
// scalar cache.  A column with gaps (SKIP mode only: PROPAGATE answers QNAN) re-reads its rows in the finishing launch and
// accumulates its own G, as many rows of G per pass as TR_GRAM_BUDGET doubles of registers hold (one pass up to class 8, two in
// class 16), into a per-lane array; the factorisation walks that array with run-time loops.  The finishing launch runs one
// element per lane whatever the chunk of the sums was: the columns with gaps are latency- and VALU-bound, not bandwidth-bound,
// and four times the workgroups serve them better than 16-byte loads.  Slab sums of an own G would be K (K + 1) / 2 doubles per
// element and slab, up to half the size of the series: not built.
//
// The factorisation and the solves round every product: they stand under fp contract(off), their quotients are __ddiv_rn.
//
// No profiler tags: the launch profiler's registry is the convolution family's (tests/test_conv_coverage_tags.py), as for the
// other verification kernels.
#include <math.h>
#include "strided.h"

namespace dlwpcs {

namespace {

constexpr int TR_THREADS = 256;
constexpr int TR_UNROLL = 4;                        // rows per batch of the evaluation
// rows per batch of the sums, two batches in flight per lane: 2 x 4 x 16 bytes, or 2 x 8 x 4
__host__ __device__ constexpr int tr_unroll(int V) { return V == 4 ? 4 : 8; }
constexpr int TR_GRAM_UNROLL = 16;                  // rows per batch of an own G (one element per lane): 2 x 16 x 4 bytes in flight
constexpr int TR_STAGE_ROWS = 256;                  // basis rows the shared G stages in LDS at a time (16 KiB)
constexpr int TR_MAX_TERMS = DLWPCS_REGRESSION_MAX_TERMS;
constexpr int TR_VEC_MAX_CLASS = 8;                 // 16-byte chunks up to this class: c is 2 x 4 x 8 = 64 registers
constexpr int64_t TR_TARGET_BLOCKS = 512;           // as group_mean: fewer column tiles than this and more than one slab split
constexpr int TR_GRAM_BUDGET = 96;                  // doubles of an own G a lane accumulates per pass over its column
constexpr int TR_FACTOR_THREADS = 192;              // >= 136 pairs
// the shared factor in scratch, in doubles: L packed by rows (tri), d, and 1.0 where no column was singular
constexpr int TR_NP = TR_MAX_TERMS * (TR_MAX_TERMS + 1) / 2;
// behind it the slab sums of that G, TR_NP doubles per slab
constexpr int TR_FAC_D = TR_NP, TR_FAC_OK = TR_NP + TR_MAX_TERMS, TR_FAC_DOUBLES = 160;

__host__ __device__ constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }

// the rows of G [i0, i1) one pass accumulates: as many as the budget holds, at least one
__host__ __device__ constexpr int tr_pass_end(int KC, int V, int i0) {
    int i1 = i0 + 1, ent = i0 + 1;
    while (i1 < KC && (ent + i1 + 1) * V <= TR_GRAM_BUDGET) { ent += i1 + 1; ++i1; }
    return i1;
}

struct TrGeom {
    RowsAddr A;
    int32_t out_vec;
    int32_t K, mode, own_all;
    int64_t T, S, slabs;                            // rows, rows per slab, slabs
    int64_t min_count, term_stride, inner;
    double pivot_tol;
};

struct TrApplyGeom {
    RowsAddr A;
    int32_t out_vec, coef_vec;
    int32_t K;
    int64_t cst[DLWPCS_SCORE_MAX_DIMS];             // the coefficients' stride per inner dim
    int64_t T, slab_rows, term_stride;
};

// ---- the factorisation and the solves: every product rounded -----------------------------------------------------------
// G packed by rows in g[]; on return L below the diagonal of g[], d[]; false: a singular column (g, d then hold nothing)
__device__ __forceinline__ bool tr_factor(const int K, double *g, double *d, const double tol) {
#pragma clang fp contract(off)
    for (int j = 0; j < K; ++j) {
        double s = 0.0;
        for (int p = 0; p < j; ++p) {
            const double l = g[tri(j, p)];
            s = s + (l * l) * d[p];
        }
        const double gjj = g[tri(j, j)];
        const double dj = gjj - s;
        if (!(dj > tol * gjj)) return false;
        d[j] = dj;
        for (int i = j + 1; i < K; ++i) {
            double t = 0.0;
            for (int p = 0; p < j; ++p) t = t + (g[tri(i, p)] * g[tri(j, p)]) * d[p];
            g[tri(i, j)] = __ddiv_rn(g[tri(i, j)] - t, dj);
        }
    }
    return true;
}

// a[] = the solution of L D L^T a = c; a[] first holds z, then w, then a
__device__ __forceinline__ void tr_solve(const int K, const double *__restrict__ L, const double *__restrict__ d, const double *c,
                                         double *a) {
#pragma clang fp contract(off)
    for (int i = 0; i < K; ++i) {
        double s = 0.0;
        for (int p = 0; p < i; ++p) s = s + L[tri(i, p)] * a[p];
        a[i] = c[i] - s;
    }
    for (int i = 0; i < K; ++i) a[i] = __ddiv_rn(a[i], d[i]);
    for (int i = K - 1; i >= 0; --i) {
        double s = 0.0;
        for (int p = i + 1; p < K; ++p) s = s + L[tri(p, i)] * a[p];
        a[i] = a[i] - s;
    }
}

// ---- the streaming sums ----------------------------------------------------------------------------------------------------
// U rows from row r on, a row at or past r1 as zeros (never used)
template <int V, int U>
__device__ __forceinline__ void tr_load_rows(const float *__restrict__ p, int64_t rs, int64_t r, int64_t r1, float x[U][V]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (r + u < r1) {
            load_chunk<V>(p + (r + u) * rs, x[u]);
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) x[u][v] = 0.f;
        }
    }
}

// rows [r0, r1) of the lane's column added to c / n row by row; the next batch of rows is in flight while one is summed
template <int V, int KC>
__device__ __forceinline__ void tr_slab_sums(const TrGeom &G, const float *__restrict__ p, const float *__restrict__ basis, int64_t r0,
                                             int64_t r1, double c[KC][V], int32_t n[V]) {
    constexpr int U = tr_unroll(V);
    float x[U][V];
    tr_load_rows<V, U>(p, G.A.src_row_stride, r0, r1, x);
    for (int64_t r = r0; r < r1; r += U) {
        float nx[U][V];
        tr_load_rows<V, U>(p, G.A.src_row_stride, r + U, r1, nx);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (r + u < r1) {
                const float *__restrict__ b = basis + (r + u) * G.K;
                double xz[V];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const bool present = !isnan(x[u][v]);
                    xz[v] = present ? (double)x[u][v] : 0.0;
                    n[v] += present ? 1 : 0;
                }
#pragma unroll
                for (int k = 0; k < KC; ++k)
                    if (k < KC / 2 || k < G.K) {                // (K > KC / 2 is what put K into this class)
                        const double bk = (double)b[k];
#pragma unroll
                        for (int v = 0; v < V; ++v) c[k][v] = fma(bk, xz[v], c[k][v]);
                    }
            }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int v = 0; v < V; ++v) x[u][v] = nx[u][v];
    }
}

// the passes of an own G over the whole column, pass by pass from row I0 of G: slab sums from zero, added to gm[] in slab order
template <int V, int KC, int I0>
__device__ __forceinline__ void tr_gram_passes(const TrGeom &G, const float *__restrict__ p, const float *__restrict__ basis,
                                               double (&gm)[V][KC * (KC + 1) / 2]) {
    if constexpr (I0 < KC) {
        constexpr int I1 = tr_pass_end(KC, V, I0);
        constexpr int E0 = tri(I0, 0), NE = tri(I1, 0) - E0;
        if (I0 < G.K) {
#pragma unroll
            for (int e = 0; e < NE; ++e)
#pragma unroll
                for (int v = 0; v < V; ++v) gm[v][E0 + e] = 0.0;
            for (int64_t r0 = 0; r0 < G.T; r0 += G.S) {
                const int64_t r1 = r0 + G.S < G.T ? r0 + G.S : G.T;
                double g[NE][V];
#pragma unroll
                for (int e = 0; e < NE; ++e)
#pragma unroll
                    for (int v = 0; v < V; ++v) g[e][v] = 0.0;
                constexpr int U = TR_GRAM_UNROLL;
                float x[U][V];
                tr_load_rows<V, U>(p, G.A.src_row_stride, r0, r1, x);
                for (int64_t r = r0; r < r1; r += U) {
                    float nx[U][V];
                    tr_load_rows<V, U>(p, G.A.src_row_stride, r + U, r1, nx);
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (r + u < r1) {
                            const float *__restrict__ b = basis + (r + u) * G.K;
                            double pm[V];
#pragma unroll
                            for (int v = 0; v < V; ++v) pm[v] = isnan(x[u][v]) ? 0.0 : 1.0;
#pragma unroll
                            for (int i = I0; i < I1; ++i)
                                if (i < KC / 2 || i < G.K) {
                                    const double bi = (double)b[i];
#pragma unroll
                                    for (int j = 0; j <= i; ++j) {
                                        const double bb = bi * (double)b[j];            // exact: 24 x 24 bits
#pragma unroll
                                        for (int v = 0; v < V; ++v) g[tri(i, j) - E0][v] = fma(bb, pm[v], g[tri(i, j) - E0][v]);
                                    }
                                }
                        }
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int v = 0; v < V; ++v) x[u][v] = nx[u][v];
                }
#pragma unroll
                for (int e = 0; e < NE; ++e)
#pragma unroll
                    for (int v = 0; v < V; ++v) gm[v][E0 + e] += g[e][v];
            }
        }
        tr_gram_passes<V, KC, I1>(G, p, basis, gm);
    }
}

// totals -> coefficients of the lane's chunk
template <int V, int KC>
__device__ __forceinline__ void tr_finish(const TrGeom &G, const float *__restrict__ p, const float *__restrict__ basis,
                                          const double *__restrict__ fac, const double tot[KC][V], const int32_t n[V],
                                          float *__restrict__ coef, int32_t *__restrict__ count, int64_t ooff) {
    bool keep[V], own[V];
    bool any_own = false;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        keep[v] = n[v] >= G.min_count && !(G.mode == DLWPCS_FIT_PROPAGATE && n[v] < G.T);
        own[v] = keep[v] && (G.own_all || n[v] < G.T);
        any_own = any_own || own[v];
    }
    double gm[V][KC * (KC + 1) / 2];
    if (any_own) tr_gram_passes<V, KC, 0>(G, p, basis, gm);
    float res[KC][V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        double c[KC], a[KC], d[KC];
#pragma unroll
        for (int k = 0; k < KC; ++k) { c[k] = tot[k][v]; a[k] = 0.0; }
        bool ok = keep[v];
        if (ok) {
            if (own[v]) {
                ok = tr_factor(G.K, gm[v], d, G.pivot_tol);
                if (ok) tr_solve(G.K, gm[v], d, c, a);
            } else {
                ok = fac[TR_FAC_OK] != 0.0;
                if (ok) tr_solve(G.K, fac, fac + TR_FAC_D, c, a);
            }
        }
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            res[k][v] = (float)a[k];
            if (k < G.K && nonfinite(res[k][v])) ok = false;
        }
        if (!ok) {
#pragma unroll
            for (int k = 0; k < KC; ++k) res[k][v] = quiet_nan();
        }
    }
    const int64_t st = G.A.last_out_stride();
#pragma unroll
    for (int k = 0; k < KC; ++k)
        if (k < G.K) store_chunk<V>(coef + k * G.term_stride + ooff, res[k], G.out_vec != 0, st);
    if (count) {
#pragma unroll
        for (int v = 0; v < V; ++v) count[ooff + v * st] = n[v];
    }
}

// The sums of c and n.  SPLIT: a workgroup per (tile, slab), the slab sums stored as part `slab`.  Else a lane walks its slabs
// and adds their sums in slab order: one part.  The finishing launch takes it from there, so that this kernel keeps the registers,
// and with them the occupancy, of a streaming kernel.
template <int V, int KC, bool SPLIT>
__global__ void __launch_bounds__(TR_THREADS) time_regression_kernel(TrGeom G, const float *__restrict__ src,
                                                                    const float *__restrict__ basis, double *__restrict__ psum,
                                                                    int32_t *__restrict__ pcnt) {
    const int64_t bid = flat_block();
    if (bid >= G.A.nblk) return;
    const int64_t slab = bid / G.A.tiles;
    const int64_t q = (bid - slab * G.A.tiles) * TR_THREADS + threadIdx.x;
    if (q >= G.A.ncol) return;
    int64_t soff, ooff;
    rows_offsets<V, false>(G.A, q, soff, ooff);
    const float *p = src + soff;
    int32_t n[V];
    double tot[KC][V];
#pragma unroll
    for (int v = 0; v < V; ++v) n[v] = 0;
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int v = 0; v < V; ++v) tot[k][v] = 0.0;
    if constexpr (SPLIT) {
        const int64_t r0 = slab * G.S;
        tr_slab_sums<V, KC>(G, p, basis, r0, r0 + G.S < G.T ? r0 + G.S : G.T, tot, n);
    } else {
        for (int64_t r0 = 0; r0 < G.T; r0 += G.S) {
            double s[KC][V];
#pragma unroll
            for (int k = 0; k < KC; ++k)
#pragma unroll
                for (int v = 0; v < V; ++v) s[k][v] = 0.0;
            tr_slab_sums<V, KC>(G, p, basis, r0, r0 + G.S < G.T ? r0 + G.S : G.T, s, n);
#pragma unroll
            for (int k = 0; k < KC; ++k)
#pragma unroll
                for (int v = 0; v < V; ++v) tot[k][v] += s[k][v];
        }
    }
#pragma unroll
    for (int k = 0; k < KC; ++k)
        if (k < KC / 2 || k < G.K) {
#pragma unroll
            for (int v = 0; v < V; ++v) psum[(slab * G.K + k) * G.inner + q * V + v] = tot[k][v];
        }
#pragma unroll
    for (int v = 0; v < V; ++v) pcnt[slab * G.inner + q * V + v] = n[v];
}

// The parts added in order, then the solves: one ELEMENT per lane whatever the chunk of the sums was, so that the columns with
// gaps, which walk their rows again for G, are spread over four times as many workgroups
template <int KC>
__global__ void __launch_bounds__(TR_THREADS) time_regression_finish_kernel(TrGeom G, const float *__restrict__ src,
                                                                           const float *__restrict__ basis,
                                                                           const double *__restrict__ fac,
                                                                           const double *__restrict__ psum,
                                                                           const int32_t *__restrict__ pcnt, float *__restrict__ coef,
                                                                           int32_t *__restrict__ count) {
    const int64_t bid = flat_block();
    if (bid >= G.A.nblk) return;
    const int64_t q = bid * TR_THREADS + threadIdx.x;
    if (q >= G.A.ncol) return;
    int64_t soff, ooff;
    rows_offsets<1, false>(G.A, q, soff, ooff);
    double tot[KC][1];
    int32_t n[1] = {0};
#pragma unroll
    for (int k = 0; k < KC; ++k) tot[k][0] = 0.0;
    for (int64_t part = 0; part < G.slabs; ++part) {
#pragma unroll
        for (int k = 0; k < KC; ++k)
            if (k < KC / 2 || k < G.K) tot[k][0] += psum[(part * G.K + k) * G.inner + q];
        n[0] += pcnt[part * G.inner + q];
    }
    tr_finish<1, KC>(G, src + soff, basis, fac, tot, n, coef, count, ooff);
}

// G of a column with every row present: a workgroup per slab, a pair (i, j) per lane, the rows in the definition's order out of
// LDS (staged TR_STAGE_ROWS at a time, whatever the slab length); the slab sums go to gs
__global__ void __launch_bounds__(TR_THREADS) time_regression_gram_kernel(int32_t K, int64_t T, int64_t S, int64_t slabs,
                                                                         const float *__restrict__ basis, double *__restrict__ gs) {
    __shared__ float stage[TR_STAGE_ROWS * TR_MAX_TERMS];
    const int64_t slab = flat_block();
    if (slab >= slabs) return;
    const int t = (int)threadIdx.x, np = tri(K, 0);
    int i = 0;
    while (i + 1 < K && tri(i + 1, 0) <= t) ++i;
    const int j = t < np ? t - tri(i, 0) : 0;
    const int64_t r0 = slab * S, r1 = r0 + S < T ? r0 + S : T;
    double s = 0.0;
    for (int64_t rc = r0; rc < r1; rc += TR_STAGE_ROWS) {
        const int rows = (int)(r1 - rc < TR_STAGE_ROWS ? r1 - rc : TR_STAGE_ROWS);
        for (int at = t; at < rows * K; at += TR_THREADS) stage[at] = basis[rc * K + at];
        __syncthreads();
        if (t < np)
            for (int rr = 0; rr < rows; ++rr) s = fma((double)stage[rr * K + i], (double)stage[rr * K + j], s);
        __syncthreads();
    }
    if (t < np) gs[slab * TR_NP + t] = s;
}

// the slab sums added in slab order, then L and d: column j of L by the lanes i > j at once, each entry by the operations of
// tr_factor in their order
__global__ void __launch_bounds__(TR_FACTOR_THREADS) time_regression_factor_kernel(int32_t K, int64_t slabs, double pivot_tol,
                                                                                  const double *__restrict__ gs,
                                                                                  double *__restrict__ fac) {
#pragma clang fp contract(off)
    __shared__ double g[TR_NP], d[TR_MAX_TERMS];
    __shared__ int ok;
    const int t = (int)threadIdx.x, np = tri(K, 0);
    if (t < np) {
        double tot = 0.0;
        for (int64_t slab = 0; slab < slabs; ++slab) tot += gs[slab * TR_NP + t];
        g[t] = tot;
    }
    if (t == 0) ok = 1;
    for (int j = 0; j < K; ++j) {
        __syncthreads();
        if (t == 0) {
            double s = 0.0;
            for (int p = 0; p < j; ++p) {
                const double l = g[tri(j, p)];
                s = s + (l * l) * d[p];
            }
            const double gjj = g[tri(j, j)];
            const double dj = gjj - s;
            d[j] = dj;
            if (!(dj > pivot_tol * gjj)) ok = 0;
        }
        __syncthreads();
        if (!ok) break;
        if (t > j && t < K) {
            double s = 0.0;
            for (int p = 0; p < j; ++p) s = s + (g[tri(t, p)] * g[tri(j, p)]) * d[p];
            g[tri(t, j)] = __ddiv_rn(g[tri(t, j)] - s, d[j]);
        }
    }
    __syncthreads();
    if (t < np) fac[t] = g[t];
    if (t < K) fac[TR_FAC_D + t] = d[t];
    if (t == 0) fac[TR_FAC_OK] = ok ? 1.0 : 0.0;
}

// fitted values or residuals: the coefficients of the lane's chunk stay in registers, every row of the slab is read once
template <int V, int KC, bool RESID>
__global__ void __launch_bounds__(TR_THREADS) time_regression_apply_kernel(TrApplyGeom G, const float *__restrict__ src,
                                                                          const float *__restrict__ basis,
                                                                          const float *__restrict__ coef, float *__restrict__ out) {
    const int64_t bid = flat_block();
    if (bid >= G.A.nblk) return;
    const int64_t slab = bid / G.A.tiles;
    const int64_t q = (bid - slab * G.A.tiles) * TR_THREADS + threadIdx.x;
    if (q >= G.A.ncol) return;
    int64_t soff, ooff, coff;
    flat_offsets<V, false>(G.A.n_inner, G.A.ext, q, Strided{G.A.sst, soff}, Strided{G.A.ost, ooff}, Strided{G.cst, coff});
    const int64_t cs = G.A.n_inner ? G.cst[G.A.n_inner - 1] : 1;
    double cf[KC][V];
    bool bad[V];
#pragma unroll
    for (int v = 0; v < V; ++v) bad[v] = false;
#pragma unroll
    for (int k = 0; k < KC; ++k)
        if (k < G.K) {
            float c[V];
            if (G.coef_vec) {
                load_chunk<V>(coef + k * G.term_stride + coff, c);
            } else {
#pragma unroll
                for (int v = 0; v < V; ++v) c[v] = coef[k * G.term_stride + coff + v * cs];
            }
#pragma unroll
            for (int v = 0; v < V; ++v) {
                cf[k][v] = (double)c[v];
                bad[v] = bad[v] || isnan(c[v]);
            }
        }
    const int64_t r0 = slab * G.slab_rows;
    const int64_t r1 = r0 + G.slab_rows < G.T ? r0 + G.slab_rows : G.T;
    const int64_t st = G.A.last_out_stride();
    for (int64_t r = r0; r < r1; r += TR_UNROLL) {
        float x[TR_UNROLL][V];
        if constexpr (RESID) {
#pragma unroll
            for (int u = 0; u < TR_UNROLL; ++u)
                if (r + u < r1) load_chunk<V>(src + (r + u) * G.A.src_row_stride + soff, x[u]);
        }
#pragma unroll
        for (int u = 0; u < TR_UNROLL; ++u)
            if (r + u < r1) {
                const float *__restrict__ b = basis + (r + u) * G.K;
                double f[V];
#pragma unroll
                for (int v = 0; v < V; ++v) f[v] = 0.0;
#pragma unroll
                for (int k = 0; k < KC; ++k)
                    if (k < G.K) {
                        const double bk = (double)b[k];
#pragma unroll
                        for (int v = 0; v < V; ++v) f[v] = fma(bk, cf[k][v], f[v]);
                    }
                float y[V];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    y[v] = RESID ? (float)((double)x[u][v] - f[v]) : (float)f[v];
                    if (bad[v] || isnan(y[v])) y[v] = quiet_nan();
                }
                store_chunk<V>(out + (r + u) * G.A.out_row_stride + ooff, y, G.out_vec != 0, st);
            }
    }
}

// ---- the planner (restated in tests/time_regression_ref.py) --------------------------------------------
struct TrPlan {
    TrGeom G;
    int cls;
    bool vec, split, own_all;
    int64_t inner;
};

int tr_class(int K) {
    int c = 1;
    while (c < K) c *= 2;
    return c;
}

bool tr_want_split(int64_t inner, bool vec, int64_t slabs, int split) {
    if (split >= 0) return split != 0;
    const int64_t tiles = (inner / (vec ? 4 : 1) + TR_THREADS - 1) / TR_THREADS;
    return slabs > 1 && tiles < TR_TARGET_BLOCKS;
}

int64_t tr_slabs(int64_t n_rows, int64_t S) {
    const int64_t n = (n_rows + S - 1) / S;
    return n < 1 ? 1 : n;
}

// src / coef: looked at for 16-byte alignment only
int tr_plan(const dlwpcs_rows_desc *d, const void *src, const void *coef, int64_t n_rows, int n_terms, int mode, int64_t min_count,
            double pivot_tol, int64_t slab_rows, int split, int gram, int64_t term_stride, TrPlan &P) {
    TrGeom &G = P.G;
    memset(&G, 0, sizeof(G));
    const int rc = rows_addr_init(d, "time_regression", G.A, P.inner);
    if (rc != DLWPCS_OK) return rc;
    if (n_terms < 1 || n_terms > TR_MAX_TERMS) return fail(DLWPCS_E_INVALID, "time_regression: %d terms (1 .. %d)", n_terms, TR_MAX_TERMS);
    if (n_rows < 0 || n_rows > (1ll << 31)) return fail(DLWPCS_E_INVALID, "time_regression: %lld rows", (long long)n_rows);
    if (mode != DLWPCS_FIT_SKIP && mode != DLWPCS_FIT_PROPAGATE) return fail(DLWPCS_E_INVALID, "time_regression: mode %d", mode);
    if (min_count < n_terms || min_count > (1ll << 31))
        return fail(DLWPCS_E_INVALID, "time_regression: min_count %lld below the %d terms", (long long)min_count, n_terms);
    if (!(pivot_tol >= 0.0) || !(pivot_tol < 1.0)) return fail(DLWPCS_E_INVALID, "time_regression: pivot_tol %g outside [0, 1)", pivot_tol);
    if (slab_rows < 0 || slab_rows > (1ll << 31)) return fail(DLWPCS_E_INVALID, "time_regression: slab_rows %lld", (long long)slab_rows);
    if (split < -1 || split > 1 || gram < -1 || gram > 1) return fail(DLWPCS_E_INVALID, "time_regression: split %d, gram %d", split, gram);
    G.K = n_terms; G.mode = mode; G.T = n_rows; G.min_count = min_count; G.term_stride = term_stride; G.inner = P.inner;
    G.S = slab_rows ? slab_rows : DLWPCS_REGRESSION_SLAB_ROWS;
    G.pivot_tol = pivot_tol != 0.0 ? pivot_tol : 0x1p-40;
    G.slabs = tr_slabs(n_rows, G.S);
    P.cls = tr_class(n_terms);
    P.own_all = gram == 1;                              // the planner's own choice is the shared factor: it is never slower
    G.own_all = P.own_all ? 1 : 0;
    bool vec, ovec;
    rows_vector_ok(d, vec, ovec);
    vec = vec && aligned16(src) && P.cls <= TR_VEC_MAX_CLASS;
    ovec = ovec && vec && aligned16(coef) && term_stride % 4 == 0;
    P.vec = vec;
    G.out_vec = ovec;
    if (vec) G.A.ext[d->n_inner - 1] /= 4;
    G.A.ncol = P.inner / (vec ? 4 : 1);
    G.A.tiles = (G.A.ncol + TR_THREADS - 1) / TR_THREADS;
    P.split = tr_want_split(P.inner, vec, G.slabs, split);
    G.A.nblk = P.split ? G.A.tiles * G.slabs : G.A.tiles;
    if (G.A.nblk > MAX_BLOCKS || (P.inner + TR_THREADS - 1) / TR_THREADS > MAX_BLOCKS)
        return fail(DLWPCS_E_INVALID, "time_regression: %lld workgroups is too many", (long long)G.A.nblk);
    return DLWPCS_OK;
}

size_t tr_split_bytes(int64_t slabs, int64_t inner, int K) {
    return (size_t)(slabs * inner) * ((size_t)K * sizeof(double) + sizeof(int32_t));
}

template <int V, int KC>
void tr_launch(const TrPlan &P, const float *src, const float *basis, const double *fac, double *psum, int32_t *pcnt, float *coef,
               int32_t *count, hipStream_t s) {
    const TrGeom &G = P.G;
    const dim3 blk(TR_THREADS);
    if (P.split) hipLaunchKernelGGL((time_regression_kernel<V, KC, true>), launch_grid(G.A.nblk), blk, 0, s, G, src, basis, psum, pcnt);
    else hipLaunchKernelGGL((time_regression_kernel<V, KC, false>), launch_grid(G.A.nblk), blk, 0, s, G, src, basis, psum, pcnt);
    // the finishing launch: one element per lane, G.slabs = the parts to add
    TrGeom F = G;
    if (P.vec) F.A.ext[F.A.n_inner - 1] *= 4;
    F.out_vec = 0;
    F.A.ncol = P.inner;
    F.A.tiles = (F.A.ncol + TR_THREADS - 1) / TR_THREADS;
    F.A.nblk = F.A.tiles;
    if (!P.split) F.slabs = 1;
    hipLaunchKernelGGL((time_regression_finish_kernel<KC>), launch_grid(F.A.nblk), blk, 0, s, F, src, basis, fac, psum, pcnt, coef, count);
}

template <int V>
void tr_launch_class(const TrPlan &P, const float *src, const float *basis, const double *fac, double *psum, int32_t *pcnt, float *coef,
                     int32_t *count, hipStream_t s) {
    switch (P.cls) {
    case 1: tr_launch<V, 1>(P, src, basis, fac, psum, pcnt, coef, count, s); break;
    case 2: tr_launch<V, 2>(P, src, basis, fac, psum, pcnt, coef, count, s); break;
    case 4: tr_launch<V, 4>(P, src, basis, fac, psum, pcnt, coef, count, s); break;
    case 8: tr_launch<V, 8>(P, src, basis, fac, psum, pcnt, coef, count, s); break;
    default:
        if constexpr (V == 1) tr_launch<1, 16>(P, src, basis, fac, psum, pcnt, coef, count, s);   // (class 16: one element per lane)
        break;
    }
}

template <int V, int KC>
void tr_apply_launch(const TrApplyGeom &G, bool resid, const float *src, const float *basis, const float *coef, float *out, hipStream_t s) {
    const dim3 grid = launch_grid(G.A.nblk), blk(TR_THREADS);
    if (resid) hipLaunchKernelGGL((time_regression_apply_kernel<V, KC, true>), grid, blk, 0, s, G, src, basis, coef, out);
    else hipLaunchKernelGGL((time_regression_apply_kernel<V, KC, false>), grid, blk, 0, s, G, src, basis, coef, out);
}

template <int V>
void tr_apply_class(const TrApplyGeom &G, int cls, bool resid, const float *src, const float *basis, const float *coef, float *out,
                    hipStream_t s) {
    switch (cls) {
    case 1: tr_apply_launch<V, 1>(G, resid, src, basis, coef, out, s); break;
    case 2: tr_apply_launch<V, 2>(G, resid, src, basis, coef, out, s); break;
    case 4: tr_apply_launch<V, 4>(G, resid, src, basis, coef, out, s); break;
    case 8: tr_apply_launch<V, 8>(G, resid, src, basis, coef, out, s); break;
    default:
        if constexpr (V == 1) tr_apply_launch<1, 16>(G, resid, src, basis, coef, out, s);
        break;
    }
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" size_t dlwpcs_time_regression_scratch_bytes(const dlwpcs_rows_desc *d, int64_t n_rows, int n_terms, int64_t slab_rows,
                                                       int split) {
    RowsAddr A;
    int64_t inner;
    if (rows_addr_init(d, "time_regression", A, inner) != DLWPCS_OK || n_rows < 0 || n_terms < 1 || n_terms > TR_MAX_TERMS || slab_rows < 0)
        return 0;
    const int64_t slabs = tr_slabs(n_rows, slab_rows ? slab_rows : DLWPCS_REGRESSION_SLAB_ROWS);
    const size_t fac = (size_t)(TR_FAC_DOUBLES + slabs * TR_NP) * sizeof(double);
    // sized for either load width (the pointers' alignment is not known here): the parts are the slabs if either would split
    bool vec, ovec;
    rows_vector_ok(d, vec, ovec);
    vec = vec && tr_class(n_terms) <= TR_VEC_MAX_CLASS;
    const bool sp = tr_want_split(inner, vec, slabs, split) || tr_want_split(inner, false, slabs, split);
    return fac + tr_split_bytes(sp ? slabs : 1, inner, n_terms);
}

extern "C" int dlwpcs_time_regression(const dlwpcs_rows_desc *d, const float *src, int64_t n_rows, const float *basis, int n_terms,
                                      int mode, int64_t min_count, double pivot_tol, int64_t slab_rows, int split, int gram, float *coef,
                                      int64_t coef_term_stride, int32_t *count, void *scratch, size_t scratch_bytes,
                                      dlwpcs_stream_t stream) {
    TrPlan P;
    int rc = tr_plan(d, src, coef, n_rows, n_terms, mode, min_count, pivot_tol, slab_rows, split, gram, coef_term_stride, P);
    if (rc != DLWPCS_OK) return rc;
    if (P.inner == 0) return DLWPCS_OK;
    if (!coef || (n_rows > 0 && (!src || !basis))) return fail(DLWPCS_E_INVALID, "time_regression: null operand");
    if ((((uintptr_t)src) | ((uintptr_t)basis) | ((uintptr_t)coef) | ((uintptr_t)count)) & 3)
        return fail(DLWPCS_E_INVALID, "time_regression: an operand is not aligned to its 4-byte elements");
    const size_t fac_doubles = (size_t)(TR_FAC_DOUBLES + P.G.slabs * TR_NP), fac_bytes = fac_doubles * sizeof(double);
    const int64_t parts = P.split ? P.G.slabs : 1;
    const size_t need = fac_bytes + tr_split_bytes(parts, P.inner, n_terms);
    if (!scratch || scratch_bytes < need || (((uintptr_t)scratch) & 7))
        return fail(DLWPCS_E_INVALID, "time_regression: scratch of %zu bytes, need %zu (8-byte aligned)", scratch_bytes, need);
    double *fac = (double *)scratch;
    double *gs = fac + TR_FAC_DOUBLES;
    double *psum = fac + fac_doubles;
    int32_t *pcnt = (int32_t *)(psum + (size_t)(parts * P.inner) * n_terms);
    hipStream_t s = (hipStream_t)stream;
    if (!P.own_all) {
        if (P.G.slabs > MAX_BLOCKS) return fail(DLWPCS_E_INVALID, "time_regression: %lld slabs is too many", (long long)P.G.slabs);
        hipLaunchKernelGGL(time_regression_gram_kernel, launch_grid(P.G.slabs), dim3(TR_THREADS), 0, s, (int32_t)n_terms, n_rows, P.G.S,
                           P.G.slabs, basis, gs);
        hipLaunchKernelGGL(time_regression_factor_kernel, dim3(1), dim3(TR_FACTOR_THREADS), 0, s, (int32_t)n_terms, P.G.slabs,
                           P.G.pivot_tol, gs, fac);
    }
    if (P.vec) tr_launch_class<4>(P, src, basis, fac, psum, pcnt, coef, count, s);
    else tr_launch_class<1>(P, src, basis, fac, psum, pcnt, coef, count, s);
    return check_launch("time_regression");
}

extern "C" int dlwpcs_time_regression_plan_info(const dlwpcs_rows_desc *d, const void *src, const void *coef, int64_t n_rows, int n_terms,
                                                int mode, int64_t min_count, int64_t slab_rows, int split, int gram,
                                                int64_t coef_term_stride, int32_t info[8]) {
    if (!info) return fail(DLWPCS_E_INVALID, "time_regression_plan_info: null info");
    TrPlan P;
    int rc = tr_plan(d, src, coef, n_rows, n_terms, mode, min_count, 0.0, slab_rows, split, gram, coef_term_stride, P);
    if (rc != DLWPCS_OK) return rc;
    const bool empty = P.inner == 0;
    if (!empty && (!coef || (n_rows > 0 && !src))) return fail(DLWPCS_E_INVALID, "time_regression: null operand");
    const dim3 grid = launch_grid(empty ? 0 : P.G.A.nblk);
    info[0] = P.split ? 1 : 0;
    info[1] = P.own_all ? 1 : 0;
    info[2] = P.cls;
    info[3] = P.vec ? 4 : 1;
    info[4] = (int32_t)grid.x;
    info[5] = (int32_t)grid.y;
    info[6] = 0;
    info[7] = (int32_t)(P.G.S > 0x7fffffff ? 0x7fffffff : P.G.S);
    return DLWPCS_OK;
}

extern "C" int dlwpcs_time_regression_apply(const dlwpcs_rows_desc *d, const float *src, int64_t n_rows, const float *basis, int n_terms,
                                            const float *coef, int64_t coef_term_stride, const int64_t *coef_stride, int mode, float *out,
                                            dlwpcs_stream_t stream) {
    TrApplyGeom G;
    memset(&G, 0, sizeof(G));
    int64_t inner;
    int rc = rows_addr_init(d, "time_regression_apply", G.A, inner);
    if (rc != DLWPCS_OK) return rc;
    if (n_terms < 1 || n_terms > TR_MAX_TERMS)
        return fail(DLWPCS_E_INVALID, "time_regression_apply: %d terms (1 .. %d)", n_terms, TR_MAX_TERMS);
    if (n_rows < 0 || n_rows > (1ll << 31)) return fail(DLWPCS_E_INVALID, "time_regression_apply: %lld rows", (long long)n_rows);
    if (mode != DLWPCS_FIT_FITTED && mode != DLWPCS_FIT_RESIDUAL) return fail(DLWPCS_E_INVALID, "time_regression_apply: mode %d", mode);
    if (n_rows == 0 || inner == 0) return DLWPCS_OK;
    const bool resid = mode == DLWPCS_FIT_RESIDUAL;
    if (!basis || !coef || !out || (resid && !src)) return fail(DLWPCS_E_INVALID, "time_regression_apply: null operand");
    if ((((uintptr_t)src) | ((uintptr_t)basis) | ((uintptr_t)coef) | ((uintptr_t)out)) & 3)
        return fail(DLWPCS_E_INVALID, "time_regression_apply: an operand is not aligned to its 4-byte elements");
    for (int i = 0; i < d->n_inner; ++i) G.cst[i] = coef_stride ? coef_stride[i] : d->out_stride[i];
    G.K = n_terms; G.T = n_rows; G.term_stride = coef_term_stride;
    const int cls = tr_class(n_terms);
    // 16-byte chunks: the output always, the source where it is read, the coefficients where their layout allows
    const int L = d->n_inner - 1;
    bool vec = L >= 0 && d->inner_ext[L] % 4 == 0 && cls <= TR_VEC_MAX_CLASS && d->out_stride[L] == 1 && d->out_row_stride % 4 == 0 &&
               aligned16(out);
    for (int i = 0; i < L && vec; ++i) vec = d->out_stride[i] % 4 == 0;
    if (resid) {
        bool svec, ovec;
        rows_vector_ok(d, svec, ovec);
        vec = vec && svec && aligned16(src);
    }
    bool cvec = vec && G.cst[L < 0 ? 0 : L] == 1 && coef_term_stride % 4 == 0 && aligned16(coef);
    for (int i = 0; i < L && cvec; ++i) cvec = G.cst[i] % 4 == 0;
    G.out_vec = vec ? 1 : 0;
    G.coef_vec = cvec ? 1 : 0;
    if (vec) G.A.ext[L] /= 4;
    G.A.ncol = inner / (vec ? 4 : 1);
    G.A.tiles = (G.A.ncol + TR_THREADS - 1) / TR_THREADS;
    // enough slabs to fill the chip, none shorter than 8 rows (the coefficients are loaded once per slab)
    const int64_t want = (2 * TR_TARGET_BLOCKS + G.A.tiles - 1) / G.A.tiles;
    int64_t nsl = n_rows / 8 < want ? n_rows / 8 : want;
    if (nsl < 1) nsl = 1;
    G.slab_rows = (n_rows + nsl - 1) / nsl;
    G.A.nblk = G.A.tiles * ((n_rows + G.slab_rows - 1) / G.slab_rows);
    if (G.A.nblk > MAX_BLOCKS) return fail(DLWPCS_E_INVALID, "time_regression_apply: %lld workgroups is too many", (long long)G.A.nblk);
    hipStream_t s = (hipStream_t)stream;
    if (vec) tr_apply_class<4>(G, cls, resid, src, basis, coef, out, s);
    else tr_apply_class<1>(G, cls, resid, src, basis, coef, out, s);
    return check_launch("time_regression_apply");
}
