// Lagged covariances along the row axis (dlwpcs_time_lag; include/dlwpcs.h states the operation, the tests compare bits against
// it): per column of a dlwpcs_rows_desc row set and per lag l of an arithmetic progression, the mean over the pairs present of
// (a[t] - ca) * (b[t + l] - cb), b = a itself (auto), a second series of a's layout (pair) or one vector shared by every column
// (index).  No atomics, nothing crosses lanes, no LDS: 256 lanes, a lane owns one chunk of a row (a float4 where rows_vector_ok
// and the pointers allow it, one element otherwise).
//
// A pass serves a block of up to W consecutive lags, W a compile-time class (1, 4, 8, 16) so that the W x V fp64 sums and the
// pair counts are indexed statically and stay in registers.  The deviations are fp32 (one subtraction), so every product is
// exact in fp64: fma has the bits of a multiply and an add.  A missing entry enters as +0: the sums start at +0, a sum of
// doubles is -0 only when both terms are, so adding the +-0 of a missing pair changes nothing (the argument of
// time_regression.hip).  A pair outside the series is never formed: inf * 0 would not be nothing.
//
// lag_step = 1: the lane walks the a rows of a slab in order and keeps the b rows t + l_lo .. t + l_lo + W - 1 as a ring of
// deviations in registers, one new b row per a row; the walk is unrolled over one period of the ring so that every slot and
// accumulator index is a compile-time constant (the TfLive trick of time_filter.hip).  Only the rows whose lags all pair inside
// the series go through the ring; the rows at the ends of the series, the remainder of a period and every row of a longer
// step load their W partners directly and leave them to the caches.  Either way a lag's products are added in row order.
// Presence is one 16-bit field per element, two to a register: a row's pair counts are one AND and one ADD per two elements
// (a slab has 512 rows: a field cannot overflow).  In the index form the b values are uniform over the workgroup and come
// through the scalar cache.
//
// Rows are cut into slabs of DLWPCS_TIME_LAG_SLAB_ROWS (the slab of a pair is the slab of its a row).  split = 0: a lane walks
// its slabs, adds every finished slab sum to the total in slab order, divides and stores.  split = 1: every (column tile, slab,
// lag block) is a tile of its own and stores fp64 slab sums and int32 counts to scratch; the finishing launch adds them in slab
// order from zero and divides -- the same additions, the same bits.  The grid is TL_SLOTS persistent workgroups that stride
// over the int64 list of tiles (lag block fastest, so that the passes over one stretch of the series meet in the L2); which
// workgroup computes a tile influences nothing.  At most two launches.  No profiler tags, as for the other verification kernels.
#include <math.h>
#include "strided.h"

namespace dlwpcs {

namespace {

constexpr int TL_THREADS = 256;
constexpr int TL_SLAB = DLWPCS_TIME_LAG_SLAB_ROWS;
constexpr int TL_MAX_BLOCK = 16;                    // the widest class
constexpr int64_t TL_SLOTS = 1024;                  // persistent workgroups: 256 compute units x 4; placement only
// split < 0: slabs get tiles of their own below this many (column tile, lag block) tiles.  Measured at 270 and at 648 tiles under 9
// slabs: the split form won both times (the slab sums are a fortieth of what a pass reads), so the bar lies well above them.
constexpr int64_t TL_SPLIT_BELOW = 2048;
constexpr int64_t TL_FINISH_BLOCKS = 2048;
constexpr uint32_t TL_BOTH = 0x00010001u;           // both presence fields of a register

// lags per pass the planner grants a chunk of V elements: the widest class without spills that measured fastest.
// The walking lane also carries the totals over its slabs: 8 lags of a float4 would leave it one wave per SIMD AND cost more
// than 4 did.
__host__ __device__ constexpr int tl_max_block(int V, bool split) { return V == 4 ? (split ? 8 : 4) : 16; }
// waves per SIMD the compiler is held to: two where the register report allows it without spills, else one (the pair form's ring
// of 8 float4 rows needs 262 registers: one wave, and still 1.7 times faster than 9 passes of 4 lags)
__host__ __device__ constexpr int tl_waves(int V, int W, bool index, bool split) {
    return (V == 1 || W <= 4 || (index && split && W <= 8)) ? 2 : 1;
}

struct TlGeom {
    RowsAddr A;                                     // ext in chunks; ncol = chunks per row, tiles = column tiles, nblk = tiles of the launch
    int64_t cst[DLWPCS_SCORE_MAX_DIMS];             // the centres' stride per inner dim
    int32_t out_vec, n_lags, lag_block, n_lb, mode, min_count, split, has_ca, has_cb;
    int64_t T, lag0, lag_step, n_slab, inner;
};

__host__ __device__ inline int64_t tl_need(const TlGeom &G, int64_t l) {
    if (G.mode == DLWPCS_LAG_SKIP) return G.min_count > 1 ? G.min_count : 1;
    const int64_t m = G.T - (l < 0 ? -l : l);
    return m > 1 ? m : 1;
}

// the stored value: one fp64 division, rounded once; every NaN that is stored is 0x7fc00000
__device__ __forceinline__ float tl_value(double s, int32_t n, int64_t need) {
    if ((int64_t)n < need) return quiet_nan();
    const float v = (float)__ddiv_rn(s, (double)n);
    return isnan(v) ? quiet_nan() : v;
}

// one row of an operand -> deviations (one fp32 subtraction, widened once; a missing entry: +0) and presence fields
template <int V>
__device__ __forceinline__ void tl_deviations(const float x[V], const float c[V], double d[V], uint32_t p[(V + 1) / 2]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < (V + 1) / 2; ++j) p[j] = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const bool present = !isnan(x[v]);
        d[v] = (double)(present ? x[v] - c[v] : 0.f);
        p[v >> 1] |= present ? 1u << (16 * (v & 1)) : 0u;
    }
}

// row `row` of b as it lies in memory: INDEX: one value for every element of the chunk; a row outside the series reads as missing
template <int V, bool INDEX>
__device__ __forceinline__ void tl_fetch_b(const float *__restrict__ pb, int64_t brs, int64_t row, int64_t T, float x[INDEX ? 1 : V]) {
    const bool in = row >= 0 && row < T;
    if constexpr (INDEX) {
        x[0] = in ? pb[row] : quiet_nan();
    } else if (in) {
        load_chunk<V>(pb + row * brs, x);
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v) x[v] = quiet_nan();
    }
}

template <int V, bool INDEX>
__device__ __forceinline__ void tl_deviations_b(const float x[INDEX ? 1 : V], const float cb[V], double d[INDEX ? 1 : V],
                                                uint32_t p[(V + 1) / 2]) {
#pragma clang fp contract(off)
    if constexpr (INDEX) {
        const bool present = !isnan(x[0]);
        d[0] = (double)(present ? x[0] - cb[0] : 0.f);
#pragma unroll
        for (int j = 0; j < (V + 1) / 2; ++j) p[j] = present ? TL_BOTH : 0u;
    } else {
        tl_deviations<V>(x, cb, d, p);
    }
}

template <int V, bool INDEX>
__device__ __forceinline__ void tl_load_b(const float *__restrict__ pb, int64_t brs, int64_t row, int64_t T, const float cb[V],
                                          double d[INDEX ? 1 : V], uint32_t p[(V + 1) / 2]) {
    float x[INDEX ? 1 : V];
    tl_fetch_b<V, INDEX>(pb, brs, row, T, x);
    tl_deviations_b<V, INDEX>(x, cb, d, p);
}

template <int V, bool INDEX>
__device__ __forceinline__ void tl_add(const double da[V], const uint32_t pa[(V + 1) / 2], const double db[INDEX ? 1 : V],
                                       const uint32_t pb[(V + 1) / 2], double acc[V], uint32_t cnt[(V + 1) / 2]) {
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = fma(da[v], db[INDEX ? 0 : v], acc[v]);
#pragma unroll
    for (int j = 0; j < (V + 1) / 2; ++j) cnt[j] += pa[j] & pb[j];
}

// a row that loads its partners itself: the lags w < nw whose partner lies inside the series
template <int V, int W, bool INDEX>
__device__ __forceinline__ void tl_row_direct(const TlGeom &G, const float *__restrict__ pa, const float *__restrict__ pb, int64_t brs,
                                              const float ca[V], const float cb[V], int64_t t, int64_t l_lo, int nw, double acc[W][V],
                                              uint32_t cnt[W][(V + 1) / 2]) {
    constexpr int VB = INDEX ? 1 : V, NP = (V + 1) / 2;
    constexpr int GW = W < 4 ? W : 4;                   // partners in flight together
    float x[V];
    double da[V];
    uint32_t qa[NP];
    load_chunk<V>(pa + t * G.A.src_row_stride, x);
    tl_deviations<V>(x, ca, da, qa);
#pragma unroll
    for (int g = 0; g < W; g += GW) {
        if (g >= nw) break;
        float xb[GW][VB];
#pragma unroll
        for (int k = 0; k < GW; ++k)
            if (g + k < nw) tl_fetch_b<V, INDEX>(pb, brs, t + l_lo + (g + k) * G.lag_step, G.T, xb[k]);
#pragma unroll
        for (int k = 0; k < GW; ++k)
            if (g + k < nw) {
                const int64_t tb = t + l_lo + (g + k) * G.lag_step;
                if (tb >= 0 && tb < G.T) {
                    double db[VB];
                    uint32_t qb[NP];
                    tl_deviations_b<V, INDEX>(xb[k], cb, db, qb);
                    tl_add<V, INDEX>(da, qa, db, qb, acc[g + k], cnt[g + k]);
                }
            }
    }
}

// the a rows [r0, r1) of one slab added to acc / cnt, a lag's products in row order
template <int V, int W, bool INDEX>
__device__ __forceinline__ void tl_slab(const TlGeom &G, const float *__restrict__ pa, const float *__restrict__ pb, int64_t brs,
                                        const float ca[V], const float cb[V], int64_t r0, int64_t r1, int64_t l_lo, int nw,
                                        double acc[W][V], uint32_t cnt[W][(V + 1) / 2]) {
    constexpr int VB = INDEX ? 1 : V, NP = (V + 1) / 2;
    constexpr int UL = V == 4 ? (W >= 8 ? 2 : 4) : 8;   // rows of either operand a lane has in flight: what the registers leave
    constexpr int U = W < UL ? UL : W;                  // rows per unrolled batch: whole periods of the ring, whole groups of loads
    // [i0, i1): whole batches of rows whose nw lags all pair inside the series (step 1 only)
    int64_t i0 = r0, i1 = r0;
    if (G.lag_step == 1) {
        i0 = -l_lo > r0 ? -l_lo : r0;
        if (i0 > r1) i0 = r1;
        i1 = G.T - (l_lo + nw - 1);
        if (i1 > r1) i1 = r1;
        if (i1 < i0) i1 = i0;
        i1 = i0 + (i1 - i0) / U * U;
    }
    for (int64_t t = r0; t < i0; ++t) tl_row_direct<V, W, INDEX>(G, pa, pb, brs, ca, cb, t, l_lo, nw, acc, cnt);
    if (i1 > i0) {
        // slot s holds the b row whose distance from i0 + l_lo is s modulo W; a row past the series (nw < W) holds nothing
        double rb[W][VB];
        uint32_t rp[W][NP];
#pragma unroll
        for (int j = 0; j < W - 1; ++j) tl_load_b<V, INDEX>(pb, brs, i0 + l_lo + j, G.T, cb, rb[j], rp[j]);
        for (int64_t t0 = i0; t0 < i1; t0 += U) {
#pragma unroll
            for (int g = 0; g < U; g += UL) {               // UL rows of either operand in flight
                float xa[UL][V], xb[UL][VB];
#pragma unroll
                for (int k = 0; k < UL; ++k) load_chunk<V>(pa + (t0 + g + k) * G.A.src_row_stride, xa[k]);
#pragma unroll
                for (int k = 0; k < UL; ++k) tl_fetch_b<V, INDEX>(pb, brs, t0 + g + k + l_lo + W - 1, G.T, xb[k]);
#pragma unroll
                for (int k = 0; k < UL; ++k) {
                    const int u = g + k;
                    tl_deviations_b<V, INDEX>(xb[k], cb, rb[(u + W - 1) % W], rp[(u + W - 1) % W]);
                    double da[V];
                    uint32_t qa[NP];
                    tl_deviations<V>(xa[k], ca, da, qa);
#pragma unroll
                    for (int w = 0; w < W; ++w) tl_add<V, INDEX>(da, qa, rb[(u + w) % W], rp[(u + w) % W], acc[w], cnt[w]);
                }
                __builtin_amdgcn_sched_barrier(0);          // the next group's loads stay behind these sums: they would cost its registers
            }
        }
    }
    for (int64_t t = i1; t < r1; ++t) tl_row_direct<V, W, INDEX>(G, pa, pb, brs, ca, cb, t, l_lo, nw, acc, cnt);
}

template <int V, int W, bool INDEX, bool SPLIT>
__global__ void __launch_bounds__(TL_THREADS, tl_waves(V, W, INDEX, SPLIT)) time_lag_kernel(TlGeom G, const float *__restrict__ a, const float *__restrict__ b,
                                                             const float *__restrict__ center_a, const float *__restrict__ center_b,
                                                             double *__restrict__ psum, int32_t *__restrict__ pcnt,
                                                             float *__restrict__ out, int32_t *__restrict__ count) {
    constexpr int NP = (V + 1) / 2;
    const int64_t slabs_t = SPLIT ? G.n_slab : 1;       // slabs that are tiles of their own
    for (int64_t tile = blockIdx.x; tile < G.A.nblk; tile += gridDim.x) {
        const int lb = (int)(tile % G.n_lb);
        const int64_t rest = tile / G.n_lb;
        const int64_t slab_t = rest % slabs_t, ct = rest / slabs_t;
        const int64_t q = ct * TL_THREADS + threadIdx.x;
        if (q >= G.A.ncol) continue;
        int64_t soff, ooff, coff;
        flat_offsets<V, false>(G.A.n_inner, G.A.ext, q, Strided{G.A.sst, soff}, Strided{G.A.ost, ooff}, Strided{G.cst, coff});
        const int64_t cs = G.A.n_inner ? G.cst[G.A.n_inner - 1] : 1;
        float ca[V], cb[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            ca[v] = G.has_ca ? center_a[coff + v * cs] : 0.f;
            cb[v] = G.has_cb ? (INDEX ? center_b[0] : center_b[coff + v * cs]) : 0.f;
        }
        const float *pa = a + soff;
        const float *pb = INDEX ? b : b + soff;
        const int64_t brs = INDEX ? 1 : G.A.src_row_stride;
        const int i_lo = lb * G.lag_block;                              // the first lag of this pass
        const int left = G.n_lags - i_lo, nw = left < G.lag_block ? left : G.lag_block;
        const int64_t l_lo = G.lag0 + i_lo * G.lag_step;

        double acc[W][V];
        uint32_t cnt[W][NP];
        auto clear = [&]() {
#pragma unroll
            for (int w = 0; w < W; ++w) {
#pragma unroll
                for (int v = 0; v < V; ++v) acc[w][v] = 0.0;
#pragma unroll
                for (int j = 0; j < NP; ++j) cnt[w][j] = 0;
            }
        };
        if constexpr (SPLIT) {
            clear();
            const int64_t r0 = slab_t * TL_SLAB, r1 = r0 + TL_SLAB < G.T ? r0 + TL_SLAB : G.T;
            tl_slab<V, W, INDEX>(G, pa, pb, brs, ca, cb, r0, r1, l_lo, nw, acc, cnt);
            // psum / pcnt [slab][lag][element]
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (w < nw) {
                    const int64_t at = (slab_t * G.n_lags + i_lo + w) * G.inner + q * V;
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        psum[at + v] = acc[w][v];
                        pcnt[at + v] = (int32_t)((cnt[w][v >> 1] >> (16 * (v & 1))) & 0xffffu);
                    }
                }
        } else {
            double tot[W][V];
            int32_t n[W][V];
#pragma unroll
            for (int w = 0; w < W; ++w)
#pragma unroll
                for (int v = 0; v < V; ++v) { tot[w][v] = 0.0; n[w][v] = 0; }
            for (int64_t r0 = 0; r0 < G.T; r0 += TL_SLAB) {
                clear();
                tl_slab<V, W, INDEX>(G, pa, pb, brs, ca, cb, r0, r0 + TL_SLAB < G.T ? r0 + TL_SLAB : G.T, l_lo, nw, acc, cnt);
#pragma unroll
                for (int w = 0; w < W; ++w)
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        tot[w][v] += acc[w][v];
                        n[w][v] += (int32_t)((cnt[w][v >> 1] >> (16 * (v & 1))) & 0xffffu);
                    }
            }
            const int64_t st = G.A.last_out_stride();
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (w < nw) {
                    const int64_t need = tl_need(G, l_lo + w * G.lag_step);
                    float res[V];
#pragma unroll
                    for (int v = 0; v < V; ++v) res[v] = tl_value(tot[w][v], n[w][v], need);
                    const int64_t at = (i_lo + w) * G.A.out_row_stride + ooff;
                    store_chunk<V>(out + at, res, G.out_vec != 0, st);
                    if (count) store_chunk<V>(count + at, n[w], G.out_vec != 0, st);
                }
        }
    }
}

// launch 2 (split = 1): one element and lag per lane; the slab sums added in slab order from zero, as the walking lane adds them.
// G.A counts elements here (V = 1).
__global__ void __launch_bounds__(256) time_lag_finish_kernel(TlGeom G, const double *__restrict__ psum, const int32_t *__restrict__ pcnt,
                                                             float *__restrict__ out, int32_t *__restrict__ count) {
    const int64_t total = (int64_t)G.n_lags * G.inner;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t e = i % G.inner, lag = i / G.inner;
        double tot = 0.0;
        int32_t n = 0;
        for (int64_t s = 0; s < G.n_slab; ++s) {
            tot += psum[(s * G.n_lags + lag) * G.inner + e];
            n += pcnt[(s * G.n_lags + lag) * G.inner + e];
        }
        int64_t soff, ooff;
        rows_offsets<1, false>(G.A, e, soff, ooff);
        const int64_t at = lag * G.A.out_row_stride + ooff;
        out[at] = tl_value(tot, n, tl_need(G, G.lag0 + lag * G.lag_step));
        if (count) count[at] = n;
    }
}

struct TlPlan {
    TlGeom G;
    int form, cls;
    bool vec;
    int64_t inner, grid, finish_grid;
    size_t psum_bytes, pcnt_bytes;
};

int tl_class(int block) { return block <= 1 ? 1 : (block <= 4 ? 4 : (block <= 8 ? 8 : 16)); }

// lags per pass, passes, tiles and the split for a chunk of V elements
void tl_shape(TlGeom &G, int64_t inner, int V, int n_lags, int split, int lag_block) {
    G.A.ncol = inner / V;
    G.A.tiles = (G.A.ncol + TL_THREADS - 1) / TL_THREADS;
    // the lags are spread evenly over the fewest passes the form's widest block allows
    auto blocks = [&](bool sp) {
        if (lag_block > 0) {
            G.lag_block = lag_block < n_lags ? lag_block : n_lags;
        } else {
            // (a longer step loads every partner row by row: 5 passes of 4 lags measured 3.3 ms where 3 passes of 6 took 4.4 ms)
            const int widest = tl_max_block(V, sp), most = G.lag_step > 1 && widest > 4 ? 4 : widest;
            const int passes = (n_lags + most - 1) / most;
            G.lag_block = (n_lags + passes - 1) / passes;
        }
        G.n_lb = (n_lags + G.lag_block - 1) / G.lag_block;
    };
    // one slab (or none: NaN everywhere) is walked whatever was asked for: there is nothing to add up
    blocks(true);
    G.split = G.n_slab < 2 ? 0 : (split >= 0 ? split : (G.A.tiles * G.n_lb < TL_SPLIT_BELOW ? 1 : 0));
    if (!G.split) blocks(false);
    G.A.nblk = G.A.tiles * G.n_lb * (G.split ? G.n_slab : 1);
}

// a, b: looked at for 16-byte alignment only
int tl_plan(const dlwpcs_rows_desc *d, const void *a, const void *b, int form, int64_t n_rows, int64_t lag_step, int n_lags, int split,
            int lag_block, TlPlan &P) {
    TlGeom &G = P.G;
    memset(&G, 0, sizeof(G));
    const int rc = rows_addr_init(d, "time_lag", G.A, P.inner);
    if (rc != DLWPCS_OK) return rc;
    if (form != DLWPCS_LAG_AUTO && form != DLWPCS_LAG_PAIR && form != DLWPCS_LAG_INDEX) return fail(DLWPCS_E_INVALID, "time_lag: form %d", form);
    if (n_rows < 0 || n_rows > 0x7fffffffll) return fail(DLWPCS_E_INVALID, "time_lag: %lld rows", (long long)n_rows);
    if (n_lags < 1 || n_lags > DLWPCS_TIME_LAG_MAX_LAGS)
        return fail(DLWPCS_E_INVALID, "time_lag: %d lags (1 .. %d)", n_lags, DLWPCS_TIME_LAG_MAX_LAGS);
    if (lag_step < 1 || lag_step > (1ll << 31)) return fail(DLWPCS_E_INVALID, "time_lag: lag_step %lld", (long long)lag_step);
    if (split < -1 || split > 1) return fail(DLWPCS_E_INVALID, "time_lag: split %d", split);
    if (lag_block < 0 || lag_block > TL_MAX_BLOCK)
        return fail(DLWPCS_E_INVALID, "time_lag: lag_block %d (1 .. %d, 0: chosen)", lag_block, TL_MAX_BLOCK);
    P.form = form;
    G.T = n_rows;
    G.lag_step = lag_step;
    G.n_lags = n_lags;
    G.inner = P.inner;
    G.n_slab = (n_rows + TL_SLAB - 1) / TL_SLAB;
    bool vec, ovec;
    rows_vector_ok(d, vec, ovec);
    P.vec = vec && aligned16(a) && (form != DLWPCS_LAG_PAIR || aligned16(b));
    G.out_vec = P.vec && ovec ? 1 : 0;                          // (the output's own alignment: the entry point's)
    if (P.vec) G.A.ext[d->n_inner - 1] /= 4;
    tl_shape(G, P.inner, P.vec ? 4 : 1, n_lags, split, lag_block);
    P.cls = tl_class(G.lag_block);
    if (G.A.tiles >= (1ll << 40) || G.A.nblk >= (1ll << 48)) return fail(DLWPCS_E_UNSUPPORTED, "time_lag: too many tiles");
    P.grid = G.A.nblk < TL_SLOTS ? G.A.nblk : TL_SLOTS;
    P.psum_bytes = P.pcnt_bytes = 0;
    P.finish_grid = 0;
    if (G.split) {
        const size_t n = (size_t)G.n_slab * (size_t)n_lags * (size_t)P.inner;
        P.psum_bytes = n * sizeof(double);
        P.pcnt_bytes = n * sizeof(int32_t);
        const int64_t blocks = ((int64_t)n_lags * P.inner + 255) / 256;
        P.finish_grid = blocks < TL_FINISH_BLOCKS ? blocks : TL_FINISH_BLOCKS;
    }
    return DLWPCS_OK;
}

template <int V, int W, bool INDEX>
void tl_launch(const TlPlan &P, const float *a, const float *b, const float *ca, const float *cb, double *psum, int32_t *pcnt, float *out,
               int32_t *count, hipStream_t s) {
    const dim3 grid((unsigned)P.grid), blk(TL_THREADS);
    if (P.G.split) hipLaunchKernelGGL((time_lag_kernel<V, W, INDEX, true>), grid, blk, 0, s, P.G, a, b, ca, cb, psum, pcnt, out, count);
    else hipLaunchKernelGGL((time_lag_kernel<V, W, INDEX, false>), grid, blk, 0, s, P.G, a, b, ca, cb, psum, pcnt, out, count);
}

template <int V, bool INDEX>
void tl_launch_class(const TlPlan &P, const float *a, const float *b, const float *ca, const float *cb, double *psum, int32_t *pcnt,
                     float *out, int32_t *count, hipStream_t s) {
    switch (P.cls) {
    case 1: tl_launch<V, 1, INDEX>(P, a, b, ca, cb, psum, pcnt, out, count, s); break;
    case 4: tl_launch<V, 4, INDEX>(P, a, b, ca, cb, psum, pcnt, out, count, s); break;
    case 8: tl_launch<V, 8, INDEX>(P, a, b, ca, cb, psum, pcnt, out, count, s); break;
    default: tl_launch<V, 16, INDEX>(P, a, b, ca, cb, psum, pcnt, out, count, s); break;
    }
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" size_t dlwpcs_time_lag_scratch_bytes(const dlwpcs_rows_desc *d, int form, int64_t n_rows, int64_t lag_step, int n_lags, int split,
                                                int lag_block) {
    // sized for either load width (the pointers' alignment is not known here): the slab sums if either would split
    static const float some[8] = {0.f};
    const void *al = (const void *)(((uintptr_t)some + 15) & ~(uintptr_t)15), *un = (const char *)al + 4;
    size_t need = 0;
    for (const void *p : {al, un}) {
        TlPlan P;
        if (tl_plan(d, p, form == DLWPCS_LAG_AUTO ? nullptr : p, form, n_rows, lag_step, n_lags, split, lag_block, P) != DLWPCS_OK) return 0;
        if (P.psum_bytes + P.pcnt_bytes > need) need = P.psum_bytes + P.pcnt_bytes;
    }
    return need;
}

extern "C" int dlwpcs_time_lag(const dlwpcs_rows_desc *d, const float *a, const float *b, int form, int64_t n_rows, int64_t lag0,
                               int64_t lag_step, int n_lags, const float *center_a, const float *center_b, const int64_t *center_stride,
                               int mode, int min_count, int split, int lag_block, float *out, int32_t *count, void *scratch,
                               size_t scratch_bytes, dlwpcs_stream_t stream) {
    TlPlan P;
    const int rc = tl_plan(d, a, b, form, n_rows, lag_step, n_lags, split, lag_block, P);
    if (rc != DLWPCS_OK) return rc;
    if (mode != DLWPCS_LAG_SKIP && mode != DLWPCS_LAG_PROPAGATE) return fail(DLWPCS_E_INVALID, "time_lag: mode %d", mode);
    if (min_count < 0) return fail(DLWPCS_E_INVALID, "time_lag: min_count %d", min_count);
    if (lag0 < -(1ll << 40) || lag0 > (1ll << 40)) return fail(DLWPCS_E_INVALID, "time_lag: lag0 %lld", (long long)lag0);
    if ((form == DLWPCS_LAG_AUTO) != (b == nullptr) && n_rows > 0 && P.inner > 0)
        return fail(DLWPCS_E_INVALID, "time_lag: the auto form takes b = NULL, the pair and index forms a second operand");
    if (P.inner == 0) return DLWPCS_OK;
    if (!out || (n_rows > 0 && !a)) return fail(DLWPCS_E_INVALID, "time_lag: null operand");
    if ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)center_a) | ((uintptr_t)center_b) | ((uintptr_t)out) | ((uintptr_t)count)) & 3)
        return fail(DLWPCS_E_INVALID, "time_lag: an operand is not aligned to its 4-byte elements");
    TlGeom &G = P.G;
    if (P.psum_bytes && (!scratch || (((uintptr_t)scratch) & 7) || scratch_bytes < P.psum_bytes + P.pcnt_bytes))
        return fail(DLWPCS_E_INVALID, "time_lag: this call needs an 8-byte aligned scratch of %zu bytes", P.psum_bytes + P.pcnt_bytes);
    G.lag0 = lag0;
    G.mode = mode;
    G.min_count = min_count;
    G.has_ca = center_a ? 1 : 0;
    G.has_cb = center_b ? 1 : 0;
    for (int i = 0; i < d->n_inner; ++i) G.cst[i] = center_stride ? center_stride[i] : d->out_stride[i];
    if (!(aligned16(out) && (!count || aligned16(count)))) G.out_vec = 0;
    if (form == DLWPCS_LAG_AUTO) {
        b = a;
        if (!center_b) { center_b = center_a; G.has_cb = G.has_ca; }
    }
    double *psum = (double *)scratch;
    int32_t *pcnt = (int32_t *)((char *)scratch + P.psum_bytes);
    hipStream_t s = (hipStream_t)stream;
    const bool index = form == DLWPCS_LAG_INDEX;
    if (P.vec) {
        if (index) tl_launch_class<4, true>(P, a, b, center_a, center_b, psum, pcnt, out, count, s);
        else tl_launch_class<4, false>(P, a, b, center_a, center_b, psum, pcnt, out, count, s);
    } else {
        if (index) tl_launch_class<1, true>(P, a, b, center_a, center_b, psum, pcnt, out, count, s);
        else tl_launch_class<1, false>(P, a, b, center_a, center_b, psum, pcnt, out, count, s);
    }
    if (P.finish_grid) {
        TlGeom F = G;                                           // one element per lane
        if (P.vec) F.A.ext[F.A.n_inner - 1] *= 4;
        F.A.ncol = P.inner;
        hipLaunchKernelGGL(time_lag_finish_kernel, dim3((unsigned)P.finish_grid), dim3(256), 0, s, F, psum, pcnt, out, count);
    }
    return check_launch("time_lag");
}

extern "C" int dlwpcs_time_lag_plan_info(const dlwpcs_rows_desc *d, const void *a, const void *b, int form, int64_t n_rows,
                                         int64_t lag_step, int n_lags, int split, int lag_block, int64_t info[8]) {
    if (!info) return fail(DLWPCS_E_INVALID, "time_lag_plan_info: null info");
    TlPlan P;
    const int rc = tl_plan(d, a, b, form, n_rows, lag_step, n_lags, split, lag_block, P);
    if (rc != DLWPCS_OK) return rc;
    const bool empty = P.inner == 0;
    if (!empty && n_rows > 0 && !a) return fail(DLWPCS_E_INVALID, "time_lag: null operand");
    info[0] = P.G.lag_block;
    info[1] = P.G.n_lb;
    info[2] = P.vec ? 4 : 1;
    info[3] = P.G.n_slab;
    info[4] = P.G.split;
    info[5] = empty ? 0 : P.G.A.nblk;
    info[6] = empty ? 0 : P.grid;
    info[7] = (int64_t)(P.psum_bytes + P.pcnt_bytes);
    return DLWPCS_OK;
}
