// Rank statistics along the row axis (dlwpcs_time_rank): per row the counts of smaller and equal values of its column (the
// mid-rank), per column the counts of concordant, discordant and tied pairs of rows.  include/dlwpcs.h states the definition; every
// result is an integer (the mid-rank: an exact fp32), so every plan below gives the same bits.
//
// A workgroup of eight waves owns a column tile: two waves a SIMD, which the one workgroup that a 160 KB tile admits to a compute
// unit needs to issue a vector instruction every 2 cycles.  Staged: the tile (and b's, in the pair form) is copied into LDS once, row
// t of the tile's TC columns contiguous, so a lane per column reads row j without a bank conflict; a missing row (NaN in a, or in its
// partner) is staged as NaN in both, after which every comparison with it is false and it takes part in no count.  Direct: the same
// loops read memory, a lane's column coalesced across the 64 lanes, and mask on the fly.  TC is 64, 32 or 16: with fewer columns
// than lanes the 64 / TC sub-groups of a wave take neighbouring blocks of rows and read the same row j (a broadcast).
//
// A lane holds RK_IB rows i of its column in registers, so one read of row j serves RK_IB comparisons.  The rows are dealt out in
// super-blocks (RK_IB rows per sub-group) round robin over the waves of the tile's `splits` workgroups; the j loop is uniform over
// a wave.  Ranks: every i meets every j, and the rows are written as they finish: a split needs no partial.  Statistics: the
// triangular loop j > i; the first rows of it, inside the super-block, carry the predicate j > i, the rest run bare.  eq per row is
// not needed for tie3: a tie group of g rows has, in row order, g-1, g-2, .. 0 equal rows BEHIND each member, and
// g(g-1)(2g+5) = sum over k < g of 6k(k+2), so tie3 = sum over i of 6 e(e+2) with e the equal rows behind i, which the triangular
// loop counts anyway.  Per lane: n_valid of its rows, concordant, discordant, both-tied, the sums of e for a and b and the two tie3
// sums; the lanes of a column are joined through LDS and stored (splits == 1) or left in scratch as eight int64 per (split, column)
// for the finishing launch.  The index-form partner b[j] has a uniform address: it is fetched into scalar registers.
//
// No profiler tags: the launch profiler's registry is the convolution family's, as for the other verification kernels.
#include <string.h>
#include "strided.h"

namespace dlwpcs {

namespace {

constexpr int RK_THREADS = 512;                     // two waves a SIMD: one alone issues a vector instruction every 4 cycles, not 2
constexpr int RK_WAVES = RK_THREADS / 64;
constexpr int RK_IB = 8;                            // rows i a lane holds in registers
constexpr int RK_UNROLL = 4;                        // rows j in flight
constexpr int RK_STAGE_UNROLL = 4;
constexpr int RK_RAW = 8;                           // int64 per (split, column) partial
constexpr int RK_LDS_FULL = 40960;                  // floats: 160 KB, one workgroup per CU
constexpr int RK_LDS_SMALL = 10240;                 // 40 KB: four workgroups per CU for short series
constexpr int RK_LDS_JOIN = RK_THREADS * RK_RAW * 2;   // floats the join of the partials needs
constexpr int64_t RK_CUS = 256;                     // placement only, no bit depends on it
constexpr int64_t RK_MAX_SPLITS = 4096;
constexpr int64_t RK_FINISH_THREADS = 256;
constexpr int64_t RK_MAX_GRID = 1 << 22;              // work items of a launch: one grid dimension, 2^22 x 512 work-items fit 32 bits

enum { RK_NV, RK_CONC, RK_DISC, RK_BOTH, RK_SEA, RK_SEB, RK_T3A, RK_T3B };

struct RkGeom {
    RowsAddr A;                                     // nblk: work items (tile, split), one workgroup each; ncol: chunks per row
    int64_t inner;                                  // elements per row
    int64_t stat_stride;
    int64_t splits;
    int32_t T, missing;
};

struct RkPtrs {
    const float *a, *b;
    float *rank_a, *rank_b;
    int64_t *stats, *scratch;
};

// the column of one lane: get(j) gives row j of a and of its partner, both NaN where the row is missing
template <int FORM, int TC, bool STAGED>
struct RkColumn {
    const float *a, *b;                             // staged: the lane's column of the tile(s); direct: of the operands
    const float *bv;                                // the index form's vector
    int64_t stride;                                 // direct: the source's row stride
    __device__ __forceinline__ void get(int32_t j, float &x, float &y) const {
        y = 0.f;
        if constexpr (STAGED) {
            x = a[j * TC];
            if constexpr (FORM == DLWPCS_RANK_PAIR) y = b[j * TC];
            if constexpr (FORM == DLWPCS_RANK_INDEX) y = x != x ? quiet_nan() : bv[j];   // (the vector is shared: masked per column here)
        } else {
            x = a[(int64_t)j * stride];
            if constexpr (FORM == DLWPCS_RANK_PAIR) y = b[(int64_t)j * stride];
            if constexpr (FORM == DLWPCS_RANK_INDEX) y = bv[j];
            if constexpr (FORM != DLWPCS_RANK_TREND) {
                const bool miss = x != x || y != y;
                x = miss ? quiet_nan() : x;
                y = miss ? quiet_nan() : y;
            }
        }
    }
};

// the tile of column tile ct into LDS: sa[t * TC + c], and sb likewise in the pair form; columns past the last are all NaN
template <int FORM, int TC, int V>
__device__ __forceinline__ void rk_stage(const RkGeom &G, const RkPtrs &P, int64_t ct, float *sa, float *sb) {
    constexpr int CH = TC / V;                      // chunks of a tile row
    constexpr int RPP = RK_THREADS / CH;            // rows staged per pass of the workgroup
    const int sc = threadIdx.x % CH, sr = threadIdx.x / CH;
    const int64_t q = ct * CH + sc;
    const bool ok = q < G.A.ncol;
    int64_t soff = 0, ooff;
    if (ok) rows_offsets<V, false>(G.A, q, soff, ooff);
    for (int32_t r0 = sr; r0 < G.T; r0 += RPP * RK_STAGE_UNROLL) {
        float x[RK_STAGE_UNROLL][V], y[RK_STAGE_UNROLL][V], h[RK_STAGE_UNROLL];
#pragma unroll
        for (int u = 0; u < RK_STAGE_UNROLL; ++u) {
            const int32_t r = r0 + u * RPP;
#pragma unroll
            for (int k = 0; k < V; ++k) x[u][k] = y[u][k] = quiet_nan();
            h[u] = 0.f;
            if (ok && r < G.T) {
                load_chunk<V>(P.a + soff + (int64_t)r * G.A.src_row_stride, x[u]);
                if constexpr (FORM == DLWPCS_RANK_PAIR) load_chunk<V>(P.b + soff + (int64_t)r * G.A.src_row_stride, y[u]);
                if constexpr (FORM == DLWPCS_RANK_INDEX) h[u] = P.b[r];
            }
        }
#pragma unroll
        for (int u = 0; u < RK_STAGE_UNROLL; ++u) {
            const int32_t r = r0 + u * RPP;
            if (r < G.T) {
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    bool miss = x[u][k] != x[u][k];
                    if constexpr (FORM == DLWPCS_RANK_PAIR) miss = miss || y[u][k] != y[u][k];
                    if constexpr (FORM == DLWPCS_RANK_INDEX) miss = miss || h[u] != h[u];
                    sa[r * TC + sc * V + k] = miss ? quiet_nan() : x[u][k];
                    if constexpr (FORM == DLWPCS_RANK_PAIR) sb[r * TC + sc * V + k] = miss ? quiet_nan() : y[u][k];
                }
            }
        }
    }
}

// what a lane is: its column of the tile, its sub-group of the wave, its column's offsets
template <int FORM, int TC, int LDSF, int V>
struct RkLane {
    static constexpr bool STAGED = LDSF > 0;
    static constexpr int SG = 64 / TC;              // sub-groups of a wave
    static constexpr int SBR = RK_IB * SG;          // rows of a super-block
    static constexpr int ROWS = STAGED ? LDSF / (TC * (FORM == DLWPCS_RANK_PAIR ? 2 : 1)) : 0;
    RkColumn<FORM, TC, STAGED> col;
    int64_t ooff;
    int64_t first_wave, n_waves;                    // this wave among those that share the tile's rows
    int c, sub;
    bool active;
};

template <int FORM, int TC, int LDSF, int V>
__device__ __forceinline__ void rk_lane_init(const RkGeom &G, const RkPtrs &P, float *lds, int64_t item, RkLane<FORM, TC, LDSF, V> &L) {
    using Lane = RkLane<FORM, TC, LDSF, V>;
    const int64_t ct = item / G.splits, sp = item - ct * G.splits;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    L.c = lane % TC;
    L.sub = lane / TC;
    L.first_wave = sp * RK_WAVES + wave;
    L.n_waves = G.splits * RK_WAVES;
    const int64_t e = ct * TC + L.c;
    L.active = e < G.inner;
    const int64_t ee = L.active ? e : G.inner - 1;  // (an idle lane of the direct form reads the last column and stores nothing)
    int64_t soff;
    rows_offsets<V, false>(G.A, ee / V, soff, L.ooff);
    soff += (ee % V) * (G.A.n_inner ? G.A.sst[G.A.n_inner - 1] : 1);
    L.ooff += (ee % V) * G.A.last_out_stride();
    L.col.bv = P.b;
    L.col.stride = G.A.src_row_stride;
    if constexpr (Lane::STAGED) {
        float *sa = lds, *sb = lds + Lane::ROWS * TC;
        rk_stage<FORM, TC, V>(G, P, ct, sa, sb);
        __syncthreads();
        L.col.a = sa + L.c;
        L.col.b = sb + L.c;
    } else {
        L.col.a = P.a + soff;
        L.col.b = P.b + soff;
    }
}

// the RK_IB rows from i0 on; rows past the series are missing rows
template <class Column>
__device__ __forceinline__ void rk_load_block(const Column &col, int32_t i0, int32_t T, float ai[RK_IB], float bi[RK_IB]) {
#pragma unroll
    for (int u = 0; u < RK_IB; ++u) {
        ai[u] = bi[u] = quiet_nan();
        if (i0 + u < T) col.get(i0 + u, ai[u], bi[u]);
    }
}

// Per-row outputs: every row i of the lane against every row j
template <int FORM, int TC, int LDSF, int V, bool WB>
__global__ void __launch_bounds__(RK_THREADS) rank_rows_kernel(RkGeom G, RkPtrs P) {
    using Lane = RkLane<FORM, TC, LDSF, V>;
    __shared__ __align__(16) float s_lds[LDSF > 0 ? LDSF : 4];
    const int32_t T = G.T;
    const int64_t nsb = (T + Lane::SBR - 1) / Lane::SBR;
    const int64_t item = blockIdx.x;                // (one grid dimension: the plan admits at most RK_MAX_GRID work items)
    Lane L;
    rk_lane_init<FORM, TC, LDSF, V>(G, P, s_lds, item, L);
    for (int64_t sb = L.first_wave; sb < nsb; sb += L.n_waves) {
        const int32_t i0 = (int32_t)sb * Lane::SBR + L.sub * RK_IB;
        float ai[RK_IB], bi[RK_IB];
        rk_load_block(L.col, i0, T, ai, bi);
        int32_t lta[RK_IB], eqa[RK_IB], ltb[RK_IB], eqb[RK_IB];
#pragma unroll
        for (int u = 0; u < RK_IB; ++u) lta[u] = eqa[u] = ltb[u] = eqb[u] = 0;
        int32_t present = 0;
#pragma unroll RK_UNROLL
        for (int32_t j = 0; j < T; ++j) {
            float x, y;
            L.col.get(j, x, y);
            present += x == x ? 1 : 0;
#pragma unroll
            for (int u = 0; u < RK_IB; ++u) {
                lta[u] += x < ai[u] ? 1 : 0;
                eqa[u] += x == ai[u] ? 1 : 0;
                if constexpr (WB) {
                    ltb[u] += y < bi[u] ? 1 : 0;
                    eqb[u] += y == bi[u] ? 1 : 0;
                }
            }
        }
        if (!L.active) continue;
        const bool spoiled = G.missing == DLWPCS_RANK_PROPAGATE && present < T;
#pragma unroll
        for (int u = 0; u < RK_IB; ++u) {
            if (i0 + u < T) {
                const bool ok = ai[u] == ai[u] && !spoiled;
                const int64_t o = (int64_t)(i0 + u) * G.A.out_row_stride + L.ooff;
                if (P.rank_a) P.rank_a[o] = ok ? (float)lta[u] + 0.5f * (float)(eqa[u] + 1) : quiet_nan();
                if constexpr (WB) P.rank_b[o] = ok ? (float)ltb[u] + 0.5f * (float)(eqb[u] + 1) : quiet_nan();
            }
        }
    }
}

struct RkPart {
    int32_t nv, conc, disc, both, sea, seb;
    int64_t t3a, t3b;
};

// one pair (i, j), j behind i; PRED: only where the lane's row lies before j
template <int FORM, bool PRED>
__device__ __forceinline__ void rk_pair(RkPart &p, bool before, float ai, float bi, float x, float y, int32_t &ea, int32_t &eb) {
    bool la = ai < x, ga = ai > x, qa = ai == x;
    if constexpr (PRED) {
        la = la && before;
        ga = ga && before;
        qa = qa && before;
    }
    ea += qa ? 1 : 0;
    if constexpr (FORM == DLWPCS_RANK_TREND) {      // the partner is the row number: always rising
        p.conc += la ? 1 : 0;
        p.disc += ga ? 1 : 0;
    } else {
        const bool lb = bi < y, gb = bi > y, qb = bi == y;
        p.conc += (la && lb) || (ga && gb) ? 1 : 0;
        p.disc += (la && gb) || (ga && lb) ? 1 : 0;
        p.both += qa && qb ? 1 : 0;
        eb += (PRED ? qb && before : qb) ? 1 : 0;
    }
}

// the statistics of a column from the sums of its lanes
__device__ __forceinline__ void rk_store_stats(const RkGeom &G, const RkPtrs &P, int64_t ooff, const int64_t r[RK_RAW]) {
    const bool spoiled = G.missing == DLWPCS_RANK_PROPAGATE && r[RK_NV] < G.T;
    int64_t v[DLWPCS_RANK_STATS];
    v[0] = r[RK_NV];
    v[1] = r[RK_CONC];
    v[2] = r[RK_DISC];
    v[3] = r[RK_SEA] - r[RK_BOTH];
    v[4] = r[RK_SEB] - r[RK_BOTH];
    v[5] = r[RK_BOTH];
    v[6] = r[RK_T3A];
    v[7] = r[RK_T3B];
#pragma unroll
    for (int k = 0; k < DLWPCS_RANK_STATS; ++k) P.stats[(int64_t)k * G.stat_stride + ooff] = k && spoiled ? -1 : v[k];
}

// Statistics: every pair i < j once
template <int FORM, int TC, int LDSF, int V>
__global__ void __launch_bounds__(RK_THREADS) rank_stats_kernel(RkGeom G, RkPtrs P) {
    using Lane = RkLane<FORM, TC, LDSF, V>;
    __shared__ __align__(16) float s_lds[LDSF > RK_LDS_JOIN ? LDSF : RK_LDS_JOIN];
    const int32_t T = G.T;
    const int64_t nsb = (T + Lane::SBR - 1) / Lane::SBR;
    const int64_t item = blockIdx.x;                // (one grid dimension: the plan admits at most RK_MAX_GRID work items)
    Lane L;
    rk_lane_init<FORM, TC, LDSF, V>(G, P, s_lds, item, L);
    RkPart p = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t sb = L.first_wave; sb < nsb; sb += L.n_waves) {
        const int32_t s0 = (int32_t)sb * Lane::SBR;
        const int32_t i0 = s0 + L.sub * RK_IB;
        float ai[RK_IB], bi[RK_IB];
        rk_load_block(L.col, i0, T, ai, bi);
        int32_t ea[RK_IB], eb[RK_IB];
#pragma unroll
        for (int u = 0; u < RK_IB; ++u) {
            ea[u] = eb[u] = 0;
            p.nv += ai[u] == ai[u] ? 1 : 0;
        }
        const int32_t je = s0 + Lane::SBR < T ? s0 + Lane::SBR : T;
        for (int32_t j = s0 + 1; j < je; ++j) {
            float x, y;
            L.col.get(j, x, y);
#pragma unroll
            for (int u = 0; u < RK_IB; ++u) rk_pair<FORM, true>(p, i0 + u < j, ai[u], bi[u], x, y, ea[u], eb[u]);
        }
#pragma unroll RK_UNROLL
        for (int32_t j = je; j < T; ++j) {
            float x, y;
            L.col.get(j, x, y);
#pragma unroll
            for (int u = 0; u < RK_IB; ++u) rk_pair<FORM, false>(p, true, ai[u], bi[u], x, y, ea[u], eb[u]);
        }
#pragma unroll
        for (int u = 0; u < RK_IB; ++u) {
            p.sea += ea[u];
            p.seb += eb[u];
            p.t3a += 6 * (int64_t)ea[u] * (ea[u] + 2);
            p.t3b += 6 * (int64_t)eb[u] * (eb[u] + 2);
        }
    }
    // the lanes of a column: thread g * TC + c holds part g of column c
    __syncthreads();                                // the tile's readers are done
    int64_t *sj = reinterpret_cast<int64_t *>(s_lds);
    const int64_t mine[RK_RAW] = {p.nv, p.conc, p.disc, p.both, p.sea, p.seb, p.t3a, p.t3b};
#pragma unroll
    for (int k = 0; k < RK_RAW; ++k) sj[k * RK_THREADS + threadIdx.x] = mine[k];
    __syncthreads();
    if (threadIdx.x < TC && L.active) {
        int64_t r[RK_RAW];
#pragma unroll
        for (int k = 0; k < RK_RAW; ++k) {
            r[k] = 0;
            for (int g = 0; g < RK_THREADS / TC; ++g) r[k] += sj[k * RK_THREADS + g * TC + threadIdx.x];
        }
        if (G.splits == 1) {
            rk_store_stats(G, P, L.ooff, r);
        } else {
            const int64_t ct = item / G.splits, sp = item - ct * G.splits;
#pragma unroll
            for (int k = 0; k < RK_RAW; ++k) P.scratch[(sp * RK_RAW + k) * G.inner + ct * TC + threadIdx.x] = r[k];
        }
    }
}

// one lane per column adds the partials of the splits
template <int V>
__global__ void __launch_bounds__(RK_FINISH_THREADS) rank_finish_kernel(RkGeom G, RkPtrs P) {
    for (int64_t e = (int64_t)blockIdx.x * RK_FINISH_THREADS + threadIdx.x; e < G.inner; e += (int64_t)gridDim.x * RK_FINISH_THREADS) {
        int64_t r[RK_RAW];
#pragma unroll
        for (int k = 0; k < RK_RAW; ++k) r[k] = 0;
        for (int64_t sp = 0; sp < G.splits; ++sp) {
#pragma unroll
            for (int k = 0; k < RK_RAW; ++k) r[k] += P.scratch[(sp * RK_RAW + k) * G.inner + e];
        }
        int64_t soff, ooff;
        rows_offsets<V, false>(G.A, e / V, soff, ooff);
        ooff += (e % V) * G.A.last_out_stride();
        rk_store_stats(G, P, ooff, r);
    }
}

struct RkClass {
    int tc, ldsf;
};
// in the order of preference: the row caps are ldsf / tc (the pair form: half)
constexpr RkClass RK_CLASSES[4] = {{64, RK_LDS_SMALL}, {64, RK_LDS_FULL}, {32, RK_LDS_FULL}, {16, RK_LDS_FULL}};
static_assert(RK_LDS_SMALL / 64 == DLWPCS_RANK_STAGE_ROWS_SMALL && RK_LDS_FULL / 64 == DLWPCS_RANK_STAGE_ROWS_64 &&
              RK_LDS_FULL / 32 == DLWPCS_RANK_STAGE_ROWS_32 && RK_LDS_FULL / 16 == DLWPCS_RANK_STAGE_ROWS_16, "the header's row caps");
static_assert(RK_LDS_FULL * 4 <= 160 * 1024 && RK_LDS_JOIN <= RK_LDS_SMALL, "LDS of gfx950; the join fits the smallest tile");

struct RkPlan {
    RkGeom G;
    int staged;                                         // 1 staged, 0 direct
    int cls;                                            // index into RK_CLASSES (staged)
    int tc, rows, v;
    int64_t tiles, items, nblk, finish_blk;         // nblk, finish_blk: workgroups of the main and the finishing launch
    int launches;
    size_t scratch_bytes;
};

// the plan of one launch family: per_row = the ranks, else the statistics
int rk_plan(const dlwpcs_rows_desc *d, const void *a, const void *b, int rank_form, int64_t n_rows, int per_row, int form, int64_t splits,
            RkPlan &P) {
    RkGeom &G = P.G;
    memset(&P, 0, sizeof(P));
    int rc = rows_addr_init(d, "time_rank", G.A, G.inner);
    if (rc != DLWPCS_OK) return rc;
    if (rank_form < DLWPCS_RANK_TREND || rank_form > DLWPCS_RANK_INDEX) return fail(DLWPCS_E_INVALID, "time_rank: rank form %d", rank_form);
    if (form < 0 || form > 2) return fail(DLWPCS_E_INVALID, "time_rank: form %d (0 chosen, 1 staged, 2 direct)", form);
    if (splits < 0 || splits > RK_MAX_SPLITS) return fail(DLWPCS_E_INVALID, "time_rank: splits %lld (0 .. %lld)", (long long)splits,
                                                           (long long)RK_MAX_SPLITS);
    if (n_rows < 0) return fail(DLWPCS_E_INVALID, "time_rank: %lld rows", (long long)n_rows);
    if (n_rows > DLWPCS_RANK_MAX_ROWS) return fail(DLWPCS_E_UNSUPPORTED, "time_rank: %lld rows (at most %d)", (long long)n_rows,
                                                    DLWPCS_RANK_MAX_ROWS);
    P.v = 1;
    if (n_rows == 0 || G.inner == 0) return DLWPCS_OK;
    if ((rank_form == DLWPCS_RANK_TREND) != (b == nullptr))
        return fail(DLWPCS_E_INVALID, "time_rank: b must be given in the pair and index forms and only there");
    if (!a) return fail(DLWPCS_E_INVALID, "time_rank: null operand");
    if ((((uintptr_t)a) | ((uintptr_t)b)) & 3) return fail(DLWPCS_E_INVALID, "time_rank: an operand is not aligned to its 4-byte elements");
    G.T = (int32_t)n_rows;
    const int64_t T = n_rows;
    const int nsrc = rank_form == DLWPCS_RANK_PAIR ? 2 : 1;
    P.cls = -1;
    for (int k = 0; k < 4 && P.cls < 0; ++k)
        if (T <= RK_CLASSES[k].ldsf / (RK_CLASSES[k].tc * nsrc)) P.cls = k;
    if (form == 1 && P.cls < 0) return fail(DLWPCS_E_UNSUPPORTED, "time_rank: %lld rows do not fit the staged form", (long long)T);
    P.staged = form == 2 ? 0 : P.cls >= 0;
    if (P.staged) {
        bool vec, ovec;
        rows_vector_ok(d, vec, ovec);
        if (!aligned16(a) || (rank_form == DLWPCS_RANK_PAIR && !aligned16(b))) vec = false;
        P.v = vec ? 4 : 1;
        P.tc = RK_CLASSES[P.cls].tc;
        P.rows = RK_CLASSES[P.cls].ldsf / (P.tc * nsrc);
    } else {
        P.cls = -1;
        P.tc = 64;
        P.rows = 0;
    }
    if (P.v == 4) G.A.ext[G.A.n_inner - 1] /= 4;
    G.A.ncol = G.inner / P.v;
    P.tiles = (G.inner + P.tc - 1) / P.tc;
    G.A.tiles = P.tiles;
    const int64_t nsb = (T + RK_IB * (64 / P.tc) - 1) / (RK_IB * (64 / P.tc));
    int64_t sp = splits;
    if (sp == 0) {                                      // fill the device, a wave keeping at least one super-block
        const int64_t want = P.staged ? RK_CUS : RK_CUS * 4;
        sp = (want + P.tiles - 1) / P.tiles;
        if (sp > nsb / RK_WAVES) sp = nsb / RK_WAVES;
        if (sp > 256) sp = 256;
        if (sp < 1) sp = 1;
    }
    G.splits = sp;
    if (P.tiles > RK_MAX_GRID / sp) return fail(DLWPCS_E_UNSUPPORTED, "time_rank: %lld column tiles x %lld splits (at most 2^22 work items)",
                                                (long long)P.tiles, (long long)sp);
    P.items = P.tiles * sp;
    G.A.nblk = P.items;
    P.nblk = P.items;
    P.finish_blk = (G.inner + RK_FINISH_THREADS - 1) / RK_FINISH_THREADS;
    if (P.finish_blk > 65536) P.finish_blk = 65536;     // (its lanes stride over the columns)
    P.launches = !per_row && sp > 1 ? 2 : 1;
    P.scratch_bytes = !per_row && sp > 1 ? (size_t)8 * RK_RAW * sp * G.inner : 0;
    return DLWPCS_OK;
}

template <int FORM, int TC, int LDSF, int V>
void rk_launch_one(const RkPlan &P, const RkPtrs &A, bool per_row, hipStream_t s) {
    const dim3 grid((unsigned)P.nblk), blk(RK_THREADS);
    if (per_row) {
        if constexpr (FORM != DLWPCS_RANK_TREND) {
            if (A.rank_b) {
                hipLaunchKernelGGL((rank_rows_kernel<FORM, TC, LDSF, V, true>), grid, blk, 0, s, P.G, A);
                return;
            }
        }
        hipLaunchKernelGGL((rank_rows_kernel<FORM, TC, LDSF, V, false>), grid, blk, 0, s, P.G, A);
    } else {
        hipLaunchKernelGGL((rank_stats_kernel<FORM, TC, LDSF, V>), grid, blk, 0, s, P.G, A);
    }
}

template <int FORM>
void rk_launch(const RkPlan &P, const RkPtrs &A, bool per_row, hipStream_t s) {
    if (!P.staged) {
        rk_launch_one<FORM, 64, 0, 1>(P, A, per_row, s);
    } else if (P.v == 4) {
        switch (P.cls) {
        case 0: rk_launch_one<FORM, 64, RK_LDS_SMALL, 4>(P, A, per_row, s); break;
        case 1: rk_launch_one<FORM, 64, RK_LDS_FULL, 4>(P, A, per_row, s); break;
        case 2: rk_launch_one<FORM, 32, RK_LDS_FULL, 4>(P, A, per_row, s); break;
        default: rk_launch_one<FORM, 16, RK_LDS_FULL, 4>(P, A, per_row, s); break;
        }
    } else {
        switch (P.cls) {
        case 0: rk_launch_one<FORM, 64, RK_LDS_SMALL, 1>(P, A, per_row, s); break;
        case 1: rk_launch_one<FORM, 64, RK_LDS_FULL, 1>(P, A, per_row, s); break;
        case 2: rk_launch_one<FORM, 32, RK_LDS_FULL, 1>(P, A, per_row, s); break;
        default: rk_launch_one<FORM, 16, RK_LDS_FULL, 1>(P, A, per_row, s); break;
        }
    }
    if (!per_row && P.G.splits > 1) {
        const dim3 grid((unsigned)P.finish_blk), blk((unsigned)RK_FINISH_THREADS);
        if (P.v == 4) hipLaunchKernelGGL((rank_finish_kernel<4>), grid, blk, 0, s, P.G, A);
        else hipLaunchKernelGGL((rank_finish_kernel<1>), grid, blk, 0, s, P.G, A);
    }
}

void rk_launch_form(int rank_form, const RkPlan &P, const RkPtrs &A, bool per_row, hipStream_t s) {
    if (rank_form == DLWPCS_RANK_TREND) rk_launch<DLWPCS_RANK_TREND>(P, A, per_row, s);
    else if (rank_form == DLWPCS_RANK_PAIR) rk_launch<DLWPCS_RANK_PAIR>(P, A, per_row, s);
    else rk_launch<DLWPCS_RANK_INDEX>(P, A, per_row, s);
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" size_t dlwpcs_time_rank_scratch_bytes(const dlwpcs_rows_desc *d, const void *a, const void *b, int rank_form, int64_t n_rows,
                                                 int per_row, int form, int64_t splits) {
    RkPlan P;
    if (rk_plan(d, a, b, rank_form, n_rows, per_row, form, splits, P) != DLWPCS_OK) return 0;
    return P.scratch_bytes;
}

extern "C" int dlwpcs_time_rank(const dlwpcs_rows_desc *d, const float *a, const float *b, int rank_form, int64_t n_rows, int missing,
                                int form, int64_t splits, float *rank_a, float *rank_b, int64_t *stats, int64_t stat_stride,
                                void *scratch, size_t scratch_bytes, dlwpcs_stream_t stream) {
    RkPlan R, S;
    int rc = rk_plan(d, a, b, rank_form, n_rows, 1, form, splits, R);
    if (rc != DLWPCS_OK) return rc;
    rc = rk_plan(d, a, b, rank_form, n_rows, 0, form, splits, S);
    if (rc != DLWPCS_OK) return rc;
    if (missing != DLWPCS_RANK_SKIP && missing != DLWPCS_RANK_PROPAGATE) return fail(DLWPCS_E_INVALID, "time_rank: missing mode %d", missing);
    if (rank_b && rank_form == DLWPCS_RANK_TREND) return fail(DLWPCS_E_INVALID, "time_rank: rank_b in the trend form");
    if (n_rows == 0 || R.G.inner == 0) return DLWPCS_OK;
    if (!rank_a && !rank_b && !stats) return DLWPCS_OK;
    if ((((uintptr_t)rank_a) | ((uintptr_t)rank_b)) & 3 || ((uintptr_t)stats) & 7)
        return fail(DLWPCS_E_INVALID, "time_rank: a result is not aligned to its elements");
    if (stats && S.scratch_bytes && (!scratch || scratch_bytes < S.scratch_bytes || !aligned16(scratch)))
        return fail(DLWPCS_E_INVALID, "time_rank: scratch of %zu bytes on 16 bytes needed, got %zu", S.scratch_bytes, scratch_bytes);
    R.G.missing = S.G.missing = missing;
    S.G.stat_stride = stat_stride;
    const RkPtrs A = {a, b, rank_a, rank_b, stats, (int64_t *)scratch};
    hipStream_t s = (hipStream_t)stream;
    if (rank_a || rank_b) rk_launch_form(rank_form, R, A, true, s);
    if (stats) rk_launch_form(rank_form, S, A, false, s);
    return check_launch("time_rank");
}

extern "C" int dlwpcs_time_rank_plan_info(const dlwpcs_rows_desc *d, const void *a, const void *b, int rank_form, int64_t n_rows,
                                          int per_row, int form, int64_t splits, int64_t info[8]) {
    if (!info) return fail(DLWPCS_E_INVALID, "time_rank_plan_info: null info");
    RkPlan P;
    int rc = rk_plan(d, a, b, rank_form, n_rows, per_row, form, splits, P);
    if (rc != DLWPCS_OK) return rc;
    const bool any = n_rows > 0 && P.G.inner > 0;
    info[0] = any ? (P.staged ? 1 : 2) : 0;
    info[1] = any ? P.tc : 0;
    info[2] = any ? P.rows : 0;
    info[3] = P.v;
    info[4] = any ? P.G.splits : 0;
    info[5] = any ? P.nblk : 0;
    info[6] = any ? P.launches : 0;
    info[7] = (int64_t)P.scratch_bytes;
    return DLWPCS_OK;
}
