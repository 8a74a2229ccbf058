// Spells along the row axis (dlwpcs_time_spell): per column the maximal runs of rows on which x cmp threshold holds, as per-row
// position / length and as per-column statistics.  include/dlwpcs.h states the definition and the combine rule of two adjacent
// runs of rows; every result is an integer, so every form below gives the same bits.
//
// A lane owns one chunk of columns (four with 16-byte loads, else one) and walks rows in order; a wave is a workgroup and a column
// tile is its 64 chunks.  Work items are (column tile, time slab); a fixed number of persistent workgroups strides over them.
//
// Statistics only.  The lane carries the partial (head, tail, n_valid, n_true, cnt, spell_rows, longest, start) of the rows it has
// seen.  One slab: it closes the ends of the series and stores the statistics, one launch at any T.  Several slabs (few column
// tiles): launch 1 stores the partial of every (slab, column), launch 2 joins them in slab order with one lane per column.
//
// Per-row outputs.  A spell's length is known only at its end, so the lane first packs the condition of its slab into W words of
// 32 rows held in registers (W is a template argument and every word loop is unrolled: a register array indexed at run time would
// live in scratch memory), derives per word how many trues follow its last row (backward over the words, starting from the
// carry of the slab behind), and then writes pos and len row by row.  One slab (T <= 32 W): a single launch that also carries the
// partial and stores the statistics.  Several slabs: launch 1 as above, launch 2 also scans the partials forward and backward
// into every slab's carry from before and from after and the column's propagate flag, launch 3 packs each slab again from the
// series (it is read twice; condition bits left in scratch by launch 1 would save that read: not built) and writes the rows.
//
// No profiler tags: the launch profiler's registry is the convolution family's, as for the other verification kernels.
#include <string.h>
#include "strided.h"

namespace dlwpcs {

namespace {

constexpr int SP_THREADS = 64;                      // a workgroup is one wave: no LDS, no barrier
constexpr int SP_UNROLL = 8;                        // rows in flight per lane
constexpr int SP_JOIN_THREADS = 256;
constexpr int SP_JOIN_UNROLL = 4;                   // slabs whose partials are fetched together
constexpr int64_t SP_CUS = 256;                     // compute units: placement only, no bit depends on it
constexpr int64_t SP_SLOTS = SP_CUS * 16;           // persistent workgroups (waves)
constexpr int64_t SP_FILL = SP_CUS * 2;             // work items wanted before a slab grows (rows form)
constexpr int64_t SP_SINGLE_TILES = SP_CUS;         // column tiles from which one slab of up to 1024 rows fills the device
constexpr int64_t SP_SINGLE_ROWS = 128;             // ... and the rows below which one launch wins whatever the tiles
constexpr int64_t SP_STATS_MIN_SLAB = 256;          // rows of a chosen statistics slab at the least
constexpr int SP_MAX_W = 32;
constexpr int SP_VEC_MAX_W = 8;                     // the class cap of the four-column chunk: at 16 the compiler spills
constexpr int SP_FIELDS = 8;

enum { SP_HEAD, SP_TAIL, SP_NVALID, SP_NTRUE, SP_CNT, SP_ROWS, SP_LONGEST, SP_START };
enum { SP_FORM_STATS, SP_FORM_STATS_SLABS, SP_FORM_ROWS, SP_FORM_ROWS_SLABS };

struct SpGeom {
    RowsAddr A;                                     // nblk: workgroups of the launch; ncol: chunks per row
    int64_t tst[DLWPCS_SCORE_MAX_DIMS];             // the threshold's stride per inner dim
    int64_t thr_row_stride, stat_stride;
    int64_t inner;                                  // elements per row
    int64_t items, nslab, slab_rows;
    int64_t min_length;
    int32_t T, cmp, missing;
    int32_t wide, tvec;                             // 16-byte stores / threshold loads
};

struct SpPtrs {
    const float *src, *thr;
    const int32_t *thr_index;
    int32_t *pos, *len, *stats, *scratch;
};

struct SpPart {
    int32_t head, tail, nv, nt, cnt, rows, longest, start;
};

__device__ __forceinline__ void sp_init(SpPart &p) {
    p.head = -1;                                    // (walking: no false row seen yet)
    p.tail = 0;
    p.nv = p.nt = p.cnt = p.rows = p.longest = 0;
    p.start = -1;
}

// a spell of run rows that starts at row start and has a false row (or an end of the series) on both sides; spells close in row order
__device__ __forceinline__ void sp_close(SpPart &p, int32_t run, int32_t start, int64_t min_length) {
    if (run > 0 && (int64_t)run >= min_length) {
        p.cnt += 1;
        p.rows += run;
        if (run > p.longest) {
            p.longest = run;
            p.start = start;
        }
    }
}

// one row of a walk: p.tail is the running count of trues
__device__ __forceinline__ void sp_step(SpPart &p, bool c, bool m, int32_t t, int64_t min_length) {
    p.nv += m ? 0 : 1;
    if (c) {
        p.tail += 1;
        p.nt += 1;
    } else {
        if (p.head < 0) p.head = p.tail;
        else sp_close(p, p.tail, t - p.tail, min_length);
        p.tail = 0;
    }
}

__device__ __forceinline__ void sp_walk_end(SpPart &p) {
    if (p.head < 0) p.head = p.tail;                // all true: head == tail == rows
}

// A (na rows) before B (nb rows, the first of them row b_first): the combine rule of include/dlwpcs.h
__device__ __forceinline__ void sp_join(SpPart &a, int32_t na, const SpPart &b, int32_t nb, int32_t b_first, int64_t min_length) {
    const bool all_a = a.head == na, all_b = b.head == nb;
    a.nv += b.nv;
    a.nt += b.nt;
    if (all_a && all_b) {
        a.head = a.tail = na + nb;
        return;
    }
    if (all_a) {
        a.head = na + b.head;
        a.tail = b.tail;
    } else if (all_b) {
        a.tail += nb;
        return;
    } else {
        sp_close(a, a.tail + b.head, b_first - a.tail, min_length);
        a.tail = b.tail;
    }
    a.cnt += b.cnt;
    a.rows += b.rows;
    if (b.longest > a.longest) {
        a.longest = b.longest;
        a.start = b.start;
    }
}

// the ends of the series close the head (start 0: it wins a tie) and the tail
__device__ __forceinline__ void sp_finish(SpPart &p, int32_t n, int64_t min_length) {
    const int32_t head = p.head, tail = p.head == n ? 0 : p.tail;
    if (head > 0 && (int64_t)head >= min_length) {
        p.cnt += 1;
        p.rows += head;
        if (head >= p.longest) {
            p.longest = head;
            p.start = 0;
        }
    }
    sp_close(p, tail, n - tail, min_length);
}

__device__ __forceinline__ void sp_field(const SpPart &p, int32_t f[SP_FIELDS]) {
    f[SP_HEAD] = p.head; f[SP_TAIL] = p.tail; f[SP_NVALID] = p.nv; f[SP_NTRUE] = p.nt;
    f[SP_CNT] = p.cnt; f[SP_ROWS] = p.rows; f[SP_LONGEST] = p.longest; f[SP_START] = p.start;
}

// the six statistics of a finished column, -1 under propagate where a row is missing
__device__ __forceinline__ void sp_stat_values(const SpPart &p, bool spoiled, int32_t v[6]) {
    v[0] = p.nv;
    v[1] = spoiled ? -1 : p.nt;
    v[2] = spoiled ? -1 : p.cnt;
    v[3] = spoiled ? -1 : p.rows;
    v[4] = spoiled ? -1 : p.longest;
    v[5] = spoiled ? -1 : p.start;
}

// LT and LE are GT and GE of the negated operands (a NaN stays a NaN, the zeros stay equal)
__device__ __forceinline__ void sp_compare(const SpGeom &G, float x, float h, bool &c, bool &m) {
    const uint32_t flip = (G.cmp & 2) ? 0x80000000u : 0u;
    const float a = __uint_as_float(__float_as_uint(x) ^ flip), b = __uint_as_float(__float_as_uint(h) ^ flip);
    c = (G.cmp & 1) ? a >= b : a > b;
    m = isnan(x) || isnan(h);
}

// where this lane's chunk lies in the source, the output and the threshold table
template <int V>
struct SpLane {
    int64_t soff, ooff, toff;
    int64_t tls;                                    // the threshold's stride along the lanes
    float h[V];                                     // the threshold when every row uses table row 0
};

template <int V>
__device__ __forceinline__ void sp_lane_init(const SpGeom &G, const SpPtrs &P, int64_t q, SpLane<V> &L) {
    flat_offsets<V, false>(G.A.n_inner, G.A.ext, q, Strided{G.A.sst, L.soff}, Strided{G.A.ost, L.ooff}, Strided{G.tst, L.toff});
    L.tls = G.A.n_inner ? G.tst[G.A.n_inner - 1] : 0;
#pragma unroll
    for (int j = 0; j < V; ++j) L.h[j] = 0.f;
    if (!P.thr_index) {
#pragma unroll
        for (int j = 0; j < V; ++j) L.h[j] = P.thr[L.toff + j * L.tls];
    }
}

// the thresholds of row t (ti: its table row, uniform)
template <int V>
__device__ __forceinline__ void sp_load_thr(const SpGeom &G, const SpPtrs &P, const SpLane<V> &L, int32_t ti, float h[V]) {
    const float *p = P.thr + (int64_t)ti * G.thr_row_stride + L.toff;
    if constexpr (V == 4) {
        if (G.tvec) {
            load_chunk<4>(p, h);
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) h[j] = p[j * L.tls];
}

// SP_UNROLL rows from t on (those below t_end), loads first: x, and h where the rows have table rows of their own
template <int V>
__device__ __forceinline__ void sp_load_rows(const SpGeom &G, const SpPtrs &P, const SpLane<V> &L, int32_t t, int32_t t_end,
                                             float x[SP_UNROLL][V], float h[SP_UNROLL][V]) {
    const float *p = P.src + L.soff;
#pragma unroll
    for (int u = 0; u < SP_UNROLL; ++u) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            x[u][j] = 0.f;
            h[u][j] = L.h[j];
        }
        if (t + u < t_end) {
            load_chunk<V>(p + (int64_t)(t + u) * G.A.src_row_stride, x[u]);
            if (P.thr_index) sp_load_thr<V>(G, P, L, P.thr_index[t + u], h[u]);
        }
    }
}

__device__ __forceinline__ int32_t *sp_scratch_field(const SpGeom &G, const SpPtrs &P, int f, int64_t slab) {
    return P.scratch + ((int64_t)f * G.nslab + slab) * G.inner;
}
// behind the partials: the carries of every slab and the propagate flag of every column (rows form)
__device__ __forceinline__ int32_t *sp_scratch_before(const SpGeom &G, const SpPtrs &P, int64_t slab) {
    return P.scratch + ((int64_t)SP_FIELDS * G.nslab + slab) * G.inner;
}
__device__ __forceinline__ int32_t *sp_scratch_after(const SpGeom &G, const SpPtrs &P, int64_t slab) {
    return P.scratch + ((int64_t)(SP_FIELDS + 1) * G.nslab + slab) * G.inner;
}
__device__ __forceinline__ int32_t *sp_scratch_flag(const SpGeom &G, const SpPtrs &P) {
    return P.scratch + (int64_t)(SP_FIELDS + 2) * G.nslab * G.inner;
}

template <int V>
__device__ __forceinline__ void sp_store_stats(const SpGeom &G, const SpPtrs &P, int64_t ooff, const SpPart p[V]) {
    int32_t v[V][6];
#pragma unroll
    for (int j = 0; j < V; ++j) sp_stat_values(p[j], G.missing == DLWPCS_SPELL_PROPAGATE && p[j].nv < G.T, v[j]);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        int32_t o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = v[j][k];
        store_chunk<V, int32_t>(P.stats + (int64_t)k * G.stat_stride + ooff, o, G.wide, G.A.last_out_stride());
    }
}

// Statistics only.  SLABS: the partial of every (slab, column) goes to scratch; else the one slab is the series.
template <int V, bool SLABS>
__global__ void __launch_bounds__(SP_THREADS) spell_stats_kernel(SpGeom G, SpPtrs P) {
    for (int64_t item = blockIdx.x; item < G.items; item += G.A.nblk) {
        const int64_t ct = item / G.nslab, slab = item - ct * G.nslab;
        const int64_t q = ct * SP_THREADS + threadIdx.x;
        if (q >= G.A.ncol) continue;
        SpLane<V> L;
        sp_lane_init<V>(G, P, q, L);
        const int32_t t0 = (int32_t)(slab * G.slab_rows);
        const int32_t t1 = (int64_t)t0 + G.slab_rows < G.T ? (int32_t)(t0 + G.slab_rows) : G.T;
        SpPart p[V];
#pragma unroll
        for (int j = 0; j < V; ++j) sp_init(p[j]);
        for (int32_t t = t0; t < t1; t += SP_UNROLL) {
            float x[SP_UNROLL][V], h[SP_UNROLL][V];
            sp_load_rows<V>(G, P, L, t, t1, x, h);
#pragma unroll
            for (int u = 0; u < SP_UNROLL; ++u) {
                if (t + u < t1) {
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        bool c, m;
                        sp_compare(G, x[u][j], h[u][j], c, m);
                        sp_step(p[j], c, m, t + u, G.min_length);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) sp_walk_end(p[j]);
        if constexpr (SLABS) {
            int32_t f[V][SP_FIELDS];
#pragma unroll
            for (int j = 0; j < V; ++j) sp_field(p[j], f[j]);
#pragma unroll
            for (int k = 0; k < SP_FIELDS; ++k) {
                int32_t o[V];
#pragma unroll
                for (int j = 0; j < V; ++j) o[j] = f[j][k];
                store_chunk<V, int32_t>(sp_scratch_field(G, P, k, slab) + q * V, o, true, 1);   // (inner and every field: multiples of 4)
            }
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) sp_finish(p[j], G.T, G.min_length);
            if (P.stats) sp_store_stats<V>(G, P, L.ooff, p);
        }
    }
}

__device__ __forceinline__ void sp_fetch_part(const SpGeom &G, const SpPtrs &P, int64_t slab, int64_t e, SpPart &p) {
    p.head = sp_scratch_field(G, P, SP_HEAD, slab)[e];
    p.tail = sp_scratch_field(G, P, SP_TAIL, slab)[e];
    p.nv = sp_scratch_field(G, P, SP_NVALID, slab)[e];
    p.nt = sp_scratch_field(G, P, SP_NTRUE, slab)[e];
    p.cnt = sp_scratch_field(G, P, SP_CNT, slab)[e];
    p.rows = sp_scratch_field(G, P, SP_ROWS, slab)[e];
    p.longest = sp_scratch_field(G, P, SP_LONGEST, slab)[e];
    p.start = sp_scratch_field(G, P, SP_START, slab)[e];
}

__device__ __forceinline__ int32_t sp_slab_len(const SpGeom &G, int64_t slab) {
    const int64_t t0 = slab * G.slab_rows;
    return (int32_t)(t0 + G.slab_rows < G.T ? G.slab_rows : G.T - t0);
}

// One lane per column joins the partials in slab order and stores the statistics.  CARRIES (rows form): it also stores, per slab,
// the trues that end right before it and those that begin right behind it, and the column's propagate flag.
template <int V, bool CARRIES>
__global__ void __launch_bounds__(SP_JOIN_THREADS) spell_join_kernel(SpGeom G, SpPtrs P) {
    for (int64_t e = (int64_t)blockIdx.x * SP_JOIN_THREADS + threadIdx.x; e < G.inner; e += G.A.nblk * SP_JOIN_THREADS) {
        SpPart acc;
        sp_init(acc);
        int32_t n = 0;
        for (int64_t s0 = 0; s0 < G.nslab; s0 += SP_JOIN_UNROLL) {
            SpPart b[SP_JOIN_UNROLL];
#pragma unroll
            for (int u = 0; u < SP_JOIN_UNROLL; ++u)
                if (s0 + u < G.nslab) sp_fetch_part(G, P, s0 + u, e, b[u]);
#pragma unroll
            for (int u = 0; u < SP_JOIN_UNROLL; ++u) {
                if (s0 + u < G.nslab) {
                    const int32_t nb = sp_slab_len(G, s0 + u);
                    if constexpr (CARRIES) sp_scratch_before(G, P, s0 + u)[e] = n ? acc.tail : 0;
                    if (n == 0) acc = b[u];
                    else sp_join(acc, n, b[u], nb, n, G.min_length);
                    n += nb;
                }
            }
        }
        const bool spoiled = G.missing == DLWPCS_SPELL_PROPAGATE && acc.nv < G.T;
        if constexpr (CARRIES) {
            sp_scratch_flag(G, P)[e] = spoiled ? 1 : 0;
            int32_t after = 0;                                      // the trues that begin at the first row of the slab behind
            for (int64_t s = G.nslab - 1; s >= 0; --s) {
                sp_scratch_after(G, P, s)[e] = after;
                const int32_t nb = sp_slab_len(G, s);
                const int32_t head = sp_scratch_field(G, P, SP_HEAD, s)[e];
                after = head == nb ? nb + after : head;
            }
        }
        if (P.stats) {
            sp_finish(acc, G.T, G.min_length);
            int64_t soff, ooff;
            rows_offsets<V, false>(G.A, e / V, soff, ooff);
            ooff += (e % V) * G.A.last_out_stride();
            int32_t v[6];
            sp_stat_values(acc, spoiled, v);
#pragma unroll
            for (int k = 0; k < 6; ++k) P.stats[(int64_t)k * G.stat_stride + ooff] = v[k];
        }
    }
}

// Per-row outputs of one slab of at most 32 W rows.  SINGLE: the slab is the series, and the statistics are stored here too.
template <int V, int W, bool SINGLE>
__global__ void __launch_bounds__(SP_THREADS) spell_rows_kernel(SpGeom G, SpPtrs P) {
    for (int64_t item = blockIdx.x; item < G.items; item += G.A.nblk) {
        const int64_t ct = item / G.nslab, slab = item - ct * G.nslab;
        const int64_t q = ct * SP_THREADS + threadIdx.x;
        if (q >= G.A.ncol) continue;
        SpLane<V> L;
        sp_lane_init<V>(G, P, q, L);
        const int32_t t0 = (int32_t)(slab * G.slab_rows);
        const int32_t t1 = (int64_t)t0 + G.slab_rows < G.T ? (int32_t)(t0 + G.slab_rows) : G.T;
        uint32_t bits[W][V];
        SpPart p[V];
#pragma unroll
        for (int j = 0; j < V; ++j) sp_init(p[j]);
        // the condition of the slab, 32 rows a word
#pragma unroll
        for (int w = 0; w < W; ++w) {
#pragma unroll
            for (int j = 0; j < V; ++j) bits[w][j] = 0;
            const int32_t tw = t0 + w * 32;
            if (tw < t1) {
#pragma unroll 1
                for (int b0 = 0; b0 < 32; b0 += SP_UNROLL) {
                    float x[SP_UNROLL][V], h[SP_UNROLL][V];
                    sp_load_rows<V>(G, P, L, tw + b0, t1, x, h);
#pragma unroll
                    for (int u = 0; u < SP_UNROLL; ++u) {
                        if (tw + b0 + u < t1) {
#pragma unroll
                            for (int j = 0; j < V; ++j) {
                                bool c, m;
                                sp_compare(G, x[u][j], h[u][j], c, m);
                                bits[w][j] |= (c ? 1u : 0u) << (b0 + u);
                                if constexpr (SINGLE) sp_step(p[j], c, m, tw + b0 + u, G.min_length);
                            }
                        }
                    }
                }
            }
        }
        // the carries of the neighbouring slabs and the propagate flag
        int32_t run[V], after[V];
        bool spoiled[V];
        if constexpr (SINGLE) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                sp_walk_end(p[j]);
                sp_finish(p[j], G.T, G.min_length);
                run[j] = after[j] = 0;
                spoiled[j] = G.missing == DLWPCS_SPELL_PROPAGATE && p[j].nv < G.T;
            }
            if (P.stats) sp_store_stats<V>(G, P, L.ooff, p);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                run[j] = sp_scratch_before(G, P, slab)[q * V + j];
                after[j] = sp_scratch_after(G, P, slab)[q * V + j];
                spoiled[j] = sp_scratch_flag(G, P)[q * V + j] != 0;
            }
        }
        // per word: the trues that follow its last row
        int32_t follow[W][V];
#pragma unroll
        for (int w = W - 1; w >= 0; --w) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                follow[w][j] = after[j];
                const uint32_t inv = ~bits[w][j];
                after[j] = inv ? __builtin_ctz(inv) : 32 + after[j];
            }
        }
        // the rows, in row order
        bool prev[V];
        int32_t cur[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            prev[j] = false;
            cur[j] = 0;
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const int32_t tw = t0 + w * 32;
            if (tw < t1) {
                const int nb = t1 - tw < 32 ? t1 - tw : 32;
                uint32_t word[V];
                int32_t fol[V];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    word[j] = bits[w][j];
                    fol[j] = follow[w][j];
                }
                for (int b = 0; b < nb; ++b) {
                    int32_t vp[V], vl[V];
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        const bool c = (word[j] >> b) & 1u;
                        if (c && !prev[j]) {                        // a spell begins here, or goes on from the slab before
                            const uint32_t inv = ~(word[j] >> b);   // (the zeros shifted in end the count at the word's end)
                            const int32_t ones = inv ? __builtin_ctz(inv) : 32;
                            cur[j] = run[j] + ones + (b + ones == 32 ? fol[j] : 0);
                        }
                        run[j] = c ? run[j] + 1 : 0;
                        prev[j] = c;
                        const bool in = c && (int64_t)cur[j] >= G.min_length;
                        vp[j] = spoiled[j] ? -1 : (in ? run[j] : 0);
                        vl[j] = spoiled[j] ? -1 : (in ? cur[j] : 0);
                    }
                    const int64_t o = (int64_t)(tw + b) * G.A.out_row_stride + L.ooff;
                    if (P.pos) store_chunk<V, int32_t>(P.pos + o, vp, G.wide, G.A.last_out_stride());
                    if (P.len) store_chunk<V, int32_t>(P.len + o, vl, G.wide, G.A.last_out_stride());
                }
            }
        }
    }
}

struct SpPlan {
    SpGeom G;
    int form;
    int w;                                              // register class (rows forms), else 0
    int v;
    int64_t tiles, nblk, join_blk;
    int launches;
    size_t scratch_bytes;
};

inline int sp_class_of(int64_t rows) {
    int w = 1;
    while (32 * w < rows) w *= 2;
    return w;
}

int sp_plan(const dlwpcs_rows_desc *d, const void *src, int64_t n_rows, int64_t slab_rows, int per_row, SpPlan &P) {
    SpGeom &G = P.G;
    memset(&P, 0, sizeof(P));
    int rc = rows_addr_init(d, "time_spell", G.A, G.inner);
    if (rc != DLWPCS_OK) return rc;
    if (n_rows < 0) return fail(DLWPCS_E_INVALID, "time_spell: %lld rows", (long long)n_rows);
    if (n_rows > DLWPCS_SPELL_MAX_ROWS) return fail(DLWPCS_E_UNSUPPORTED, "time_spell: %lld rows (at most 2^31 - 1)", (long long)n_rows);
    if (slab_rows < 0 || slab_rows % 32) return fail(DLWPCS_E_INVALID, "time_spell: slab_rows %lld (0 or a multiple of 32)", (long long)slab_rows);
    if (per_row && slab_rows && (slab_rows > 32 * SP_MAX_W || (slab_rows & (slab_rows - 1))))
        return fail(DLWPCS_E_INVALID, "time_spell: slab_rows %lld with per-row outputs (32, 64, 128, 256, 512 or 1024)", (long long)slab_rows);
    P.form = per_row ? SP_FORM_ROWS : SP_FORM_STATS;
    P.v = 1;
    if (n_rows == 0 || G.inner == 0) return DLWPCS_OK;
    if (((uintptr_t)src) & 3) return fail(DLWPCS_E_INVALID, "time_spell: an operand is not aligned to its 4-byte elements");
    bool vec, ovec;
    rows_vector_ok(d, vec, ovec);
    if (vec && !aligned16(src)) vec = false;
    G.T = (int32_t)n_rows;
    const int64_t T = n_rows;
    if (!per_row) {
        P.v = vec ? 4 : 1;
        P.tiles = (G.inner / P.v + SP_THREADS - 1) / SP_THREADS;
        int64_t sr = slab_rows;
        if (sr == 0) {
            sr = (T + 31) / 32 * 32;                    // one slab
            if (P.tiles < SP_SLOTS && T >= 2 * SP_STATS_MIN_SLAB) {
                int64_t n = (SP_SLOTS + P.tiles - 1) / P.tiles;
                if (n > T / SP_STATS_MIN_SLAB) n = T / SP_STATS_MIN_SLAB;
                if (n > 1) sr = ((T + n - 1) / n + 31) / 32 * 32;
            }
        }
        G.slab_rows = sr;
        G.nslab = (T + sr - 1) / sr;
        P.form = G.nslab > 1 ? SP_FORM_STATS_SLABS : SP_FORM_STATS;
        P.w = 0;
    } else {
        // the four-column chunk holds classes up to SP_VEC_MAX_W; a larger slab takes the one-column chunk
        int w;
        if (slab_rows) {
            w = (int)(slab_rows / 32);
        } else {
            const int cap = vec ? SP_VEC_MAX_W : SP_MAX_W;
            const int64_t vt = (G.inner / (vec ? 4 : 1) + SP_THREADS - 1) / SP_THREADS;
            const int64_t st = (G.inner + SP_THREADS - 1) / SP_THREADS;
            if (T <= 32 * cap && (vt >= SP_SINGLE_TILES || T <= SP_SINGLE_ROWS)) {
                w = sp_class_of(T);
            } else if (T <= 32 * SP_MAX_W && st >= SP_SINGLE_TILES) {
                w = sp_class_of(T);                     // one slab beyond the cap: one launch with the one-column chunk
            } else {
                w = cap;                                // slabs: the largest class that still leaves SP_FILL work items
                while (w > 1 && vt * ((T + 32 * w - 1) / (32 * w)) < SP_FILL) w /= 2;
            }
        }
        if (w > SP_VEC_MAX_W) vec = false;
        P.v = vec ? 4 : 1;
        P.w = w;
        P.tiles = (G.inner / P.v + SP_THREADS - 1) / SP_THREADS;
        G.slab_rows = 32 * (int64_t)w;
        G.nslab = (T + G.slab_rows - 1) / G.slab_rows;
        P.form = G.nslab > 1 ? SP_FORM_ROWS_SLABS : SP_FORM_ROWS;
    }
    if (P.v == 4) G.A.ext[G.A.n_inner - 1] /= 4;
    G.A.ncol = G.inner / P.v;
    G.A.tiles = P.tiles;
    if (P.tiles > MAX_BLOCKS / G.nslab) return fail(DLWPCS_E_UNSUPPORTED, "time_spell: %lld x %lld work items is too many",
                                                     (long long)P.tiles, (long long)G.nslab);
    G.items = P.tiles * G.nslab;
    P.nblk = G.items < SP_SLOTS ? G.items : SP_SLOTS;
    const int64_t jb = (G.inner + SP_JOIN_THREADS - 1) / SP_JOIN_THREADS;
    P.join_blk = jb < SP_SLOTS ? jb : SP_SLOTS;
    G.wide = P.v == 4 && ovec;
    switch (P.form) {
    case SP_FORM_STATS: P.launches = 1; P.scratch_bytes = 0; break;
    case SP_FORM_ROWS: P.launches = 1; P.scratch_bytes = 0; break;
    case SP_FORM_STATS_SLABS: P.launches = 2; P.scratch_bytes = (size_t)4 * SP_FIELDS * G.nslab * G.inner; break;
    default: P.launches = 3; P.scratch_bytes = (size_t)4 * ((SP_FIELDS + 2) * G.nslab + 1) * G.inner; break;
    }
    return DLWPCS_OK;
}

template <int V, int W>
void sp_launch_rows(const SpPlan &P, const SpGeom &G, const SpPtrs &A, hipStream_t s) {
    const dim3 grid((unsigned)P.nblk), blk(SP_THREADS);             // (at most SP_SLOTS workgroups: one grid dimension)
    if (P.form == SP_FORM_ROWS) hipLaunchKernelGGL((spell_rows_kernel<V, W, true>), grid, blk, 0, s, G, A);
    else hipLaunchKernelGGL((spell_rows_kernel<V, W, false>), grid, blk, 0, s, G, A);
}

template <int V>
void sp_launch_rows_class(const SpPlan &P, const SpGeom &G, const SpPtrs &A, hipStream_t s) {
    switch (P.w) {
    case 1: sp_launch_rows<V, 1>(P, G, A, s); break;
    case 2: sp_launch_rows<V, 2>(P, G, A, s); break;
    case 4: sp_launch_rows<V, 4>(P, G, A, s); break;
    case 8: sp_launch_rows<V, 8>(P, G, A, s); break;
    default:                                                        // (the plan gives 16 and 32 to the one-column chunk only)
        if constexpr (V == 1) {
            if (P.w == 16) sp_launch_rows<1, 16>(P, G, A, s);
            else sp_launch_rows<1, 32>(P, G, A, s);
        }
        break;
    }
}

template <int V>
void sp_launch(const SpPlan &P, const SpPtrs &A, hipStream_t s) {
    const SpGeom &G = P.G;
    const dim3 grid((unsigned)P.nblk), blk(SP_THREADS);
    if (P.form == SP_FORM_STATS) {
        hipLaunchKernelGGL((spell_stats_kernel<V, false>), grid, blk, 0, s, G, A);
        return;
    }
    if (P.form == SP_FORM_ROWS) {
        sp_launch_rows_class<V>(P, G, A, s);
        return;
    }
    hipLaunchKernelGGL((spell_stats_kernel<V, true>), grid, blk, 0, s, G, A);
    SpGeom J = G;
    J.A.nblk = P.join_blk;
    const dim3 jgrid((unsigned)P.join_blk), jblk(SP_JOIN_THREADS);
    if (P.form == SP_FORM_STATS_SLABS) {
        hipLaunchKernelGGL((spell_join_kernel<V, false>), jgrid, jblk, 0, s, J, A);
        return;
    }
    hipLaunchKernelGGL((spell_join_kernel<V, true>), jgrid, jblk, 0, s, J, A);
    sp_launch_rows_class<V>(P, G, A, s);
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" size_t dlwpcs_time_spell_scratch_bytes(const dlwpcs_rows_desc *d, const void *src, int64_t n_rows, int64_t slab_rows,
                                                  int per_row) {
    SpPlan P;
    if (sp_plan(d, src, n_rows, slab_rows, per_row, P) != DLWPCS_OK) return 0;
    return P.scratch_bytes;
}

extern "C" int dlwpcs_time_spell(const dlwpcs_rows_desc *d, const float *src, int64_t n_rows, const float *thr, int64_t thr_row_stride,
                                 const int64_t *thr_stride, const int32_t *thr_index, int cmp, int64_t min_length, int missing,
                                 int64_t slab_rows, int32_t *pos, int32_t *len, int32_t *stats, int64_t stat_stride, void *scratch,
                                 size_t scratch_bytes, dlwpcs_stream_t stream) {
    SpPlan P;
    int rc = sp_plan(d, src, n_rows, slab_rows, pos || len, P);
    if (rc != DLWPCS_OK) return rc;
    if (cmp < DLWPCS_SPELL_GT || cmp > DLWPCS_SPELL_LE) return fail(DLWPCS_E_INVALID, "time_spell: cmp %d", cmp);
    if (missing != DLWPCS_SPELL_BREAK && missing != DLWPCS_SPELL_PROPAGATE) return fail(DLWPCS_E_INVALID, "time_spell: missing mode %d", missing);
    if (min_length < 1) return fail(DLWPCS_E_INVALID, "time_spell: min_length %lld (at least 1)", (long long)min_length);
    if (n_rows == 0 || P.G.inner == 0) return DLWPCS_OK;
    if (!pos && !len && !stats) return DLWPCS_OK;
    if (!src || !thr) return fail(DLWPCS_E_INVALID, "time_spell: null operand");
    if ((((uintptr_t)thr) | ((uintptr_t)thr_index) | ((uintptr_t)pos) | ((uintptr_t)len) | ((uintptr_t)stats)) & 3)
        return fail(DLWPCS_E_INVALID, "time_spell: an operand is not aligned to its 4-byte elements");
    if (P.scratch_bytes && (!scratch || scratch_bytes < P.scratch_bytes || !aligned16(scratch)))
        return fail(DLWPCS_E_INVALID, "time_spell: scratch of %zu bytes on 16 bytes needed, got %zu", P.scratch_bytes, scratch_bytes);
    SpGeom &G = P.G;
    const int L = G.A.n_inner - 1;
    for (int i = 0; i <= L; ++i) G.tst[i] = thr_stride ? thr_stride[i] : 0;
    G.thr_row_stride = thr_row_stride;
    G.stat_stride = stat_stride;
    G.min_length = min_length;
    G.cmp = cmp;
    G.missing = missing;
    if (G.wide && !(aligned16(pos) && aligned16(len) && aligned16(stats) && stat_stride % 4 == 0)) G.wide = 0;
    G.tvec = P.v == 4 && aligned16(thr) && G.tst[L] == 1 && thr_row_stride % 4 == 0;
    for (int i = 0; i < L && G.tvec; ++i) G.tvec = G.tst[i] % 4 == 0;
    G.A.nblk = P.nblk;
    const SpPtrs A = {src, thr, thr_index, pos, len, stats, (int32_t *)scratch};
    hipStream_t s = (hipStream_t)stream;
    if (P.v == 4) sp_launch<4>(P, A, s);
    else sp_launch<1>(P, A, s);
    return check_launch("time_spell");
}

extern "C" int dlwpcs_time_spell_plan_info(const dlwpcs_rows_desc *d, const void *src, int64_t n_rows, int64_t slab_rows, int per_row,
                                           int64_t info[8]) {
    if (!info) return fail(DLWPCS_E_INVALID, "time_spell_plan_info: null info");
    SpPlan P;
    int rc = sp_plan(d, src, n_rows, slab_rows, per_row, P);
    if (rc != DLWPCS_OK) return rc;
    const bool any = n_rows > 0 && P.G.inner > 0;
    if (any && !src) return fail(DLWPCS_E_INVALID, "time_spell: null operand");
    info[0] = P.form;
    info[1] = any ? P.G.slab_rows : 0;
    info[2] = any ? P.G.nslab : 0;
    info[3] = P.w;
    info[4] = P.v;
    info[5] = any ? P.nblk : 0;
    info[6] = any ? P.launches : 0;
    info[7] = (int64_t)P.scratch_bytes;
    return DLWPCS_OK;
}
