// Filters along the row axis (dlwpcs_time_filter): a finite-impulse-response filter with a decimation step over the rows of a
// dlwpcs_rows_desc row set, with the project's missing-value rules (include/dlwpcs.h states the operation; the tests compare bits
// against it).  One launch, no atomics, no scratch, nothing crosses lanes: grid = column tiles x time slabs of output rows, 256
// lanes, a lane owns one chunk of a row (a float4 on the vector path, one element otherwise) as in group_mean_kernel.
//
// With r' = r + o, output j reads the rows r' = j*s .. j*s + K - 1, and row r' = m*s + t (0 <= t < s) is tap k = t + a*s of output
// j = m - a for every age a with k < K: at most A = ceil(K / s) outputs are live at once.
//
// Streaming form (chosen up to class 8, the classes with 16-byte chunks; forced up to 32).  A lane walks the rows of its slab
// once, in order, and keeps the live outputs in AC registers per element, AC
// the power of two >= A (classes 1 .. 32).  Output j lives in slot j % AC.  The walk goes step by step (a step is the s rows of one
// m) and is unrolled over one period of AC steps, so that in the code of step p the slot (p - a) % AC of every age is a
// compile-time index: no register is indexed at run time, nothing moves between registers.  At the start of step m slot m % AC
// is cleared for output m; at its end the output of age AC - 1 is stored from the slot that the next step clears.  Ages below
// AC / 2 always have a tap (A > AC / 2 is what put K and s into this class); the others are tested, k < K, a condition uniform
// over the workgroup.  A slot whose output lies outside the slab, or is past its last tap, collects values nobody stores.
// The taps are uniform over the workgroup.  s = 1 (every K <= 32; a row is a step): tap a belongs to age a whatever the row, the
// taps are loop constants read through the scalar cache, and a ring of rows is kept in flight across the steps.  Any other s:
// the rows of a step are loaded in batches, and with each row one vector load brings its taps, tap t + a * s into lane a, from
// where a lane read hands them to the wave (32 scalar loads per row, their addresses live at once, ran out of scalar registers).
//
// NaN handling without a flag per output.  acc starts at +0 and a sum of floats is -0 only when both terms are, so acc is never
// -0 and adding a +-0 never changes it.  MEAN mode therefore adds h * 0 for a missing entry (the taps are finite) and
// (present ? h : 0) to w, which are the bits of adding nothing.  n = 0 leaves acc = w = +0 and q = 0 / 0 = NaN, so the value
// needs no n.  SUM mode lets a missing entry enter as NaN: acc stays NaN, the output is QNAN as for bad.  n is kept (one more
// register per output) only where a count is asked for.
//
// Gather form (A > 8, or forced): a lane computes the outputs of its slab eight at a time from one pass over the K + 7 s rows
// they read between them, each row entering every output it is a tap of -- per output the same additions in the same order,
// hence the same bits.  (One output at a time, K loads each, was built first: 22.3 ms for 121 taps over 1 GB, bound by the
// loads; EXPERIMENTS.md.)  Consecutive blocks re-read rows the slab has just read: the caches serve them.
//
// No profiler tags: the launch profiler's registry is the convolution family's (tests/test_conv_coverage_tags.py), as for the
// other verification kernels.
#include <math.h>
#include "strided.h"

namespace dlwpcs {

namespace {

constexpr int TF_THREADS = 256;
constexpr int TF_MAX_CLASS = 32;
// the largest class the planner takes by itself, the largest with 16-byte chunks.  Measured on 1 GB at step 1, MEAN: 28 taps run
// 2.25 ms in class 32 and 16 taps 1.34 ms in class 16 (one element per lane), 1.68 ms and 1.10 ms in the gather form (16-byte
// chunks, eight outputs per pass); class 8 (28 taps at step 4) 0.33 ms against 0.60 ms
constexpr int TF_AUTO_MAX_CLASS = 8;
constexpr int TF_VEC_MAX_CLASS = 8;                 // 16-byte chunks up to this class: 4 x (acc, w, n) x 8 = 96 registers of state
constexpr int64_t TF_TARGET_BLOCKS = 1024;          // 256 CUs x 4
constexpr int TF_GATHER_UNROLL = 8;                 // loads in flight per lane in the gather form
constexpr int TF_GATHER_BLOCK = 8;                  // outputs a lane computes from one pass over their rows
constexpr int64_t TF_GATHER_MIN_SLAB = 8;

struct TfGeom {
    RowsAddr A;
    int32_t out_vec;
    int64_t step_stride;                            // s * src_row_stride
    int64_t T, o, J, slab_rows;
    int32_t K, s;
    int32_t alo, rem;                               // K = alo * s + rem: row t of a step has a tap for alo + (t < rem) ages
    float min_weight;
};

// source row r of the lane's column, off = r * src_row_stride; a row outside the source, or past the last row the slab needs
// (r_last), is missing
template <int V>
__device__ __forceinline__ void tf_load_row(const TfGeom &G, const float *__restrict__ p, int64_t r, int64_t off, int64_t r_last,
                                            float x[V]) {
    if (r >= 0 && r < G.T && r <= r_last) {
        load_chunk<V>(p + off, x);
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v) x[v] = quiet_nan();
    }
}

template <int V>
__device__ __forceinline__ void tf_store(const TfGeom &G, float *__restrict__ out, int32_t *__restrict__ count, int64_t off,
                                         const float r[V], const int32_t n[V], bool with_count) {
    if constexpr (V == 4) {
        if (G.out_vec) {
            *reinterpret_cast<float4 *>(out + off) = make_float4(r[0], r[1], r[2], r[3]);
            if (with_count) {
                if (aligned16(count)) {
                    *reinterpret_cast<int4 *>(count + off) = make_int4(n[0], n[1], n[2], n[3]);
                } else {
#pragma unroll
                    for (int v = 0; v < V; ++v) count[off + v] = n[v];
                }
            }
        } else {
            const int64_t st = G.A.ost[G.A.n_inner - 1];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                out[off + v * st] = r[v];
                if (with_count) count[off + v * st] = n[v];
            }
        }
    } else {
        out[off] = r[0];
        if (with_count) count[off] = n[0];
    }
}

template <bool MEAN>
__device__ __forceinline__ float tf_finish(float acc, float w, float min_weight) {
#pragma clang fp contract(off)
    const float nan = quiet_nan();
    if constexpr (MEAN) {
        const float q = __fdiv_rn(acc, w);
        return (w >= min_weight && !isnan(q)) ? q : nan;
    } else {
        return isnan(acc) ? nan : acc;
    }
}

// the live outputs of a lane: every index below is a compile-time constant once the walk is unrolled
template <int V, int AC, bool MEAN, bool CNT>
struct TfLive {
    float acc[AC][V];
    float w[MEAN ? AC : 1][V];
    int32_t n[CNT ? AC : 1][V];
};

// the taps of row t of a step, one per lane: lane a holds h[t + a * s] for the na ages that have a tap (one vector load per row,
// not one per tap; tf_row hands each to the whole wave with a lane read)
__device__ __forceinline__ float tf_row_taps(const TfGeom &G, const float *__restrict__ taps, int32_t t, int32_t &na) {
    na = t < G.rem ? G.alo + 1 : G.alo;
    const int32_t lane = (int32_t)(threadIdx.x & 63u);
    return lane < na ? taps[t + lane * G.s] : 0.f;
}

// one row enters: tap t + a * s of the output of age a, for every age that has a tap.  pp: the step within the unrolled period.
// S1: t = 0 and the taps are loop constants, read through the scalar cache; else hv / na of tf_row_taps.
template <int V, int AC, bool MEAN, bool CNT, bool S1>
__device__ __forceinline__ void tf_row(const TfGeom &G, const float *__restrict__ taps, TfLive<V, AC, MEAN, CNT> &L, const int pp,
                                       const float hv, const int32_t na, const float x[V]) {
#pragma clang fp contract(off)
    float xz[V], one[V];
    int32_t pi[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const bool present = !isnan(x[v]);
        xz[v] = (MEAN && !present) ? 0.f : x[v];
        one[v] = present ? 1.f : 0.f;
        pi[v] = present ? 1 : 0;
    }
#pragma unroll
    for (int a = 0; a < AC; ++a) {
        const int slot = ((pp % AC) - a + AC) % AC;
        if (a < AC / 2 || a < (S1 ? G.K : na)) {
            const float h = S1 ? taps[a] : __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hv), a));
#pragma unroll
            for (int v = 0; v < V; ++v) {
                L.acc[slot][v] = L.acc[slot][v] + h * xz[v];
                if constexpr (MEAN) L.w[slot][v] = __fmaf_rn(h, one[v], L.w[slot][v]);      // h * 1 and h * 0 are exact: w + h, w
                if constexpr (CNT) L.n[slot][v] += pi[v];
            }
        }
    }
}

template <int V, int AC, bool MEAN, bool CNT>
__device__ __forceinline__ void tf_clear(TfLive<V, AC, MEAN, CNT> &L, const int slot) {
#pragma unroll
    for (int v = 0; v < V; ++v) {
        L.acc[slot][v] = 0.f;
        if constexpr (MEAN) L.w[slot][v] = 0.f;
        if constexpr (CNT) L.n[slot][v] = 0;
    }
}

template <int V, int AC, bool MEAN, bool CNT>
__device__ __forceinline__ void tf_emit(const TfGeom &G, const TfLive<V, AC, MEAN, CNT> &L, const int slot, float *__restrict__ out,
                                        int32_t *__restrict__ count, int64_t off) {
    float r[V];
    int32_t n[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        r[v] = tf_finish<MEAN>(L.acc[slot][v], MEAN ? L.w[MEAN ? slot : 0][v] : 0.f, G.min_weight);
        n[v] = CNT ? L.n[CNT ? slot : 0][v] : 0;
    }
    tf_store<V>(G, out, count, off, r, n, CNT);
}

// what a step of the walk reads besides the live outputs
template <int V, int AC, bool MEAN, bool CNT, bool S1, int U>
struct TfWalk {
    const TfGeom &G;
    const float *__restrict__ p;
    const float *__restrict__ taps;
    float *__restrict__ out;
    int32_t *__restrict__ count;
    int64_t ooff, j0, r_last, m_last;
    bool live;
    // s > 1: the first source row of the next step and its offset, carried from step to step (computed from the step's number they
    // are all computed at the head of the period and kept in scalar registers, more than there are)
    int64_t r, off;
};

// step m = mb + PP of the walk; PP, and with it every slot, is a compile-time constant
template <int PP, int V, int AC, bool MEAN, bool CNT, bool S1, int U>
__device__ __forceinline__ void tf_step(TfWalk<V, AC, MEAN, CNT, S1, U> &W, TfLive<V, AC, MEAN, CNT> &L,
                                        float (&ring)[S1 ? U : 1][V], const int64_t mb) {
    const TfGeom &G = W.G;
    const int64_t m = mb + PP;
    if (m < W.j0 || m > W.m_last) return;
    tf_clear(L, PP % AC);
    if constexpr (S1) {
        float x[V];
#pragma unroll
        for (int v = 0; v < V; ++v) x[v] = ring[PP % U][v];
        tf_load_row<V>(G, W.p, m + U - G.o, (m + U - G.o) * G.A.src_row_stride, W.r_last, ring[PP % U]);
        if (m - G.o <= W.r_last) tf_row<V, AC, MEAN, CNT, true>(G, W.taps, L, PP, 0.f, 0, x);
    } else {
        if (W.r <= W.r_last) {
            int64_t r = W.r, off = W.off;
            for (int32_t t0 = 0; t0 < G.s; t0 += U) {
                float x[U][V], hv[U];
                int32_t na[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (t0 + u < G.s) {
                        tf_load_row<V>(G, W.p, r, off, W.r_last, x[u]);
                        hv[u] = tf_row_taps(G, W.taps, t0 + u, na[u]);
                        r += 1;
                        off += G.A.src_row_stride;
                    }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (t0 + u < G.s) tf_row<V, AC, MEAN, CNT, false>(G, W.taps, L, PP, hv[u], na[u], x[u]);
            }
        }
        W.r += G.s;
        W.off += G.step_stride;
    }
    const int64_t j = m - (AC - 1);
    if (j >= W.j0 && W.live) tf_emit<V, AC, MEAN, CNT>(G, L, (PP + 1) % AC, W.out, W.count, j * G.A.out_row_stride + W.ooff);
}

template <int PP, int P, int V, int AC, bool MEAN, bool CNT, bool S1, int U>
__device__ __forceinline__ void tf_period(TfWalk<V, AC, MEAN, CNT, S1, U> &W, TfLive<V, AC, MEAN, CNT> &L,
                                          float (&ring)[S1 ? U : 1][V], const int64_t mb) {
    if constexpr (PP < P) {
        tf_step<PP>(W, L, ring, mb);
        tf_period<PP + 1, P>(W, L, ring, mb);
    }
}

template <int V, int AC, bool MEAN, bool CNT, bool S1>
__global__ void __launch_bounds__(TF_THREADS) time_filter_stream_kernel(TfGeom G, const float *__restrict__ src,
                                                                       const float *__restrict__ taps, float *__restrict__ out,
                                                                       int32_t *__restrict__ count) {
    // rows in flight per lane: a ring across the steps (s = 1), else a batch within a step (short where the unrolled code is long)
    constexpr int U = S1 ? (V == 4 ? 4 : 8) : (AC <= 8 ? 4 : 1);
    constexpr int P = S1 && U > AC ? U : AC;            // steps per unrolled period: a multiple of AC and of the ring
    const int64_t bid = flat_block();
    if (bid >= G.A.nblk) return;
    const int64_t slab = bid / G.A.tiles;
    int64_t q = (bid - slab * G.A.tiles) * TF_THREADS + threadIdx.x;
    // a lane past the last column stays (the taps of a row are read lane by lane): it walks the last column and stores nothing
    const bool live = q < G.A.ncol;
    if (!live) q = G.A.ncol - 1;
    const int64_t j0 = slab * G.slab_rows;
    const int64_t j1 = j0 + G.slab_rows < G.J ? j0 + G.slab_rows : G.J;
    int64_t soff, ooff;
    rows_offsets<V, false>(G.A, q, soff, ooff);
    const float *p = src + soff;
    const int64_t r_last = (j1 - 1) * (int64_t)G.s + G.K - 1 - G.o;     // the last source row an output of the slab reads
    const int64_t m_last = j1 - 1 + (AC - 1);           // the step at whose end output j1 - 1 is stored
    TfLive<V, AC, MEAN, CNT> L;
#pragma unroll
    for (int a = 0; a < AC; ++a) tf_clear(L, a);
    const int64_t m_first = j0 - j0 % P;
    float ring[S1 ? U : 1][V];
    int64_t r = j0 * (int64_t)G.s - G.o;                // step j0 begins at source row j0 * s - o
    if constexpr (S1) {
#pragma unroll
        for (int u = 0; u < U; ++u) {                   // ring[u]: the first row at or after step j0 whose step % U == u
            int64_t m = j0 - j0 % U + u;
            if (m < j0) m += U;
            tf_load_row<V>(G, p, m - G.o, (m - G.o) * G.A.src_row_stride, r_last, ring[u]);
        }
    }
    TfWalk<V, AC, MEAN, CNT, S1, U> W = {G, p, taps, out, count, ooff, j0, r_last, m_last, live, r, r * G.A.src_row_stride};
    for (int64_t mb = m_first; mb <= m_last; mb += P) tf_period<0, P>(W, L, ring, mb);
}

template <int V, bool MEAN>
__global__ void __launch_bounds__(TF_THREADS) time_filter_gather_kernel(TfGeom G, const float *__restrict__ src,
                                                                       const float *__restrict__ taps, float *__restrict__ out,
                                                                       int32_t *__restrict__ count) {
#pragma clang fp contract(off)
    constexpr int U = TF_GATHER_UNROLL, R = TF_GATHER_BLOCK;
    const int64_t bid = flat_block();
    if (bid >= G.A.nblk) return;
    const int64_t slab = bid / G.A.tiles;
    const int64_t q = (bid - slab * G.A.tiles) * TF_THREADS + threadIdx.x;
    if (q >= G.A.ncol) return;
    const int64_t j0 = slab * G.slab_rows;
    const int64_t j1 = j0 + G.slab_rows < G.J ? j0 + G.slab_rows : G.J;
    int64_t soff, ooff;
    rows_offsets<V, false>(G.A, q, soff, ooff);
    const float *p = src + soff;
    for (int64_t jb = j0; jb < j1; jb += R) {
        float acc[R][V], w[R][V];
        int32_t n[R][V];
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
            for (int v = 0; v < V; ++v) { acc[i][v] = 0.f; w[i][v] = 0.f; n[i][v] = 0; }
        const int nj = j1 - jb < R ? (int)(j1 - jb) : R;
        const int64_t r0 = jb * (int64_t)G.s - G.o;                 // the first row output jb reads; row r0 + rr is tap rr - i s of output jb + i
        const int64_t nrow = (int64_t)(nj - 1) * G.s + G.K;
        for (int64_t rr0 = 0; rr0 < nrow; rr0 += U) {
            float x[U][V];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t rr = rr0 + u;
                const bool read = rr < nrow && (G.s <= G.K || rr % G.s < G.K);      // (K < s: rows between the windows)
                tf_load_row<V>(G, p, r0 + rr, (r0 + rr) * G.A.src_row_stride, read ? G.T : -1, x[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t rr = rr0 + u;
                if (rr < nrow) {
                    float xz[V], one[V];
                    int32_t pi[V];
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const bool present = !isnan(x[u][v]);
                        xz[v] = (MEAN && !present) ? 0.f : x[u][v];
                        one[v] = present ? 1.f : 0.f;
                        pi[v] = present ? 1 : 0;
                    }
#pragma unroll
                    for (int i = 0; i < R; ++i) {
                        const int64_t k = rr - (int64_t)i * G.s;
                        if (k >= 0 && k < G.K) {
                            const float h = taps[k];
#pragma unroll
                            for (int v = 0; v < V; ++v) {
                                acc[i][v] = acc[i][v] + h * xz[v];
                                if constexpr (MEAN) w[i][v] = __fmaf_rn(h, one[v], w[i][v]);
                                n[i][v] += pi[v];
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < R; ++i)
            if (i < nj) {
                float r[V];
#pragma unroll
                for (int v = 0; v < V; ++v) r[v] = tf_finish<MEAN>(acc[i][v], w[i][v], G.min_weight);
                tf_store<V>(G, out, count, (jb + i) * G.A.out_row_stride + ooff, r, n[i], count != nullptr);
            }
    }
}

struct TfPlan {
    TfGeom G;
    int form, cls;                                      // cls: the accumulator class, 0 in the gather form
    bool vec;
    int64_t inner;
};

// The planner (restated in tests/time_filter_ref.py).  src / out: looked at for 16-byte alignment only.
int tf_plan(const dlwpcs_rows_desc *d, const void *src, const void *out, int64_t n_rows, int n_taps, int64_t step, int64_t origin,
            int64_t n_out, int mode, int form, int64_t slab_rows, TfPlan &P) {
    TfGeom &G = P.G;
    memset(&G, 0, sizeof(G));
    const int rc = rows_addr_init(d, "time_filter", G.A, P.inner);
    if (rc != DLWPCS_OK) return rc;
    if (n_taps < 1 || n_taps > DLWPCS_TIME_FILTER_MAX_TAPS)
        return fail(DLWPCS_E_INVALID, "time_filter: %d taps (1 .. %d)", n_taps, DLWPCS_TIME_FILTER_MAX_TAPS);
    if (step < 1 || step > (1ll << 30)) return fail(DLWPCS_E_INVALID, "time_filter: step %lld", (long long)step);
    if (origin < 0 || origin >= n_taps) return fail(DLWPCS_E_INVALID, "time_filter: origin %lld outside the %d taps", (long long)origin, n_taps);
    if (n_rows < 0 || n_rows > (1ll << 31) || n_out < 0 || n_out > (1ll << 31))
        return fail(DLWPCS_E_INVALID, "time_filter: %lld source rows, %lld output rows", (long long)n_rows, (long long)n_out);
    if (mode != DLWPCS_FILTER_SUM && mode != DLWPCS_FILTER_MEAN) return fail(DLWPCS_E_INVALID, "time_filter: mode %d", mode);
    if (form < -1 || form > 1) return fail(DLWPCS_E_INVALID, "time_filter: form %d", form);
    if (slab_rows < 0) return fail(DLWPCS_E_INVALID, "time_filter: slab_rows %lld", (long long)slab_rows);
    G.T = n_rows; G.K = n_taps; G.s = (int32_t)step; G.o = origin; G.J = n_out;
    G.step_stride = step * d->src_row_stride;
    G.alo = (int32_t)(n_taps / step);
    G.rem = (int32_t)(n_taps - G.alo * step);
    const int64_t A = step >= n_taps ? 1 : (n_taps + step - 1) / step;
    if (form == 0 && A > TF_MAX_CLASS)
        return fail(DLWPCS_E_INVALID, "time_filter: the streaming form holds %d live outputs, %d taps at step %lld need %lld",
                    TF_MAX_CLASS, n_taps, (long long)step, (long long)A);
    P.form = form >= 0 ? form : (A <= TF_AUTO_MAX_CLASS ? 0 : 1);
    P.cls = 0;
    if (P.form == 0)
        for (P.cls = 1; P.cls < A; P.cls *= 2) {}
    // 16-byte chunks along the last dim; every other offset keeps a chunk on 16 bytes
    bool vec, ovec;
    rows_vector_ok(d, vec, ovec);
    vec = vec && aligned16(src) && !(P.form == 0 && P.cls > TF_VEC_MAX_CLASS);
    ovec = ovec && vec && aligned16(out);
    P.vec = vec;
    G.out_vec = ovec;
    if (vec) G.A.ext[d->n_inner - 1] /= 4;
    G.A.ncol = P.inner / (vec ? 4 : 1);
    G.A.tiles = (G.A.ncol + TF_THREADS - 1) / TF_THREADS;
    if (slab_rows > 0) {
        G.slab_rows = slab_rows;
    } else {
        // enough slabs to fill the chip, none so short that the rows it shares with its neighbour (and, streaming, the steps in
        // which its pipeline fills) are more than an eighth of its own
        const int64_t lmin = P.form == 0 ? 8 * (int64_t)P.cls : TF_GATHER_MIN_SLAB;
        const int64_t want = G.A.tiles > 0 ? (TF_TARGET_BLOCKS + G.A.tiles - 1) / G.A.tiles : 1;
        int64_t nsl = n_out / lmin < want ? n_out / lmin : want;
        if (nsl < 1) nsl = 1;
        G.slab_rows = (n_out + nsl - 1) / nsl;
    }
    if (G.slab_rows < 1) G.slab_rows = 1;
    if (G.slab_rows > n_out && n_out > 0) G.slab_rows = n_out;
    const int64_t slabs = (n_out + G.slab_rows - 1) / G.slab_rows;
    G.A.nblk = G.A.tiles * slabs;
    if (G.A.nblk > MAX_BLOCKS) return fail(DLWPCS_E_INVALID, "time_filter: %lld workgroups is too many", (long long)G.A.nblk);
    return DLWPCS_OK;
}

template <int V, int AC, bool MEAN, bool CNT>
void tf_launch_stream(const TfPlan &P, const float *src, const float *taps, float *out, int32_t *count, hipStream_t s) {
    const dim3 grid = launch_grid(P.G.A.nblk), blk(TF_THREADS);
    if (P.G.s == 1) hipLaunchKernelGGL((time_filter_stream_kernel<V, AC, MEAN, CNT, true>), grid, blk, 0, s, P.G, src, taps, out, count);
    else hipLaunchKernelGGL((time_filter_stream_kernel<V, AC, MEAN, CNT, false>), grid, blk, 0, s, P.G, src, taps, out, count);
}

template <int V, int AC>
void tf_launch_class(const TfPlan &P, bool mean, const float *src, const float *taps, float *out, int32_t *count, hipStream_t s) {
    if (mean) {
        if (count) tf_launch_stream<V, AC, true, true>(P, src, taps, out, count, s);
        else tf_launch_stream<V, AC, true, false>(P, src, taps, out, count, s);
    } else {
        if (count) tf_launch_stream<V, AC, false, true>(P, src, taps, out, count, s);
        else tf_launch_stream<V, AC, false, false>(P, src, taps, out, count, s);
    }
}

template <int V>
void tf_launch(const TfPlan &P, bool mean, const float *src, const float *taps, float *out, int32_t *count, hipStream_t s) {
    if (P.form == 1) {
        const dim3 grid = launch_grid(P.G.A.nblk), blk(TF_THREADS);
        if (mean) hipLaunchKernelGGL((time_filter_gather_kernel<V, true>), grid, blk, 0, s, P.G, src, taps, out, count);
        else hipLaunchKernelGGL((time_filter_gather_kernel<V, false>), grid, blk, 0, s, P.G, src, taps, out, count);
        return;
    }
    switch (P.cls) {
    case 1: tf_launch_class<V, 1>(P, mean, src, taps, out, count, s); break;
    case 2: tf_launch_class<V, 2>(P, mean, src, taps, out, count, s); break;
    case 4: tf_launch_class<V, 4>(P, mean, src, taps, out, count, s); break;
    case 8: tf_launch_class<V, 8>(P, mean, src, taps, out, count, s); break;
    default:
        if constexpr (V == 1) {                         // (the planner gives the classes above 8 one element per lane)
            if (P.cls == 16) tf_launch_class<1, 16>(P, mean, src, taps, out, count, s);
            else tf_launch_class<1, 32>(P, mean, src, taps, out, count, s);
        }
        break;
    }
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" int dlwpcs_time_filter(const dlwpcs_rows_desc *d, const float *src, int64_t n_rows, const float *taps, int n_taps,
                                  int64_t step, int64_t origin, int64_t n_out, int mode, float min_weight, int form,
                                  int64_t slab_rows, float *out, int32_t *count, dlwpcs_stream_t stream) {
    TfPlan P;
    int rc = tf_plan(d, src, out, n_rows, n_taps, step, origin, n_out, mode, form, slab_rows, P);
    if (rc != DLWPCS_OK) return rc;
    if (n_out == 0 || P.inner == 0) return DLWPCS_OK;
    if (!src || !taps || !out) return fail(DLWPCS_E_INVALID, "time_filter: null operand");
    if ((((uintptr_t)src) | ((uintptr_t)taps) | ((uintptr_t)out) | ((uintptr_t)count)) & 3)
        return fail(DLWPCS_E_INVALID, "time_filter: an operand is not aligned to its 4-byte elements");
    P.G.min_weight = min_weight;
    hipStream_t s = (hipStream_t)stream;
    if (P.vec) tf_launch<4>(P, mode == DLWPCS_FILTER_MEAN, src, taps, out, count, s);
    else tf_launch<1>(P, mode == DLWPCS_FILTER_MEAN, src, taps, out, count, s);
    return check_launch("time_filter");
}

extern "C" int dlwpcs_time_filter_plan_info(const dlwpcs_rows_desc *d, const void *src, const void *out, int64_t n_rows, int n_taps,
                                            int64_t step, int64_t n_out, int mode, int form, int64_t slab_rows, int32_t info[8]) {
    if (!info) return fail(DLWPCS_E_INVALID, "time_filter_plan_info: null info");
    TfPlan P;
    int rc = tf_plan(d, src, out, n_rows, n_taps, step, 0, n_out, mode, form, slab_rows, P);
    if (rc != DLWPCS_OK) return rc;
    const bool empty = n_out == 0 || P.inner == 0;
    if (!empty && (!src || !out)) return fail(DLWPCS_E_INVALID, "time_filter: null operand");
    const dim3 grid = launch_grid(empty ? 0 : P.G.A.nblk);
    info[0] = P.form;
    info[1] = P.cls;
    info[2] = P.vec ? 1 : 0;
    info[3] = (int32_t)P.G.slab_rows;
    info[4] = (int32_t)grid.x;
    info[5] = (int32_t)grid.y;
    info[6] = 0;
    info[7] = 0;
    return DLWPCS_OK;
}
