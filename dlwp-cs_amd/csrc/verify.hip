// Forecast verification scores (reference DLWP/verify.py:18-164): one fp32 strided reduction that every method maps onto.
//
// For each output (lead f, kept index o, channel k of the kept innermost axis) the kernel reduces pairs x = a[...], y = b[...]
// over t < n_f and every reduced index (see dlwpcs_score_desc).  Operands are strided views (stride 0 = broadcast).
//
// Launch 1 (score_partial_kernel): grid = groups x slabs, 256 threads.  A group is one (f, o); its rows x row-length element
// space is cut into `slabs` contiguous ranges.  Every lane accumulates a short run (UNROLL chunks) in fp32, then adds it into
// fp64 per-lane sums; lanes and waves are summed in a fixed shuffle / LDS order.  With one slab the block finalises its own
// outputs; otherwise it writes fp64 partials and launch 2 (score_finalize_kernel) adds the slabs in slab order.  No atomics:
// bitwise reproducible run to run.
//
// Vector path: when a and b are contiguous along the row (row stride = kc, channel stride 1) and every row starts on 16 B, a lane
// reads one float4 of each per chunk; slot j of the float4 belongs to channel j % kc (kc = 1, 2 or 4).
//
// Indexed form (dlwpcs_score_indexed, IDX instantiations): one operand is a (K, inner...) table whose row for (lead f, time t)
// is row_tab[f * t_len + t] -- one load where a row's offsets are computed, nothing else differs, so the plan, the slabs
// and the order of every sum are those of the materialised operand.  Which operand it is follows from the method (idx_operand).
#include <string.h>
#include "strided.h"

namespace dlwpcs {

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_UNROLL = 4;
constexpr int SC_NM = 6;                // moments: three sums, three non-NaN counts
constexpr int SC_TARGET_BLOCKS = 2048;  // 256 CUs x 8
constexpr int64_t SC_MIN_CHUNKS = 4096; // per block

struct ScoreGeom {
    int32_t method, n_lead, t_len, t_cap, t_slope, n_keep, n_outer, kc, kc_shift;
    int64_t keep_ext[DLWPCS_SCORE_MAX_DIMS];
    int64_t outer_ext[DLWPCS_SCORE_MAX_DIMS];
    int64_t keep_total, red_outer, row_len;     // row_len = elements of the innermost reduced dim
    int64_t lead_stride[4], t_stride[4], kc_stride[4], row_stride[4];
    int64_t keep_stride[4][DLWPCS_SCORE_MAX_DIMS];
    int64_t outer_stride[4][DLWPCS_SCORE_MAX_DIMS];
    int32_t slabs, has_c, has_w, out_f32;
    int32_t cmode, wmode;                       // vector path: how c / w are read (AUX_*)
    int32_t idx_op;                             // indexed form: the operand looked up by row (idx_operand), else -1
    int64_t idx_stride;                         // indexed form: elements between rows of its table
    int64_t nblk;                               // workgroups of the launch (the grid may round up)
};

// vector path: how a chunk's four climatology / weight values are read
constexpr int AUX_ELEM = 0;                     // one load per element (any strides)
constexpr int AUX_VEC = 1;                      // one float4: contiguous along (row, channel) like a and b
constexpr int AUX_CELL = 2;                     // one load: kc = 4 and constant along the channels (a per-cell field)

template <int V>
__device__ __forceinline__ void load_aux(const float *__restrict__ p, bool has, int mode, int64_t off, int64_t e0, int shift,
                                         int kmask, int64_t rs, int64_t ks, float dflt, float out[V]) {
    if (!has) {
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = dflt;
    } else if (V == 4 && mode == AUX_VEC) {
        float4 v = *reinterpret_cast<const float4 *>(p + off + e0);
        out[0] = v.x; out[V > 1 ? 1 : 0] = v.y; out[V > 2 ? 2 : 0] = v.z; out[V - 1] = v.w;
    } else if (V == 4 && mode == AUX_CELL) {
        const float v = p[off + (e0 >> 2) * rs];
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = v;
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int64_t e = e0 + j;
            out[j] = p[off + (e >> shift) * rs + (e & kmask) * ks];
        }
    }
}

__device__ __forceinline__ int64_t n_rows_of(const ScoreGeom &G, int f) {
    int64_t nf = (int64_t)G.t_cap - (int64_t)G.t_slope * f;
    if (nf > G.t_len) nf = G.t_len;
    if (nf < 0) nf = 0;
    return nf * G.red_outer;
}

// offsets of row r (t, outer reduced coordinates) relative to the group base
// the operand the indexed form looks up: the climatology c of ACC / COS, else a (the climatology as the forecast of an error)
__host__ __device__ constexpr int idx_operand(int M) { return (M == DLWPCS_SCORE_ACC || M == DLWPCS_SCORE_COS) ? 2 : 0; }

template <int IOP>
__device__ __forceinline__ void row_offsets(const ScoreGeom &G, int64_t r, const int64_t base[4], int64_t off[4],
                                            const int32_t *__restrict__ lead_rows) {
    int64_t t = r / G.red_outer, rr = r - t * G.red_outer;
#pragma unroll
    for (int op = 0; op < 4; ++op) off[op] = base[op] + t * G.t_stride[op];
    if constexpr (IOP >= 0) off[IOP] += (int64_t)lead_rows[t] * G.idx_stride;
    for (int d = G.n_outer - 1; d >= 0; --d) {
        int64_t e = G.outer_ext[d];
        int64_t c = rr % e;
        rr /= e;
#pragma unroll
        for (int op = 0; op < 4; ++op) off[op] += c * G.outer_stride[op][d];
    }
}

template <int M>
__device__ __forceinline__ void term(float x, float y, float c, float w, float &s0, float &s1, float &s2,
                                     uint32_t &n0, uint32_t &n1, uint32_t &n2) {
    if (M == DLWPCS_SCORE_MEAN) {
        if (!isnan(y)) { s0 += y; ++n0; }
    } else if (M == DLWPCS_SCORE_MSE || M == DLWPCS_SCORE_RMSE) {
        float d = y - x;
        float v = d * d * w;
        if (!isnan(v)) { s0 += v; ++n0; }
    } else if (M == DLWPCS_SCORE_MAE) {
        float v = fabsf((y - x) * w);
        if (!isnan(v)) { s0 += v; ++n0; }
    } else if (M == DLWPCS_SCORE_ACC) {
        float av = y - c, af = x - c;
        float p = av * af * w, qv = av * av * w, qf = af * af * w;
        if (!isnan(p)) { s0 += p; ++n0; }
        if (!isnan(qv)) { s1 += qv; ++n1; }
        if (!isnan(qf)) { s2 += qf; ++n2; }
    } else {                                            // COS: dot((x-c), (y-c)*w) / (|(x-c)*w| |(y-c)*w|), no NaN skipping
        float av = y - c, af = x - c;
        float fw = af * w, vw = av * w;
        s0 += af * vw;
        s1 += fw * fw;
        s2 += vw * vw;
    }
}

__device__ __forceinline__ double finalize(int M, const double m[SC_NM]) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (M == DLWPCS_SCORE_COS) return m[0] / (sqrt(m[1]) * sqrt(m[2]));
    if (M == DLWPCS_SCORE_ACC) {
        if (m[3] == 0.0 || m[4] == 0.0 || m[5] == 0.0) return nan;
        return (m[0] / m[3]) / sqrt((m[1] / m[4]) * (m[2] / m[5]));
    }
    if (m[3] == 0.0) return nan;
    double v = m[0] / m[3];
    return M == DLWPCS_SCORE_RMSE ? sqrt(v) : v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int M, bool VEC, bool IDX>
__global__ void __launch_bounds__(SC_THREADS) score_partial_kernel(ScoreGeom G, const float *__restrict__ a,
                                                                  const float *__restrict__ b, const float *__restrict__ c,
                                                                  const float *__restrict__ w, double *__restrict__ partial,
                                                                  void *__restrict__ out, const int32_t *__restrict__ row_tab) {
    constexpr int V = VEC ? 4 : 1;                      // elements per chunk
    const int64_t bid = flat_block();
    if (bid >= G.nblk) return;
    const int64_t g = bid / G.slabs;
    const int slab = (int)(bid - g * G.slabs);
    const int f = (int)(g / G.keep_total);
    int64_t ko = g - (int64_t)f * G.keep_total;
    int64_t base[4];
#pragma unroll
    for (int op = 0; op < 4; ++op) base[op] = (int64_t)f * G.lead_stride[op];
    for (int d = G.n_keep - 1; d >= 0; --d) {
        int64_t e = G.keep_ext[d];
        int64_t cidx = ko % e;
        ko /= e;
#pragma unroll
        for (int op = 0; op < 4; ++op) base[op] += cidx * G.keep_stride[op][d];
    }
    const int32_t *lead_rows = IDX ? row_tab + (int64_t)f * G.t_len : nullptr;    // the table rows of this lead
    const int64_t rows = n_rows_of(G, f);
    const int64_t rl = G.row_len * G.kc;                // elements per row
    const int64_t cpr = rl / V;                         // chunks per row
    const int64_t Q = rows * cpr;
    const int64_t q0 = Q * slab / G.slabs, q1 = Q * (slab + 1) / G.slabs;

    double acc[4][SC_NM];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int m = 0; m < SC_NM; ++m) acc[j][m] = 0.0;

    int64_t q = q0 + threadIdx.x;
    int64_t row = cpr ? q / cpr : 0, col = cpr ? q - row * cpr : 0;
    int64_t roff[4];
    if (q < q1) row_offsets<IDX ? idx_operand(M) : -1>(G, row, base, roff, lead_rows);
    const int kmask = G.kc - 1;
    while (q < q1) {
        float x[SC_UNROLL][V], y[SC_UNROLL][V], cc[SC_UNROLL][V], ww[SC_UNROLL][V];
        int chan[SC_UNROLL];                            // scalar path: the channel of the chunk's element
        int nvalid = 0;
#pragma unroll
        for (int u = 0; u < SC_UNROLL; ++u) {
            if (q < q1) {
                const int64_t e0 = col * V;
                if constexpr (VEC) {
                    float4 xa = *reinterpret_cast<const float4 *>(a + roff[0] + e0);
                    float4 yb = *reinterpret_cast<const float4 *>(b + roff[1] + e0);
                    x[u][0] = xa.x; x[u][1] = xa.y; x[u][2] = xa.z; x[u][3] = xa.w;
                    y[u][0] = yb.x; y[u][1] = yb.y; y[u][2] = yb.z; y[u][3] = yb.w;
                }
                chan[u] = (int)(col & kmask);
                if constexpr (!VEC) {
                    const int64_t l = col >> G.kc_shift;
                    const int k = (int)(col & kmask);
                    x[u][0] = a[roff[0] + l * G.row_stride[0] + k * G.kc_stride[0]];
                    y[u][0] = b[roff[1] + l * G.row_stride[1] + k * G.kc_stride[1]];
                }
                load_aux<V>(c, G.has_c, G.cmode, roff[2], e0, G.kc_shift, kmask, G.row_stride[2], G.kc_stride[2], 0.f, cc[u]);
                load_aux<V>(w, G.has_w, G.wmode, roff[3], e0, G.kc_shift, kmask, G.row_stride[3], G.kc_stride[3], 1.f, ww[u]);
                ++nvalid;
                q += SC_THREADS;
                col += SC_THREADS;
                if (col >= cpr) {
                    row += col / cpr;
                    col %= cpr;
                    if (q < q1) row_offsets<IDX ? idx_operand(M) : -1>(G, row, base, roff, lead_rows);
                }
            }
        }
        // fp32 over this run, one slot per float4 lane (vector path) or per channel (scalar path)
        float s[4][3];
        uint32_t n[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int m = 0; m < 3; ++m) { s[j][m] = 0.f; n[j][m] = 0; }
#pragma unroll
        for (int u = 0; u < SC_UNROLL; ++u) {
            if (u < nvalid) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const int slot = VEC ? j : chan[u];
#pragma unroll
                    for (int sl = 0; sl < 4; ++sl)
                        if (sl == slot)
                            term<M>(x[u][j], y[u][j], cc[u][j], ww[u][j], s[sl][0], s[sl][1], s[sl][2], n[sl][0], n[sl][1],
                                    n[sl][2]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int m = 0; m < 3; ++m) { acc[j][m] += (double)s[j][m]; acc[j][3 + m] += (double)n[j][m]; }
    }

    // fold float4 slots onto channels: slot j -> channel j % kc (fixed order)
    double ch[4][SC_NM];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int m = 0; m < SC_NM; ++m) ch[k][m] = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int m = 0; m < SC_NM; ++m) {
            double v = acc[j][m];
            if ((j & kmask) == 0) ch[0][m] += v;
            if ((j & kmask) == 1) ch[1][m] += v;
            if ((j & kmask) == 2) ch[2][m] += v;
            if ((j & kmask) == 3) ch[3][m] += v;
        }

    __shared__ double red[SC_THREADS / 64][4 * SC_NM];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int m = 0; m < SC_NM; ++m) {
            double v = wave_sum(ch[k][m]);
            if (lane == 0) red[wid][k * SC_NM + m] = v;
        }
    __syncthreads();
    if (threadIdx.x < G.kc) {
        const int k = threadIdx.x;
        double m6[SC_NM];
#pragma unroll
        for (int m = 0; m < SC_NM; ++m) {
            double v = 0.0;
#pragma unroll
            for (int wv = 0; wv < SC_THREADS / 64; ++wv) v += red[wv][k * SC_NM + m];
            m6[m] = v;
        }
        if (G.slabs == 1) {
            const double r = finalize(M, m6);
            if (G.out_f32) reinterpret_cast<float *>(out)[g * G.kc + k] = (float)r;
            else reinterpret_cast<double *>(out)[g * G.kc + k] = r;
        } else {
#pragma unroll
            for (int m = 0; m < SC_NM; ++m) partial[((g * G.slabs + slab) * G.kc + k) * SC_NM + m] = m6[m];
        }
    }
}

template <int M>
__global__ void __launch_bounds__(256) score_finalize_kernel(const double *__restrict__ partial, int64_t n_out, int kc,
                                                             int slabs, int out_f32, void *__restrict__ out) {
    const int64_t i = flat_block() * 256 + threadIdx.x;
    if (i >= n_out) return;
    const int64_t g = i / kc;
    const int k = (int)(i - g * kc);
    double m6[SC_NM];
#pragma unroll
    for (int m = 0; m < SC_NM; ++m) m6[m] = 0.0;
    for (int s = 0; s < slabs; ++s)
#pragma unroll
        for (int m = 0; m < SC_NM; ++m) m6[m] += partial[((g * slabs + s) * kc + k) * SC_NM + m];
    const double r = finalize(M, m6);
    if (out_f32) reinterpret_cast<float *>(out)[i] = (float)r;
    else reinterpret_cast<double *>(out)[i] = r;
}

// Column form, for many outputs with short reductions (e.g. a kept innermost spatial axis): one lane per output reduces its
// elements serially (fp32 runs of 16 terms, fp64 beyond) and finishes it; neighbouring lanes read neighbouring outputs.
template <int M, bool IDX>
__global__ void __launch_bounds__(256) score_column_kernel(ScoreGeom G, int64_t n_out, const float *__restrict__ a,
                                                           const float *__restrict__ b, const float *__restrict__ c,
                                                           const float *__restrict__ w, void *__restrict__ out,
                                                           const int32_t *__restrict__ row_tab) {
    const int64_t i = flat_block() * 256 + threadIdx.x;
    if (i >= n_out) return;
    const int64_t g = i / G.kc;
    const int k = (int)(i - g * G.kc);
    const int f = (int)(g / G.keep_total);
    int64_t ko = g - (int64_t)f * G.keep_total;
    int64_t base[4];
#pragma unroll
    for (int op = 0; op < 4; ++op) base[op] = (int64_t)f * G.lead_stride[op] + k * G.kc_stride[op];
    for (int d = G.n_keep - 1; d >= 0; --d) {
        int64_t e = G.keep_ext[d];
        int64_t cidx = ko % e;
        ko /= e;
#pragma unroll
        for (int op = 0; op < 4; ++op) base[op] += cidx * G.keep_stride[op][d];
    }
    const int32_t *lead_rows = IDX ? row_tab + (int64_t)f * G.t_len : nullptr;
    const int64_t rows = n_rows_of(G, f);
    double m6[SC_NM];
#pragma unroll
    for (int m = 0; m < SC_NM; ++m) m6[m] = 0.0;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    uint32_t n0 = 0, n1 = 0, n2 = 0;
    int run = 0;
    for (int64_t r = 0; r < rows; ++r) {
        int64_t roff[4];
        row_offsets<IDX ? idx_operand(M) : -1>(G, r, base, roff, lead_rows);
        for (int64_t l = 0; l < G.row_len; ++l) {
            const float x = a[roff[0] + l * G.row_stride[0]];
            const float y = b[roff[1] + l * G.row_stride[1]];
            const float cv = G.has_c ? c[roff[2] + l * G.row_stride[2]] : 0.f;
            const float wv = G.has_w ? w[roff[3] + l * G.row_stride[3]] : 1.f;
            term<M>(x, y, cv, wv, s0, s1, s2, n0, n1, n2);
            if (++run == 16) {
                m6[0] += s0; m6[1] += s1; m6[2] += s2; m6[3] += n0; m6[4] += n1; m6[5] += n2;
                s0 = s1 = s2 = 0.f;
                n0 = n1 = n2 = 0;
                run = 0;
            }
        }
    }
    m6[0] += s0; m6[1] += s1; m6[2] += s2; m6[3] += n0; m6[4] += n1; m6[5] += n2;
    const double r = finalize(M, m6);
    if (G.out_f32) reinterpret_cast<float *>(out)[i] = (float)r;
    else reinterpret_cast<double *>(out)[i] = r;
}

struct Plan {
    ScoreGeom G;
    int64_t groups, n_out;
    bool vec, column;
};

static int aux_mode(const ScoreGeom &G, int op) {
    bool v4 = (G.kc == 1 || G.kc_stride[op] == 1) && G.row_stride[op] == G.kc && G.lead_stride[op] % 4 == 0 &&
              G.t_stride[op] % 4 == 0 && (op != G.idx_op || G.idx_stride % 4 == 0);
    for (int i = 0; i < G.n_keep && v4; ++i) v4 = G.keep_stride[op][i] % 4 == 0;
    for (int i = 0; i < G.n_outer && v4; ++i) v4 = G.outer_stride[op][i] % 4 == 0;
    if (v4) return AUX_VEC;
    if (G.kc == 4 && G.kc_stride[op] == 0) return AUX_CELL;
    return AUX_ELEM;
}

int make_plan(const dlwpcs_score_desc *d, Plan &P, int idx_op = -1, int64_t idx_stride = 0) {
    if (!d) return fail(DLWPCS_E_INVALID, "score: null descriptor");
    if (d->method < DLWPCS_SCORE_MSE || d->method > DLWPCS_SCORE_MEAN) return fail(DLWPCS_E_INVALID, "score: unknown method %d", d->method);
    if (d->n_lead < 1 || d->t_len < 0 || d->t_slope < 0) return fail(DLWPCS_E_INVALID, "score: bad lead / time extents");
    if (d->n_keep < 0 || d->n_keep > DLWPCS_SCORE_MAX_DIMS || d->n_red < 0 || d->n_red > DLWPCS_SCORE_MAX_DIMS)
        return fail(DLWPCS_E_INVALID, "score: n_keep %d / n_red %d out of range", d->n_keep, d->n_red);
    if (d->kc != 1 && d->kc != 2 && d->kc != 4) return fail(DLWPCS_E_INVALID, "score: kc must be 1, 2 or 4 (got %d)", d->kc);
    ScoreGeom &G = P.G;
    memset(&G, 0, sizeof(G));
    G.method = d->method;
    G.n_lead = d->n_lead;
    G.t_len = d->t_len;
    G.t_cap = d->t_cap;
    G.t_slope = d->t_slope;
    G.kc = d->kc;
    G.kc_shift = d->kc == 4 ? 2 : d->kc == 2 ? 1 : 0;
    G.idx_op = idx_op;
    G.idx_stride = idx_stride;
    G.n_keep = d->n_keep;
    G.keep_total = 1;
    for (int i = 0; i < d->n_keep; ++i) {
        if (d->keep_ext[i] < 1) return fail(DLWPCS_E_INVALID, "score: kept extent %lld", (long long)d->keep_ext[i]);
        G.keep_ext[i] = d->keep_ext[i];
        G.keep_total *= d->keep_ext[i];
    }
    G.red_outer = 1;
    G.row_len = d->n_red > 0 ? d->red_ext[d->n_red - 1] : 1;
    G.n_outer = d->n_red > 0 ? d->n_red - 1 : 0;
    for (int i = 0; i < d->n_red; ++i)
        if (d->red_ext[i] < 0) return fail(DLWPCS_E_INVALID, "score: reduced extent %lld", (long long)d->red_ext[i]);
    for (int i = 0; i < G.n_outer; ++i) {
        G.outer_ext[i] = d->red_ext[i];
        G.red_outer *= d->red_ext[i];
    }
    for (int op = 0; op < 4; ++op) {
        G.lead_stride[op] = d->lead_stride[op];
        G.t_stride[op] = d->t_stride[op];
        G.kc_stride[op] = d->kc_stride[op];
        G.row_stride[op] = d->n_red > 0 ? d->red_stride[op][d->n_red - 1] : 0;
        for (int i = 0; i < d->n_keep; ++i) G.keep_stride[op][i] = d->keep_stride[op][i];
        for (int i = 0; i < G.n_outer; ++i) G.outer_stride[op][i] = d->red_stride[op][i];
    }
    if (d->method == DLWPCS_SCORE_MEAN) {             // a is not read; it mirrors b so that every load stays in bounds
        G.lead_stride[0] = G.lead_stride[1];
        G.t_stride[0] = G.t_stride[1];
        G.kc_stride[0] = G.kc_stride[1];
        G.row_stride[0] = G.row_stride[1];
        for (int i = 0; i < DLWPCS_SCORE_MAX_DIMS; ++i) {
            G.keep_stride[0][i] = G.keep_stride[1][i];
            G.outer_stride[0][i] = G.outer_stride[1][i];
        }
    }
    P.groups = (int64_t)d->n_lead * G.keep_total;
    P.n_out = P.groups * d->kc;
    // vector path: a and b contiguous along (row, channel), every row start 16 B aligned
    bool vec = (G.row_len * G.kc) % 4 == 0;
    for (int op = 0; op < 2 && vec; ++op) {
        vec = (G.kc == 1 || G.kc_stride[op] == 1) && G.row_stride[op] == G.kc && G.lead_stride[op] % 4 == 0 &&
              G.t_stride[op] % 4 == 0 && (op != G.idx_op || G.idx_stride % 4 == 0);
        for (int i = 0; i < G.n_keep && vec; ++i) vec = G.keep_stride[op][i] % 4 == 0;
        for (int i = 0; i < G.n_outer && vec; ++i) vec = G.outer_stride[op][i] % 4 == 0;
    }
    P.vec = vec;
    G.cmode = aux_mode(G, 2);
    G.wmode = aux_mode(G, 3);
    int64_t max_rows = 0;
    for (int f = 0; f < d->n_lead; ++f) {
        int64_t nf = (int64_t)d->t_cap - (int64_t)d->t_slope * f;
        if (nf > d->t_len) nf = d->t_len;
        if (nf < 0) nf = 0;
        if (nf * G.red_outer > max_rows) max_rows = nf * G.red_outer;
        if (d->t_slope == 0) break;
    }
    const int64_t chunks = max_rows * (G.row_len * G.kc / (vec ? 4 : 1));
    int64_t slabs = (SC_TARGET_BLOCKS + P.groups - 1) / P.groups;
    const int64_t by_work = chunks / SC_MIN_CHUNKS;
    if (slabs > by_work) slabs = by_work;
    if (slabs < 1 || d->method == DLWPCS_SCORE_MEAN) slabs = 1;   // the mean finishes in one launch (climo_error: 3 in all)
    // many outputs with short reductions: one lane per output instead of one workgroup (which would idle most of its lanes)
    const int64_t elems = max_rows * G.row_len;
    P.column = elems * G.kc < SC_THREADS || (P.n_out >= 131072 && elems <= 4096);
    if (P.column) slabs = 1;
    G.slabs = (int32_t)slabs;
    G.nblk = P.column ? (P.n_out + 255) / 256 : P.groups * slabs;
    if (G.nblk > MAX_BLOCKS) return fail(DLWPCS_E_INVALID, "score: %lld outputs is too many", (long long)P.n_out);
    return DLWPCS_OK;
}

template <int M, bool IDX>
void launch(const Plan &P, const float *a, const float *b, const float *c, const float *w, double *partial, void *out,
            const int32_t *row_tab, hipStream_t s) {
    const dim3 grid = launch_grid(P.G.nblk);
    if (P.column) {
        hipLaunchKernelGGL((score_column_kernel<M, IDX>), grid, dim3(256), 0, s, P.G, P.n_out, a, b, c, w, out, row_tab);
        return;
    }
    if (P.vec)
        hipLaunchKernelGGL((score_partial_kernel<M, true, IDX>), grid, dim3(SC_THREADS), 0, s, P.G, a, b, c, w, partial, out,
                           row_tab);
    else
        hipLaunchKernelGGL((score_partial_kernel<M, false, IDX>), grid, dim3(SC_THREADS), 0, s, P.G, a, b, c, w, partial, out,
                           row_tab);
    if (P.G.slabs > 1)
        hipLaunchKernelGGL((score_finalize_kernel<M>), launch_grid((P.n_out + 255) / 256), dim3(256), 0, s, partial, P.n_out,
                           P.G.kc, P.G.slabs, P.G.out_f32, out);
}

// the entry points' common head: the indexed form's own refusals, then the plan of the shapes and strides
int plan_of(const dlwpcs_score_desc *d, Plan &P, bool indexed, int64_t table_row_stride) {
    if (!indexed) return make_plan(d, P);
    if (!d) return fail(DLWPCS_E_INVALID, "score: null descriptor");
    if (d->method == DLWPCS_SCORE_MEAN) return fail(DLWPCS_E_INVALID, "score_indexed: the mean has no indexed operand");
    const int indexed_op = idx_operand(d->method);
    if ((d->lead_stride[indexed_op] != 0 || d->t_stride[indexed_op] != 0))
        return fail(DLWPCS_E_INVALID, "score_indexed: the indexed operand's lead and time strides must be 0");
    return make_plan(d, P, indexed_op, table_row_stride);
}

// what the operand pointers settle (NULL and alignment only, nothing is read): required operands, the mean's a, the load
// widths, which of c / w exist.  run() launches exactly what this leaves in P; dlwpcs_score_plan_info reports it.
int settle(const dlwpcs_score_desc *d, Plan &P, const float *&a, const float *b, const float *c, const float *w) {
    if (!b || (d->method != DLWPCS_SCORE_MEAN && !a)) return fail(DLWPCS_E_INVALID, "score: null operand");
    if (P.G.idx_op >= 0 && !(P.G.idx_op == 0 ? a : c)) return fail(DLWPCS_E_INVALID, "score_indexed: null table");
    if (d->method == DLWPCS_SCORE_MEAN) a = b;
    if (P.vec && !(aligned16(a) && aligned16(b))) P.vec = false;
    if (P.G.cmode == AUX_VEC && !aligned16(c)) P.G.cmode = AUX_ELEM;
    if (P.G.wmode == AUX_VEC && !aligned16(w)) P.G.wmode = AUX_ELEM;
    P.G.has_c = c != nullptr;
    P.G.has_w = w != nullptr;
    return DLWPCS_OK;
}

// the entry points' common tail: settle the operands, check the scratch, launch
template <bool IDX>
int run(const dlwpcs_score_desc *d, Plan &P, const float *a, const float *b, const float *c, const float *w, void *out,
        int out_f32, void *scratch, size_t scratch_bytes, const int32_t *row_tab, dlwpcs_stream_t stream) {
    if (!out) return fail(DLWPCS_E_INVALID, "score: null operand");
    const int rc = settle(d, P, a, b, c, w);
    if (rc != DLWPCS_OK) return rc;
    const size_t need = P.G.slabs > 1 ? (size_t)(P.groups * P.G.slabs * P.G.kc * SC_NM) * sizeof(double) : 0;
    if (need && (!scratch || scratch_bytes < need))
        return fail(DLWPCS_E_INVALID, "score: scratch of %zu bytes, need %zu", scratch_bytes, need);
    P.G.out_f32 = out_f32 != 0;
    if (P.n_out == 0) return DLWPCS_OK;
    hipStream_t s = (hipStream_t)stream;
    double *partial = (double *)scratch;
    switch (d->method) {
    case DLWPCS_SCORE_MSE: launch<DLWPCS_SCORE_MSE, IDX>(P, a, b, c, w, partial, out, row_tab, s); break;
    case DLWPCS_SCORE_RMSE: launch<DLWPCS_SCORE_RMSE, IDX>(P, a, b, c, w, partial, out, row_tab, s); break;
    case DLWPCS_SCORE_MAE: launch<DLWPCS_SCORE_MAE, IDX>(P, a, b, c, w, partial, out, row_tab, s); break;
    case DLWPCS_SCORE_ACC: launch<DLWPCS_SCORE_ACC, IDX>(P, a, b, c, w, partial, out, row_tab, s); break;
    case DLWPCS_SCORE_COS: launch<DLWPCS_SCORE_COS, IDX>(P, a, b, c, w, partial, out, row_tab, s); break;
    default:
        if constexpr (!IDX) launch<DLWPCS_SCORE_MEAN, false>(P, a, b, c, w, partial, out, row_tab, s);
        break;
    }
    return check_launch("score");
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" size_t dlwpcs_score_scratch_bytes(const dlwpcs_score_desc *d) {
    Plan P;
    if (make_plan(d, P) != DLWPCS_OK) return 0;
    return P.G.slabs > 1 ? (size_t)(P.groups * P.G.slabs * P.G.kc * SC_NM) * sizeof(double) : 0;
}

extern "C" int dlwpcs_score(const dlwpcs_score_desc *d, const float *a, const float *b, const float *c, const float *w, void *out,
                            int out_f32, void *scratch, size_t scratch_bytes, dlwpcs_stream_t stream) {
    Plan P;
    int rc = plan_of(d, P, false, 0);
    if (rc != DLWPCS_OK) return rc;
    return run<false>(d, P, a, b, c, w, out, out_f32, scratch, scratch_bytes, nullptr, stream);
}

extern "C" int dlwpcs_score_indexed(const dlwpcs_score_desc *d, const float *a, const float *b, const float *c, const float *w,
                                    const int32_t *row_dev, int64_t table_row_stride, void *out, int out_f32,
                                    void *scratch, size_t scratch_bytes, dlwpcs_stream_t stream) {
    Plan P;
    int rc = plan_of(d, P, true, table_row_stride);
    if (rc != DLWPCS_OK) return rc;
    if (!row_dev) return fail(DLWPCS_E_INVALID, "score_indexed: null table");
    return run<true>(d, P, a, b, c, w, out, out_f32, scratch, scratch_bytes, row_dev, stream);
}

extern "C" int dlwpcs_score_plan_info(const dlwpcs_score_desc *d, const void *a, const void *b, const void *c, const void *w,
                                      int indexed, int64_t table_row_stride, int32_t info[8]) {
    if (!info) return fail(DLWPCS_E_INVALID, "score_plan_info: null info");
    Plan P;
    int rc = plan_of(d, P, indexed != 0, table_row_stride);
    if (rc != DLWPCS_OK) return rc;
    const float *pa = (const float *)a;
    rc = settle(d, P, pa, (const float *)b, (const float *)c, (const float *)w);
    if (rc != DLWPCS_OK) return rc;
    const dim3 grid = launch_grid(P.G.nblk);
    info[0] = P.column ? 2 : P.vec ? 1 : 0;
    info[1] = P.G.slabs;
    info[2] = P.G.has_c ? P.G.cmode : -1;
    info[3] = P.G.has_w ? P.G.wmode : -1;
    info[4] = (int32_t)grid.x;
    info[5] = (int32_t)grid.y;
    info[6] = info[7] = 0;
    return DLWPCS_OK;
}
