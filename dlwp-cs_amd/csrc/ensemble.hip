// Ensemble scores (dlwpcs_ensemble_stats): the member axis x_1..x_M of an fp32 ensemble collapsed element by element into the mean,
// the spread, the continuous ranked probability score against a verification y, and the rank of y among the members.  One lane
// owns an element (the 16-byte form: four neighbours along the last dim) and does everything for it; nothing crosses lanes, no
// barrier, no scratch, one launch.
//
// Differences first.  Mean and variance are formed from t_i = x_i - x_1 (two passes: tbar = sum t_i / M, then sum (t_i - tbar)^2),
// the score from d_i = x_i - y: an offset of the data (280 K under a spread of 1 K) never reaches the error.
//
// CRPS without A and B.  With the d_i sorted, crps = integral (F(t) - 1{t >= 0})^2 dt is a sum over the gaps between neighbours:
// below zero gap k (k members to its left) weighs (k / M)^2, above zero ((M - k) / M)^2, the gap that holds zero is cut there, and
// the stretch between zero and an ensemble that lies wholly to one side weighs 1.  Every term is >= 0, so the sum is as accurate
// relative to the score itself as a sum of M terms can be -- the textbook A - B / 2 cancels.  The fair form subtracts
// sum_k k (M - k) gap_k / (M^2 (M - 1)) (= B / (2 (M - 1))), again a sum of non-negative terms.  M identical members: every gap is
// exactly 0 and the tail is |d|, so crps is the fp32 |x - y| bit for bit.
//
// Order.  M <= 32: the d_i sit in registers and go through a bitonic network in its all-ascending form (a flip pass, then
// half-cleaners), unrolled so that every index is a compile-time constant (a register array indexed at run time would live in
// scratch memory); classes of 4, 8, 16 and 32 slots, the unused slots hold +inf, sort to the end and are never summed.
// 33 <= M <= 128: the members lie in a lane-private column of LDS laid out [member][lane] (a lane's bank is its lane number: no
// conflicts whatever row a lane is at), classes of 64 and 128 slots with 256 and 128 lanes per workgroup (64 KiB each, two
// workgroups per CU).  Runs of 32 go through the register network and back; the sorted runs are then merged as a stream, one head
// per run in registers, straight into the gap sums.  About 5 LDS accesses per member (a whole network in LDS: 55 at M = 128).
#include "strided.h"

namespace dlwpcs {

constexpr int ENS_THREADS = 256;                    // register classes
constexpr int ENS_LDS_FLOATS = 16384;               // LDS classes: slots x lanes (64 KiB)
constexpr int ENS_RUN = 32;                         // LDS classes: members sorted in registers at a time
constexpr int ENS_VEC_MAX_CLASS = 16;               // the 16-byte form holds 4 x slots members in registers

struct EnsGeom {
    int32_t M, n_dims, fair, ddof, variance;
    int32_t vmode;                                  // valid: -1 absent, 0 element by element, 1 16-byte loads
    int32_t ovec;                                   // the 16-byte form may store 16 bytes (every output pointer allows it)
    int32_t small;                                  // every extent product fits 31 bits: 32-bit index arithmetic
    int64_t E, mstride;
    int64_t ext[DLWPCS_SCORE_MAX_DIMS], es[DLWPCS_SCORE_MAX_DIMS], vs[DLWPCS_SCORE_MAX_DIMS];
};

// offsets (elements) of element e in ens and valid
__device__ __forceinline__ void ens_offsets(const EnsGeom &G, int64_t e, int64_t &eo, int64_t &vo) {
    flat_offsets_either<1>(G.small != 0, G.n_dims, G.ext, e, Strided{G.es, eo}, Strided{G.vs, vo});
}

struct EnsOut { float mean, spread, crps; int32_t rank; };

// what follows the sums, spelled once so that every class rounds alike
__device__ __forceinline__ float ens_spread_of(float q, const EnsGeom &G) {
    const float var = q / (float)(G.M - G.ddof);
    return G.variance ? var : sqrtf(var);
}
struct EnsGapSums {
    float below = 0.f, above = 0.f, pair = 0.f;
    __device__ __forceinline__ void add(int k, int M, float lo, float hi) {     // gap k: k members at or left of lo
#pragma clang fp contract(off)
        const float bl = fminf(hi, 0.f) - fminf(lo, 0.f), ab = fmaxf(hi, 0.f) - fmaxf(lo, 0.f);
        below = __builtin_fmaf((float)(k * k), bl, below);
        above = __builtin_fmaf((float)((M - k) * (M - k)), ab, above);
        pair = __builtin_fmaf((float)(k * (M - k)), hi - lo, pair);
    }
    __device__ __forceinline__ float crps(float first, float last, const EnsGeom &G) const {
#pragma clang fp contract(off)
        const float m2 = (float)(G.M * G.M);
        const float tails = fmaxf(first, 0.f) + fmaxf(-last, 0.f);              // at most one of the two is not zero
        const float c = tails + (below + above) / m2;
        return G.fair ? c - pair / (m2 * (float)(G.M - 1)) : c;
    }
};

#define ENS_CE(A, B) do { const float ce_a = (A), ce_b = (B); (A) = fminf(ce_a, ce_b); (B) = fmaxf(ce_a, ce_b); } while (0)

// ---- members in registers ------------------------------------------------------------------------------------------------
template <int MC>
__device__ __forceinline__ void ens_sort_regs(float (&d)[MC]) {
#pragma unroll
    for (int k = 2; k <= MC; k *= 2) {
#pragma unroll
        for (int i = 0; i < MC; ++i) {
            const int l = i ^ (k - 1);
            if (l > i) ENS_CE(d[i], d[l]);
        }
#pragma unroll
        for (int j = k / 4; j > 0; j /= 2) {
#pragma unroll
            for (int i = 0; i < MC; ++i) {
                const int l = i ^ j;
                if (l > i) ENS_CE(d[i], d[l]);
            }
        }
    }
}

template <int MC>
__device__ __forceinline__ EnsOut ens_element_regs(float (&x)[MC], float y, const EnsGeom &G, bool want_ms, bool want_crps) {
#pragma clang fp contract(off)
    const int M = G.M;
    const bool has_y = G.vmode >= 0;
    EnsOut o;
    bool bad = false;
    int rank = 0;
#pragma unroll
    for (int i = 0; i < MC; ++i)
        if (i < M) {
            bad |= nonfinite(x[i]);
            rank += (has_y && x[i] < y) ? 1 : 0;
        }
    const bool ybad = has_y && nonfinite(y);
    o.mean = o.spread = o.crps = quiet_nan();
    if (want_ms) {
        const float p = x[0];
        float s = 0.f;
#pragma unroll
        for (int i = 1; i < MC; ++i)
            if (i < M) s += x[i] - p;
        const float tbar = s / (float)M;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < MC; ++i)
            if (i < M) {
                const float dv = (x[i] - p) - tbar;
                q = __builtin_fmaf(dv, dv, q);
            }
        if (!bad) {
            o.mean = p + tbar;
            o.spread = ens_spread_of(q, G);
        }
    }
    if (want_crps) {
#pragma unroll
        for (int i = 0; i < MC; ++i) x[i] = i < M ? x[i] - y : pos_inf();
        ens_sort_regs<MC>(x);
        EnsGapSums g;
        float last = x[0];
#pragma unroll
        for (int k = 1; k < MC; ++k)
            if (k < M) {
                g.add(k, M, x[k - 1], x[k]);
                last = x[k];
            }
        if (!bad && !ybad) o.crps = g.crps(x[0], last, G);
    }
    o.rank = (bad || ybad) ? -1 : rank;
    return o;
}

template <int MC, bool VEC>
__global__ void __launch_bounds__(ENS_THREADS) ensemble_reg_kernel(EnsGeom G, const float *__restrict__ ens,
                                                                   const float *__restrict__ valid, float *__restrict__ o_mean,
                                                                   float *__restrict__ o_spread, float *__restrict__ o_crps,
                                                                   int32_t *__restrict__ o_rank) {
    constexpr int V = VEC ? 4 : 1;
    const int64_t item = flat_block() * ENS_THREADS + threadIdx.x;
    const int64_t e0 = item * V;
    if (e0 >= G.E) return;                              // (16-byte form: the last extent is a multiple of 4, so is E)
    int64_t eo, vo;
    ens_offsets(G, e0, eo, vo);
    const int M = G.M;
    float x[V][MC];
#pragma unroll
    for (int i = 0; i < MC; ++i) {
        if (i < M) {
            const float *p = ens + eo + (int64_t)i * G.mstride;
            if constexpr (VEC) {
                const float4 t = *reinterpret_cast<const float4 *>(p);
                x[0][i] = t.x; x[V > 1 ? 1 : 0][i] = t.y; x[V > 2 ? 2 : 0][i] = t.z; x[V - 1][i] = t.w;
            } else {
                x[0][i] = *p;
            }
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) x[v][i] = 0.f;
        }
    }
    float y[V];
#pragma unroll
    for (int v = 0; v < V; ++v) y[v] = 0.f;
    if (G.vmode == 1 && VEC) {
        const float4 t = *reinterpret_cast<const float4 *>(valid + vo);
        y[0] = t.x; y[V > 1 ? 1 : 0] = t.y; y[V > 2 ? 2 : 0] = t.z; y[V - 1] = t.w;
    } else if (G.vmode >= 0) {
        const int64_t vl = G.n_dims ? G.vs[G.n_dims - 1] : 0;
#pragma unroll
        for (int v = 0; v < V; ++v) y[v] = valid[vo + v * vl];
    }
    const bool want_ms = o_mean || o_spread, want_crps = o_crps != nullptr;
    EnsOut o[V];
#pragma unroll
    for (int v = 0; v < V; ++v) o[v] = ens_element_regs<MC>(x[v], y[v], G, want_ms, want_crps);
    if (VEC && G.ovec) {
        if (o_mean) *reinterpret_cast<float4 *>(o_mean + e0) = make_float4(o[0].mean, o[V > 1 ? 1 : 0].mean, o[V > 2 ? 2 : 0].mean, o[V - 1].mean);
        if (o_spread) *reinterpret_cast<float4 *>(o_spread + e0) = make_float4(o[0].spread, o[V > 1 ? 1 : 0].spread, o[V > 2 ? 2 : 0].spread, o[V - 1].spread);
        if (o_crps) *reinterpret_cast<float4 *>(o_crps + e0) = make_float4(o[0].crps, o[V > 1 ? 1 : 0].crps, o[V > 2 ? 2 : 0].crps, o[V - 1].crps);
        if (o_rank) *reinterpret_cast<int4 *>(o_rank + e0) = make_int4(o[0].rank, o[V > 1 ? 1 : 0].rank, o[V > 2 ? 2 : 0].rank, o[V - 1].rank);
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if (o_mean) o_mean[e0 + v] = o[v].mean;
            if (o_spread) o_spread[e0 + v] = o[v].spread;
            if (o_crps) o_crps[e0 + v] = o[v].crps;
            if (o_rank) o_rank[e0 + v] = o[v].rank;
        }
    }
}

// ---- members in LDS ------------------------------------------------------------------------------------------------------
template <int MC>
__global__ void __launch_bounds__(ENS_LDS_FLOATS / MC) ensemble_lds_kernel(EnsGeom G, const float *__restrict__ ens,
                                                                           const float *__restrict__ valid,
                                                                           float *__restrict__ o_mean, float *__restrict__ o_spread,
                                                                           float *__restrict__ o_crps, int32_t *__restrict__ o_rank) {
#pragma clang fp contract(off)
    constexpr int T = ENS_LDS_FLOATS / MC;              // lanes of a workgroup = stride between a lane's members
    __shared__ float s_col[MC * T];
    const int64_t e = flat_block() * T + threadIdx.x;
    if (e >= G.E) return;                               // (no barrier anywhere: a column belongs to its lane)
    float *col = s_col + threadIdx.x;                   // member i of this lane: col[i * T]
    int64_t eo, vo;
    ens_offsets(G, e, eo, vo);
    const int M = G.M;
    const bool has_y = G.vmode >= 0;
    const float y = has_y ? valid[vo] : 0.f;
    bool bad = false;
    int rank = 0;
    float p = 0.f, s = 0.f;
    constexpr int NR = MC / ENS_RUN;
#pragma unroll
    for (int r = 0; r < NR; ++r)
        if (r * ENS_RUN < M) {                          // (uniform) a run's loads are issued together: 32 in flight per lane
            float xr[ENS_RUN];
#pragma unroll
            for (int i = 0; i < ENS_RUN; ++i)
                xr[i] = r * ENS_RUN + i < M ? ens[eo + (int64_t)(r * ENS_RUN + i) * G.mstride] : 0.f;
#pragma unroll
            for (int i = 0; i < ENS_RUN; ++i)
                if (r * ENS_RUN + i < M) {
                    col[(r * ENS_RUN + i) * T] = xr[i];
                    bad |= nonfinite(xr[i]);
                    rank += (has_y && xr[i] < y) ? 1 : 0;
                    if (r == 0 && i == 0) p = xr[0]; else s += xr[i] - p;
                }
        }
    const bool ybad = has_y && nonfinite(y);
    float mean = quiet_nan(), spread = quiet_nan(), crps = quiet_nan();
    if (o_mean || o_spread) {
        const float tbar = s / (float)M;
        float q = 0.f;
        for (int i = 0; i < M; ++i) {
            const float dv = (col[i * T] - p) - tbar;
            q = __builtin_fmaf(dv, dv, q);
        }
        if (!bad) {
            mean = p + tbar;
            spread = ens_spread_of(q, G);
        }
    }
    if (o_crps) {
        // runs of 32: each goes through the register network and back into its rows, then the sorted runs are merged as a stream
        // (one head per run in registers, the smallest leaves; ties: the first run) that feeds the gap sums -- the merged order
        // is never stored
        float head[NR];
        int pos[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            head[r] = pos_inf();
            pos[r] = ENS_RUN;
            if (r * ENS_RUN < M) {                      // (uniform: a run without members stays exhausted)
                float d[ENS_RUN];
#pragma unroll
                for (int i = 0; i < ENS_RUN; ++i) d[i] = r * ENS_RUN + i < M ? col[(r * ENS_RUN + i) * T] - y : pos_inf();
                ens_sort_regs<ENS_RUN>(d);
#pragma unroll
                for (int i = 1; i < ENS_RUN; ++i) col[(r * ENS_RUN + i) * T] = d[i];
                head[r] = d[0];
                pos[r] = 0;
            }
        }
        EnsGapSums g;
        float first = 0.f, lo = 0.f;
        for (int k = 0; k < M; ++k) {
            float hi = head[0];
#pragma unroll
            for (int r = 1; r < NR; ++r) hi = fminf(hi, head[r]);
            int sel = -1, row = 0;                      // the first run whose head leaves; one LDS read per step
#pragma unroll
            for (int r = NR - 1; r >= 0; --r)
                if (head[r] == hi && pos[r] < ENS_RUN) sel = r;
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if (sel == r) row = r * ENS_RUN + ++pos[r];
            const float fresh = (sel >= 0 && (row & (ENS_RUN - 1))) ? col[row * T] : pos_inf();      // (row % 32 == 0: the run is exhausted)
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if (sel == r) head[r] = fresh;
            if (k == 0) first = hi; else g.add(k, M, lo, hi);
            lo = hi;
        }
        if (!bad && !ybad) crps = g.crps(first, lo, G);
    }
    if (o_mean) o_mean[e] = mean;
    if (o_spread) o_spread[e] = spread;
    if (o_crps) o_crps[e] = crps;
    if (o_rank) o_rank[e] = (bad || ybad) ? -1 : rank;
}

namespace {

struct EnsPlan {
    EnsGeom G;
    int cls;                                            // slots: 4 .. 128
    bool lds, vec_ok, vvec_ok, vec;
    int threads, per_lane;
    int64_t nblk;
};

// everything the descriptor decides: the class, whether extents and strides allow 16-byte loads
int ens_plan(const dlwpcs_ensemble_desc *d, EnsPlan &P) {
    if (!d) return fail(DLWPCS_E_INVALID, "ensemble_stats: null descriptor");
    if (d->M < 2) return fail(DLWPCS_E_INVALID, "ensemble_stats: M = %d (at least 2 members)", d->M);
    if (d->M > DLWPCS_ENSEMBLE_MAX_M)
        return fail(DLWPCS_E_UNSUPPORTED, "ensemble_stats: M = %d, this build serves 2 <= M <= %d", d->M, DLWPCS_ENSEMBLE_MAX_M);
    if (d->n_dims < 0 || d->n_dims > DLWPCS_SCORE_MAX_DIMS)
        return fail(DLWPCS_E_INVALID, "ensemble_stats: n_dims %d out of range", d->n_dims);
    if (d->ddof != 0 && d->ddof != 1) return fail(DLWPCS_E_INVALID, "ensemble_stats: ddof = %d (0 or 1)", d->ddof);
    EnsGeom &G = P.G;
    memset(&G, 0, sizeof(G));
    G.M = d->M;
    G.n_dims = d->n_dims;
    G.fair = d->fair != 0;
    G.ddof = d->ddof;
    G.variance = d->variance != 0;
    G.mstride = d->member_stride;
    G.E = 1;
    const int n = d->n_dims;
    bool vec = n >= 1 && d->member_stride % 4 == 0, vvec = n >= 1;
    for (int i = 0; i < n; ++i) {
        const int64_t e = d->ext[i];
        if (e < 0 || e >= (1ll << 31)) return fail(DLWPCS_E_INVALID, "ensemble_stats: extent %lld of dim %d", (long long)e, i);
        G.ext[i] = e;
        G.es[i] = d->stride[0][i];
        G.vs[i] = d->stride[1][i];
        if (i == n - 1) {
            vec = vec && e % 4 == 0 && G.es[i] == 1;
            vvec = vvec && G.vs[i] == 1;
        } else {
            vec = vec && G.es[i] % 4 == 0;
            vvec = vvec && G.vs[i] % 4 == 0;
        }
        G.E *= e;
        if (G.E >= (1ll << 40)) return fail(DLWPCS_E_UNSUPPORTED, "ensemble_stats: too many elements");
    }
    G.small = G.E < (1ll << 31);
    P.cls = d->M <= 4 ? 4 : d->M <= 8 ? 8 : d->M <= 16 ? 16 : d->M <= 32 ? 32 : d->M <= 64 ? 64 : 128;
    P.lds = P.cls > 32;
    P.vec_ok = vec && P.cls <= ENS_VEC_MAX_CLASS;
    P.vvec_ok = vvec;
    return DLWPCS_OK;
}

// what the operand pointers settle (NULL and alignment only, nothing is read): the load forms and with them the grid.  The entry
// point launches exactly what this leaves in P; dlwpcs_ensemble_plan_info reports it.
int ens_settle(EnsPlan &P, const void *ens, const void *valid) {
    if (P.G.E > 0 && !ens) return fail(DLWPCS_E_INVALID, "ensemble_stats: null ensemble");
    if ((((uintptr_t)ens) | ((uintptr_t)valid)) & 3)
        return fail(DLWPCS_E_INVALID, "ensemble_stats: an operand is not aligned to its 4-byte elements");
    P.vec = P.vec_ok && aligned16(ens);
    P.G.vmode = !valid ? -1 : (P.vec && P.vvec_ok && aligned16(valid)) ? 1 : 0;
    P.threads = P.lds ? ENS_LDS_FLOATS / P.cls : ENS_THREADS;
    P.per_lane = P.vec ? 4 : 1;
    const int64_t per_blk = (int64_t)P.threads * P.per_lane;
    P.nblk = (P.G.E + per_blk - 1) / per_blk;
    if (P.nblk > MAX_BLOCKS) return fail(DLWPCS_E_UNSUPPORTED, "ensemble_stats: %lld workgroups is too many", (long long)P.nblk);
    return DLWPCS_OK;
}

// No profiler tags: the launch profiler's registry is the convolution family's (tests/test_conv_coverage_tags.py closes it over the
// convolution case table), as for the other verification kernels.
template <int MC, bool VEC>
void ens_launch_reg(const EnsPlan &P, const float *ens, const float *valid, float *m, float *sp, float *c, int32_t *r, hipStream_t s) {
    hipLaunchKernelGGL((ensemble_reg_kernel<MC, VEC>), launch_grid(P.nblk), dim3(ENS_THREADS), 0, s, P.G, ens, valid, m, sp, c, r);
}
template <int MC>
void ens_launch_lds(const EnsPlan &P, const float *ens, const float *valid, float *m, float *sp, float *c, int32_t *r, hipStream_t s) {
    hipLaunchKernelGGL((ensemble_lds_kernel<MC>), launch_grid(P.nblk), dim3(ENS_LDS_FLOATS / MC), 0, s, P.G, ens, valid, m, sp, c, r);
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" int dlwpcs_ensemble_stats(const dlwpcs_ensemble_desc *d, const float *ens, const float *valid, float *out_mean,
                                     float *out_spread, float *out_crps, int32_t *out_rank, dlwpcs_stream_t stream) {
    EnsPlan P;
    int rc = ens_plan(d, P);
    if (rc != DLWPCS_OK) return rc;
    if (P.G.E == 0) return DLWPCS_OK;
    rc = ens_settle(P, ens, valid);
    if (rc != DLWPCS_OK) return rc;
    if (!valid && (out_crps || out_rank)) return fail(DLWPCS_E_INVALID, "ensemble_stats: crps and rank need a verification");
    if (!out_mean && !out_spread && !out_crps && !out_rank) return fail(DLWPCS_E_INVALID, "ensemble_stats: no output requested");
    const uintptr_t outs = ((uintptr_t)out_mean) | ((uintptr_t)out_spread) | ((uintptr_t)out_crps) | ((uintptr_t)out_rank);
    if (outs & 3) return fail(DLWPCS_E_INVALID, "ensemble_stats: an output is not aligned to its 4-byte elements");
    P.G.ovec = !(outs & 15);
    hipStream_t s = (hipStream_t)stream;
#define ENS_REG(MC) \
    do { if (P.vec) ens_launch_reg<MC, true>(P, ens, valid, out_mean, out_spread, out_crps, out_rank, s); \
         else ens_launch_reg<MC, false>(P, ens, valid, out_mean, out_spread, out_crps, out_rank, s); } while (0)
    switch (P.cls) {
    case 4: ENS_REG(4); break;
    case 8: ENS_REG(8); break;
    case 16: ENS_REG(16); break;
    case 32: ens_launch_reg<32, false>(P, ens, valid, out_mean, out_spread, out_crps, out_rank, s); break;
    case 64: ens_launch_lds<64>(P, ens, valid, out_mean, out_spread, out_crps, out_rank, s); break;
    default: ens_launch_lds<128>(P, ens, valid, out_mean, out_spread, out_crps, out_rank, s); break;
    }
#undef ENS_REG
    return check_launch("ensemble_stats");
}

extern "C" int dlwpcs_ensemble_plan_info(const dlwpcs_ensemble_desc *d, const void *ens, const void *valid, int32_t info[8]) {
    if (!info) return fail(DLWPCS_E_INVALID, "ensemble_plan_info: null info");
    EnsPlan P;
    int rc = ens_plan(d, P);
    if (rc != DLWPCS_OK) return rc;
    rc = ens_settle(P, ens, valid);
    if (rc != DLWPCS_OK) return rc;
    const dim3 grid = launch_grid(P.nblk);
    info[0] = P.cls;
    info[1] = P.vec ? 1 : 0;
    info[2] = P.G.vmode;
    info[3] = P.lds ? 1 : 0;
    info[4] = (int32_t)grid.x;
    info[5] = (int32_t)grid.y;
    info[6] = P.threads;
    info[7] = 0;
    return DLWPCS_OK;
}
