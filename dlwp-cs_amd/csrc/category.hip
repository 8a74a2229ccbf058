// Category scores of an ensemble (dlwpcs_ensemble_category): per element the number of members at or below each of Q thresholds,
// k_j = #{i : x_i <= t_j}, and from it and o_j = 1{y <= t_j} the category probabilities, the Brier scores, the ranked probability
// score, that of a reference forecast and the codes 2 k_j + o_j a reliability diagram is counted from.  No sort: one lane owns an
// element (the 16-byte form: four neighbours along the last dim), holds the thresholds and the counters in registers (classes of
// 1, 2, 4, 8, 16 thresholds, unrolled at compile time; unused slots hold +inf and are never stored) and streams the members once.
// Nothing crosses lanes, no barrier, no scratch, no atomics, one launch.
//
// Every fp32 operation of the definition (include/dlwpcs.h) happens once, in the order written there, with contraction off, and
// the integers are exact: a float32 emulation reproduces the bits, and the 16-byte form gives the bits of the scalar form.
//
// No profiler tags: the launch profiler's registry is the convolution family's (tests/test_conv_coverage_tags.py closes it over the
// convolution case table), as for the other verification kernels.
#include "strided.h"

namespace dlwpcs {

namespace {

constexpr int CAT_THREADS = 256;
constexpr int CAT_MAXQ = DLWPCS_CATEGORY_MAX_Q;
constexpr int CAT_VEC_MAX_CLASS = 8;                // the 16-byte form holds 4 x (thresholds + counters) in registers
constexpr int CAT_UNROLL = 4;                       // members in flight per lane

struct CatGeom {
    int32_t M, Q, n_dims, fair;
    int32_t vmode;                                  // valid: -1 absent, 0 element by element, 1 16-byte loads
    int32_t tmode;                                  // thr: 0 element by element, 1 16-byte loads, 2 one vector for every element
    int32_t ovec;                                   // the 16-byte form may store 16 bytes (every output pointer allows it)
    int32_t small;                                  // every extent product fits 31 bits: 32-bit index arithmetic
    int64_t E, mstride, tstride;
    int64_t ext[DLWPCS_SCORE_MAX_DIMS], es[DLWPCS_SCORE_MAX_DIMS], vs[DLWPCS_SCORE_MAX_DIMS], ts[DLWPCS_SCORE_MAX_DIMS];
    float ref[CAT_MAXQ];
};

// offsets (elements) of element e in ens, valid and thr
__device__ __forceinline__ void cat_offsets(const CatGeom &G, int64_t e, int64_t &eo, int64_t &vo, int64_t &to) {
    flat_offsets_either<1>(G.small != 0, G.n_dims, G.ext, e, Strided{G.es, eo}, Strided{G.vs, vo}, Strided{G.ts, to});
}

template <int QC, bool VEC>
__global__ void __launch_bounds__(CAT_THREADS) ensemble_category_kernel(CatGeom G, const float *__restrict__ ens,
                                                                        const float *__restrict__ valid,
                                                                        const float *__restrict__ thr, float *__restrict__ o_prob,
                                                                        float *__restrict__ o_brier, float *__restrict__ o_rps,
                                                                        float *__restrict__ o_ref, int32_t *__restrict__ o_code) {
#pragma clang fp contract(off)
    constexpr int V = VEC ? 4 : 1;
    const int64_t item = flat_block() * CAT_THREADS + threadIdx.x;
    const int64_t e0 = item * V;
    if (e0 >= G.E) return;                              // (16-byte form: the last extent is a multiple of 4, so is E)
    int64_t eo, vo, to;
    cat_offsets(G, e0, eo, vo, to);
    const int M = G.M, Q = G.Q;
    const int64_t vl = G.n_dims ? G.vs[G.n_dims - 1] : 0, tl = G.n_dims ? G.ts[G.n_dims - 1] : 0;

    float t[QC][V];
    int32_t k[QC][V];
#pragma unroll
    for (int j = 0; j < QC; ++j) {
        if (j < Q) {
            const float *p = thr + to + (int64_t)j * G.tstride;
            if (VEC && G.tmode == 1) {
                load_chunk<V>(p, t[j]);
            } else {
#pragma unroll
                for (int v = 0; v < V; ++v) t[j][v] = p[v * tl];
            }
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) t[j][v] = pos_inf();
        }
#pragma unroll
        for (int v = 0; v < V; ++v) k[j][v] = 0;
    }

    bool bad[V];
#pragma unroll
    for (int v = 0; v < V; ++v) bad[v] = false;
    const float *pe = ens + eo;
    for (int i0 = 0; i0 < M; i0 += CAT_UNROLL) {
        float x[CAT_UNROLL][V];
#pragma unroll
        for (int u = 0; u < CAT_UNROLL; ++u) {
            if (i0 + u < M) {
                load_chunk<V>(pe + (int64_t)(i0 + u) * G.mstride, x[u]);
            } else {
#pragma unroll
                for (int v = 0; v < V; ++v) x[u][v] = pos_inf();
            }
        }
#pragma unroll
        for (int u = 0; u < CAT_UNROLL; ++u)
            if (i0 + u < M) {
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    bad[v] |= nonfinite(x[u][v]);
#pragma unroll
                    for (int j = 0; j < QC; ++j) k[j][v] += x[u][v] <= t[j][v] ? 1 : 0;
                }
            }
    }

    const bool has_y = G.vmode >= 0;
    float y[V];
#pragma unroll
    for (int v = 0; v < V; ++v) y[v] = 0.f;
    if (VEC && G.vmode == 1) {
        load_chunk<V>(valid + vo, y);
    } else if (has_y) {
#pragma unroll
        for (int v = 0; v < V; ++v) y[v] = valid[vo + v * vl];
    }

    const float fm = (float)M;
    const bool wide = VEC && G.ovec;
    float rps[V], ref[V];
    int32_t pair[V];
    bool anyt[V], ybad[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        rps[v] = 0.f; ref[v] = 0.f; pair[v] = 0; anyt[v] = false;
        ybad[v] = !has_y || nonfinite(y[v]);
    }
#pragma unroll
    for (int j = 0; j < QC; ++j)
        if (j < Q) {
            float pr[V], br[V];
            int32_t cd[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const bool tnan = t[j][v] != t[j][v];
                const int32_t kk = k[j][v], o = (has_y && y[v] <= t[j][v]) ? 1 : 0;
                const float ej = (float)(kk - o * M) / fm;
                const float b = ej * ej;
                const float dr = G.ref[j] - (float)o;
                rps[v] = rps[v] + b;
                ref[v] = ref[v] + dr * dr;
                pair[v] += kk * (M - kk);
                anyt[v] |= tnan;
                const bool miss = bad[v] || tnan;
                pr[v] = miss ? quiet_nan() : (float)kk / fm;
                br[v] = (miss || ybad[v]) ? quiet_nan() : b;
                cd[v] = (miss || ybad[v]) ? -1 : 2 * kk + o;
            }
            const int64_t at = (int64_t)j * G.E + e0;
            if (o_prob) store_chunk<V>(o_prob + at, pr, wide, 1);
            if (o_brier) store_chunk<V>(o_brier + at, br, wide, 1);
            if (o_code) store_chunk<V>(o_code + at, cd, wide, 1);
        }
    if (o_rps || o_ref) {
        float r[V], f[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const bool miss = bad[v] || ybad[v] || anyt[v];
            float s = rps[v];
            if (G.fair) s = s - (float)pair[v] / ((float)(M * M) * (float)(M - 1));
            r[v] = miss ? quiet_nan() : s;
            f[v] = miss ? quiet_nan() : ref[v];
        }
        if (o_rps) store_chunk<V>(o_rps + e0, r, wide, 1);
        if (o_ref) store_chunk<V>(o_ref + e0, f, wide, 1);
    }
}

struct CatPlan {
    CatGeom G;
    int cls;                                            // threshold slots: 1 .. 16
    bool vec_ok, vvec_ok, tvec_ok, tuniform, vec;
    int64_t nblk;
};

// everything the descriptor decides: the class, whether extents and strides allow 16-byte loads
int cat_plan(const dlwpcs_category_desc *d, CatPlan &P) {
    if (!d) return fail(DLWPCS_E_INVALID, "ensemble_category: null descriptor");
    if (d->M < 1) return fail(DLWPCS_E_INVALID, "ensemble_category: M = %d (at least 1 member)", d->M);
    if (d->Q < 1) return fail(DLWPCS_E_INVALID, "ensemble_category: Q = %d (at least 1 threshold)", d->Q);
    if (d->M > DLWPCS_CATEGORY_MAX_M)
        return fail(DLWPCS_E_UNSUPPORTED, "ensemble_category: M = %d, this build serves 1 <= M <= %d", d->M, DLWPCS_CATEGORY_MAX_M);
    if (d->Q > DLWPCS_CATEGORY_MAX_Q)
        return fail(DLWPCS_E_UNSUPPORTED, "ensemble_category: Q = %d, this build serves 1 <= Q <= %d", d->Q, DLWPCS_CATEGORY_MAX_Q);
    if (d->n_dims < 0 || d->n_dims > DLWPCS_SCORE_MAX_DIMS)
        return fail(DLWPCS_E_INVALID, "ensemble_category: n_dims %d out of range", d->n_dims);
    if (d->fair && d->M < 2) return fail(DLWPCS_E_INVALID, "ensemble_category: the fair score needs at least 2 members");
    CatGeom &G = P.G;
    memset(&G, 0, sizeof(G));
    G.M = d->M;
    G.Q = d->Q;
    G.n_dims = d->n_dims;
    G.fair = d->fair != 0;
    G.mstride = d->member_stride;
    G.tstride = d->thr_stride;
    G.E = 1;
    for (int j = 0; j < CAT_MAXQ; ++j) G.ref[j] = d->ref_prob[j];
    const int n = d->n_dims;
    bool vec = n >= 1 && d->member_stride % 4 == 0, vvec = n >= 1, tvec = n >= 1 && d->thr_stride % 4 == 0, uni = true;
    for (int i = 0; i < n; ++i) {
        const int64_t e = d->ext[i];
        if (e < 0 || e >= (1ll << 31)) return fail(DLWPCS_E_INVALID, "ensemble_category: extent %lld of dim %d", (long long)e, i);
        G.ext[i] = e;
        G.es[i] = d->stride[0][i];
        G.vs[i] = d->stride[1][i];
        G.ts[i] = d->stride[2][i];
        uni = uni && G.ts[i] == 0;
        if (i == n - 1) {
            vec = vec && e % 4 == 0 && G.es[i] == 1;
            vvec = vvec && G.vs[i] == 1;
            tvec = tvec && G.ts[i] == 1;
        } else {
            vec = vec && G.es[i] % 4 == 0;
            vvec = vvec && G.vs[i] % 4 == 0;
            tvec = tvec && G.ts[i] % 4 == 0;
        }
        G.E *= e;
        if (G.E >= (1ll << 40)) return fail(DLWPCS_E_UNSUPPORTED, "ensemble_category: too many elements");
    }
    if ((int64_t)d->Q * G.E >= (1ll << 44)) return fail(DLWPCS_E_UNSUPPORTED, "ensemble_category: too many elements");
    G.small = G.E < (1ll << 31);
    P.cls = d->Q <= 1 ? 1 : d->Q <= 2 ? 2 : d->Q <= 4 ? 4 : d->Q <= 8 ? 8 : 16;
    P.vec_ok = vec && P.cls <= CAT_VEC_MAX_CLASS;
    P.vvec_ok = vvec;
    P.tvec_ok = tvec;
    P.tuniform = uni;
    return DLWPCS_OK;
}

// what the operand pointers settle (NULL and alignment only, nothing is read): the load forms and with them the grid
int cat_settle(CatPlan &P, const void *ens, const void *valid, const void *thr) {
    if (P.G.E > 0 && (!ens || !thr)) return fail(DLWPCS_E_INVALID, "ensemble_category: null ensemble or thresholds");
    if ((((uintptr_t)ens) | ((uintptr_t)valid) | ((uintptr_t)thr)) & 3)
        return fail(DLWPCS_E_INVALID, "ensemble_category: an operand is not aligned to its 4-byte elements");
    P.vec = P.vec_ok && aligned16(ens);
    P.G.vmode = !valid ? -1 : (P.vec && P.vvec_ok && aligned16(valid)) ? 1 : 0;
    P.G.tmode = P.tuniform ? 2 : (P.vec && P.tvec_ok && aligned16(thr)) ? 1 : 0;
    const int64_t per_blk = (int64_t)CAT_THREADS * (P.vec ? 4 : 1);
    P.nblk = (P.G.E + per_blk - 1) / per_blk;
    if (P.nblk > MAX_BLOCKS) return fail(DLWPCS_E_UNSUPPORTED, "ensemble_category: %lld workgroups is too many", (long long)P.nblk);
    return DLWPCS_OK;
}

template <int QC, bool VEC>
void cat_launch(const CatPlan &P, const float *ens, const float *valid, const float *thr, float *pr, float *br, float *rps, float *ref,
                int32_t *code, hipStream_t s) {
    hipLaunchKernelGGL((ensemble_category_kernel<QC, VEC>), launch_grid(P.nblk), dim3(CAT_THREADS), 0, s, P.G, ens, valid, thr, pr, br,
                       rps, ref, code);
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" int dlwpcs_ensemble_category(const dlwpcs_category_desc *d, const float *ens, const float *valid, const float *thr,
                                        float *out_prob, float *out_brier, float *out_rps, float *out_rps_ref, int32_t *out_code,
                                        dlwpcs_stream_t stream) {
    CatPlan P;
    int rc = cat_plan(d, P);
    if (rc != DLWPCS_OK) return rc;
    if (P.G.E == 0) return DLWPCS_OK;
    rc = cat_settle(P, ens, valid, thr);
    if (rc != DLWPCS_OK) return rc;
    if (!valid && (out_brier || out_rps || out_rps_ref || out_code))
        return fail(DLWPCS_E_INVALID, "ensemble_category: brier, rps, rps_ref and code need a verification");
    if (!out_prob && !out_brier && !out_rps && !out_rps_ref && !out_code)
        return fail(DLWPCS_E_INVALID, "ensemble_category: no output requested");
    const uintptr_t outs = ((uintptr_t)out_prob) | ((uintptr_t)out_brier) | ((uintptr_t)out_rps) | ((uintptr_t)out_rps_ref) |
                           ((uintptr_t)out_code);
    if (outs & 3) return fail(DLWPCS_E_INVALID, "ensemble_category: an output is not aligned to its 4-byte elements");
    P.G.ovec = !(outs & 15);
    hipStream_t s = (hipStream_t)stream;
#define CAT_GO(QC) cat_launch<QC, false>(P, ens, valid, thr, out_prob, out_brier, out_rps, out_rps_ref, out_code, s)
#define CAT_GO_VEC(QC) \
    do { if (P.vec) cat_launch<QC, true>(P, ens, valid, thr, out_prob, out_brier, out_rps, out_rps_ref, out_code, s); \
         else CAT_GO(QC); } while (0)
    switch (P.cls) {
    case 1: CAT_GO_VEC(1); break;
    case 2: CAT_GO_VEC(2); break;
    case 4: CAT_GO_VEC(4); break;
    case 8: CAT_GO_VEC(8); break;
    default: CAT_GO(16); break;
    }
#undef CAT_GO_VEC
#undef CAT_GO
    return check_launch("ensemble_category");
}

extern "C" int dlwpcs_ensemble_category_plan_info(const dlwpcs_category_desc *d, const void *ens, const void *valid, const void *thr,
                                                  int32_t info[8]) {
    if (!info) return fail(DLWPCS_E_INVALID, "ensemble_category_plan_info: null info");
    CatPlan P;
    int rc = cat_plan(d, P);
    if (rc != DLWPCS_OK) return rc;
    rc = cat_settle(P, ens, valid, thr);
    if (rc != DLWPCS_OK) return rc;
    const dim3 grid = launch_grid(P.nblk);
    info[0] = P.cls;
    info[1] = P.vec ? 1 : 0;
    info[2] = P.G.vmode;
    info[3] = P.G.tmode;
    info[4] = (int32_t)grid.x;
    info[5] = (int32_t)grid.y;
    info[6] = CAT_THREADS;
    info[7] = 0;
    return DLWPCS_OK;
}
