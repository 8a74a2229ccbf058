// The Gram matrix of a row set (dlwpcs_row_gram; include/dlwpcs.h states the definition): out[s, t] = sum over the columns of
// y_a[s] y_b[t] with y = r (x - mean), centred, weighted and with the excluded columns taken out while staging, so no second copy
// of the series exists.  b == NULL is the symmetric form (b = a): only the tile pairs on or below the diagonal are computed.
//
// Launch 1 (row_gram_column_kernel) reads the data once: a lane owns a column (or four adjacent ones), adds its rows in row order
// in fp64 and writes to scratch, indexed by the column number q, the fp32 mean of either operand (NaN: the column is excluded) and
// the weight root (0 there), and per workgroup the number of columns it kept.
//
// Launch 2 (row_gram_kernel): a 128 x 128 output tile per workgroup, four waves with a 64 x 64 quadrant each = 2 x 2 accumulators
// of v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered fmaf chain), k = the column number.  A chunk is [128 rows][32 columns] of y
// per operand in LDS (on a diagonal tile the A chunk is the B chunk and is staged once); the next chunk's global loads wait in
// registers under the current chunk's MFMAs.  The LDS row pitch is 36 words: a lane reads 16 bytes = the operands of two k steps,
// both halves of the wave the same address.  After a slab of 512 columns the lane widens its 64 fp32 accumulators into fp64 group
// sums and zeroes them; after a group of 16 slabs the group sums are added to the workgroup's fp64 totals, which wait in scratch
// between groups (split = 0), or go to scratch as they are (split = 1: the (tile pair, group) is a tile of its own and launch 3
// adds the group sums in group order -- the same additions, the same bits).
// Workgroup 0 also adds up the kept-column counts of launch 1 (integers: any order).
//
// The grid is RG_SLOTS persistent workgroups that stride over the int64 list of tiles; which workgroup computes a tile influences
// nothing.  No atomics, at most three launches.  No profiler tags, as for the other verification kernels.
#include <math.h>
#include "mfma_common.h"
#include "strided.h"

namespace dlwpcs {

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_TM = 128;                  // rows of either operand in a tile
constexpr int RG_KC = 32;                   // columns per staged chunk
constexpr int RG_PITCH = RG_KC + 4;         // words per LDS row (16-byte rows)
constexpr int RG_SLAB_CHUNKS = DLWPCS_ROW_GRAM_SLAB_COLS / RG_KC;
constexpr int RG_GROUP_CHUNKS = DLWPCS_ROW_GRAM_GROUP_SLABS * RG_SLAB_CHUNKS;
constexpr int RG_TILE_ELEMS = RG_TM * RG_TM;
constexpr int64_t RG_SLOTS = 256;           // persistent workgroups: one per compute unit (one wave per SIMD); placement only
constexpr int64_t RG_SPLIT_BELOW = 256;     // split < 0: groups get tiles of their own below this many tile pairs
constexpr int64_t RG_COL_BLOCKS = 2048;     // workgroups of the column pass at most (= kept-column counts in scratch)
constexpr int64_t RG_FINISH_BLOCKS = 2048;
static_assert(DLWPCS_ROW_GRAM_SLAB_COLS % RG_KC == 0, "a slab is a whole number of chunks");

struct RgGeom {
    RowsAddr A;                              // operand a; ext in elements, ncol = columns, nblk = tiles of the product launch
    int64_t b_sst[DLWPCS_SCORE_MAX_DIMS];    // operand b (the symmetric form: a's)
    int64_t b_row_stride;
    int64_t Ta, Tb, ld;
    int64_t ta, tb, pairs;                   // row tiles of a and of b, tile pairs
    int64_t n_chunk, n_slab, n_group;
    int64_t col_blocks;
    int32_t sym, split, center_a, center_b;
};

// tile pair -> (row tile of a, row tile of b); the symmetric form counts the pairs on or below the diagonal row by row
__device__ __forceinline__ void rg_pair(const RgGeom &G, int64_t p, int64_t &ti, int64_t &tj) {
    if (!G.sym) {
        ti = p / G.tb;
        tj = p % G.tb;
        return;
    }
    int64_t t = (int64_t)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while (t * (t + 1) / 2 > p) --t;
    while ((t + 1) * (t + 2) / 2 <= p) ++t;
    ti = t;
    tj = p - t * (t + 1) / 2;
}

// element e = (m * 2 + n) * 16 + i of thread tid -> row and column inside the tile (the C/D map of the 32 x 32 MFMA)
__device__ __forceinline__ void rg_elem(int tid, int e, int &row, int &col) {
    const int lane = tid & 63, wv = tid >> 6, i = e & 15, n = (e >> 4) & 1, m = e >> 5;
    row = (wv >> 1) * 64 + m * 32 + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
    col = (wv & 1) * 64 + n * 32 + (lane & 31);
}

// the store of one element: the symmetric form keeps s >= t and mirrors it
__device__ __forceinline__ void rg_store(const RgGeom &G, double *__restrict__ out, int64_t s, int64_t t, double v) {
    if (s >= G.Ta || t >= G.Tb) return;
    if (G.sym) {
        if (s < t) return;
        if (s != t) out[t * G.ld + s] = v;
    }
    out[s * G.ld + t] = v;
}

// launch 1: per column the means, the weight root and the exclusion; per workgroup the number of columns kept
template <bool VEC>
__global__ void __launch_bounds__(256) row_gram_column_kernel(RgGeom G, const float *__restrict__ a, const float *__restrict__ b,
                                                              const float *__restrict__ wr, const float *__restrict__ given_a,
                                                              const float *__restrict__ given_b, float *__restrict__ mu_a,
                                                              float *__restrict__ mu_b, float *__restrict__ rt,
                                                              float *__restrict__ mean_out, int64_t *__restrict__ part_cnt) {
    constexpr int V = VEC ? 4 : 1;
    __shared__ int s_cnt[256];
    const int64_t nchunk = G.A.ncol / V;    // (VEC: the last extent is a multiple of 4, so is the number of columns)
    const int64_t los = G.A.last_out_stride();
    int kept = 0;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < nchunk; c += G.col_blocks * 256) {
        const int64_t q = c * V;
        int64_t soa, sob, oo;
        flat_offsets<1, false>(G.A.n_inner, G.A.ext, q, Strided{G.A.sst, soa}, Strided{G.b_sst, sob}, Strided{G.A.ost, oo});
        double sum_a[V], sum_b[V];
        bool bad[V];
#pragma unroll
        for (int j = 0; j < V; ++j) { sum_a[j] = sum_b[j] = 0.0; bad[j] = false; }
        const float *pa = a + soa;
#pragma unroll 4
        for (int64_t t = 0; t < G.Ta; ++t) {
            float x[V];
            load_chunk<V>(pa + t * G.A.src_row_stride, x);
#pragma unroll
            for (int j = 0; j < V; ++j) { sum_a[j] += (double)x[j]; bad[j] |= nonfinite(x[j]); }
        }
        if (!G.sym) {
            const float *pb = b + sob;
#pragma unroll 4
            for (int64_t t = 0; t < G.Tb; ++t) {
                float x[V];
                load_chunk<V>(pb + t * G.b_row_stride, x);
#pragma unroll
                for (int j = 0; j < V; ++j) { sum_b[j] += (double)x[j]; bad[j] |= nonfinite(x[j]); }
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int64_t o = oo + j * los;
            float r = wr ? wr[o] : 1.f;
            bool ex = bad[j] || nonfinite(r);
            float ma = 0.f, mb = 0.f;
            if (G.center_a == 1) ma = (float)(sum_a[j] / (double)G.Ta);
            else if (G.center_a == 2) { ma = given_a[o]; ex |= ma != ma; }
            if (!G.sym) {
                if (G.center_b == 1) mb = (float)(sum_b[j] / (double)G.Tb);
                else if (G.center_b == 2) { mb = given_b[o]; ex |= mb != mb; }
            }
            if (ex) { ma = mb = quiet_nan(); r = 0.f; }
            mu_a[q + j] = ma;
            if (!G.sym) mu_b[q + j] = mb;
            rt[q + j] = r;
            if (mean_out) mean_out[o] = ma;
            kept += ex ? 0 : 1;
        }
    }
    s_cnt[threadIdx.x] = kept;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_cnt[threadIdx.x] += s_cnt[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part_cnt[blockIdx.x] = s_cnt[0];
}

// launch 2: the products
template <bool VEC>
__global__ void __launch_bounds__(RG_THREADS) row_gram_kernel(RgGeom G, const float *__restrict__ a, const float *__restrict__ b,
                                                              const float *__restrict__ mu_a, const float *__restrict__ mu_b,
                                                              const float *__restrict__ rt, const int64_t *__restrict__ part_cnt,
                                                              int64_t *__restrict__ n_valid, double *__restrict__ partial,
                                                              double *__restrict__ out) {
    constexpr int NLD = VEC ? 4 : 16;                   // loads of a thread per chunk and operand
    constexpr int NE = VEC ? 4 : 1;
    constexpr int ld_rows = VEC ? 32 : 8;
    __shared__ __attribute__((aligned(16))) float s_y[2][RG_TM * RG_PITCH];
    __shared__ int64_t s_cnt[RG_THREADS];

    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    const int qi = wv >> 1, qj = wv & 1;

    if (n_valid && blockIdx.x == 0) {
        int64_t n = 0;
        for (int64_t i = tid; i < G.col_blocks; i += RG_THREADS) n += part_cnt[i];
        s_cnt[tid] = n;
        __syncthreads();
        for (int w = RG_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) s_cnt[tid] += s_cnt[tid + w];
            __syncthreads();
        }
        if (tid == 0) *n_valid = s_cnt[0];
    }

    // staging: the columns of this thread's loads are the same in every row, its rows are ld_row0 + i * ld_rows
    const int ld_col = VEC ? (tid & 7) * 4 : tid & 31;
    const int ld_row0 = VEC ? tid >> 3 : tid >> 5;

    for (int64_t tile = blockIdx.x; tile < G.A.nblk; tile += gridDim.x) {
        const int64_t pair = G.split ? tile / G.n_group : tile;
        const int64_t g_lo = G.split ? tile % G.n_group : 0, g_hi = G.split ? g_lo + 1 : G.n_group;
        int64_t ti, tj;
        rg_pair(G, pair, ti, tj);
        const bool diag = G.sym && ti == tj;
        const int64_t row_a0 = ti * RG_TM, row_b0 = tj * RG_TM;
        // whole 32-row blocks past the last row are skipped (uniform over the wave); rows past it inside a block are staged
        // as they come and meet only elements that are not stored
        const bool on_m0 = row_a0 + qi * 64 < G.Ta, on_m1 = row_a0 + qi * 64 + 32 < G.Ta;
        const bool on_n0 = row_b0 + qj * 64 < G.Tb, on_n1 = row_b0 + qj * 64 + 32 < G.Tb;

        // the running total of a walking workgroup waits in scratch between groups (64 more fp64 per lane do not fit the registers)
        double grp[4][16];
        f32x16 acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) { grp[u][i] = 0.0; acc[u][i] = 0.f; }
        double *ws = partial + ((G.split ? tile : (int64_t)blockIdx.x) * RG_THREADS + tid) * 64;   // [tile or workgroup][thread][element]

        int64_t c_hi = g_hi * RG_GROUP_CHUNKS;
        if (c_hi > G.n_chunk) c_hi = G.n_chunk;
        const int64_t c_lo = g_lo * RG_GROUP_CHUNKS;

        float xa[NLD][NE], xb[NLD][NE], cma[NE], cmb[NE], cr[NE];
        auto fetch = [&](int64_t c) {
            const int64_t q = c * RG_KC + ld_col;
            const bool ok = q < G.A.ncol;               // (VEC: the four columns of a chunk are inside together)
            int64_t soa = 0, sob = 0;
            if (ok) flat_offsets<1, false>(G.A.n_inner, G.A.ext, q, Strided{G.A.sst, soa}, Strided{G.b_sst, sob});
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                cma[e] = ok ? mu_a[q + e] : quiet_nan();
                cmb[e] = ok ? mu_b[q + e] : quiet_nan();
                cr[e] = ok ? rt[q + e] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int row = ld_row0 + i * ld_rows;
                {
                    const int64_t r = row_a0 + row;
                    const bool in = ok && r < G.Ta;
                    const float *p = a + soa + r * G.A.src_row_stride;
                    if constexpr (VEC) {
                        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (in) v = *reinterpret_cast<const float4 *>(p);
                        xa[i][0] = v.x; xa[i][VEC ? 1 : 0] = v.y; xa[i][VEC ? 2 : 0] = v.z; xa[i][VEC ? 3 : 0] = v.w;
                    } else {
                        xa[i][0] = in ? *p : 0.f;
                    }
                }
                if (!diag) {
                    const int64_t r = row_b0 + row;
                    const bool in = ok && r < G.Tb;
                    const float *p = b + sob + r * G.b_row_stride;
                    if constexpr (VEC) {
                        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (in) v = *reinterpret_cast<const float4 *>(p);
                        xb[i][0] = v.x; xb[i][VEC ? 1 : 0] = v.y; xb[i][VEC ? 2 : 0] = v.z; xb[i][VEC ? 3 : 0] = v.w;
                    } else {
                        xb[i][0] = in ? *p : 0.f;
                    }
                }
            }
        };

        const float *pa0 = &s_y[0][(qi * 64 + r32) * RG_PITCH];
        const float *pb0 = &s_y[diag ? 0 : 1][(qj * 64 + r32) * RG_PITCH];

        if (c_lo < c_hi) fetch(c_lo);
        for (int64_t c = c_lo; c < c_hi; ++c) {
            __syncthreads();                            // the previous chunk has been consumed
            {
#pragma clang fp contract(off)
#pragma unroll
                for (int i = 0; i < NLD; ++i) {
                    const int row = ld_row0 + i * ld_rows;
                    float ya[NE], yb[NE];
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        // an excluded column (its mean is NaN) enters as 0 * 0
                        const bool ex = cma[e] != cma[e];
                        const float da = xa[i][e] - cma[e];
                        ya[e] = ex ? 0.f : cr[e] * da;
                        if (!diag) {
                            const float db = xb[i][e] - cmb[e];
                            yb[e] = ex ? 0.f : cr[e] * db;
                        }
                    }
                    float *dst = &s_y[0][row * RG_PITCH + ld_col];
                    if constexpr (VEC) *reinterpret_cast<float4 *>(dst) = make_float4(ya[0], ya[VEC ? 1 : 0], ya[VEC ? 2 : 0], ya[VEC ? 3 : 0]);
                    else *dst = ya[0];
                    if (!diag) {
                        dst = &s_y[1][row * RG_PITCH + ld_col];
                        if constexpr (VEC) *reinterpret_cast<float4 *>(dst) = make_float4(yb[0], yb[VEC ? 1 : 0], yb[VEC ? 2 : 0], yb[VEC ? 3 : 0]);
                        else *dst = yb[0];
                    }
                }
            }
            __syncthreads();
            if (c + 1 < c_hi) fetch(c + 1);
#pragma unroll
            for (int j = 0; j < RG_KC / 4; ++j) {
                // 16 bytes = columns 4 j .. 4 j + 3 = two k steps; lane half h takes column 2 step + h
                const float4 a0 = *reinterpret_cast<const float4 *>(pa0 + 4 * j);
                const float4 a1 = *reinterpret_cast<const float4 *>(pa0 + 32 * RG_PITCH + 4 * j);
                const float4 b0 = *reinterpret_cast<const float4 *>(pb0 + 4 * j);
                const float4 b1 = *reinterpret_cast<const float4 *>(pb0 + 32 * RG_PITCH + 4 * j);
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const float va0 = s ? (h ? a0.w : a0.z) : (h ? a0.y : a0.x);
                    const float va1 = s ? (h ? a1.w : a1.z) : (h ? a1.y : a1.x);
                    const float vb0 = s ? (h ? b0.w : b0.z) : (h ? b0.y : b0.x);
                    const float vb1 = s ? (h ? b1.w : b1.z) : (h ? b1.y : b1.x);
                    if (on_m0 && on_n0) acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(va0, vb0, acc[0], 0, 0, 0);
                    if (on_m0 && on_n1) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(va0, vb1, acc[1], 0, 0, 0);
                    if (on_m1 && on_n0) acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(va1, vb0, acc[2], 0, 0, 0);
                    if (on_m1 && on_n1) acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(va1, vb1, acc[3], 0, 0, 0);
                }
            }
            const bool last = c + 1 == c_hi;
            if (last || (c + 1) % RG_SLAB_CHUNKS == 0) {
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int i = 0; i < 16; ++i) { grp[u][i] += (double)acc[u][i]; acc[u][i] = 0.f; }
            }
            if (!last && (c + 1) % RG_GROUP_CHUNKS == 0) {
                // a walking workgroup: the total so far goes to scratch (0 + the first group sum is that group sum)
                const bool first = c + 1 - c_lo == RG_GROUP_CHUNKS;
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        ws[u * 16 + i] = first ? grp[u][i] : ws[u * 16 + i] + grp[u][i];
                        grp[u][i] = 0.0;
                    }
            }
        }
        // grp: the last group sum of the walk (zeros when there are no columns), or the group sum of this tile
        if (G.split) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int i = 0; i < 16; ++i) ws[u * 16 + i] = grp[u][i];
        } else {
            const bool only = c_hi - c_lo <= RG_GROUP_CHUNKS;
            const int row0 = qi * 64 + 4 * h, col0 = qj * 64 + r32;
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const double v = only ? grp[u][i] : ws[u * 16 + i] + grp[u][i];
                    rg_store(G, out, row_a0 + row0 + (u >> 1) * 32 + 8 * (i >> 2) + (i & 3), row_b0 + col0 + (u & 1) * 32, v);
                }
        }
    }
}

// launch 3 (split = 1): the group sums added in group order from zero, as the walking workgroup adds them
__global__ void __launch_bounds__(256) row_gram_finish_kernel(RgGeom G, const double *__restrict__ partial, double *__restrict__ out) {
    const int64_t n = G.pairs * RG_TILE_ELEMS;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t pair = i / RG_TILE_ELEMS;
        const int rem = (int)(i % RG_TILE_ELEMS);
        double total = 0.0;
        for (int64_t g = 0; g < G.n_group; ++g) total += partial[(pair * G.n_group + g) * RG_TILE_ELEMS + rem];
        int64_t ti, tj;
        rg_pair(G, pair, ti, tj);
        int row, col;
        rg_elem(rem / 64, rem % 64, row, col);
        rg_store(G, out, ti * RG_TM + row, tj * RG_TM + col, total);
    }
}

struct RgPlan {
    RgGeom G;
    bool vec;
    int64_t grid, finish_grid;
    size_t off_mu_b, off_rt, off_cnt, off_partial, bytes;
};

// a, b: looked at for NULL (b: the symmetric form) and 16-byte alignment only
int rg_plan(const dlwpcs_rows_desc *da, const void *a, int64_t n_rows_a, const dlwpcs_rows_desc *db, const void *b, int64_t n_rows_b,
            int split, RgPlan &P) {
    RgGeom &G = P.G;
    memset(&G, 0, sizeof(G));
    int64_t inner;
    int rc = rows_addr_init(da, "row_gram", G.A, inner);
    if (rc != DLWPCS_OK) return rc;
    G.sym = b ? 0 : 1;
    if (n_rows_a < 0 || n_rows_a > (1ll << 24)) return fail(DLWPCS_E_INVALID, "row_gram: %lld rows", (long long)n_rows_a);
    if (split < -1 || split > 1) return fail(DLWPCS_E_INVALID, "row_gram: split %d", split);
    G.Ta = n_rows_a;
    if (G.sym) {
        G.Tb = G.Ta;
        G.b_row_stride = G.A.src_row_stride;
        for (int i = 0; i < G.A.n_inner; ++i) G.b_sst[i] = G.A.sst[i];
    } else {
        RowsAddr B;
        int64_t inner_b;
        rc = rows_addr_init(db, "row_gram (b)", B, inner_b);
        if (rc != DLWPCS_OK) return rc;
        if (n_rows_b < 0 || n_rows_b > (1ll << 24)) return fail(DLWPCS_E_INVALID, "row_gram: %lld rows of b", (long long)n_rows_b);
        if (B.n_inner != G.A.n_inner) return fail(DLWPCS_E_INVALID, "row_gram: b has %d inner dims, a %d", B.n_inner, G.A.n_inner);
        for (int i = 0; i < B.n_inner; ++i)
            if (B.ext[i] != G.A.ext[i] || B.ost[i] != G.A.ost[i])
                return fail(DLWPCS_E_INVALID, "row_gram: inner dim %d of b (extent %lld, out stride %lld) is not a's (%lld, %lld)", i,
                            (long long)B.ext[i], (long long)B.ost[i], (long long)G.A.ext[i], (long long)G.A.ost[i]);
        G.Tb = n_rows_b;
        G.b_row_stride = B.src_row_stride;
        for (int i = 0; i < B.n_inner; ++i) G.b_sst[i] = B.sst[i];
    }
    if (inner > (1ll << 40)) return fail(DLWPCS_E_UNSUPPORTED, "row_gram: %lld columns", (long long)inner);
    G.A.ncol = inner;
    G.ta = (G.Ta + RG_TM - 1) / RG_TM;
    G.tb = (G.Tb + RG_TM - 1) / RG_TM;
    G.pairs = G.sym ? G.ta * (G.ta + 1) / 2 : G.ta * G.tb;
    G.n_chunk = (inner + RG_KC - 1) / RG_KC;
    G.n_slab = (inner + DLWPCS_ROW_GRAM_SLAB_COLS - 1) / DLWPCS_ROW_GRAM_SLAB_COLS;
    G.n_group = (G.n_slab + DLWPCS_ROW_GRAM_GROUP_SLABS - 1) / DLWPCS_ROW_GRAM_GROUP_SLABS;
    // one group (or none: zeros) is walked whatever was asked for: there is nothing to add up
    G.split = G.n_group < 2 ? 0 : (split >= 0 ? split : (G.pairs < RG_SPLIT_BELOW ? 1 : 0));
    G.A.tiles = G.pairs;
    G.A.nblk = G.split ? G.pairs * G.n_group : G.pairs;
    if (G.A.nblk >= (1ll << 40)) return fail(DLWPCS_E_UNSUPPORTED, "row_gram: too many tiles");
    bool vec, ovec;
    rows_vector_ok(da, vec, ovec);
    P.vec = vec && aligned16(a);
    if (!G.sym && P.vec) {
        rows_vector_ok(db, vec, ovec);
        P.vec = vec && aligned16(b);
    }
    const int64_t nchunk = P.vec ? inner / 4 : inner;
    G.col_blocks = (nchunk + 255) / 256 < RG_COL_BLOCKS ? (nchunk + 255) / 256 : RG_COL_BLOCKS;
    P.grid = G.A.nblk < RG_SLOTS ? G.A.nblk : RG_SLOTS;
    const size_t epad = ((size_t)inner + 3) / 4 * 4;
    P.off_mu_b = epad * sizeof(float);
    P.off_rt = 2 * epad * sizeof(float);
    P.off_cnt = 3 * epad * sizeof(float);               // (a multiple of 16)
    P.off_partial = P.off_cnt + RG_COL_BLOCKS * sizeof(int64_t);
    // group sums per tile (split), or the running totals of the walking workgroups (more than one group)
    P.bytes = P.off_partial + (G.n_group < 2 ? 0 : (size_t)(G.split ? G.A.nblk : P.grid) * RG_TILE_ELEMS * sizeof(double));
    P.finish_grid = 0;
    if (G.split) {
        const int64_t n = G.pairs * (RG_TILE_ELEMS / 256);
        P.finish_grid = n < RG_FINISH_BLOCKS ? n : RG_FINISH_BLOCKS;
    }
    return DLWPCS_OK;
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" size_t dlwpcs_row_gram_scratch_bytes(const dlwpcs_rows_desc *da, int64_t n_rows_a, const dlwpcs_rows_desc *db,
                                                int64_t n_rows_b, int split) {
    RgPlan P;
    static const float some = 0.f;
    if (rg_plan(da, nullptr, n_rows_a, db, db ? &some : nullptr, n_rows_b, split, P) != DLWPCS_OK) return 0;
    if (P.G.Ta == 0 || P.G.Tb == 0) return 0;
    return P.bytes;
}

extern "C" int dlwpcs_row_gram(const dlwpcs_rows_desc *da, const float *a, int64_t n_rows_a, const dlwpcs_rows_desc *db,
                               const float *b, int64_t n_rows_b, const float *weight_root, int center_a, const float *mean_a,
                               int center_b, const float *mean_b, int split, double *out, int64_t ld_out, float *mean_out,
                               int64_t *n_valid, void *scratch, size_t scratch_bytes, dlwpcs_stream_t stream) {
    RgPlan P;
    const int rc = rg_plan(da, a, n_rows_a, db, b, n_rows_b, split, P);
    if (rc != DLWPCS_OK) return rc;
    RgGeom &G = P.G;
    if (center_a < 0 || center_a > 2 || (!G.sym && (center_b < 0 || center_b > 2)))
        return fail(DLWPCS_E_INVALID, "row_gram: centring modes %d, %d (0 none, 1 own mean, 2 given mean)", center_a, center_b);
    if (ld_out < G.Tb) return fail(DLWPCS_E_INVALID, "row_gram: leading dimension %lld below the %lld rows of b", (long long)ld_out, (long long)G.Tb);
    if (G.Ta == 0 || G.Tb == 0) return DLWPCS_OK;      // an empty output: nothing to launch
    if (!out) return fail(DLWPCS_E_INVALID, "row_gram: null output");
    if (G.A.ncol > 0 && (!a || (center_a == 2 && !mean_a) || (!G.sym && center_b == 2 && !mean_b)))
        return fail(DLWPCS_E_INVALID, "row_gram: null operand");
    if ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)weight_root) | ((uintptr_t)mean_a) | ((uintptr_t)mean_b) | ((uintptr_t)mean_out)) & 3)
        return fail(DLWPCS_E_INVALID, "row_gram: an operand is not aligned to its 4-byte elements");
    if ((((uintptr_t)out) | ((uintptr_t)n_valid)) & 7) return fail(DLWPCS_E_INVALID, "row_gram: out or n_valid is not aligned to 8 bytes");
    if (!scratch || (((uintptr_t)scratch) & 7) || scratch_bytes < P.bytes)
        return fail(DLWPCS_E_INVALID, "row_gram: this call needs an 8-byte aligned scratch of %zu bytes", P.bytes);
    G.center_a = center_a;
    G.center_b = G.sym ? center_a : center_b;
    G.ld = ld_out;
    char *ws = (char *)scratch;
    float *mu_a = (float *)ws, *mu_b = G.sym ? mu_a : (float *)(ws + P.off_mu_b), *rt = (float *)(ws + P.off_rt);
    int64_t *part_cnt = (int64_t *)(ws + P.off_cnt);
    double *partial = (double *)(ws + P.off_partial);
    hipStream_t s = (hipStream_t)stream;
    if (G.col_blocks) {
        const dim3 grid((unsigned)G.col_blocks), blk(256);
        if (P.vec) hipLaunchKernelGGL((row_gram_column_kernel<true>), grid, blk, 0, s, G, a, b, weight_root, mean_a, mean_b, mu_a, mu_b, rt, mean_out, part_cnt);
        else hipLaunchKernelGGL((row_gram_column_kernel<false>), grid, blk, 0, s, G, a, b, weight_root, mean_a, mean_b, mu_a, mu_b, rt, mean_out, part_cnt);
    }
    {
        const dim3 grid((unsigned)P.grid), blk(RG_THREADS);
        // the symmetric form reads b's rows from a
        const float *pb = G.sym ? a : b;
        if (P.vec) hipLaunchKernelGGL((row_gram_kernel<true>), grid, blk, 0, s, G, a, pb, mu_a, mu_b, rt, part_cnt, n_valid, partial, out);
        else hipLaunchKernelGGL((row_gram_kernel<false>), grid, blk, 0, s, G, a, pb, mu_a, mu_b, rt, part_cnt, n_valid, partial, out);
    }
    if (P.finish_grid) hipLaunchKernelGGL(row_gram_finish_kernel, dim3((unsigned)P.finish_grid), dim3(256), 0, s, G, partial, out);
    return check_launch("row_gram");
}

extern "C" int dlwpcs_row_gram_plan_info(const dlwpcs_rows_desc *da, const void *a, int64_t n_rows_a, const dlwpcs_rows_desc *db,
                                         const void *b, int64_t n_rows_b, int split, int64_t info[8]) {
    if (!info) return fail(DLWPCS_E_INVALID, "row_gram_plan_info: null info");
    RgPlan P;
    const int rc = rg_plan(da, a, n_rows_a, db, b, n_rows_b, split, P);
    if (rc != DLWPCS_OK) return rc;
    const bool empty = P.G.Ta == 0 || P.G.Tb == 0;
    if (!empty && P.G.A.ncol > 0 && !a) return fail(DLWPCS_E_INVALID, "row_gram: null operand");
    info[0] = P.G.ta;
    info[1] = P.G.tb;
    info[2] = P.G.pairs;
    info[3] = P.G.n_slab;
    info[4] = P.G.n_group;
    info[5] = P.G.split;
    info[6] = P.vec ? 1 : 0;
    info[7] = empty ? 0 : P.grid;
    return DLWPCS_OK;
}
