// Offline-map remapping (DLWP/remap): y[o, r, k] = sum_j val[j] * x[o, col[j], k] over the CSR segment of row r.
//
// Mapping: a workgroup of 256 lanes covers one tile of 256 consecutive (row, inner) pairs and MR_U consecutive outer slices.
// The lanes run along whichever of y's row and inner axes has the smaller stride, so the stores of a wave are contiguous
// when y is.  Each lane reads its row's CSR segment once (a few entries, L1/L2-hot: neighbouring lanes share rows or read
// neighbouring ones) and, per pair of entries, issues one load for each entry and each of its MR_U outer slices: 2 * MR_U
// independent gathers in flight per lane.  The terms of each output are added in CSR order with fp32 fma, so results are
// bitwise repeatable.
//
// Workgroups are numbered tile-fastest and dealt to the XCDs in contiguous ranges (xcd_remap), so an XCD works through whole
// outer slices and the source cells shared by neighbouring rows are read from its own L2.  No LDS, no atomics.
#include <string.h>
#include "common.h"

namespace dlwpcs {

namespace {

constexpr int MR_THREADS = 256;
constexpr int MR_U = 4;                         // outer slices per lane
constexpr int64_t MR_MAX_GRID = 1ll << 24;      // workgroups of one launch; beyond this the grid strides

struct MapGeom {
    int64_t ext[3];                             // outer extents, padded with 1 (ext[2] fastest)
    int64_t xo[3], yo[3];                       // outer strides
    int64_t xs, ys, xk, yk;                     // space and inner strides
    int64_t n_outer, n_chunks, nblk;
    int32_t n_b, K, kfast, n_lanes, n_tiles, remap;
};

template <typename T> __device__ __forceinline__ float load_x(const T *p);
template <> __device__ __forceinline__ float load_x<float>(const float *p) { return *p; }
template <> __device__ __forceinline__ float load_x<bf16_t>(const bf16_t *p) { return bf2f(*p); }

template <typename T>
__global__ __launch_bounds__(MR_THREADS) void sparse_map_kernel(MapGeom G, const int32_t *__restrict__ row_ptr,
                                                                const int32_t *__restrict__ col, const float *__restrict__ val,
                                                                const T *__restrict__ x, float *__restrict__ y) {
    for (int64_t b = blockIdx.x; b < G.nblk; b += gridDim.x) {
        const int64_t w = G.remap ? (int64_t)xcd_remap((uint32_t)b, (uint32_t)G.nblk) : b;
        const int64_t chunk = w / G.n_tiles;
        const int32_t tile = (int32_t)(w - chunk * G.n_tiles);
        const int32_t idx = tile * MR_THREADS + (int32_t)threadIdx.x;
        if (idx >= G.n_lanes) continue;
        int32_t r, k;
        if (G.kfast) {
            r = (int32_t)((uint32_t)idx / (uint32_t)G.K);
            k = idx - r * G.K;
        } else {
            k = (int32_t)((uint32_t)idx / (uint32_t)G.n_b);
            r = idx - k * G.n_b;
        }
        // the first outer slice of the chunk as (i0, i1, i2); the next ones by carrying
        const int64_t o0 = chunk * MR_U;
        int64_t i2 = o0 % G.ext[2], q = o0 / G.ext[2];
        int64_t i1 = q % G.ext[1], i0 = q / G.ext[1];
        int64_t xoff[MR_U], yoff[MR_U];
        bool live[MR_U];
#pragma unroll
        for (int u = 0; u < MR_U; ++u) {
            live[u] = o0 + u < G.n_outer;
            xoff[u] = i0 * G.xo[0] + i1 * G.xo[1] + i2 * G.xo[2] + (int64_t)k * G.xk;
            yoff[u] = i0 * G.yo[0] + i1 * G.yo[1] + i2 * G.yo[2] + (int64_t)r * G.ys + (int64_t)k * G.yk;
            if (++i2 == G.ext[2]) {
                i2 = 0;
                if (++i1 == G.ext[1]) { i1 = 0; ++i0; }
            }
        }
        // slots past the last outer slice re-read slice o0 (always in bounds) and are not stored: the gathers below need no
        // branch, so all of them are in flight together
#pragma unroll
        for (int u = 1; u < MR_U; ++u)
            if (!live[u]) xoff[u] = xoff[0];
        float acc[MR_U];
#pragma unroll
        for (int u = 0; u < MR_U; ++u) acc[u] = 0.f;
        const int32_t j1 = row_ptr[r + 1];
        int32_t j = row_ptr[r];
        // two entries per step: both entries' gathers are issued before the first fma; the adds stay in CSR order
        for (; j + 1 < j1; j += 2) {
            const int64_t c0 = (int64_t)col[j] * G.xs, c1 = (int64_t)col[j + 1] * G.xs;
            const float v0 = val[j], v1 = val[j + 1];
            float a0[MR_U], a1[MR_U];
#pragma unroll
            for (int u = 0; u < MR_U; ++u) {
                a0[u] = load_x(x + xoff[u] + c0);
                a1[u] = load_x(x + xoff[u] + c1);
            }
#pragma unroll
            for (int u = 0; u < MR_U; ++u) acc[u] = fmaf(v1, a1[u], fmaf(v0, a0[u], acc[u]));
        }
        if (j < j1) {
            const int64_t c0 = (int64_t)col[j] * G.xs;
            const float v0 = val[j];
#pragma unroll
            for (int u = 0; u < MR_U; ++u) acc[u] = fmaf(v0, load_x(x + xoff[u] + c0), acc[u]);
        }
#pragma unroll
        for (int u = 0; u < MR_U; ++u)
            if (live[u]) y[yoff[u]] = acc[u];
    }
}

int make_geom(const dlwpcs_sparse_map_desc *d, MapGeom &G, bool &empty) {
    if (!d) return fail(DLWPCS_E_INVALID, "sparse_map: null descriptor");
    if (d->x_dtype != DLWPCS_F32 && d->x_dtype != DLWPCS_BF16)
        return fail(DLWPCS_E_INVALID, "sparse_map: x_dtype %d is neither DLWPCS_F32 nor DLWPCS_BF16", d->x_dtype);
    if (d->n_outer < 0 || d->n_outer > 3) return fail(DLWPCS_E_INVALID, "sparse_map: n_outer %d (0..3)", d->n_outer);
    if (d->n_a < 0 || d->n_b < 0 || d->nnz < 0 || d->inner_ext < 0)
        return fail(DLWPCS_E_INVALID, "sparse_map: negative extent (n_a %lld, n_b %lld, nnz %lld, inner %lld)", (long long)d->n_a,
                    (long long)d->n_b, (long long)d->nnz, (long long)d->inner_ext);
    if (d->nnz >= (1ll << 31)) return fail(DLWPCS_E_INVALID, "sparse_map: %lld entries (< 2^31)", (long long)d->nnz);
    if (d->n_a == 0 && d->nnz > 0) return fail(DLWPCS_E_INVALID, "sparse_map: entries but no source cells");
    memset(&G, 0, sizeof(G));
    G.n_outer = 1;
    for (int i = 0; i < 3; ++i) G.ext[i] = 1;
    for (int i = 0; i < d->n_outer; ++i) {
        const int s = 3 - d->n_outer + i;        // right-aligned: the last outer dim is the fastest
        if (d->outer_ext[i] < 0) return fail(DLWPCS_E_INVALID, "sparse_map: outer extent %lld", (long long)d->outer_ext[i]);
        G.ext[s] = d->outer_ext[i];
        G.xo[s] = d->x_outer_stride[i];
        G.yo[s] = d->y_outer_stride[i];
        G.n_outer *= d->outer_ext[i];
    }
    empty = G.n_outer == 0 || d->n_b == 0 || d->inner_ext == 0;
    if (empty) return DLWPCS_OK;
    if (d->n_b * d->inner_ext >= (1ll << 31))
        return fail(DLWPCS_E_INVALID, "sparse_map: %lld rows x %lld inner is too many (< 2^31)", (long long)d->n_b,
                    (long long)d->inner_ext);
    G.xs = d->x_space_stride;
    G.ys = d->y_space_stride;
    G.xk = d->x_inner_stride;
    G.yk = d->y_inner_stride;
    G.n_b = (int32_t)d->n_b;
    G.K = (int32_t)d->inner_ext;
    const int64_t ayk = G.yk < 0 ? -G.yk : G.yk, ays = G.ys < 0 ? -G.ys : G.ys;
    G.kfast = G.K > 1 && ayk <= ays;
    G.n_lanes = G.n_b * G.K;
    G.n_tiles = (G.n_lanes + MR_THREADS - 1) / MR_THREADS;
    G.n_chunks = (G.n_outer + MR_U - 1) / MR_U;
    G.nblk = G.n_chunks * G.n_tiles;
    G.remap = G.nblk <= MR_MAX_GRID;
    return DLWPCS_OK;
}

// The same map applied to data with holes (dlwpcs_sparse_map_apply_masked): a NaN source value is MISSING, an entry of weight 0 is
// not there at all.  Same lanes, tiles, XCD dealing and outer slices as sparse_map_kernel, same gathers (all issued before the
// first fma, dead slots re-reading slice o0); what a gathered value contributes is chosen by selects on `a == a`, never by a
// branch.  Per output: acc, the fma chain over the present entries; wval, their weights added in CSR order; the counts of present
// and missing entries; per lane: wall, the weights of all entries added in CSR order (adding the +0 of a skipped entry changes no
// bit).  Where nothing is missing wval == wall bitwise and acc is sparse_map_kernel's chain: the same bits as the plain launch.
template <typename T>
__global__ __launch_bounds__(MR_THREADS) void sparse_map_masked_kernel(MapGeom G, const int32_t *__restrict__ row_ptr,
                                                                       const int32_t *__restrict__ col,
                                                                       const float *__restrict__ val, const T *__restrict__ x,
                                                                       float *__restrict__ y, float *__restrict__ frac,
                                                                       float min_valid, int renorm) {
#pragma clang fp contract(off)
    for (int64_t b = blockIdx.x; b < G.nblk; b += gridDim.x) {
        const int64_t w = G.remap ? (int64_t)xcd_remap((uint32_t)b, (uint32_t)G.nblk) : b;
        const int64_t chunk = w / G.n_tiles;
        const int32_t tile = (int32_t)(w - chunk * G.n_tiles);
        const int32_t idx = tile * MR_THREADS + (int32_t)threadIdx.x;
        if (idx >= G.n_lanes) continue;
        int32_t r, k;
        if (G.kfast) {
            r = (int32_t)((uint32_t)idx / (uint32_t)G.K);
            k = idx - r * G.K;
        } else {
            k = (int32_t)((uint32_t)idx / (uint32_t)G.n_b);
            r = idx - k * G.n_b;
        }
        const int64_t o0 = chunk * MR_U;
        int64_t i2 = o0 % G.ext[2], q = o0 / G.ext[2];
        int64_t i1 = q % G.ext[1], i0 = q / G.ext[1];
        int64_t xoff[MR_U], yoff[MR_U];
        bool live[MR_U];
#pragma unroll
        for (int u = 0; u < MR_U; ++u) {
            live[u] = o0 + u < G.n_outer;
            xoff[u] = i0 * G.xo[0] + i1 * G.xo[1] + i2 * G.xo[2] + (int64_t)k * G.xk;
            yoff[u] = i0 * G.yo[0] + i1 * G.yo[1] + i2 * G.yo[2] + (int64_t)r * G.ys + (int64_t)k * G.yk;
            if (++i2 == G.ext[2]) {
                i2 = 0;
                if (++i1 == G.ext[1]) { i1 = 0; ++i0; }
            }
        }
#pragma unroll
        for (int u = 1; u < MR_U; ++u)
            if (!live[u]) xoff[u] = xoff[0];
        float acc[MR_U], wval[MR_U];
        int32_t nval[MR_U], nmiss[MR_U];
#pragma unroll
        for (int u = 0; u < MR_U; ++u) { acc[u] = 0.f; wval[u] = 0.f; nval[u] = 0; nmiss[u] = 0; }
        float wall = 0.f;
        const int32_t j1 = row_ptr[r + 1];
        int32_t j = row_ptr[r];
        for (; j + 1 < j1; j += 2) {
            const int64_t c0 = (int64_t)col[j] * G.xs, c1 = (int64_t)col[j + 1] * G.xs;
            const float v0 = val[j], v1 = val[j + 1];
            float a0[MR_U], a1[MR_U];
#pragma unroll
            for (int u = 0; u < MR_U; ++u) {
                a0[u] = load_x(x + xoff[u] + c0);
                a1[u] = load_x(x + xoff[u] + c1);
            }
            const bool e0 = v0 != 0.f, e1 = v1 != 0.f;
            wall += e0 ? v0 : 0.f;
            wall += e1 ? v1 : 0.f;
#pragma unroll
            for (int u = 0; u < MR_U; ++u) {
                const bool p0 = e0 & (a0[u] == a0[u]), p1 = e1 & (a1[u] == a1[u]);
                const float t0 = fmaf(v0, a0[u], acc[u]);
                acc[u] = p0 ? t0 : acc[u];
                const float t1 = fmaf(v1, a1[u], acc[u]);
                acc[u] = p1 ? t1 : acc[u];
                wval[u] += p0 ? v0 : 0.f;
                wval[u] += p1 ? v1 : 0.f;
                nval[u] += (int32_t)p0 + (int32_t)p1;
                nmiss[u] += (int32_t)(e0 & !p0) + (int32_t)(e1 & !p1);
            }
        }
        if (j < j1) {
            const int64_t c0 = (int64_t)col[j] * G.xs;
            const float v0 = val[j];
            float a0[MR_U];
#pragma unroll
            for (int u = 0; u < MR_U; ++u) a0[u] = load_x(x + xoff[u] + c0);
            const bool e0 = v0 != 0.f;
            wall += e0 ? v0 : 0.f;
#pragma unroll
            for (int u = 0; u < MR_U; ++u) {
                const bool p0 = e0 & (a0[u] == a0[u]);
                const float t0 = fmaf(v0, a0[u], acc[u]);
                acc[u] = p0 ? t0 : acc[u];
                wval[u] += p0 ? v0 : 0.f;
                nval[u] += (int32_t)p0;
                nmiss[u] += (int32_t)(e0 & !p0);
            }
        }
        const float need = min_valid * wall;        // one rounded multiply: the host twin takes the same decision
#pragma unroll
        for (int u = 0; u < MR_U; ++u) {
            if (!live[u]) continue;
            const bool holes = nmiss[u] > 0;
            const bool missing = holes && (wval[u] < need || nval[u] == 0 || min_valid >= 1.f);
            const float scale = (renorm && holes) ? wall / wval[u] : 1.f;
            const float out = (renorm && holes) ? acc[u] * scale : acc[u];
            y[yoff[u]] = missing ? __uint_as_float(0x7fc00000u) : out;
            if (frac) frac[yoff[u]] = (nval[u] + nmiss[u] > 0) ? wval[u] / wall : 0.f;
        }
    }
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" int dlwpcs_sparse_map_apply(const dlwpcs_sparse_map_desc *d, const int32_t *row_ptr, const int32_t *col,
                                       const float *val, const void *x, float *y, dlwpcs_stream_t stream) {
    MapGeom G;
    bool empty = false;
    int rc = make_geom(d, G, empty);
    if (rc != DLWPCS_OK) return rc;
    if (empty) return DLWPCS_OK;
    if (!row_ptr || !x || !y || (d->nnz > 0 && (!col || !val))) return fail(DLWPCS_E_INVALID, "sparse_map: null operand");
    const dim3 grid((unsigned)(G.nblk < MR_MAX_GRID ? G.nblk : MR_MAX_GRID));
    hipStream_t s = (hipStream_t)stream;
    if (d->x_dtype == DLWPCS_BF16)
        hipLaunchKernelGGL((sparse_map_kernel<bf16_t>), grid, dim3(MR_THREADS), 0, s, G, row_ptr, col, val,
                           (const bf16_t *)x, y);
    else
        hipLaunchKernelGGL((sparse_map_kernel<float>), grid, dim3(MR_THREADS), 0, s, G, row_ptr, col, val, (const float *)x, y);
    return check_launch("sparse_map");
}

extern "C" int dlwpcs_sparse_map_apply_masked(const dlwpcs_sparse_map_desc *d, const int32_t *row_ptr, const int32_t *col,
                                              const float *val, const void *x, float *y, float *frac, float min_valid, int flags,
                                              dlwpcs_stream_t stream) {
    MapGeom G;
    bool empty = false;
    int rc = make_geom(d, G, empty);
    if (rc != DLWPCS_OK) return rc;
    if (!(min_valid >= 0.f && min_valid <= 1.f))
        return fail(DLWPCS_E_INVALID, "sparse_map_masked: min_valid %g is not in [0, 1]", (double)min_valid);
    if (flags & ~DLWPCS_MAP_RENORMALIZE) return fail(DLWPCS_E_INVALID, "sparse_map_masked: unknown flags 0x%x", flags);
    if (empty) return DLWPCS_OK;
    if (!row_ptr || !x || !y || (d->nnz > 0 && (!col || !val))) return fail(DLWPCS_E_INVALID, "sparse_map_masked: null operand");
    const dim3 grid((unsigned)(G.nblk < MR_MAX_GRID ? G.nblk : MR_MAX_GRID));
    hipStream_t s = (hipStream_t)stream;
    const int renorm = (flags & DLWPCS_MAP_RENORMALIZE) ? 1 : 0;
    const bool bf = d->x_dtype == DLWPCS_BF16;
    if (bf)
        hipLaunchKernelGGL((sparse_map_masked_kernel<bf16_t>), grid, dim3(MR_THREADS), 0, s, G, row_ptr, col, val,
                           (const bf16_t *)x, y, frac, min_valid, renorm);
    else
        hipLaunchKernelGGL((sparse_map_masked_kernel<float>), grid, dim3(MR_THREADS), 0, s, G, row_ptr, col, val, (const float *)x, y,
                           frac, min_valid, renorm);
    return check_launch("sparse_map_masked");
}
