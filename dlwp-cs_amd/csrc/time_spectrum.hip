// Spectra along the row axis (dlwpcs_time_spectrum; include/dlwpcs.h states the definitions): Welch's segment-averaged power
// spectrum of a row set, its pair form (two powers, co-spectrum, quadrature spectrum) and the plain coefficients per segment.
//
// The transform of one segment is the matrix product (frequencies x M) . (M x columns) on v_mfma_f32_32x32x2_f32 (exact fp32, a
// k-ordered fmaf chain over the rows of the segment) with the operands of sht_fourier_kernel: the twiddles are the A operand, the
// data rows the B operand, so a lane ends up with ONE column and 16 frequencies and Re and Im of a frequency meet in one lane.
// The columns of a row set lie along the lanes already, so a staged chunk is [64 rows][32 columns] in LDS and the B operand is a
// conflict-free 4-byte read.  The twiddles come from the length-M table {cos, -sin}(2 pi m / M) in LDS at the reduced index
// m = (f t) mod M, which every lane carries along in integers.
//
// A tile is (32 columns, 128 frequencies, slab of TS_SLAB segments); four waves own 32 frequencies each.  Per segment: (detrend)
// a first pass stages the raw rows and 32 lanes per operand add their column in row order in fp64; then the rows are staged again
// as y = fl(w_t * fl(x - mean)) chunk by chunk (the next chunk waits in registers) and the matrix cores run over them.  A thread
// that stages a value that is not finite flags its column: the segment does not count there.
//
// Epilogue.  Power and pair form: the lane widens its fp32 products (ts_product, spelled once) to fp64 and adds them to the slab
// sum of its (column, frequency, quantity) in segment order.  split = 0: the workgroup walks the slabs of its (column, frequency)
// tile and adds every finished slab sum to the total, in slab order.  split = 1: every slab is a tile of its own and writes its
// sums to scratch; the finishing launch adds them in slab order -- the same additions, hence the same bits.  Coefficient form:
// the lane stores Re and Im of its 16 frequencies per segment.
//
// The grid is TS_SLOTS persistent workgroups that stride over the int64 list of tiles; which workgroup computes a tile
// influences nothing.  No atomics, at most two launches.  No profiler tags, as for the other verification kernels.
#include <math.h>
#include "mfma_common.h"
#include "strided.h"

namespace dlwpcs {

namespace {

constexpr int TS_THREADS = 256;
constexpr int TS_COLS = 32;                 // columns of a tile (the N of the MFMA)
constexpr int TS_RC = 64;                   // rows per staged chunk
constexpr int TS_FW = 32;                   // frequencies per wave
constexpr int TS_FT = 4 * TS_FW;            // frequencies per tile
constexpr int TS_SLAB = DLWPCS_TIME_SPECTRUM_SLAB_SEGMENTS;
constexpr int64_t TS_SLOTS = 512;           // persistent workgroups: 256 compute units x 2; placement only
constexpr int64_t TS_SPLIT_BELOW = 256;     // split < 0: slabs get tiles of their own below this many (column, frequency) tiles
constexpr int64_t TS_FINISH_BLOCKS = 2048;

enum { TS_POWER = 0, TS_PAIR = 1, TS_COEF = 2 };

struct TsGeom {
    RowsAddr A;                              // ext in elements; ncol = columns, tiles = column tiles, nblk = tiles of the launch
    int32_t M, K, detrend, min_count, split, n_ft;
    int64_t hop, n_seg, n_slab;
    int64_t outer_stride, part_stride;       // pair: between the quantities; coefficients: between segments, between Re and Im
    double scale;                            // 1 / (M * S_w)
};

// the four fp32 products of the pair form (q = 0 alone in the single form), spelled once so that every instantiation rounds alike
__device__ __forceinline__ float ts_product(int q, float ca, float sa, float cb, float sb) {
#pragma clang fp contract(off)
    if (q == 0) return __builtin_fmaf(sa, sa, ca * ca);
    if (q == 1) return __builtin_fmaf(sb, sb, cb * cb);
    if (q == 2) return __builtin_fmaf(sa, sb, ca * cb);                 // Re(A conj B)
    return __builtin_fmaf(sa, cb, -(ca * sb));                          // Im(A conj B)
}

// the value stored for (frequency f, quantity): the fp64 sum over the n counted segments, scaled, averaged, rounded once
__host__ __device__ inline float ts_result(double total, int n, int min_count, double scale, int f, int M) {
#pragma clang fp contract(off)
    if (n < min_count || n < 1) return __builtin_bit_cast(float, 0x7fc00000u);
    const double c = (f == 0 || 2 * f == M) ? 1.0 : 2.0;
    return (float)((total * (c * scale)) / (double)n);
}

template <int MODE, bool VEC>
__global__ void __launch_bounds__(TS_THREADS) time_spectrum_kernel(TsGeom G, const float *__restrict__ a, const float *__restrict__ b,
                                                                   const float *__restrict__ window, const float2 *__restrict__ twiddle,
                                                                   double *__restrict__ partial, int32_t *__restrict__ part_cnt,
                                                                   float *__restrict__ out, int32_t *__restrict__ count) {
    constexpr int NOP = MODE == TS_PAIR ? 2 : 1;
    constexpr int NQ = MODE == TS_PAIR ? 4 : 1;
    constexpr int NS = MODE == TS_COEF ? 1 : NQ;        // fp64 sums per frequency (none are used in the coefficient form)
    constexpr int NLD = VEC ? 2 : 8;                    // loads of a thread per chunk and operand
    constexpr int NE = VEC ? 4 : 1;
    __shared__ float2 s_tw[DLWPCS_TIME_SPECTRUM_MAX_M];
    __shared__ __attribute__((aligned(16))) float s_x[NOP][TS_RC * TS_COLS];
    __shared__ int64_t s_soff[TS_COLS], s_ooff[TS_COLS];
    __shared__ float s_mu[NOP][TS_COLS];
    __shared__ int s_valid[TS_COLS], s_bad[TS_COLS];

    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    const int M = G.M, K = G.K;
    for (int m = tid; m < M; m += TS_THREADS) s_tw[m] = twiddle[m];

    // staging: the column of this thread's loads is the same in every chunk, its rows are ld_row0 + i * ld_rows
    const int ld_col = VEC ? (tid & 7) * 4 : tid & 31;
    const int ld_row0 = VEC ? tid >> 3 : tid >> 5;
    constexpr int ld_rows = VEC ? 32 : 8;
    const int n_chunks = (M + TS_RC - 1) / TS_RC;
    const bool walk = MODE != TS_COEF && G.split == 0;  // this workgroup walks every slab of its (column, frequency) tile
    const int64_t slabs_w = walk ? 1 : G.n_slab;        // slabs that are tiles of their own

    for (int64_t tile = blockIdx.x; tile < G.A.nblk; tile += gridDim.x) {
        const int ft = (int)(tile % G.n_ft);
        const int64_t rest = tile / G.n_ft;
        const int64_t slab_t = rest % slabs_w, ct = rest / slabs_w;
        const int fw = ft * TS_FT + wv * TS_FW;          // the first frequency of this wave
        const bool wave_on = fw < K;
        const int fl = fw + r32;                        // this lane's frequency as the row of the A operand
        const int step2 = (int)((2ll * fl) % M);

        __syncthreads();                                // the previous tile's epilogue has read the column tables
        if (tid < TS_COLS) {
            const int64_t q = ct * TS_COLS + tid;
            const bool valid = q < G.A.ncol;
            int64_t so = 0, oo = 0;
            if (valid) rows_offsets<1, false>(G.A, q, so, oo);
            s_soff[tid] = so;
            s_ooff[tid] = oo;
            s_valid[tid] = valid;
        }
        __syncthreads();
        const int64_t my_soff = s_soff[ld_col];
        const bool my_ok = s_valid[ld_col] != 0;        // (VEC: the four columns of a chunk are valid together)
        const int64_t my_col = ct * TS_COLS + r32;
        const bool col_ok = s_valid[r32] != 0;
        const int64_t my_ooff = s_ooff[r32];

        double total[NS][16];
        int n_total = 0;
#pragma unroll
        for (int q = 0; q < NS; ++q)
#pragma unroll
            for (int i = 0; i < 16; ++i) total[q][i] = 0.0;

        const int64_t slab_lo = walk ? 0 : slab_t, slab_hi = walk ? G.n_slab : slab_t + 1;
        for (int64_t slab = slab_lo; slab < slab_hi; ++slab) {
            double run[NS][16];
            int n_run = 0;
#pragma unroll
            for (int q = 0; q < NS; ++q)
#pragma unroll
                for (int i = 0; i < 16; ++i) run[q][i] = 0.0;
            const int64_t seg_hi = (slab + 1) * TS_SLAB < G.n_seg ? (slab + 1) * TS_SLAB : G.n_seg;
            for (int64_t seg = slab * TS_SLAB; seg < seg_hi; ++seg) {
                const int64_t row0 = seg * G.hop;       // rows row0 .. row0 + M - 1 < n_rows
                float regs[NOP][NLD][NE], wreg[NLD];
                auto fetch = [&](int chunk) {
#pragma unroll
                    for (int i = 0; i < NLD; ++i) {
                        const int t = chunk * TS_RC + ld_row0 + i * ld_rows;
                        const bool in = my_ok && t < M;
                        wreg[i] = in ? window[t] : 0.f;
#pragma unroll
                        for (int op = 0; op < NOP; ++op) {
                            const float *p = (op == 0 ? a : b) + my_soff + (row0 + t) * G.A.src_row_stride;
                            if constexpr (VEC) {
                                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                                if (in) v = *reinterpret_cast<const float4 *>(p);
                                regs[op][i][0] = v.x; regs[op][i][VEC ? 1 : 0] = v.y; regs[op][i][VEC ? 2 : 0] = v.z;
                                regs[op][i][VEC ? 3 : 0] = v.w;
                            } else {
                                regs[op][i][0] = in ? *p : 0.f;
                            }
                        }
                    }
                };
                __syncthreads();                        // the previous segment's epilogue has read the flags
                if (tid < TS_COLS) s_bad[tid] = 0;

                if (G.detrend) {
                    // pass 1: the raw rows go through LDS, lane (operand, column) adds its column in row order
                    double sum = 0.0;
                    fetch(0);
                    for (int chunk = 0; chunk < n_chunks; ++chunk) {
                        __syncthreads();
#pragma unroll
                        for (int op = 0; op < NOP; ++op)
#pragma unroll
                            for (int i = 0; i < NLD; ++i) {
                                float *dst = &s_x[op][(ld_row0 + i * ld_rows) * TS_COLS + ld_col];
                                if constexpr (VEC) *reinterpret_cast<float4 *>(dst) =
                                    make_float4(regs[op][i][0], regs[op][i][VEC ? 1 : 0], regs[op][i][VEC ? 2 : 0], regs[op][i][VEC ? 3 : 0]);
                                else *dst = regs[op][i][0];
                            }
                        __syncthreads();
                        if (chunk + 1 < n_chunks) fetch(chunk + 1);
                        if (tid < NOP * TS_COLS) {
                            const int left = M - chunk * TS_RC, nt = left < TS_RC ? left : TS_RC;
                            const float *col = &s_x[tid >> 5][tid & 31];
                            for (int r = 0; r < nt; ++r) sum += (double)col[r * TS_COLS];
                        }
                    }
                    if (tid < NOP * TS_COLS) s_mu[tid >> 5][tid & 31] = (float)(sum / (double)M);
                    __syncthreads();
                }
                float mu[NOP][NE];
#pragma unroll
                for (int op = 0; op < NOP; ++op)
#pragma unroll
                    for (int e = 0; e < NE; ++e) mu[op][e] = G.detrend ? s_mu[op][ld_col + e] : 0.f;

                f32x16 acc[NOP][2];
#pragma unroll
                for (int op = 0; op < NOP; ++op)
#pragma unroll
                    for (int cs = 0; cs < 2; ++cs)
#pragma unroll
                        for (int i = 0; i < 16; ++i) acc[op][cs][i] = 0.f;
                int m = (int)(((int64_t)h * fl) % M);   // the reduced twiddle index of this lane's row t = 2 step + h
                unsigned bad_mask = 0;

                fetch(0);
                for (int chunk = 0; chunk < n_chunks; ++chunk) {
                    __syncthreads();                    // the previous chunk has been consumed
                    {
#pragma clang fp contract(off)
#pragma unroll
                        for (int op = 0; op < NOP; ++op)
#pragma unroll
                            for (int i = 0; i < NLD; ++i) {
                                const bool in = my_ok && chunk * TS_RC + ld_row0 + i * ld_rows < M;
                                float y[NE];
#pragma unroll
                                for (int e = 0; e < NE; ++e) {
                                    const float x = regs[op][i][e];
                                    if (nonfinite(x)) bad_mask |= 1u << e;
                                    const float d = x - mu[op][e];
                                    y[e] = in ? wreg[i] * d : 0.f;
                                }
                                float *dst = &s_x[op][(ld_row0 + i * ld_rows) * TS_COLS + ld_col];
                                if constexpr (VEC) *reinterpret_cast<float4 *>(dst) = make_float4(y[0], y[VEC ? 1 : 0], y[VEC ? 2 : 0], y[VEC ? 3 : 0]);
                                else *dst = y[0];
                            }
                    }
                    if (chunk + 1 == n_chunks) {
#pragma unroll
                        for (int e = 0; e < NE; ++e)
                            if (bad_mask & (1u << e)) s_bad[ld_col + e] = 1;
                    }
                    __syncthreads();
                    if (chunk + 1 < n_chunks) fetch(chunk + 1);
                    if (wave_on) {
                        const int left = M - chunk * TS_RC;
                        const int nk = left >= TS_RC ? TS_RC / 2 : (left + 1) / 2;      // (a row past M was staged as zero)
                        for (int k = 0; k < nk; ++k) {
                            const float2 tw = s_tw[m];
#pragma unroll
                            for (int op = 0; op < NOP; ++op) {
                                const float xv = s_x[op][(2 * k + h) * TS_COLS + r32];
                                acc[op][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(tw.x, xv, acc[op][0], 0, 0, 0);
                                acc[op][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(tw.y, xv, acc[op][1], 0, 0, 0);
                            }
                            m += step2; m -= m >= M ? M : 0;
                        }
                    }
                }

                // the lane holds column r32 and the frequencies fw + 8 (i >> 2) + 4 h + (i & 3)
                const bool counted = col_ok && s_bad[r32] == 0;
                if constexpr (MODE == TS_COEF) {
                    if (wave_on && col_ok) {
                        float *dst = out + seg * G.outer_stride + my_ooff;
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const int f = fw + 8 * (i >> 2) + 4 * h + (i & 3);
                            if (f < K) {
                                dst[(int64_t)f * G.A.out_row_stride] = counted ? acc[0][0][i] : quiet_nan();
                                dst[(int64_t)f * G.A.out_row_stride + G.part_stride] = counted ? acc[0][1][i] : quiet_nan();
                            }
                        }
                    }
                } else if (counted) {
                    ++n_run;
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
#pragma unroll
                        for (int i = 0; i < 16; ++i)
                            run[q][i] += (double)ts_product(q, acc[0][0][i], acc[0][1][i], acc[NOP - 1][0][i], acc[NOP - 1][1][i]);
                }
            }
            if constexpr (MODE != TS_COEF) {
                if (walk) {
                    n_total += n_run;
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
#pragma unroll
                        for (int i = 0; i < 16; ++i) total[q][i] += run[q][i];
                } else if (col_ok) {
                    // partial[slab][q][f][column], part_cnt[slab][column]
                    if (wave_on) {
#pragma unroll
                        for (int q = 0; q < NQ; ++q)
#pragma unroll
                            for (int i = 0; i < 16; ++i) {
                                const int f = fw + 8 * (i >> 2) + 4 * h + (i & 3);
                                if (f < K) partial[((slab * NQ + q) * K + f) * G.A.ncol + my_col] = run[q][i];
                            }
                    }
                    if (ft == 0 && wv == 0 && h == 0) part_cnt[slab * G.A.ncol + my_col] = n_run;
                }
            }
        }
        if constexpr (MODE != TS_COEF) {
            if (walk && col_ok) {
                if (wave_on) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const int f = fw + 8 * (i >> 2) + 4 * h + (i & 3);
                            if (f < K)
                                out[q * G.outer_stride + (int64_t)f * G.A.out_row_stride + my_ooff] =
                                    ts_result(total[q][i], n_total, G.min_count, G.scale, f, M);
                        }
                }
                if (count && ft == 0 && wv == 0 && h == 0) count[my_ooff] = n_total;
            }
        }
    }
}

// launch 2 (split = 1): the slab sums added in slab order from zero, as the walking workgroup adds them
__global__ void __launch_bounds__(256) time_spectrum_finish_kernel(TsGeom G, int nq, const double *__restrict__ partial,
                                                                  const int32_t *__restrict__ part_cnt, float *__restrict__ out,
                                                                  int32_t *__restrict__ count) {
    const int64_t n = (int64_t)nq * G.K * G.A.ncol;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t col = i % G.A.ncol, qf = i / G.A.ncol;
        const int f = (int)(qf % G.K), q = (int)(qf / G.K);
        double total = 0.0;
        int n_total = 0;
        for (int64_t s = 0; s < G.n_slab; ++s) {
            total += partial[((s * nq + q) * G.K + f) * G.A.ncol + col];
            n_total += part_cnt[s * G.A.ncol + col];
        }
        int64_t so, oo;
        rows_offsets<1, false>(G.A, col, so, oo);
        out[q * G.outer_stride + (int64_t)f * G.A.out_row_stride + oo] = ts_result(total, n_total, G.min_count, G.scale, f, G.M);
        if (count && qf == 0) count[oo] = n_total;
    }
}

struct TsPlan {
    TsGeom G;
    int mode;
    bool vec;
    int64_t inner, grid, finish_grid;
    size_t partial_bytes, cnt_bytes;
    int lds_bytes;
};

// a, b: looked at for 16-byte alignment only
int ts_plan(const dlwpcs_rows_desc *d, const void *a, const void *b, int64_t n_rows, int n_segment, int64_t hop, int n_freq, int mode,
            int split, TsPlan &P) {
    TsGeom &G = P.G;
    memset(&G, 0, sizeof(G));
    const int rc = rows_addr_init(d, "time_spectrum", G.A, P.inner);
    if (rc != DLWPCS_OK) return rc;
    if (n_segment < 2) return fail(DLWPCS_E_INVALID, "time_spectrum: segments of %d rows (at least 2)", n_segment);
    if (n_segment > DLWPCS_TIME_SPECTRUM_MAX_M)
        return fail(DLWPCS_E_UNSUPPORTED, "time_spectrum: segments of %d rows, this build serves 2 .. %d", n_segment,
                    DLWPCS_TIME_SPECTRUM_MAX_M);
    if (hop < 1 || hop > (1ll << 31)) return fail(DLWPCS_E_INVALID, "time_spectrum: hop %lld", (long long)hop);
    if (n_rows < 0 || n_rows > (1ll << 40)) return fail(DLWPCS_E_INVALID, "time_spectrum: %lld rows", (long long)n_rows);
    if (n_freq < 0 || n_freq > n_segment / 2 + 1)
        return fail(DLWPCS_E_INVALID, "time_spectrum: n_freq = %d outside 1 .. M/2 + 1 = %d (0: all)", n_freq, n_segment / 2 + 1);
    if (mode != DLWPCS_SPECTRUM_POWER && mode != DLWPCS_SPECTRUM_COEFFICIENTS) return fail(DLWPCS_E_INVALID, "time_spectrum: mode %d", mode);
    if (mode == DLWPCS_SPECTRUM_COEFFICIENTS && b) return fail(DLWPCS_E_INVALID, "time_spectrum: the coefficient form takes one operand");
    if (split < -1 || split > 1) return fail(DLWPCS_E_INVALID, "time_spectrum: split %d", split);
    P.mode = mode == DLWPCS_SPECTRUM_COEFFICIENTS ? TS_COEF : (b ? TS_PAIR : TS_POWER);
    G.M = n_segment;
    G.K = n_freq ? n_freq : n_segment / 2 + 1;
    G.hop = hop;
    G.n_seg = n_rows >= n_segment ? (n_rows - n_segment) / hop + 1 : 0;
    G.n_slab = (G.n_seg + TS_SLAB - 1) / TS_SLAB;
    G.n_ft = (G.K + TS_FT - 1) / TS_FT;
    G.A.ncol = P.inner;
    G.A.tiles = (P.inner + TS_COLS - 1) / TS_COLS;
    const int64_t base = G.A.tiles * G.n_ft;
    if (P.mode == TS_COEF) {
        G.split = 1;
        G.A.nblk = base * G.n_slab;
    } else {
        // one slab (or none: NaN everywhere) is walked whatever was asked for: there is nothing to add up
        G.split = G.n_slab < 2 ? 0 : (split >= 0 ? split : (base < TS_SPLIT_BELOW ? 1 : 0));
        G.A.nblk = G.split ? base * G.n_slab : base;
    }
    if (G.A.tiles >= (1ll << 40) || G.A.nblk >= (1ll << 48)) return fail(DLWPCS_E_UNSUPPORTED, "time_spectrum: too many tiles");
    bool vec, ovec;
    rows_vector_ok(d, vec, ovec);
    P.vec = vec && aligned16(a) && aligned16(b);
    P.grid = G.A.nblk < TS_SLOTS ? G.A.nblk : TS_SLOTS;
    const int nq = P.mode == TS_PAIR ? 4 : 1;
    P.partial_bytes = P.cnt_bytes = 0;
    P.finish_grid = 0;
    if (P.mode != TS_COEF && G.split) {
        P.partial_bytes = (size_t)G.n_slab * nq * (size_t)G.K * (size_t)P.inner * sizeof(double);
        P.cnt_bytes = (size_t)G.n_slab * (size_t)P.inner * sizeof(int32_t);
        const int64_t n = ((int64_t)nq * G.K * P.inner + 255) / 256;
        P.finish_grid = n < TS_FINISH_BLOCKS ? n : TS_FINISH_BLOCKS;
    }
    const int nop = P.mode == TS_PAIR ? 2 : 1;
    P.lds_bytes = (int)(sizeof(float2) * DLWPCS_TIME_SPECTRUM_MAX_M + nop * (TS_RC * TS_COLS + TS_COLS) * sizeof(float) +
                        TS_COLS * (2 * sizeof(int64_t) + 2 * sizeof(int)));
    return DLWPCS_OK;
}

template <int MODE>
void ts_launch(const TsPlan &P, const float *a, const float *b, const float *window, const float2 *tw, double *partial,
               int32_t *part_cnt, float *out, int32_t *count, hipStream_t s) {
    const dim3 grid((unsigned)P.grid), blk(TS_THREADS);
    if (P.vec) hipLaunchKernelGGL((time_spectrum_kernel<MODE, true>), grid, blk, 0, s, P.G, a, b, window, tw, partial, part_cnt, out, count);
    else hipLaunchKernelGGL((time_spectrum_kernel<MODE, false>), grid, blk, 0, s, P.G, a, b, window, tw, partial, part_cnt, out, count);
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" size_t dlwpcs_time_spectrum_scratch_bytes(const dlwpcs_rows_desc *d, int64_t n_rows, int n_segment, int64_t hop, int n_freq,
                                                     int pair, int split) {
    TsPlan P;
    static const float some = 0.f;
    if (ts_plan(d, nullptr, pair ? &some : nullptr, n_rows, n_segment, hop, n_freq, DLWPCS_SPECTRUM_POWER, split, P) != DLWPCS_OK) return 0;
    return P.partial_bytes + P.cnt_bytes;
}

extern "C" int dlwpcs_time_spectrum(const dlwpcs_rows_desc *d, const float *a, const float *b, int64_t n_rows, int n_segment, int64_t hop,
                                    const float *window, const float *twiddle, double window_power, int detrend, int n_freq,
                                    int min_count, int mode, int split, int64_t out_outer_stride, int64_t out_part_stride, float *out,
                                    int32_t *count, void *scratch, size_t scratch_bytes, dlwpcs_stream_t stream) {
    TsPlan P;
    const int rc = ts_plan(d, a, b, n_rows, n_segment, hop, n_freq, mode, split, P);
    if (rc != DLWPCS_OK) return rc;
    if (detrend != 0 && detrend != 1) return fail(DLWPCS_E_INVALID, "time_spectrum: detrend %d", detrend);
    if (min_count < 1) return fail(DLWPCS_E_INVALID, "time_spectrum: min_count %d (at least 1)", min_count);
    if (!(window_power > 0.0) || !isfinite(window_power))
        return fail(DLWPCS_E_INVALID, "time_spectrum: the window's sum of squares must be positive and finite");
    if (P.inner == 0 || P.G.A.nblk == 0) return DLWPCS_OK;
    if (!a || !window || !twiddle || !out) return fail(DLWPCS_E_INVALID, "time_spectrum: null operand");
    if ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)window) | ((uintptr_t)out) | ((uintptr_t)count)) & 3)
        return fail(DLWPCS_E_INVALID, "time_spectrum: an operand is not aligned to its 4-byte elements");
    if (((uintptr_t)twiddle) & 7) return fail(DLWPCS_E_INVALID, "time_spectrum: the twiddle table is not aligned to 8 bytes");
    if (P.partial_bytes && (!scratch || (((uintptr_t)scratch) & 7) || scratch_bytes < P.partial_bytes + P.cnt_bytes))
        return fail(DLWPCS_E_INVALID, "time_spectrum: this call needs an 8-byte aligned scratch of %zu bytes", P.partial_bytes + P.cnt_bytes);
    TsGeom &G = P.G;
    G.detrend = detrend;
    G.min_count = min_count;
    G.outer_stride = out_outer_stride;
    G.part_stride = out_part_stride;
    G.scale = 1.0 / ((double)n_segment * window_power);
    double *partial = (double *)scratch;
    int32_t *part_cnt = (int32_t *)((char *)scratch + P.partial_bytes);
    hipStream_t s = (hipStream_t)stream;
    const float2 *tw = (const float2 *)twiddle;
    if (P.mode == TS_COEF) ts_launch<TS_COEF>(P, a, b, window, tw, partial, part_cnt, out, count, s);
    else if (P.mode == TS_PAIR) ts_launch<TS_PAIR>(P, a, b, window, tw, partial, part_cnt, out, count, s);
    else ts_launch<TS_POWER>(P, a, b, window, tw, partial, part_cnt, out, count, s);
    if (P.finish_grid)
        hipLaunchKernelGGL(time_spectrum_finish_kernel, dim3((unsigned)P.finish_grid), dim3(256), 0, s, G, P.mode == TS_PAIR ? 4 : 1,
                           partial, part_cnt, out, count);
    return check_launch("time_spectrum");
}

extern "C" int dlwpcs_time_spectrum_plan_info(const dlwpcs_rows_desc *d, const void *a, const void *b, int64_t n_rows, int n_segment,
                                              int64_t hop, int n_freq, int mode, int split, int64_t info[8]) {
    if (!info) return fail(DLWPCS_E_INVALID, "time_spectrum_plan_info: null info");
    TsPlan P;
    const int rc = ts_plan(d, a, b, n_rows, n_segment, hop, n_freq, mode, split, P);
    if (rc != DLWPCS_OK) return rc;
    const bool empty = P.inner == 0 || P.G.A.nblk == 0;
    if (!empty && !a) return fail(DLWPCS_E_INVALID, "time_spectrum: null operand");
    info[0] = P.G.A.tiles;
    info[1] = P.G.n_ft;
    info[2] = P.G.n_slab;
    info[3] = empty ? 0 : P.G.A.nblk;
    info[4] = empty ? 0 : P.grid;
    info[5] = P.G.split;
    info[6] = P.vec ? 1 : 0;
    info[7] = P.lds_bytes;
    return DLWPCS_OK;
}
