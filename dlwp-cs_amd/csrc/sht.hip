// Spherical-harmonic power spectra (dlwpcs_sht_spectrum, include/dlwpcs.h states the definitions): power per total wavenumber n
// of fields x[i, j] on nlat latitudes and L longitudes,
//   X_m(i) = sum_j x[i,j] exp(-2 pi i j m / L),  a_n^m = sum_i t[(m,n)][i] X_m(i) / L,  S_n = sum_{m<=n} c_m |a_n^m|^2,
// t = (w_i / 2) Pbar_n^m(mu_i) the caller's fp32 Legendre table.  Two launches, no atomics.
//
// Stage A (sht_fourier_kernel), the longitude transform.  All latitude rows of all fields form one list of fields * nlat rows; a
// workgroup of four waves owns 32 of them and 128 orders m.  It is the matrix product of spectrum.hip with the operands swapped:
// the twiddles are the A operand and the rows the B operand of v_mfma_f32_32x32x2_f32, so that a lane ends up with ONE row and 16
// orders, and the 32 lanes of a half wave store 32 neighbouring latitudes of one (field, m, re | im) line of the scratch
//   xs[operand][field][m][re | im][nlat_pad]            (nlat_pad = nlat rounded up to 4; stage B reads it with unit stride along i).
// Rows come through LDS in chunks of 64 longitudes, the twiddles {cos, -sin}(2 pi k / L) from the length-L table in LDS at the
// reduced index (j m) mod L carried along in integers, exactly as in spectrum.hip.  The workgroups of the first 128 orders also
// write bad[field][i]: 1 when row i of the field holds a NaN or an infinity (pair form: in either operand).
//
// Stage B (sht_legendre_kernel), the latitude transform and the power.  A workgroup is ONE wave and owns 32 degrees x 32 fields.  It
// walks m = 0 .. its last degree in order; per m the product (32 degrees x nlat) . (nlat x 32 fields) runs twice (pair form: four
// times) with the same A operand -- the table tile, rows (m, n) -- and the same column mapping, so Re and Im of a coefficient sit
// in the same lane and register.  A lane loads 64 bytes of a table row and of an xs line per step (latitudes 32 t + 16 h ..+15, all
// loads issued before the first MFMA) and feeds sixteen MFMAs per accumulator; degrees n < m and n > T are zero operands, latitudes
// >= nlat are masked.  Then the fp32 products
// Re^2 + Im^2 (pair: also S_bb and the co-spectrum) are widened to fp64, multiplied by c_m / L^2 and added to the lane's sums
// in order of m; after the last m the sums are rounded to fp32 once.  The single form has the bits of the pair form's S_aa.
//
// The grid of stage B is (field tiles) x (degree tiles): a call with a handful of fields leaves most of the device idle, and the
// degree tiles cost unequally (the top tile walks every m).  No m-split is built.
//
// Analysis and synthesis (dlwpcs_sht_analysis, dlwpcs_sht_synthesis) share this geometry: the coefficient kernel is stage B's
// product with the coefficients as its output, the inverse pair (sht_ilegendre_kernel, sht_ifourier_kernel) is described where it
// stands below.  The vector forms (dlwpcs_sht_vector_synthesis, dlwpcs_sht_vector_analysis) are the same two products with four
// accumulators against the derivative and zonal tables, and the barotropic model's two streaming kernels close the file.
#include "mfma_common.h"
#include "strided.h"

namespace dlwpcs {

constexpr int SH_THREADS = 256;
constexpr int SH_ROWS = 32;                 // latitude rows of a stage-A tile (the N of the MFMA)
constexpr int SH_JC = 64;                   // longitudes per staged chunk
constexpr int SH_XS = SH_JC + 2;            // LDS row stride (floats), as in spectrum.hip
constexpr int SH_MW = 32;                   // orders per wave
constexpr int SH_MT = 4 * SH_MW;            // orders per workgroup
constexpr int SH_MAX_L = 1728;              // the twiddle table of 2 L floats lives in static LDS
constexpr int SH_TILE = 32;                 // stage B: degrees and fields of a workgroup
constexpr int SH_KV = 4;                    // stage B: 16-byte loads of a lane per step and line (a step covers 2 * 4 * SH_KV latitudes)
constexpr int SH_MC = 8;                    // coefficient kernel: orders per workgroup
constexpr int SH_JT = 4 * SH_TILE;          // inverse Fourier: longitudes per workgroup (32 per wave)
constexpr int SH_KU = 4;                    // inverse stages: MFMAs per accumulator whose operands are loaded together

struct ShGeom {
    int32_t nlat, nlp, L, T, n_dims, n_mt, n_nt;
    int32_t n_mc, n_lt, n_jt;                // order chunks of the coefficient kernel; latitude tiles, longitude tiles of the synthesis
    int64_t fields, rows, n_rt, n_ft;
    int64_t op_stride;                       // floats between the operands' halves of xs
    int64_t lat_stride[2];
    int64_t ext[DLWPCS_SCORE_MAX_DIMS];
    int64_t stride[2][DLWPCS_SCORE_MAX_DIMS];
};

// the three fp32 products of the pair form (q = 0 alone in the single form), spelled once so that both forms round alike
__device__ __forceinline__ float sh_product(int q, float cf, float sf, float cv, float sv) {
#pragma clang fp contract(off)
    if (q == 0) return __builtin_fmaf(sf, sf, cf * cf);
    if (q == 1) return __builtin_fmaf(sv, sv, cv * cv);
    return __builtin_fmaf(sf, sv, cf * cv);                             // Re(a conj b)
}
__device__ __forceinline__ double sh_add(double sum, double v, double scale) {
#pragma clang fp contract(off)
    return sum + v * scale;
}

template <bool PAIR, bool VEC>
__global__ void __launch_bounds__(SH_THREADS) sht_fourier_kernel(ShGeom G, const float *__restrict__ a, const float *__restrict__ b,
                                                                 const float2 *__restrict__ twiddle, float *__restrict__ xs,
                                                                 int32_t *__restrict__ bad) {
    constexpr int NOP = PAIR ? 2 : 1;
    constexpr int NLD = VEC ? 2 : 8;                    // loads of a thread per chunk and operand
    __shared__ float2 s_tw[SH_MAX_L];
    __shared__ __attribute__((aligned(16))) float s_x[NOP][SH_ROWS * SH_XS];
    __shared__ int64_t s_off[NOP][SH_ROWS];
    __shared__ int64_t s_line[SH_ROWS];                 // xs offset of (field, m = 0, re, latitude) of the slot's row
    __shared__ int64_t s_flag[SH_ROWS];
    __shared__ int s_valid[SH_ROWS], s_bad[SH_ROWS];

    const int64_t bid = flat_block();
    if (bid >= G.n_rt * G.n_mt) return;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int mt = (int)(bid % G.n_mt);
    const int64_t rt = bid / G.n_mt;
    const int L = G.L, K = G.T + 1;

    for (int m = tid; m < L; m += SH_THREADS) s_tw[m] = twiddle[m];

    const int r32 = lane & 31, h = lane >> 5;
    const int kw = mt * SH_MT + wv * SH_MW + r32;       // this lane's order as the row of the A operand
    const bool wave_on = mt * SH_MT + wv * SH_MW < K;
    const int step4 = (int)((4ll * kw) % L);

    if (tid < SH_ROWS) {
        const int64_t r = rt * SH_ROWS + tid;
        const bool valid = r < G.rows;
        int64_t off[2] = {0, 0}, f = 0;
        int i = 0;
        if (valid) {
            f = r / G.nlat;
            i = (int)(r - f * G.nlat);
            int64_t q = f;
            for (int d = G.n_dims - 1; d >= 0; --d) {
                const int64_t e = G.ext[d], c = q % e;
                q /= e;
                off[0] += c * G.stride[0][d];
                off[1] += c * G.stride[1][d];
            }
            off[0] += (int64_t)i * G.lat_stride[0];
            off[1] += (int64_t)i * G.lat_stride[1];
        }
        s_off[0][tid] = off[0];
        if (PAIR) s_off[NOP - 1][tid] = off[1];
        s_line[tid] = f * K * 2 * G.nlp + i;
        s_flag[tid] = f * G.nlat + i;
        s_valid[tid] = valid;
        s_bad[tid] = 0;
    }
    __syncthreads();

    // staging: the slot and column of this thread's loads are the same in every chunk
    int ld_row[NLD], ld_col[NLD];
    int64_t ld_off[NOP][NLD];
    bool ld_ok[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int idx = tid + i * SH_THREADS;
        ld_row[i] = VEC ? idx >> 4 : idx >> 6;
        ld_col[i] = VEC ? (idx & 15) * 4 : idx & 63;
        ld_ok[i] = s_valid[ld_row[i]] != 0;
#pragma unroll
        for (int op = 0; op < NOP; ++op) ld_off[op][i] = s_off[op][ld_row[i]];
    }
    const int n_chunks = (L + SH_JC - 1) / SH_JC;
    unsigned bad_mask = 0;

    float regs[NOP][NLD][VEC ? 4 : 1];
    auto fetch = [&](int chunk) {
        const int j0 = chunk * SH_JC;
#pragma unroll
        for (int op = 0; op < NOP; ++op) {
            const float *src = op == 0 ? a : b;
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int j = j0 + ld_col[i];
                if constexpr (VEC) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (ld_ok[i] && j < L) v = *reinterpret_cast<const float4 *>(src + ld_off[op][i] + j);   // (L % 4 == 0)
                    regs[op][i][0] = v.x; regs[op][i][1] = v.y; regs[op][i][2] = v.z; regs[op][i][3] = v.w;
                } else {
                    regs[op][i][0] = (ld_ok[i] && j < L) ? src[ld_off[op][i] + j] : 0.f;
                }
            }
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int op = 0; op < NOP; ++op)
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                float v[VEC ? 4 : 1];
#pragma unroll
                for (int e = 0; e < (VEC ? 4 : 1); ++e) {
                    v[e] = regs[op][i][e];              // (zero outside the row: fetch has seen to it)
                    if (nonfinite(v[e])) bad_mask |= 1u << i;
                }
                float *dst = &s_x[op][ld_row[i] * SH_XS + ld_col[i]];
                if constexpr (VEC) {
                    *reinterpret_cast<float2 *>(dst) = make_float2(v[0], v[1]);
                    *reinterpret_cast<float2 *>(dst + 2) = make_float2(v[VEC ? 2 : 0], v[VEC ? 3 : 0]);
                } else {
                    *dst = v[0];
                }
            }
    };

    f32x16 acc[NOP][2];
#pragma unroll
    for (int op = 0; op < NOP; ++op)
#pragma unroll
        for (int cs = 0; cs < 2; ++cs)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[op][cs][i] = 0.f;
    // reduced twiddle indices of this lane's two longitudes per step: j = 4 t + 2 h + u, u = 0, 1
    int m0 = (int)(((int64_t)(2 * h) * kw) % L), m1 = (int)(((int64_t)(2 * h + 1) * kw) % L);

    fetch(0);
    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        __syncthreads();                                // the previous chunk has been consumed
        stash();
        if (chunk + 1 == n_chunks) {
#pragma unroll
            for (int i = 0; i < NLD; ++i)
                if (bad_mask & (1u << i)) s_bad[ld_row[i]] = 1;
        }
        __syncthreads();
        if (chunk + 1 < n_chunks) fetch(chunk + 1);
        if (wave_on) {
            const int left = L - chunk * SH_JC;
            const int nt = left >= SH_JC ? SH_JC / 4 : (left + 3) / 4;
            for (int t = 0; t < nt; ++t) {
                const float2 tw0 = s_tw[m0], tw1 = s_tw[m1];
                float2 xv[NOP];
#pragma unroll
                for (int op = 0; op < NOP; ++op)
                    xv[op] = *reinterpret_cast<const float2 *>(&s_x[op][r32 * SH_XS + 4 * t + 2 * h]);
#pragma unroll
                for (int op = 0; op < NOP; ++op) {
                    acc[op][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(tw0.x, xv[op].x, acc[op][0], 0, 0, 0);
                    acc[op][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(tw0.y, xv[op].x, acc[op][1], 0, 0, 0);
                }
#pragma unroll
                for (int op = 0; op < NOP; ++op) {
                    acc[op][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(tw1.x, xv[op].y, acc[op][0], 0, 0, 0);
                    acc[op][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(tw1.y, xv[op].y, acc[op][1], 0, 0, 0);
                }
                m0 += step4; m0 -= m0 >= L ? L : 0;
                m1 += step4; m1 -= m1 >= L ? L : 0;
            }
        }
    }

    // the lane holds row slot r32 (the column of the product) and the orders 8 (i >> 2) + 4 h + (i & 3) of its wave
    if (wave_on && s_valid[r32]) {
        const int64_t line = s_line[r32];
#pragma unroll
        for (int op = 0; op < NOP; ++op) {
            float *dst = xs + op * G.op_stride + line;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int m = mt * SH_MT + wv * SH_MW + 8 * (i >> 2) + 4 * h + (i & 3);
                if (m < K) {
                    dst[((int64_t)m * 2) * G.nlp] = acc[op][0][i];
                    dst[((int64_t)m * 2 + 1) * G.nlp] = acc[op][1][i];
                }
            }
        }
    }
    if (mt == 0 && tid < SH_ROWS && s_valid[tid]) bad[s_flag[tid]] = s_bad[tid];
}

// One order m of stage B: acc[op][re | im] = (32 degrees x nlat) . (nlat x 32 fields), the table tile rows (m, nA) as the A operand,
// the lines of xs as the B operand.  Shared by the power kernel and the coefficient kernel: same tiles, operand mapping and masks.
template <int NOP>
__device__ __forceinline__ void sh_legendre_order(const ShGeom &G, const float *__restrict__ xs, const float *__restrict__ table,
                                                  int m, int nA, int64_t fB, bool f_ok, int h, f32x16 (&acc)[NOP][2]) {
    const int T = G.T, K = T + 1, nlat = G.nlat, nlp = G.nlp;
    const int n_steps = (nlp + 2 * SH_KV * 4 - 1) / (2 * SH_KV * 4);
#pragma unroll
    for (int op = 0; op < NOP; ++op)
#pragma unroll
        for (int cs = 0; cs < 2; ++cs)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[op][cs][i] = 0.f;
    const bool a_on = nA >= m && nA <= T;
    const int64_t row = (int64_t)m * K - (int64_t)m * (m - 1) / 2 + (nA - m);
    const float *pa = table + (a_on ? row : 0) * nlp;
    const float *pb = xs + (((f_ok ? fB : 0) * K + m) * 2) * nlp;
    for (int t = 0; t < n_steps; ++t) {
        // all loads of the step are issued before its first MFMA: one wait per 32 latitudes
        const int i0 = 2 * SH_KV * 4 * t + SH_KV * 4 * h;
        float4 av[SH_KV], xv[NOP][2][SH_KV];
#pragma unroll
        for (int u = 0; u < SH_KV; ++u) {
            const int iu = i0 + 4 * u;
            const bool in = iu < nlp;                // (nlp is a multiple of 4: the 16 bytes lie inside the line or outside)
            av[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (a_on && in) av[u] = *reinterpret_cast<const float4 *>(pa + iu);
#pragma unroll
            for (int op = 0; op < NOP; ++op)
#pragma unroll
                for (int cs = 0; cs < 2; ++cs) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (f_ok && in) v = *reinterpret_cast<const float4 *>(pb + op * G.op_stride + (int64_t)cs * nlp + iu);
                    v.x = iu < nlat ? v.x : 0.f;    // the padding of xs is never written
                    v.y = iu + 1 < nlat ? v.y : 0.f;
                    v.z = iu + 2 < nlat ? v.z : 0.f;
                    v.w = iu + 3 < nlat ? v.w : 0.f;
                    xv[op][cs][u] = v;
                }
        }
#pragma unroll
        for (int u = 0; u < SH_KV; ++u) {
            if (2 * SH_KV * 4 * t + 4 * u >= nlp) break;        // (wave-uniform: both halves of these MFMAs lie beyond the lines)
#pragma unroll
            for (int op = 0; op < NOP; ++op)
#pragma unroll
                for (int cs = 0; cs < 2; ++cs) {
                    const float4 x = xv[op][cs][u];
                    acc[op][cs] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u].x, x.x, acc[op][cs], 0, 0, 0);
                    acc[op][cs] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u].y, x.y, acc[op][cs], 0, 0, 0);
                    acc[op][cs] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u].z, x.z, acc[op][cs], 0, 0, 0);
                    acc[op][cs] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u].w, x.w, acc[op][cs], 0, 0, 0);
                }
        }
    }
}

template <bool PAIR>
__global__ void __launch_bounds__(64) sht_legendre_kernel(ShGeom G, const float *__restrict__ xs, const int32_t *__restrict__ bad,
                                                          const float *__restrict__ table, float *__restrict__ out,
                                                          int32_t *__restrict__ skipped) {
    constexpr int NOP = PAIR ? 2 : 1;
    constexpr int NQ = PAIR ? 3 : 1;
    const int64_t bid = flat_block();
    if (bid >= G.n_ft * G.n_nt) return;
    const int lane = (int)threadIdx.x, r32 = lane & 31, h = lane >> 5;
    const int nt = (int)(bid % G.n_nt);
    const int64_t ft = bid / G.n_nt;
    const int T = G.T, K = T + 1, nlat = G.nlat;
    const int n0 = nt * SH_TILE;
    const int nA = n0 + r32;                             // this lane's degree as the row of the A operand
    const int64_t fB = ft * SH_TILE + r32;               // this lane's field as the column of the B operand
    const bool f_ok = fB < G.fields;

    int isbad = 0;
    if (f_ok)
        for (int i = h; i < nlat; i += 2) isbad |= bad[fB * nlat + i];
    isbad |= __shfl_xor(isbad, 32, 64);

    double sum[NQ][16];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int i = 0; i < 16; ++i) sum[q][i] = 0.0;

    const int m_last = n0 + SH_TILE - 1 < T ? n0 + SH_TILE - 1 : T;
    const double inv_l2 = 1.0 / ((double)G.L * (double)G.L);
    for (int m = 0; m <= m_last; ++m) {
        f32x16 acc[NOP][2];
        sh_legendre_order<NOP>(G, xs, table, m, nA, fB, f_ok, h, acc);
        const double scale = (m == 0 ? 1.0 : 2.0) * inv_l2;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float cf = acc[0][0][i], sf = acc[0][1][i], cv = acc[NOP - 1][0][i], sv = acc[NOP - 1][1][i];
#pragma unroll
            for (int q = 0; q < NQ; ++q) sum[q][i] = sh_add(sum[q][i], (double)sh_product(q, cf, sf, cv, sv), scale);
        }
    }

    // the lane holds field fB (the column) and the degrees n0 + 8 (i >> 2) + 4 h + (i & 3)
    if (f_ok) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int n = n0 + 8 * (i >> 2) + 4 * h + (i & 3);
            if (n > T) continue;
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                out[((int64_t)q * G.fields + fB) * K + n] = isbad ? __uint_as_float(0x7fc00000u) : (float)sum[q][i];
        }
        if (skipped && nt == 0 && h == 0) skipped[fB] = isbad ? 1 : 0;
    }
}

// ---- coefficients (dlwpcs_sht_analysis) ----------------------------------------------------------------------------------------
// Stage B with the coefficients as its output: the product of sh_legendre_order in the single form, then
//   coef[field][row (m, n)] = { fl(Re / L), fl(Im / L) }:  the fp32 sum is divided by L in fp64 and rounded to fp32, which is ONE
// rounding of the exact quotient (53 >= 2 * 24 + 2 bits: the double rounding of a quotient of two fp32 numbers is innocuous).
// The orders are independent here, so a workgroup (one wave) owns 32 degrees x 32 fields x SH_MC orders: the grid is (field tiles)
// x (degree tiles) x (order chunks), and a chunk above its tile's last degree leaves at once.  The scan of the fields' row flags
// is paid once per chunk.
__device__ __forceinline__ float sh_div_l(float v, double L) { return (float)((double)v / L); }

__global__ void __launch_bounds__(64) sht_coef_kernel(ShGeom G, const float *__restrict__ xs, const int32_t *__restrict__ bad,
                                                      const float *__restrict__ table, float2 *__restrict__ coef,
                                                      int32_t *__restrict__ skipped) {
    const int64_t bid = flat_block();
    if (bid >= G.n_ft * G.n_nt * G.n_mc) return;
    const int lane = (int)threadIdx.x, r32 = lane & 31, h = lane >> 5;
    const int mc = (int)(bid % G.n_mc);
    const int nt = (int)((bid / G.n_mc) % G.n_nt);
    const int64_t ft = bid / G.n_mc / G.n_nt;
    const int T = G.T, K = T + 1, nlat = G.nlat;
    const int n0 = nt * SH_TILE;
    const int m_last = n0 + SH_TILE - 1 < T ? n0 + SH_TILE - 1 : T;
    const int m_begin = mc * SH_MC;
    if (m_begin > m_last) return;
    const int m_end = m_begin + SH_MC - 1 < m_last ? m_begin + SH_MC - 1 : m_last;
    const int nA = n0 + r32;
    const int64_t fB = ft * SH_TILE + r32;
    const bool f_ok = fB < G.fields;
    const int64_t R = (int64_t)K * (K + 1) / 2;

    int isbad = 0;
    if (f_ok)
        for (int i = h; i < nlat; i += 2) isbad |= bad[fB * nlat + i];
    isbad |= __shfl_xor(isbad, 32, 64);

    const double Ld = (double)G.L;
    const float nan = __uint_as_float(0x7fc00000u);
    for (int m = m_begin; m <= m_end; ++m) {
        f32x16 acc[1][2];
        sh_legendre_order<1>(G, xs, table, m, nA, fB, f_ok, h, acc);
        if (!f_ok) continue;
        const int64_t row0 = (int64_t)m * K - (int64_t)m * (m - 1) / 2 - m;       // row (m, n) = row0 + n
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int n = n0 + 8 * (i >> 2) + 4 * h + (i & 3);
            if (n < m || n > T) continue;
            coef[fB * R + row0 + n] = isbad ? make_float2(nan, nan) : make_float2(sh_div_l(acc[0][0][i], Ld), sh_div_l(acc[0][1][i], Ld));
        }
    }
    if (skipped && f_ok && nt == 0 && mc == 0 && h == 0) skipped[fB] = isbad ? 1 : 0;
}

// ---- synthesis (dlwpcs_sht_synthesis) ------------------------------------------------------------------------------------------
//   x[i, j] = sum_{m=0..T} c_m Re( e^{+2 pi i j m / L} G_m(i) ),   G_m(i) = sum_{n=m..T} P[(m, n)][i] fl(r_n a_n^m),
// P the UNWEIGHTED fp32 table Pbar_n^m(mu_i) (the packing of the analysis table), r the response (NULL: ones).  Two launches.
//
// Inverse Legendre (sht_ilegendre_kernel).  A workgroup is one wave and owns ONE order m, 32 latitudes and 32 fields: the product
// (32 latitudes x degrees) . (degrees x 32 fields) with the degrees m .. T as the k of v_mfma_f32_32x32x2_f32, two per MFMA (lane
// half h holds n = m + 2 t + h).  The A operand is one float of table row (m, n) per lane -- the 32 lanes of a half read 32
// neighbouring latitudes of the row --, the B operand fl(r_n Re a) and fl(r_n Im a) of the lane's field (Im a_n^0 enters as zero).
// Degrees > T, latitudes >= nlat and fields beyond the last are SELECTED to zero in both operands, never multiplied by zero.  The
// operands of SH_KU MFMAs per accumulator are loaded before the first of them.  The lane ends with its field and four runs of four
// latitudes: 16-byte stores into gs[field][m][re | im][nlat_pad] (stage A's layout of xs); the padding is not written.
// The grid is (field tiles) x (latitude tiles) x (orders): no wave walks the orders, the longest chain is T + 1 degrees.
__global__ void __launch_bounds__(64) sht_ilegendre_kernel(ShGeom G, const float2 *__restrict__ coef, const float *__restrict__ response,
                                                           const float *__restrict__ ptable, float *__restrict__ gs) {
    const int64_t bid = flat_block();
    const int T = G.T, K = T + 1, nlat = G.nlat, nlp = G.nlp;
    if (bid >= G.n_ft * G.n_lt * K) return;
    const int lane = (int)threadIdx.x, r32 = lane & 31, h = lane >> 5;
    const int m = (int)(bid % K);
    const int lt = (int)((bid / K) % G.n_lt);
    const int64_t ft = bid / K / G.n_lt;
    const int iA = lt * SH_TILE + r32;                   // this lane's latitude as the row of the A operand
    const int64_t fB = ft * SH_TILE + r32;               // this lane's field as the column of the B operand
    const bool a_ok = iA < nlat, f_ok = fB < G.fields;
    const int64_t R = (int64_t)K * (K + 1) / 2;
    const int64_t row0 = (int64_t)m * K - (int64_t)m * (m - 1) / 2;               // row (m, m)
    const int count = K - m;                             // degrees m .. T
    const float *pa = ptable + row0 * nlp + (a_ok ? iA : 0);
    const float2 *pb = coef + (f_ok ? fB : 0) * R + row0;

    f32x16 acc[2];
#pragma unroll
    for (int cs = 0; cs < 2; ++cs)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[cs][i] = 0.f;
    for (int k0 = 0; k0 < count; k0 += 2 * SH_KU) {
        float av[SH_KU];
        float2 bv[SH_KU];
#pragma unroll
        for (int u = 0; u < SH_KU; ++u) {
            const int k = k0 + 2 * u + h;
            const bool on = k < count;
            av[u] = 0.f;
            bv[u] = make_float2(0.f, 0.f);
            if (on && a_ok) av[u] = pa[(int64_t)k * nlp];
            if (on && f_ok) {
                const float2 c = pb[k];
                const float r = response ? response[m + k] : 1.f;
                bv[u] = make_float2(r * c.x, m == 0 ? 0.f : r * c.y);
            }
        }
#pragma unroll
        for (int u = 0; u < SH_KU; ++u) {
            if (k0 + 2 * u >= count) break;              // (wave-uniform)
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u].x, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u].y, acc[1], 0, 0, 0);
        }
    }

    // the lane holds field fB (the column) and the latitudes 32 lt + 8 q + 4 h + (0 .. 3)
    if (f_ok) {
        float *dst = gs + ((fB * K + m) * 2) * nlp;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = lt * SH_TILE + 8 * q + 4 * h;
            if (i >= nlat) continue;
#pragma unroll
            for (int cs = 0; cs < 2; ++cs) {
                float *p = dst + (int64_t)cs * nlp + i;
                if (i + 3 < nlat) {
                    *reinterpret_cast<float4 *>(p) = make_float4(acc[cs][4 * q], acc[cs][4 * q + 1], acc[cs][4 * q + 2], acc[cs][4 * q + 3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 3; ++e)
                        if (i + e < nlat) p[e] = acc[cs][4 * q + e];
                }
            }
        }
    }
}

// Inverse Fourier (sht_ifourier_kernel).  The rows (field, latitude) form one list as in stage A; a workgroup of four waves owns 32
// of them and SH_JT longitudes, 32 per wave.  Per order m ONE MFMA: the A operand is the twiddle of the lane's longitude -- lane
// half 0 holds c_m cos, half 1 holds -c_m sin (c_m is 1 or 2: exact) from the {cos, -sin} table in LDS at the reduced index
// (j m) mod L carried along in integers --, the B operand Re G_m (half 0) and Im G_m (half 1) of the lane's row, read from gs with
// unit stride along the latitudes.  Orders 0 .. T only, in order; longitudes >= L and rows beyond the last are selected to zero.
// The lane ends with ONE row and four runs of four longitudes: 16-byte stores (VEC) or element stores of the same registers.
template <bool VEC>
__global__ void __launch_bounds__(SH_THREADS) sht_ifourier_kernel(ShGeom G, const float *__restrict__ gs, const float2 *__restrict__ twiddle,
                                                                  float *__restrict__ out) {
    __shared__ float2 s_tw[SH_MAX_L];
    __shared__ int64_t s_off[SH_ROWS];                  // offset of the row in the output
    __shared__ int64_t s_line[SH_ROWS];                 // gs offset of (field, m = 0, re, latitude) of the slot's row
    __shared__ int s_valid[SH_ROWS];

    const int64_t bid = flat_block();
    if (bid >= G.n_rt * G.n_jt) return;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int jt = (int)(bid % G.n_jt);
    const int64_t rt = bid / G.n_jt;
    const int L = G.L, K = G.T + 1, nlp = G.nlp;

    for (int m = tid; m < L; m += SH_THREADS) s_tw[m] = twiddle[m];
    if (tid < SH_ROWS) {
        const int64_t r = rt * SH_ROWS + tid;
        const bool valid = r < G.rows;
        int64_t off = 0, f = 0;
        int i = 0;
        if (valid) {
            f = r / G.nlat;
            i = (int)(r - f * G.nlat);
            int64_t q = f;
            for (int d = G.n_dims - 1; d >= 0; --d) {
                const int64_t e = G.ext[d], c = q % e;
                q /= e;
                off += c * G.stride[0][d];
            }
            off += (int64_t)i * G.lat_stride[0];
        }
        s_off[tid] = off;
        s_line[tid] = f * K * 2 * nlp + i;
        s_valid[tid] = valid;
    }
    __syncthreads();

    const int r32 = lane & 31, h = lane >> 5;
    const int j0 = jt * SH_JT + wv * SH_TILE;
    if (j0 >= L) return;
    const int jA = j0 + r32;                            // this lane's longitude as the row of the A operand
    const bool a_ok = jA < L, b_ok = s_valid[r32] != 0;
    const int step = a_ok ? jA : 0;                     // (j m) mod L grows by j per order
    const float *tw = reinterpret_cast<const float *>(s_tw) + h;
    const float *pb = gs + (b_ok ? s_line[r32] : 0) + (int64_t)h * nlp;

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    int idx = 0;
    for (int m0 = 0; m0 < K; m0 += SH_KU) {
        float av[SH_KU], bv[SH_KU];
#pragma unroll
        for (int u = 0; u < SH_KU; ++u) {
            const int m = m0 + u;
            const bool on = m < K;
            const float t = tw[2 * idx];
            av[u] = (on && a_ok) ? (m == 0 ? t : 2.f * t) : 0.f;
            bv[u] = 0.f;
            if (on && b_ok) bv[u] = pb[(int64_t)m * 2 * nlp];
            idx += step; idx -= idx >= L ? L : 0;
        }
#pragma unroll
        for (int u = 0; u < SH_KU; ++u) {
            if (m0 + u >= K) break;                     // (wave-uniform)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
        }
    }

    // the lane holds row slot r32 (the column) and the longitudes j0 + 8 q + 4 h + (0 .. 3)
    if (b_ok) {
        float *dst = out + s_off[r32];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = j0 + 8 * q + 4 * h;
            if (j >= L) continue;
            if constexpr (VEC) {                        // (L % 4 == 0: the 16 bytes lie inside the row)
                *reinterpret_cast<float4 *>(dst + j) = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j + e < L) dst[j + e] = acc[4 * q + e];
            }
        }
    }
}

// ---- vector harmonics (dlwpcs_sht_vector_synthesis, dlwpcs_sht_vector_analysis) ------------------------------------------------
// Winds from potentials and vorticity / divergence from winds.  D = dPbar_n^m / dphi and Q = m Pbar_n^m / cos(phi) are the caller's
// fp32 tables in the packing of the Legendre table (unweighted for the synthesis, times w_i / 2 for the analysis):
//   U_m(i) = sum_n [ -D psi + i Q chi ],   V_m(i) = sum_n [ i Q psi + D chi ],      psi = fl(rpsi_n A_n^m), chi = fl(rchi_n B_n^m)
//   zeta_n^m = r_n sum_i [ i wQ V_m + wD U_m ] / L,   delta_n^m = r_n sum_i [ i wQ U_m - wD V_m ] / L.
// The factor i is carried in the B operand: a swap of Re and Im and a negation, both exact.
//
// Inverse vector Legendre (sht_vilegendre_kernel): the grid, tile and operand mapping of sht_ilegendre_kernel with four accumulators
//   U_re += D (-psi_re), Q (-chi_im)    U_im += D (-psi_im), Q (chi_re)    V_re += Q (-psi_im), D (chi_re)    V_im += Q (psi_re), D (chi_im)
// per pair of degrees, the psi term before the chi term.  An absent potential is compiled out: it costs no MFMA.  Im of order 0
// enters as zero.  Degrees > T, latitudes >= nlat and fields beyond the last are selected to zero in both operands.  The result
// goes to gs[u | v][field][m][re | im][nlat_pad]; sht_ifourier_kernel then runs once per component through that output's strides.
template <bool HAS_A, bool HAS_B>
__global__ void __launch_bounds__(64) sht_vilegendre_kernel(ShGeom G, const float2 *__restrict__ coef_a, const float2 *__restrict__ coef_b,
                                                            const float *__restrict__ rpsi, const float *__restrict__ rchi,
                                                            const float *__restrict__ dtable, const float *__restrict__ qtable,
                                                            float *__restrict__ gs) {
    const int64_t bid = flat_block();
    const int T = G.T, K = T + 1, nlat = G.nlat, nlp = G.nlp;
    if (bid >= G.n_ft * G.n_lt * K) return;
    const int lane = (int)threadIdx.x, r32 = lane & 31, h = lane >> 5;
    const int m = (int)(bid % K);
    const int lt = (int)((bid / K) % G.n_lt);
    const int64_t ft = bid / K / G.n_lt;
    const int iA = lt * SH_TILE + r32;                   // this lane's latitude as the row of the A operand
    const int64_t fB = ft * SH_TILE + r32;               // this lane's field as the column of the B operand
    const bool a_ok = iA < nlat, f_ok = fB < G.fields;
    const int64_t R = (int64_t)K * (K + 1) / 2;
    const int64_t row0 = (int64_t)m * K - (int64_t)m * (m - 1) / 2;               // row (m, m)
    const int count = K - m;                             // degrees m .. T
    const int64_t a_off = row0 * nlp + (a_ok ? iA : 0);
    const int64_t b_off = (f_ok ? fB : 0) * R + row0;

    f32x16 acc[2][2];                                    // [u | v][re | im]
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int cs = 0; cs < 2; ++cs)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[c][cs][i] = 0.f;
    for (int k0 = 0; k0 < count; k0 += 2 * SH_KU) {
        float dv[SH_KU], qv[SH_KU];
        float2 pv[SH_KU], cv[SH_KU];
#pragma unroll
        for (int u = 0; u < SH_KU; ++u) {
            const int k = k0 + 2 * u + h;
            const bool on = k < count;
            dv[u] = 0.f;
            qv[u] = 0.f;
            pv[u] = make_float2(0.f, 0.f);
            cv[u] = make_float2(0.f, 0.f);
            if (on && a_ok) {
                dv[u] = dtable[a_off + (int64_t)k * nlp];
                qv[u] = qtable[a_off + (int64_t)k * nlp];
            }
            if (on && f_ok) {
                if constexpr (HAS_A) {
                    const float2 c = coef_a[b_off + k];
                    const float r = rpsi ? rpsi[m + k] : 1.f;
                    pv[u] = make_float2(r * c.x, m == 0 ? 0.f : r * c.y);
                }
                if constexpr (HAS_B) {
                    const float2 c = coef_b[b_off + k];
                    const float r = rchi ? rchi[m + k] : 1.f;
                    cv[u] = make_float2(r * c.x, m == 0 ? 0.f : r * c.y);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < SH_KU; ++u) {
            if (k0 + 2 * u >= count) break;              // (wave-uniform)
            if constexpr (HAS_A) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[u], -pv[u].x, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[u], -pv[u].y, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(qv[u], -pv[u].y, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(qv[u], pv[u].x, acc[1][1], 0, 0, 0);
            }
            if constexpr (HAS_B) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(qv[u], -cv[u].y, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(qv[u], cv[u].x, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[u], cv[u].x, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[u], cv[u].y, acc[1][1], 0, 0, 0);
            }
        }
    }

    // the lane holds field fB (the column) and the latitudes 32 lt + 8 q + 4 h + (0 .. 3)
    if (f_ok) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float *dst = gs + c * G.op_stride + ((fB * K + m) * 2) * nlp;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = lt * SH_TILE + 8 * q + 4 * h;
                if (i >= nlat) continue;
#pragma unroll
                for (int cs = 0; cs < 2; ++cs) {
                    float *p = dst + (int64_t)cs * nlp + i;
                    if (i + 3 < nlat) {
                        *reinterpret_cast<float4 *>(p) =
                            make_float4(acc[c][cs][4 * q], acc[c][cs][4 * q + 1], acc[c][cs][4 * q + 2], acc[c][cs][4 * q + 3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 3; ++e)
                            if (i + e < nlat) p[e] = acc[c][cs][4 * q + e];
                    }
                }
            }
        }
    }
}

// Vector coefficient stage (sht_vcoef_kernel): the grid, tiles, operand mapping and masks of sht_coef_kernel on the pair-form scratch
// of stage A (operand 0 = u, operand 1 = v) with the weighted tiles wD and wQ as the A operands.  Per latitude step and accumulator
//   z_re += wD U_re, wQ (-V_im)    z_im += wD U_im, wQ V_re    d_re += wQ (-U_im), wD (-V_re)    d_im += wQ U_re, wD (-V_im)
// in that order; an absent output is compiled out.  Rounding contract: the fp32 sum is widened to fp64, divided by L and multiplied
// by the fp32 response r_n there (NULL: 1), and rounded to fp32 ONCE: coef = fl32(fl64(fl64(sum / L) r_n)), whose error is at most
// u (1 + 2^-27) of the exact sum r_n / L.  A NULL response gives the bits of a response of ones (x * 1.0 is exact).
__device__ __forceinline__ float sh_div_l_r(float v, double L, double r) {
#pragma clang fp contract(off)
    return (float)(((double)v / L) * r);
}

template <bool WZ, bool WD>
__global__ void __launch_bounds__(64) sht_vcoef_kernel(ShGeom G, const float *__restrict__ xs, const int32_t *__restrict__ bad,
                                                       const float *__restrict__ response, const float *__restrict__ wdtable,
                                                       const float *__restrict__ wqtable, float2 *__restrict__ vrt,
                                                       float2 *__restrict__ dvg, int32_t *__restrict__ skipped) {
    const int64_t bid = flat_block();
    if (bid >= G.n_ft * G.n_nt * G.n_mc) return;
    const int lane = (int)threadIdx.x, r32 = lane & 31, h = lane >> 5;
    const int mc = (int)(bid % G.n_mc);
    const int nt = (int)((bid / G.n_mc) % G.n_nt);
    const int64_t ft = bid / G.n_mc / G.n_nt;
    const int T = G.T, K = T + 1, nlat = G.nlat, nlp = G.nlp;
    const int n0 = nt * SH_TILE;
    const int m_last = n0 + SH_TILE - 1 < T ? n0 + SH_TILE - 1 : T;
    const int m_begin = mc * SH_MC;
    if (m_begin > m_last) return;
    const int m_end = m_begin + SH_MC - 1 < m_last ? m_begin + SH_MC - 1 : m_last;
    const int nA = n0 + r32;
    const int64_t fB = ft * SH_TILE + r32;
    const bool f_ok = fB < G.fields;
    const int64_t R = (int64_t)K * (K + 1) / 2;

    int isbad = 0;
    if (f_ok)
        for (int i = h; i < nlat; i += 2) isbad |= bad[fB * nlat + i];
    isbad |= __shfl_xor(isbad, 32, 64);

    const double Ld = (double)G.L;
    const float nan = __uint_as_float(0x7fc00000u);
    const int n_steps = (nlp + 2 * SH_KV * 4 - 1) / (2 * SH_KV * 4);
    for (int m = m_begin; m <= m_end; ++m) {
        f32x16 acc[2][2];                                // [vrt | div][re | im]
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int cs = 0; cs < 2; ++cs)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[c][cs][i] = 0.f;
        const bool a_on = nA >= m && nA <= T;
        const int64_t row = (int64_t)m * K - (int64_t)m * (m - 1) / 2 + (nA - m);
        const int64_t a_off = (a_on ? row : 0) * nlp;
        const float *pb = xs + (((f_ok ? fB : 0) * K + m) * 2) * nlp;
        for (int t = 0; t < n_steps; ++t) {
            const int i0 = 2 * SH_KV * 4 * t + SH_KV * 4 * h;
            float4 dv[SH_KV], qv[SH_KV], xv[2][2][SH_KV];    // xv[u | v][re | im]
#pragma unroll
            for (int u = 0; u < SH_KV; ++u) {
                const int iu = i0 + 4 * u;
                const bool in = iu < nlp;                // (nlp is a multiple of 4: the 16 bytes lie inside the line or outside)
                dv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                qv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (a_on && in) {
                    dv[u] = *reinterpret_cast<const float4 *>(wdtable + a_off + iu);
                    qv[u] = *reinterpret_cast<const float4 *>(wqtable + a_off + iu);
                }
#pragma unroll
                for (int op = 0; op < 2; ++op)
#pragma unroll
                    for (int cs = 0; cs < 2; ++cs) {
                        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (f_ok && in) v = *reinterpret_cast<const float4 *>(pb + op * G.op_stride + (int64_t)cs * nlp + iu);
                        v.x = iu < nlat ? v.x : 0.f;    // the padding of xs is never written
                        v.y = iu + 1 < nlat ? v.y : 0.f;
                        v.z = iu + 2 < nlat ? v.z : 0.f;
                        v.w = iu + 3 < nlat ? v.w : 0.f;
                        xv[op][cs][u] = v;
                    }
            }
#pragma unroll
            for (int u = 0; u < SH_KV; ++u) {
                if (2 * SH_KV * 4 * t + 4 * u >= nlp) break;        // (wave-uniform: both halves of these MFMAs lie beyond the lines)
                const float de[4] = {dv[u].x, dv[u].y, dv[u].z, dv[u].w}, qe[4] = {qv[u].x, qv[u].y, qv[u].z, qv[u].w};
                const float4 ur4 = xv[0][0][u], ui4 = xv[0][1][u], vr4 = xv[1][0][u], vi4 = xv[1][1][u];
                const float ur[4] = {ur4.x, ur4.y, ur4.z, ur4.w}, ui[4] = {ui4.x, ui4.y, ui4.z, ui4.w};
                const float vr[4] = {vr4.x, vr4.y, vr4.z, vr4.w}, vi[4] = {vi4.x, vi4.y, vi4.z, vi4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if constexpr (WZ) {
                        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(de[e], ur[e], acc[0][0], 0, 0, 0);
                        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(de[e], ui[e], acc[0][1], 0, 0, 0);
                    }
                    if constexpr (WD) {
                        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(qe[e], -ui[e], acc[1][0], 0, 0, 0);
                        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(qe[e], ur[e], acc[1][1], 0, 0, 0);
                    }
                    if constexpr (WZ) {
                        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(qe[e], -vi[e], acc[0][0], 0, 0, 0);
                        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(qe[e], vr[e], acc[0][1], 0, 0, 0);
                    }
                    if constexpr (WD) {
                        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(de[e], -vr[e], acc[1][0], 0, 0, 0);
                        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(de[e], -vi[e], acc[1][1], 0, 0, 0);
                    }
                }
            }
        }
        if (!f_ok) continue;
        const int64_t row0 = (int64_t)m * K - (int64_t)m * (m - 1) / 2 - m;       // row (m, n) = row0 + n
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int n = n0 + 8 * (i >> 2) + 4 * h + (i & 3);
            if (n < m || n > T) continue;
            const double r = response ? (double)response[n] : 1.0;
            if constexpr (WZ)
                vrt[fB * R + row0 + n] = isbad ? make_float2(nan, nan)
                                               : make_float2(sh_div_l_r(acc[0][0][i], Ld, r), sh_div_l_r(acc[0][1][i], Ld, r));
            if constexpr (WD)
                dvg[fB * R + row0 + n] = isbad ? make_float2(nan, nan)
                                               : make_float2(sh_div_l_r(acc[1][0][i], Ld, r), sh_div_l_r(acc[1][1][i], Ld, r));
        }
    }
    if (skipped && f_ok && nt == 0 && mc == 0 && h == 0) skipped[fB] = isbad ? 1 : 0;
}

// ---- the barotropic model's streaming kernels (dlwpcs_barotropic_flux, dlwpcs_barotropic_update) -------------------------------
// flux: (F, G) = ((f_i + zeta) u, (f_i + zeta) v) on dense (fields, nlat, L) fp32 grids, one Coriolis value per latitude.  A thread
// owns four neighbouring longitudes (VEC: 16-byte accesses, L % 4 == 0 so that they share a latitude) or one element.
template <bool VEC>
__global__ void __launch_bounds__(256) barotropic_flux_kernel(int64_t n, int32_t nlat, int32_t L, const float *__restrict__ coriolis,
                                                              const float *__restrict__ zeta, const float *__restrict__ u,
                                                              const float *__restrict__ v, float *__restrict__ F, float *__restrict__ Gv) {
#pragma clang fp contract(off)
    const int64_t t = flat_block() * 256 + threadIdx.x;
    const int64_t e = VEC ? 4 * t : t;
    if (e >= n) return;
    const float f = coriolis[(e / L) % nlat];
    if constexpr (VEC) {
        const float4 z = *reinterpret_cast<const float4 *>(zeta + e), a = *reinterpret_cast<const float4 *>(u + e),
                     b = *reinterpret_cast<const float4 *>(v + e);
        const float4 s = make_float4(f + z.x, f + z.y, f + z.z, f + z.w);
        *reinterpret_cast<float4 *>(F + e) = make_float4(s.x * a.x, s.y * a.y, s.z * a.z, s.w * a.w);
        *reinterpret_cast<float4 *>(Gv + e) = make_float4(s.x * b.x, s.y * b.y, s.z * b.z, s.w * b.w);
    } else {
        const float s = f + zeta[e];
        F[e] = s * u[e];
        Gv[e] = s * v[e];
    }
}

// update: one leapfrog step with implicit damping and the Robert filter on (fields, rows) complex fp32, in place:
//   t = (tend - d zeta_prev) / (1 + d dt),  d = damp[row]
//   first step:  new = zeta + dt t,  zeta' = zeta + rc (new - zeta)
//   afterwards:  z1 = zeta + rc (zeta_prev - 2 zeta),  new = zeta_prev + 2 dt t,  zeta' = z1 + rc new
//   zeta_prev <- zeta',  zeta <- new.
// Every operation is one fp32 rounding in the order written (no contraction); Re and Im alike.
__device__ __forceinline__ void baro_update1(float tend, float &z, float &zp, float d, float dt, float rc, bool first) {
#pragma clang fp contract(off)
    const float t = (tend - d * zp) / (1.f + d * dt);
    float nw, zf;
    if (first) {
        nw = z + dt * t;
        zf = z + rc * (nw - z);
    } else {
        const float z1 = z + rc * (zp - 2.f * z);
        nw = zp + (2.f * dt) * t;
        zf = z1 + rc * nw;
    }
    zp = zf;
    z = nw;
}

template <bool VEC>
__global__ void __launch_bounds__(256) barotropic_update_kernel(int64_t n, int64_t rows, const float *__restrict__ damp, float dt, float rc,
                                                                int first, const float *__restrict__ tend, float *__restrict__ zeta,
                                                                float *__restrict__ zeta_prev) {
    const int64_t t = flat_block() * 256 + threadIdx.x;     // n floats = 2 * fields * rows
    const int64_t e = VEC ? 4 * t : 2 * t;
    if (e >= n) return;
    if constexpr (VEC) {
        const float d0 = damp[(e / 2) % rows], d1 = damp[(e / 2 + 1) % rows];
        const float4 tn = *reinterpret_cast<const float4 *>(tend + e);
        float4 z = *reinterpret_cast<const float4 *>(zeta + e), zp = *reinterpret_cast<const float4 *>(zeta_prev + e);
        baro_update1(tn.x, z.x, zp.x, d0, dt, rc, first != 0);
        baro_update1(tn.y, z.y, zp.y, d0, dt, rc, first != 0);
        baro_update1(tn.z, z.z, zp.z, d1, dt, rc, first != 0);
        baro_update1(tn.w, z.w, zp.w, d1, dt, rc, first != 0);
        *reinterpret_cast<float4 *>(zeta + e) = z;
        *reinterpret_cast<float4 *>(zeta_prev + e) = zp;
    } else {
        const float d = damp[(e / 2) % rows];
        float zr = zeta[e], zi = zeta[e + 1], pr = zeta_prev[e], pi = zeta_prev[e + 1];
        baro_update1(tend[e], zr, pr, d, dt, rc, first != 0);
        baro_update1(tend[e + 1], zi, pi, d, dt, rc, first != 0);
        zeta[e] = zr; zeta[e + 1] = zi;
        zeta_prev[e] = pr; zeta_prev[e + 1] = pi;
    }
}

namespace {

struct ShPlan {
    ShGeom G;
    bool vec_ok;                                        // extents and strides allow 16-byte loads (the pointers decide the rest)
    size_t xs_bytes, bad_bytes;
};

int sh_plan(const dlwpcs_sht_spectrum_desc *d, bool pair, ShPlan &P, const char *who = "sht_spectrum") {
    if (!d) return fail(DLWPCS_E_INVALID, "%s: null descriptor", who);
    if (d->L < 2) return fail(DLWPCS_E_INVALID, "%s: L = %d (at least 2 longitudes)", who, d->L);
    if (d->L > SH_MAX_L) return fail(DLWPCS_E_UNSUPPORTED, "%s: L = %d, this build serves 2 <= L <= %d", who, d->L, SH_MAX_L);
    if (d->nlat < 2) return fail(DLWPCS_E_INVALID, "%s: nlat = %d (at least 2 latitudes)", who, d->nlat);
    if (d->nlat > DLWPCS_SHT_MAX_NLAT)
        return fail(DLWPCS_E_UNSUPPORTED, "%s: nlat = %d, this build serves 2 <= nlat <= %d", who, d->nlat, DLWPCS_SHT_MAX_NLAT);
    if (d->T < 0 || 2 * (int64_t)d->T + 1 > d->L)
        return fail(DLWPCS_E_INVALID, "%s: truncation T = %d needs 0 <= T and L >= 2 T + 1 = %lld longitudes, L = %d", who, d->T,
                    2 * (long long)d->T + 1, d->L);
    if (d->n_dims < 0 || d->n_dims > DLWPCS_SCORE_MAX_DIMS) return fail(DLWPCS_E_INVALID, "%s: n_dims %d out of range", who, d->n_dims);
    ShGeom &G = P.G;
    memset(&G, 0, sizeof(G));
    G.nlat = d->nlat;
    G.nlp = (d->nlat + 3) / 4 * 4;
    G.L = d->L;
    G.T = d->T;
    G.n_dims = d->n_dims;
    G.fields = 1;
    bool vec = d->L % 4 == 0;
    for (int op = 0; op < 2; ++op) {
        G.lat_stride[op] = d->lat_stride[op];
        if (op == 0 || pair) vec = vec && d->lat_stride[op] % 4 == 0;
    }
    for (int i = 0; i < d->n_dims; ++i) {
        const int64_t e = d->ext[i];
        if (e < 0 || e >= (1ll << 31)) return fail(DLWPCS_E_INVALID, "%s: extent %lld of dim %d", who, (long long)e, i);
        G.ext[i] = e;
        for (int op = 0; op < 2; ++op) {
            G.stride[op][i] = d->stride[op][i];
            if (op == 0 || pair) vec = vec && d->stride[op][i] % 4 == 0;
        }
        G.fields *= e;
        if (G.fields >= (1ll << 31)) return fail(DLWPCS_E_UNSUPPORTED, "%s: too many fields", who);
    }
    P.vec_ok = vec;
    G.rows = G.fields * G.nlat;
    G.n_rt = (G.rows + SH_ROWS - 1) / SH_ROWS;
    G.n_mt = (G.T + 1 + SH_MT - 1) / SH_MT;
    G.n_ft = (G.fields + SH_TILE - 1) / SH_TILE;
    G.n_nt = (G.T + 1 + SH_TILE - 1) / SH_TILE;
    G.op_stride = G.fields * (G.T + 1) * 2 * G.nlp;
    G.n_mc = (G.T + 1 + SH_MC - 1) / SH_MC;
    G.n_lt = (G.nlat + SH_TILE - 1) / SH_TILE;
    G.n_jt = (G.L + SH_JT - 1) / SH_JT;
    if (G.n_rt * G.n_mt > MAX_BLOCKS) return fail(DLWPCS_E_UNSUPPORTED, "%s: too many workgroups", who);
    P.xs_bytes = (size_t)G.op_stride * sizeof(float) * (pair ? 2 : 1);
    P.bad_bytes = (size_t)G.rows * sizeof(int32_t);
    return DLWPCS_OK;
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

// the pair form needs the larger scratch; the single form of the same descriptor never needs more
extern "C" size_t dlwpcs_sht_spectrum_scratch_bytes(const dlwpcs_sht_spectrum_desc *d) {
    ShPlan P;
    if (sh_plan(d, true, P) != DLWPCS_OK) return 0;
    return P.xs_bytes + P.bad_bytes;
}

extern "C" int dlwpcs_sht_spectrum(const dlwpcs_sht_spectrum_desc *d, const float *a, const float *b, const float *twiddle,
                                   const float *legendre, void *scratch, float *out, int32_t *skipped, dlwpcs_stream_t stream) {
    const bool pair = b != nullptr;
    ShPlan P;
    const int rc = sh_plan(d, pair, P);
    if (rc != DLWPCS_OK) return rc;
    const ShGeom &G = P.G;
    if (!twiddle || !legendre) return fail(DLWPCS_E_INVALID, "sht_spectrum: null twiddle or Legendre table");
    if (((uintptr_t)twiddle) & 7) return fail(DLWPCS_E_INVALID, "sht_spectrum: the twiddle table is not aligned to 8 bytes");
    if (((uintptr_t)legendre) & 15) return fail(DLWPCS_E_INVALID, "sht_spectrum: the Legendre table is not aligned to 16 bytes");
    if (G.fields == 0) return DLWPCS_OK;
    if (!out || !a) return fail(DLWPCS_E_INVALID, "sht_spectrum: null source or output");
    if ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)out) | ((uintptr_t)skipped)) & 3)
        return fail(DLWPCS_E_INVALID, "sht_spectrum: an operand is not aligned to its 4-byte elements");
    if (!scratch || (((uintptr_t)scratch) & 15))
        return fail(DLWPCS_E_INVALID, "sht_spectrum: this descriptor needs a 16-byte aligned scratch of %zu bytes", P.xs_bytes + P.bad_bytes);
    float *xs = (float *)scratch;
    int32_t *bad = (int32_t *)((char *)scratch + P.xs_bytes);
    const bool vec = P.vec_ok && !((((uintptr_t)a) | ((uintptr_t)b)) & 15);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid_a = launch_grid(G.n_rt * G.n_mt), grid_b = launch_grid(G.n_ft * G.n_nt);
    const float2 *tw = (const float2 *)twiddle;
#define SH_LAUNCH_A(PAIR, VEC) \
    hipLaunchKernelGGL((sht_fourier_kernel<PAIR, VEC>), grid_a, dim3(SH_THREADS), 0, s, G, a, b, tw, xs, bad)
    if (pair) { if (vec) SH_LAUNCH_A(true, true); else SH_LAUNCH_A(true, false); }
    else { if (vec) SH_LAUNCH_A(false, true); else SH_LAUNCH_A(false, false); }
#undef SH_LAUNCH_A
    if (pair) hipLaunchKernelGGL((sht_legendre_kernel<true>), grid_b, dim3(64), 0, s, G, xs, bad, legendre, out, skipped);
    else hipLaunchKernelGGL((sht_legendre_kernel<false>), grid_b, dim3(64), 0, s, G, xs, bad, legendre, out, skipped);
    return check_launch("sht_spectrum");
}

extern "C" size_t dlwpcs_sht_analysis_scratch_bytes(const dlwpcs_sht_spectrum_desc *d) {
    ShPlan P;
    if (sh_plan(d, false, P, "sht_analysis") != DLWPCS_OK) return 0;
    return P.xs_bytes + P.bad_bytes;
}

extern "C" int dlwpcs_sht_analysis(const dlwpcs_sht_spectrum_desc *d, const float *a, const float *twiddle, const float *legendre,
                                   void *scratch, float *coef, int32_t *skipped, dlwpcs_stream_t stream) {
    ShPlan P;
    const int rc = sh_plan(d, false, P, "sht_analysis");
    if (rc != DLWPCS_OK) return rc;
    const ShGeom &G = P.G;
    if (G.n_ft * G.n_nt * G.n_mc > MAX_BLOCKS) return fail(DLWPCS_E_UNSUPPORTED, "sht_analysis: too many workgroups");
    if (!twiddle || !legendre) return fail(DLWPCS_E_INVALID, "sht_analysis: null twiddle or Legendre table");
    if (((uintptr_t)twiddle) & 7) return fail(DLWPCS_E_INVALID, "sht_analysis: the twiddle table is not aligned to 8 bytes");
    if (((uintptr_t)legendre) & 15) return fail(DLWPCS_E_INVALID, "sht_analysis: the Legendre table is not aligned to 16 bytes");
    if (G.fields == 0) return DLWPCS_OK;
    if (!coef || !a) return fail(DLWPCS_E_INVALID, "sht_analysis: null source or output");
    if ((((uintptr_t)a) | ((uintptr_t)skipped)) & 3)
        return fail(DLWPCS_E_INVALID, "sht_analysis: an operand is not aligned to its 4-byte elements");
    if (((uintptr_t)coef) & 7) return fail(DLWPCS_E_INVALID, "sht_analysis: the coefficients are not aligned to their 8-byte pairs");
    if (!scratch || (((uintptr_t)scratch) & 15))
        return fail(DLWPCS_E_INVALID, "sht_analysis: this descriptor needs a 16-byte aligned scratch of %zu bytes", P.xs_bytes + P.bad_bytes);
    float *xs = (float *)scratch;
    int32_t *bad = (int32_t *)((char *)scratch + P.xs_bytes);
    const bool vec = P.vec_ok && !(((uintptr_t)a) & 15);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid_a = launch_grid(G.n_rt * G.n_mt), grid_b = launch_grid(G.n_ft * G.n_nt * G.n_mc);
    const float2 *tw = (const float2 *)twiddle;
    const float *none = nullptr;
    if (vec) hipLaunchKernelGGL((sht_fourier_kernel<false, true>), grid_a, dim3(SH_THREADS), 0, s, G, a, none, tw, xs, bad);
    else hipLaunchKernelGGL((sht_fourier_kernel<false, false>), grid_a, dim3(SH_THREADS), 0, s, G, a, none, tw, xs, bad);
    hipLaunchKernelGGL(sht_coef_kernel, grid_b, dim3(64), 0, s, G, xs, bad, legendre, (float2 *)coef, skipped);
    return check_launch("sht_analysis");
}

namespace {

int sh_synthesis_plan(const dlwpcs_sht_synthesis_desc *d, ShPlan &P) {
    if (!d) return fail(DLWPCS_E_INVALID, "sht_synthesis: null descriptor");
    if (d->n_dims < 0 || d->n_dims > DLWPCS_SCORE_MAX_DIMS) return fail(DLWPCS_E_INVALID, "sht_synthesis: n_dims %d out of range", d->n_dims);
    dlwpcs_sht_spectrum_desc sd;
    memset(&sd, 0, sizeof(sd));
    sd.nlat = d->nlat;
    sd.L = d->L;
    sd.T = d->T;
    sd.n_dims = d->n_dims;
    sd.lat_stride[0] = d->lat_stride;
    for (int i = 0; i < d->n_dims; ++i) {
        sd.ext[i] = d->ext[i];
        sd.stride[0][i] = d->stride[i];
    }
    const int rc = sh_plan(&sd, false, P, "sht_synthesis");
    if (rc != DLWPCS_OK) return rc;
    const ShGeom &G = P.G;
    if (G.n_ft * G.n_lt * (G.T + 1) > MAX_BLOCKS || G.n_rt * G.n_jt > MAX_BLOCKS)
        return fail(DLWPCS_E_UNSUPPORTED, "sht_synthesis: too many workgroups");
    return DLWPCS_OK;
}

}  // namespace

// gs alone: [field][m][re | im][nlat_pad] fp32
extern "C" size_t dlwpcs_sht_synthesis_scratch_bytes(const dlwpcs_sht_synthesis_desc *d) {
    ShPlan P;
    if (sh_synthesis_plan(d, P) != DLWPCS_OK) return 0;
    return P.xs_bytes;
}

extern "C" int dlwpcs_sht_synthesis(const dlwpcs_sht_synthesis_desc *d, const float *coef, const float *response, const float *twiddle,
                                    const float *legendre, void *scratch, float *out, dlwpcs_stream_t stream) {
    ShPlan P;
    const int rc = sh_synthesis_plan(d, P);
    if (rc != DLWPCS_OK) return rc;
    const ShGeom &G = P.G;
    if (!twiddle || !legendre) return fail(DLWPCS_E_INVALID, "sht_synthesis: null twiddle or Legendre table");
    if (((uintptr_t)twiddle) & 7) return fail(DLWPCS_E_INVALID, "sht_synthesis: the twiddle table is not aligned to 8 bytes");
    if (((uintptr_t)legendre) & 15) return fail(DLWPCS_E_INVALID, "sht_synthesis: the Legendre table is not aligned to 16 bytes");
    if (G.fields == 0) return DLWPCS_OK;
    if (!coef || !out) return fail(DLWPCS_E_INVALID, "sht_synthesis: null coefficients or output");
    if ((((uintptr_t)out) | ((uintptr_t)response)) & 3)
        return fail(DLWPCS_E_INVALID, "sht_synthesis: an operand is not aligned to its 4-byte elements");
    if (((uintptr_t)coef) & 7) return fail(DLWPCS_E_INVALID, "sht_synthesis: the coefficients are not aligned to their 8-byte pairs");
    if (!scratch || (((uintptr_t)scratch) & 15))
        return fail(DLWPCS_E_INVALID, "sht_synthesis: this descriptor needs a 16-byte aligned scratch of %zu bytes", P.xs_bytes);
    float *gs = (float *)scratch;
    const bool vec = P.vec_ok && !(((uintptr_t)out) & 15);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid_l = launch_grid(G.n_ft * G.n_lt * (G.T + 1)), grid_f = launch_grid(G.n_rt * G.n_jt);
    const float2 *tw = (const float2 *)twiddle;
    hipLaunchKernelGGL(sht_ilegendre_kernel, grid_l, dim3(64), 0, s, G, (const float2 *)coef, response, legendre, gs);
    if (vec) hipLaunchKernelGGL((sht_ifourier_kernel<true>), grid_f, dim3(SH_THREADS), 0, s, G, (const float *)gs, tw, out);
    else hipLaunchKernelGGL((sht_ifourier_kernel<false>), grid_f, dim3(SH_THREADS), 0, s, G, (const float *)gs, tw, out);
    return check_launch("sht_synthesis");
}

// gs for u and for v: the pair form's scratch without the row flags
extern "C" size_t dlwpcs_sht_vector_synthesis_scratch_bytes(const dlwpcs_sht_spectrum_desc *d) {
    ShPlan P;
    if (sh_plan(d, true, P, "sht_vector_synthesis") != DLWPCS_OK) return 0;
    return P.xs_bytes;
}

extern "C" int dlwpcs_sht_vector_synthesis(const dlwpcs_sht_spectrum_desc *d, const float *coef_a, const float *coef_b, const float *rpsi,
                                           const float *rchi, const float *twiddle, const float *dtable, const float *qtable,
                                           void *scratch, float *out_u, float *out_v, dlwpcs_stream_t stream) {
    const char *who = "sht_vector_synthesis";
    ShPlan P;
    const int rc = sh_plan(d, true, P, who);
    if (rc != DLWPCS_OK) return rc;
    const ShGeom &G = P.G;
    if (G.n_ft * G.n_lt * (G.T + 1) > MAX_BLOCKS || G.n_rt * G.n_jt > MAX_BLOCKS)
        return fail(DLWPCS_E_UNSUPPORTED, "%s: too many workgroups", who);
    if (!twiddle || !dtable || !qtable) return fail(DLWPCS_E_INVALID, "%s: null twiddle, derivative or zonal table", who);
    if (((uintptr_t)twiddle) & 7) return fail(DLWPCS_E_INVALID, "%s: the twiddle table is not aligned to 8 bytes", who);
    if ((((uintptr_t)dtable) | ((uintptr_t)qtable)) & 15) return fail(DLWPCS_E_INVALID, "%s: a table is not aligned to 16 bytes", who);
    if (!coef_a && !coef_b) return fail(DLWPCS_E_INVALID, "%s: both potentials are absent", who);
    if (G.fields == 0) return DLWPCS_OK;
    if (!out_u || !out_v) return fail(DLWPCS_E_INVALID, "%s: null output", who);
    if ((((uintptr_t)out_u) | ((uintptr_t)out_v) | ((uintptr_t)rpsi) | ((uintptr_t)rchi)) & 3)
        return fail(DLWPCS_E_INVALID, "%s: an operand is not aligned to its 4-byte elements", who);
    if ((((uintptr_t)coef_a) | ((uintptr_t)coef_b)) & 7)
        return fail(DLWPCS_E_INVALID, "%s: the coefficients are not aligned to their 8-byte pairs", who);
    if (!scratch || (((uintptr_t)scratch) & 15))
        return fail(DLWPCS_E_INVALID, "%s: this descriptor needs a 16-byte aligned scratch of %zu bytes", who, P.xs_bytes);
    float *gs = (float *)scratch;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid_l = launch_grid(G.n_ft * G.n_lt * (G.T + 1)), grid_f = launch_grid(G.n_rt * G.n_jt);
    const float2 *tw = (const float2 *)twiddle, *ca = (const float2 *)coef_a, *cb = (const float2 *)coef_b;
    if (ca && cb) hipLaunchKernelGGL((sht_vilegendre_kernel<true, true>), grid_l, dim3(64), 0, s, G, ca, cb, rpsi, rchi, dtable, qtable, gs);
    else if (ca) hipLaunchKernelGGL((sht_vilegendre_kernel<true, false>), grid_l, dim3(64), 0, s, G, ca, cb, rpsi, rchi, dtable, qtable, gs);
    else hipLaunchKernelGGL((sht_vilegendre_kernel<false, true>), grid_l, dim3(64), 0, s, G, ca, cb, rpsi, rchi, dtable, qtable, gs);
    for (int c = 0; c < 2; ++c) {
        ShGeom Gc = G;                                  // the inverse Fourier stage reads operand 0's strides
        Gc.lat_stride[0] = G.lat_stride[c];
        for (int i = 0; i < G.n_dims; ++i) Gc.stride[0][i] = G.stride[c][i];
        float *out = c == 0 ? out_u : out_v;
        const float *gc = gs + c * G.op_stride;
        bool vec = G.L % 4 == 0 && Gc.lat_stride[0] % 4 == 0 && !(((uintptr_t)out) & 15);
        for (int i = 0; i < G.n_dims; ++i) vec = vec && Gc.stride[0][i] % 4 == 0;
        if (vec) hipLaunchKernelGGL((sht_ifourier_kernel<true>), grid_f, dim3(SH_THREADS), 0, s, Gc, gc, tw, out);
        else hipLaunchKernelGGL((sht_ifourier_kernel<false>), grid_f, dim3(SH_THREADS), 0, s, Gc, gc, tw, out);
    }
    return check_launch(who);
}

extern "C" size_t dlwpcs_sht_vector_analysis_scratch_bytes(const dlwpcs_sht_spectrum_desc *d) {
    ShPlan P;
    if (sh_plan(d, true, P, "sht_vector_analysis") != DLWPCS_OK) return 0;
    return P.xs_bytes + P.bad_bytes;
}

extern "C" int dlwpcs_sht_vector_analysis(const dlwpcs_sht_spectrum_desc *d, const float *u, const float *v, const float *response,
                                          const float *twiddle, const float *wdtable, const float *wqtable, void *scratch, float *vrt,
                                          float *div, int32_t *skipped, dlwpcs_stream_t stream) {
    const char *who = "sht_vector_analysis";
    ShPlan P;
    const int rc = sh_plan(d, true, P, who);
    if (rc != DLWPCS_OK) return rc;
    const ShGeom &G = P.G;
    if (G.n_ft * G.n_nt * G.n_mc > MAX_BLOCKS) return fail(DLWPCS_E_UNSUPPORTED, "%s: too many workgroups", who);
    if (!twiddle || !wdtable || !wqtable) return fail(DLWPCS_E_INVALID, "%s: null twiddle, derivative or zonal table", who);
    if (((uintptr_t)twiddle) & 7) return fail(DLWPCS_E_INVALID, "%s: the twiddle table is not aligned to 8 bytes", who);
    if ((((uintptr_t)wdtable) | ((uintptr_t)wqtable)) & 15) return fail(DLWPCS_E_INVALID, "%s: a table is not aligned to 16 bytes", who);
    if (!vrt && !div) return fail(DLWPCS_E_INVALID, "%s: both outputs are absent", who);
    if (G.fields == 0) return DLWPCS_OK;
    if (!u || !v) return fail(DLWPCS_E_INVALID, "%s: null wind component", who);
    if ((((uintptr_t)u) | ((uintptr_t)v) | ((uintptr_t)response) | ((uintptr_t)skipped)) & 3)
        return fail(DLWPCS_E_INVALID, "%s: an operand is not aligned to its 4-byte elements", who);
    if ((((uintptr_t)vrt) | ((uintptr_t)div)) & 7)
        return fail(DLWPCS_E_INVALID, "%s: the coefficients are not aligned to their 8-byte pairs", who);
    if (!scratch || (((uintptr_t)scratch) & 15))
        return fail(DLWPCS_E_INVALID, "%s: this descriptor needs a 16-byte aligned scratch of %zu bytes", who, P.xs_bytes + P.bad_bytes);
    float *xs = (float *)scratch;
    int32_t *bad = (int32_t *)((char *)scratch + P.xs_bytes);
    const bool vec = P.vec_ok && !((((uintptr_t)u) | ((uintptr_t)v)) & 15);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid_a = launch_grid(G.n_rt * G.n_mt), grid_b = launch_grid(G.n_ft * G.n_nt * G.n_mc);
    const float2 *tw = (const float2 *)twiddle;
    if (vec) hipLaunchKernelGGL((sht_fourier_kernel<true, true>), grid_a, dim3(SH_THREADS), 0, s, G, u, v, tw, xs, bad);
    else hipLaunchKernelGGL((sht_fourier_kernel<true, false>), grid_a, dim3(SH_THREADS), 0, s, G, u, v, tw, xs, bad);
    float2 *z = (float2 *)vrt, *dv = (float2 *)div;
    const int32_t *cbad = bad;
    const float *cxs = xs;
    if (z && dv) hipLaunchKernelGGL((sht_vcoef_kernel<true, true>), grid_b, dim3(64), 0, s, G, cxs, cbad, response, wdtable, wqtable, z, dv, skipped);
    else if (z) hipLaunchKernelGGL((sht_vcoef_kernel<true, false>), grid_b, dim3(64), 0, s, G, cxs, cbad, response, wdtable, wqtable, z, dv, skipped);
    else hipLaunchKernelGGL((sht_vcoef_kernel<false, true>), grid_b, dim3(64), 0, s, G, cxs, cbad, response, wdtable, wqtable, z, dv, skipped);
    return check_launch(who);
}

extern "C" int dlwpcs_barotropic_flux(int64_t fields, int32_t nlat, int32_t L, const float *coriolis, const float *zeta, const float *u,
                                      const float *v, float *F, float *G, dlwpcs_stream_t stream) {
    if (fields < 0 || nlat < 1 || L < 1) return fail(DLWPCS_E_INVALID, "barotropic_flux: fields = %lld, nlat = %d, L = %d", (long long)fields, nlat, L);
    if (fields >= (1ll << 31) / nlat) return fail(DLWPCS_E_UNSUPPORTED, "barotropic_flux: too many fields");     // (n below fits int64)
    if (fields == 0) return DLWPCS_OK;
    if (!coriolis || !zeta || !u || !v || !F || !G) return fail(DLWPCS_E_INVALID, "barotropic_flux: null operand");
    const uintptr_t all = ((uintptr_t)coriolis) | ((uintptr_t)zeta) | ((uintptr_t)u) | ((uintptr_t)v) | ((uintptr_t)F) | ((uintptr_t)G);
    if (all & 3) return fail(DLWPCS_E_INVALID, "barotropic_flux: an operand is not aligned to its 4-byte elements");
    const int64_t n = fields * nlat * L;
    const bool vec = L % 4 == 0 && !((((uintptr_t)zeta) | ((uintptr_t)u) | ((uintptr_t)v) | ((uintptr_t)F) | ((uintptr_t)G)) & 15);
    hipStream_t s = (hipStream_t)stream;
    const int64_t threads = vec ? n / 4 : n;
    if ((threads + 255) / 256 > MAX_BLOCKS) return fail(DLWPCS_E_UNSUPPORTED, "barotropic_flux: too many workgroups");
    const dim3 grid = launch_grid((threads + 255) / 256);
    if (vec) hipLaunchKernelGGL((barotropic_flux_kernel<true>), grid, dim3(256), 0, s, n, nlat, L, coriolis, zeta, u, v, F, G);
    else hipLaunchKernelGGL((barotropic_flux_kernel<false>), grid, dim3(256), 0, s, n, nlat, L, coriolis, zeta, u, v, F, G);
    return check_launch("barotropic_flux");
}

extern "C" int dlwpcs_barotropic_update(int64_t fields, int64_t rows, const float *damp, float dt, float robert, int32_t first_step,
                                        const float *tend, float *zeta, float *zeta_prev, dlwpcs_stream_t stream) {
    if (fields < 0 || rows < 1) return fail(DLWPCS_E_INVALID, "barotropic_update: fields = %lld, rows = %lld", (long long)fields, (long long)rows);
    if (rows >= (1ll << 31) || fields >= (1ll << 31)) return fail(DLWPCS_E_UNSUPPORTED, "barotropic_update: too many coefficients");
    if (!(dt == dt) || !(robert == robert)) return fail(DLWPCS_E_INVALID, "barotropic_update: dt or the Robert coefficient is NaN");
    if (fields == 0) return DLWPCS_OK;
    if (!damp || !tend || !zeta || !zeta_prev) return fail(DLWPCS_E_INVALID, "barotropic_update: null operand");
    if (zeta == zeta_prev) return fail(DLWPCS_E_INVALID, "barotropic_update: zeta and zeta_prev are one buffer");
    if (tend == zeta || tend == zeta_prev) return fail(DLWPCS_E_INVALID, "barotropic_update: tend and a state are one buffer");
    if (((uintptr_t)damp) & 3) return fail(DLWPCS_E_INVALID, "barotropic_update: the damping table is not aligned to its 4-byte elements");
    const uintptr_t all = ((uintptr_t)tend) | ((uintptr_t)zeta) | ((uintptr_t)zeta_prev);
    if (all & 7) return fail(DLWPCS_E_INVALID, "barotropic_update: the coefficients are not aligned to their 8-byte pairs");
    const int64_t n = 2 * fields * rows;
    const bool vec = n % 4 == 0 && !(all & 15);
    hipStream_t s = (hipStream_t)stream;
    const int64_t threads = vec ? n / 4 : n / 2;                       // (n < 2^63: both factors are below 2^31)
    if ((threads + 255) / 256 > MAX_BLOCKS) return fail(DLWPCS_E_UNSUPPORTED, "barotropic_update: too many workgroups");
    const dim3 grid = launch_grid((threads + 255) / 256);
    if (vec) hipLaunchKernelGGL((barotropic_update_kernel<true>), grid, dim3(256), 0, s, n, rows, damp, dt, robert, (int)first_step, tend, zeta, zeta_prev);
    else hipLaunchKernelGGL((barotropic_update_kernel<false>), grid, dim3(256), 0, s, n, rows, damp, dt, robert, (int)first_step, tend, zeta, zeta_prev);
    return check_launch("barotropic_update");
}
