// Zonal power spectra and cross-spectra (dlwpcs_zonal_spectrum): for every row x[0..L-1] along longitude the one-sided DFT power
//   P_k = c_k |X_k|^2 / L^2,  X_k = sum_j x_j exp(-2 pi i jk / L),  c_k = 1 for k = 0 and k = L/2 (L even), else 2,
// averaged with per-row weights over the rows of a group (the kept leading dims index the groups, the averaged ones the rows of a
// group): sum w P_k / sum w over the rows that count -- rows whose L values are all finite (pair form: in both operands).
//
// The transform is the matrix product (rows x L) . (L x 2K) on v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered fmaf chain).  A
// workgroup of four waves owns a tile of 32 row slots and 128 wavenumbers; wave v forms the cosine tile and the sine tile of
// its 32 wavenumbers with the SAME column mapping, so Re and Im of a wavenumber meet in one lane.  The rows come through LDS in
// chunks of 64 longitudes (registers prefetch the next chunk while the matrix cores work on this one); the twiddles come from a
// length-L table {cos, -sin}(2 pi m / L) held in LDS and are looked up at the reduced index m = (j k) mod L, which every lane
// carries along incrementally in integers -- no fp32 angle is ever formed.
//
// Row slots.  A group of more than 16 rows has its workgroups to itself: its rows fill tile after tile (32 slots each).  Groups
// of 1..16 rows are packed floor(32 / rows) to a tile.  Either way one lane owns a (group, wavenumber, quantity) and adds the
// rows' terms ONE BY ONE, IN ROW ORDER, in fp64: term = fp32 product (Re^2 + Im^2, ...) * c_k / L^2 * weight.  A row that does not
// count adds nothing, so within one slab the sum is bitwise the sum over the same rows with the missing ones taken out.  Few
// groups of very many rows are cut into slabs of whole tiles so that the device fills: launch 1 then writes one fp64 partial per
// (slab, group, quantity, k) and launch 2 adds the slabs in order and divides.  No atomics; two runs give the same bits.
//
// remove_mean: a first pass over the tile's rows sums each row in fp64 (lane j mod 64, then a fixed butterfly), the mean rounded
// to fp32 is subtracted as the row is staged, and k = 0 reports the fp64 mean squared (pair: the products of the two means).
#include "mfma_common.h"
#include "strided.h"

namespace dlwpcs {

constexpr int ZS_THREADS = 256;
constexpr int ZS_ROWS = 32;                 // row slots of a tile (the M of the MFMA)
constexpr int ZS_JC = 64;                   // longitudes per staged chunk
constexpr int ZS_XS = ZS_JC + 2;            // LDS row stride (floats): 8-byte reads of 32 rows x 2 halves hit 64 distinct banks
constexpr int ZS_KW = 32;                   // wavenumbers per wave
constexpr int ZS_KT = 4 * ZS_KW;            // wavenumbers per workgroup
constexpr int ZS_MAX_L = 1728;              // the twiddle table {cos, -sin} of 2 L floats lives in static LDS
constexpr int ZS_PACK_ROWS = 16;            // groups of up to this many rows share a tile
constexpr int64_t ZS_SLAB_MIN_ROWS = 256;   // a slab holds at least this many rows
constexpr int64_t ZS_FILL_BLOCKS = 2048;    // slabs are made only while the launch has fewer workgroups than this (256 CUs x 8)
constexpr int64_t ZS_SLOTS = 512;           // workgroups resident at a time: 256 compute units x 2 (by LDS); placement only
constexpr int64_t ZS_MAX_SLABS = 64;

struct ZsGeom {
    int32_t L, K, remove_mean, n_keep, n_avg;
    int32_t rpt, gpt;                        // rows of a group per tile, groups per tile
    int32_t n_kt, slabs;
    int64_t groups, rpg;                     // groups, rows per group
    int64_t n_gt;                            // group tiles: workgroups along the groups
    int64_t n_tiles;                         // (one group per workgroup) tiles of the group
    int64_t nblk;
    int64_t keep_ext[DLWPCS_SCORE_MAX_DIMS], avg_ext[DLWPCS_SCORE_MAX_DIMS];
    int64_t keep_stride[3][DLWPCS_SCORE_MAX_DIMS], avg_stride[3][DLWPCS_SCORE_MAX_DIMS];
};

// the four fp32 products of the pair form (q = 0 alone in the single form), spelled once so that every instantiation rounds alike
__device__ __forceinline__ float zs_product(int q, float cf, float sf, float cv, float sv) {
#pragma clang fp contract(off)
    if (q == 0) return __builtin_fmaf(sf, sf, cf * cf);
    if (q == 1) return __builtin_fmaf(sv, sv, cv * cv);
    if (q == 2) return __builtin_fmaf(sf, sv, cf * cv);                 // Re(F conj V)
    return __builtin_fmaf(sf, cv, -(cf * sv));                          // Im(F conj V)
}
__device__ __forceinline__ double zs_term(double v, double scale, double w) {
#pragma clang fp contract(off)
    return (v * scale) * w;
}

template <bool PAIR, bool VEC>
__global__ void __launch_bounds__(ZS_THREADS) zonal_spectrum_kernel(ZsGeom G, const float *__restrict__ a, const float *__restrict__ b,
                                                                    const float *__restrict__ wts, const float2 *__restrict__ twiddle,
                                                                    double *__restrict__ partial, double *__restrict__ part_w,
                                                                    int32_t *__restrict__ part_skip, float *__restrict__ out,
                                                                    int32_t *__restrict__ skipped) {
    constexpr int NOP = PAIR ? 2 : 1;
    constexpr int NQ = PAIR ? 4 : 1;
    constexpr int NROUND = PAIR ? 2 : 1;
    constexpr int NLD = VEC ? 2 : 8;                    // loads of a thread per chunk and operand
    __shared__ float2 s_tw[ZS_MAX_L];
    __shared__ __attribute__((aligned(16))) float s_x[NOP][ZS_ROWS * ZS_XS];
    __shared__ float s_ex[4][2][ZS_ROWS * ZS_KW];       // per wave: two quantities of its 32 x 32 tile
    __shared__ int64_t s_off[NOP][ZS_ROWS];
    __shared__ int64_t s_grp[ZS_ROWS];
    __shared__ double s_mean[NOP][ZS_ROWS];
    __shared__ float s_w[ZS_ROWS];
    __shared__ int s_valid[ZS_ROWS], s_bad[ZS_ROWS];

    const int64_t bid = flat_block();
    if (bid >= G.nblk) return;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int kt = (int)(bid % G.n_kt);
    const int64_t rest = bid / G.n_kt;
    const int slab = (int)(rest % G.slabs);
    const int64_t gt = rest / G.slabs;
    const int L = G.L, K = G.K;
    const bool packed = G.gpt > 1;

    for (int m = tid; m < L; m += ZS_THREADS) s_tw[m] = twiddle[m];

    const int r32 = lane & 31, h = lane >> 5;
    const int kw = kt * ZS_KT + wv * ZS_KW + r32;       // this lane's wavenumber (the column of both of its tiles)
    const bool wave_on = kt * ZS_KT + wv * ZS_KW < K;
    const int step4 = (int)((4ll * kw) % L);
    const double scale = ((kw == 0 || 2 * kw == L) ? 1.0 : 2.0) / ((double)L * (double)L);

    int64_t t0 = 0, t1 = 1;
    if (!packed) {
        t0 = G.n_tiles * slab / G.slabs;                // slabs of whole tiles whose sizes differ by at most one tile
        t1 = G.n_tiles * (slab + 1) / G.slabs;
    }
    double run[NROUND], run_w = 0.0;                    // one group per workgroup: the sums carried from tile to tile
    int run_skip = 0;
#pragma unroll
    for (int r = 0; r < NROUND; ++r) run[r] = 0.0;

    // staging: the slot and column of this thread's loads are the same in every chunk
    int ld_row[NLD], ld_col[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int idx = tid + i * ZS_THREADS;
        ld_row[i] = VEC ? idx >> 4 : idx >> 6;
        ld_col[i] = VEC ? (idx & 15) * 4 : idx & 63;
    }
    const int n_chunks = (L + ZS_JC - 1) / ZS_JC;

    for (int64_t tile = t0; tile < t1; ++tile) {
        __syncthreads();                                // the previous tile's epilogue has read the slot tables
        if (tid < ZS_ROWS) {
            const int gi = tid / G.rpt;
            const int64_t g = packed ? gt * G.gpt + gi : gt;
            const int64_t r = packed ? tid - gi * G.rpt : tile * ZS_ROWS + tid;
            const bool valid = gi < G.gpt && g < G.groups && r < G.rpg;
            int64_t off[3] = {0, 0, 0};
            if (valid) {
                int64_t q = g;
                for (int d = G.n_keep - 1; d >= 0; --d) {
                    const int64_t e = G.keep_ext[d], c = q % e;
                    q /= e;
#pragma unroll
                    for (int op = 0; op < 3; ++op) off[op] += c * G.keep_stride[op][d];
                }
                q = r;
                for (int d = G.n_avg - 1; d >= 0; --d) {
                    const int64_t e = G.avg_ext[d], c = q % e;
                    q /= e;
#pragma unroll
                    for (int op = 0; op < 3; ++op) off[op] += c * G.avg_stride[op][d];
                }
            }
            s_off[0][tid] = off[0];
            if (PAIR) s_off[NOP - 1][tid] = off[1];
            s_grp[tid] = g;
            s_w[tid] = valid ? (wts ? wts[off[2]] : 1.f) : 0.f;
            s_valid[tid] = valid;
            s_bad[tid] = 0;
        }
        __syncthreads();
        if (G.remove_mean) {                            // wave wv: slots 8 wv .. 8 wv + 7
            for (int s = wv * 8; s < wv * 8 + 8; ++s) {
#pragma unroll
                for (int op = 0; op < NOP; ++op) {
                    double sum = 0.0;
                    if (s_valid[s]) {
                        const float *p = (op == 0 ? a : b) + s_off[op][s];
                        for (int j = lane; j < L; j += 64) sum += (double)p[j];
                    }
#pragma unroll
                    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
                    if (lane == 0) s_mean[op][s] = sum / (double)L;
                }
            }
            __syncthreads();
        }
        int64_t ld_off[NOP][NLD];
        float ld_mu[NOP][NLD];
        bool ld_ok[NLD];
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            ld_ok[i] = s_valid[ld_row[i]] != 0;
#pragma unroll
            for (int op = 0; op < NOP; ++op) {
                ld_off[op][i] = s_off[op][ld_row[i]];
                ld_mu[op][i] = (G.remove_mean && ld_ok[i]) ? (float)s_mean[op][ld_row[i]] : 0.f;
            }
        }
        unsigned bad_mask = 0;

        float regs[NOP][NLD][VEC ? 4 : 1];
        auto fetch = [&](int chunk) {
            const int j0 = chunk * ZS_JC;
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
        auto stash = [&](int chunk) {
            const int j0 = chunk * ZS_JC;
#pragma unroll
            for (int op = 0; op < NOP; ++op)
#pragma unroll
                for (int i = 0; i < NLD; ++i) {
                    const bool in = ld_ok[i] && j0 + ld_col[i] < L;
                    float v[VEC ? 4 : 1];
#pragma unroll
                    for (int e = 0; e < (VEC ? 4 : 1); ++e) {
                        const float x = regs[op][i][e];
                        if (nonfinite(x)) bad_mask |= 1u << i;
                        v[e] = in ? x - ld_mu[op][i] : 0.f;
                    }
                    float *dst = &s_x[op][ld_row[i] * ZS_XS + ld_col[i]];
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
            __syncthreads();                            // the previous chunk has been consumed
            stash(chunk);
            if (chunk + 1 == n_chunks) {
#pragma unroll
                for (int i = 0; i < NLD; ++i)
                    if (bad_mask & (1u << i)) s_bad[ld_row[i]] = 1;
            }
            __syncthreads();
            if (chunk + 1 < n_chunks) fetch(chunk + 1);
            if (wave_on) {
                const int left = L - chunk * ZS_JC;
                const int nt = left >= ZS_JC ? ZS_JC / 4 : (left + 3) / 4;
                for (int t = 0; t < nt; ++t) {
                    const float2 tw0 = s_tw[m0], tw1 = s_tw[m1];
                    float2 xv[NOP];
#pragma unroll
                    for (int op = 0; op < NOP; ++op)
                        xv[op] = *reinterpret_cast<const float2 *>(&s_x[op][r32 * ZS_XS + 4 * t + 2 * h]);
#pragma unroll
                    for (int op = 0; op < NOP; ++op) {
                        acc[op][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[op].x, tw0.x, acc[op][0], 0, 0, 0);
                        acc[op][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[op].x, tw0.y, acc[op][1], 0, 0, 0);
                    }
#pragma unroll
                    for (int op = 0; op < NOP; ++op) {
                        acc[op][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[op].y, tw1.x, acc[op][0], 0, 0, 0);
                        acc[op][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[op].y, tw1.y, acc[op][1], 0, 0, 0);
                    }
                    m0 += step4; m0 -= m0 >= L ? L : 0;
                    m1 += step4; m1 -= m1 >= L ? L : 0;
                }
            }
        }

        // epilogue: per round two quantities go through the wave's own LDS tile; lane (column r32, half h) then owns quantity
        // 2 round + h of wavenumber kw and adds its rows in slot order
        if (wave_on) {
#pragma unroll
            for (int round = 0; round < NROUND; ++round) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = 8 * (i >> 2) + 4 * h + (i & 3);
                    const float cf = acc[0][0][i], sf = acc[0][1][i], cv = acc[NOP - 1][0][i], sv = acc[NOP - 1][1][i];
                    s_ex[wv][0][row * ZS_KW + r32] = zs_product(2 * round, cf, sf, cv, sv);
                    if (PAIR) s_ex[wv][1][row * ZS_KW + r32] = zs_product(2 * round + 1, cf, sf, cv, sv);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const int q = 2 * round + h;
                const bool q_on = PAIR || h == 0;
                for (int gi = 0; gi < G.gpt; ++gi) {
                    double sum = packed ? 0.0 : run[round], sum_w = packed ? 0.0 : run_w;
                    int skip = packed ? 0 : run_skip;
                    const int s0 = gi * G.rpt;
                    if (!s_valid[s0]) break;            // (slots are valid from the front)
                    for (int s = s0; s < s0 + G.rpt; ++s) {
                        if (!s_valid[s]) break;
                        if (s_bad[s]) { ++skip; continue; }
                        const double w = (double)s_w[s];
                        sum_w += w;
                        if (!q_on) continue;
                        if (G.remove_mean && kw == 0) {
                            const double mf = s_mean[0][s], mv = s_mean[NOP - 1][s];
                            const double v = q == 0 ? mf * mf : q == 1 ? mv * mv : q == 2 ? mf * mv : 0.0;
                            sum += zs_term(v, 1.0, w);
                        } else {
                            sum += zs_term((double)s_ex[wv][h][s * ZS_KW + r32], scale, w);
                        }
                    }
                    if (!packed) {
                        run[round] = sum;
                        if (round == NROUND - 1) { run_w = sum_w; run_skip = skip; }
                    } else {
                        const int64_t g = s_grp[s0];
                        if (q_on && kw < K)
                            out[((int64_t)q * G.groups + g) * K + kw] =
                                sum_w == 0.0 ? __uint_as_float(0x7fc00000u) : (float)(sum / sum_w);
                        if (skipped && round == 0 && kt == 0 && tid == 0) skipped[g] = skip;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();        // the next round overwrites the tile
            }
        }
    }

    if (!packed && wave_on) {
        const int64_t g = gt;
#pragma unroll
        for (int round = 0; round < NROUND; ++round) {
            const int q = 2 * round + h;
            if ((PAIR || h == 0) && kw < K) {
                if (G.slabs == 1)
                    out[((int64_t)q * G.groups + g) * K + kw] =
                        run_w == 0.0 ? __uint_as_float(0x7fc00000u) : (float)(run[round] / run_w);
                else
                    partial[(((int64_t)slab * G.groups + g) * NQ + q) * K + kw] = run[round];
            }
        }
        if (kt == 0 && tid == 0) {
            if (G.slabs == 1) {
                if (skipped) skipped[g] = run_skip;
            } else {
                part_w[(int64_t)slab * G.groups + g] = run_w;
                part_skip[(int64_t)slab * G.groups + g] = run_skip;
            }
        }
    }
}

// launch 2 (slabs > 1): the slab partials added in slab order, divided by the summed weights
__global__ void __launch_bounds__(256) zonal_spectrum_finish_kernel(const double *__restrict__ partial, const double *__restrict__ part_w,
                                                                    const int32_t *__restrict__ part_skip, int64_t groups, int K,
                                                                    int nq, int slabs, float *__restrict__ out,
                                                                    int32_t *__restrict__ skipped) {
    const int64_t i = flat_block() * 256 + threadIdx.x;
    if (i >= (int64_t)nq * groups * K) return;
    const int k = (int)(i % K);
    const int64_t g = (i / K) % groups;
    const int q = (int)(i / ((int64_t)K * groups));
    double sum = 0.0, sum_w = 0.0;
    int skip = 0;
    for (int s = 0; s < slabs; ++s) {
        sum += partial[(((int64_t)s * groups + g) * nq + q) * K + k];
        sum_w += part_w[(int64_t)s * groups + g];
        skip += part_skip[(int64_t)s * groups + g];
    }
    out[i] = sum_w == 0.0 ? __uint_as_float(0x7fc00000u) : (float)(sum / sum_w);
    if (skipped && q == 0 && k == 0) skipped[g] = skip;
}

namespace {

struct ZsPlan {
    ZsGeom G;
    bool vec_ok;                                        // extents and strides allow 16-byte loads (the pointers decide the rest)
    size_t partial_bytes, w_bytes, skip_bytes;
};

int zs_plan(const dlwpcs_zonal_spectrum_desc *d, bool pair, ZsPlan &P) {
    if (!d) return fail(DLWPCS_E_INVALID, "zonal_spectrum: null descriptor");
    if (d->L < 2) return fail(DLWPCS_E_INVALID, "zonal_spectrum: L = %d (at least 2 longitudes)", d->L);
    if (d->L > ZS_MAX_L)
        return fail(DLWPCS_E_UNSUPPORTED, "zonal_spectrum: L = %d, this build serves 2 <= L <= %d", d->L, ZS_MAX_L);
    if (d->n_wave < 0 || d->n_wave > d->L / 2 + 1)
        return fail(DLWPCS_E_INVALID, "zonal_spectrum: n_wave = %d outside 1 .. L/2 + 1 = %d (0: all)", d->n_wave, d->L / 2 + 1);
    if (d->n_dims < 0 || d->n_dims > DLWPCS_SCORE_MAX_DIMS)
        return fail(DLWPCS_E_INVALID, "zonal_spectrum: n_dims %d out of range", d->n_dims);
    ZsGeom &G = P.G;
    memset(&G, 0, sizeof(G));
    G.L = d->L;
    G.K = d->n_wave ? d->n_wave : d->L / 2 + 1;
    G.remove_mean = d->remove_mean != 0;
    G.groups = 1;
    G.rpg = 1;
    bool vec = d->L % 4 == 0;
    for (int i = 0; i < d->n_dims; ++i) {
        const int64_t e = d->ext[i];
        if (e < 0 || e >= (1ll << 31)) return fail(DLWPCS_E_INVALID, "zonal_spectrum: extent %lld of dim %d", (long long)e, i);
        for (int op = 0; op < (pair ? 2 : 1); ++op) vec = vec && d->stride[op][i] % 4 == 0;
        if (d->kept[i]) {
            const int n = G.n_keep++;
            G.keep_ext[n] = e;
            for (int op = 0; op < 3; ++op) G.keep_stride[op][n] = d->stride[op][i];
            G.groups *= e;
        } else {
            const int n = G.n_avg++;
            G.avg_ext[n] = e;
            for (int op = 0; op < 3; ++op) G.avg_stride[op][n] = d->stride[op][i];
            G.rpg *= e;
        }
        if (G.groups >= (1ll << 40) || G.rpg >= (1ll << 40)) return fail(DLWPCS_E_UNSUPPORTED, "zonal_spectrum: too many rows");
    }
    P.vec_ok = vec;
    G.n_kt = (G.K + ZS_KT - 1) / ZS_KT;
    G.slabs = 1;
    if (G.rpg >= 1 && G.rpg <= ZS_PACK_ROWS) {
        G.rpt = (int32_t)G.rpg;
        G.gpt = ZS_ROWS / G.rpt;
        G.n_gt = (G.groups + G.gpt - 1) / G.gpt;
        G.n_tiles = 1;
    } else {
        G.rpt = ZS_ROWS;
        G.gpt = 1;
        G.n_gt = G.groups;
        G.n_tiles = (G.rpg + ZS_ROWS - 1) / ZS_ROWS;
        // Workgroups cost the same (every wave of one does the same work), so a launch of n of them takes ceil(n / slots) rounds
        // on the device's resident slots: among the slab counts that keep ZS_SLAB_MIN_ROWS rows per slab, take the one that
        // wastes the least of its last round (ties: the fewest slabs), and none once the launch is large anyway.
        const int64_t base = G.n_gt * G.n_kt;
        if (base > 0 && base < ZS_FILL_BLOCKS && G.rpg >= 2 * ZS_SLAB_MIN_ROWS) {
            int64_t most = G.rpg / ZS_SLAB_MIN_ROWS;
            if (most > ZS_MAX_SLABS) most = ZS_MAX_SLABS;
            int64_t best = 1;
            double best_fill = 0.0;
            for (int64_t sl = 1; sl <= most; ++sl) {
                const int64_t n = sl * base, rounds = (n + ZS_SLOTS - 1) / ZS_SLOTS;
                const double fill = (double)n / (double)(rounds * ZS_SLOTS);
                if (fill > best_fill + 1e-9) { best_fill = fill; best = sl; }
                if (n >= ZS_FILL_BLOCKS && fill >= 0.9) break;
            }
            G.slabs = (int32_t)best;
        }
    }
    G.nblk = G.n_gt * G.slabs * G.n_kt;
    if (G.nblk > MAX_BLOCKS) return fail(DLWPCS_E_UNSUPPORTED, "zonal_spectrum: %lld workgroups is too many", (long long)G.nblk);
    const size_t nq = pair ? 4 : 1;
    P.partial_bytes = P.w_bytes = P.skip_bytes = 0;
    if (G.slabs > 1) {
        P.partial_bytes = (size_t)G.slabs * (size_t)G.groups * nq * (size_t)G.K * sizeof(double);
        P.w_bytes = (size_t)G.slabs * (size_t)G.groups * sizeof(double);
        P.skip_bytes = (size_t)G.slabs * (size_t)G.groups * sizeof(int32_t);
    }
    return DLWPCS_OK;
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

// the pair form needs the larger scratch; the single form of the same descriptor never needs more
extern "C" size_t dlwpcs_zonal_spectrum_scratch_bytes(const dlwpcs_zonal_spectrum_desc *d) {
    ZsPlan P;
    if (zs_plan(d, true, P) != DLWPCS_OK) return 0;
    return P.partial_bytes + P.w_bytes + P.skip_bytes;
}

extern "C" int dlwpcs_zonal_spectrum(const dlwpcs_zonal_spectrum_desc *d, const float *a, const float *b, const float *w,
                                     const float *twiddle, void *scratch, float *out, int32_t *skipped, dlwpcs_stream_t stream) {
    const bool pair = b != nullptr;
    ZsPlan P;
    const int rc = zs_plan(d, pair, P);
    if (rc != DLWPCS_OK) return rc;
    const ZsGeom &G = P.G;
    if (G.groups == 0) return DLWPCS_OK;
    if (!out || !twiddle) return fail(DLWPCS_E_INVALID, "zonal_spectrum: null output or twiddle table");
    if (G.rpg > 0 && !a) return fail(DLWPCS_E_INVALID, "zonal_spectrum: null source");
    if ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)w) | ((uintptr_t)out)) & 3)
        return fail(DLWPCS_E_INVALID, "zonal_spectrum: an operand is not aligned to its 4-byte elements");
    if (((uintptr_t)twiddle) & 7) return fail(DLWPCS_E_INVALID, "zonal_spectrum: the twiddle table is not aligned to 8 bytes");
    if (G.slabs > 1 && (!scratch || (((uintptr_t)scratch) & 7)))
        return fail(DLWPCS_E_INVALID, "zonal_spectrum: this descriptor needs an 8-byte aligned scratch of %zu bytes",
                    P.partial_bytes + P.w_bytes + P.skip_bytes);
    double *partial = (double *)scratch;
    double *part_w = (double *)((char *)scratch + P.partial_bytes);
    int32_t *part_skip = (int32_t *)((char *)scratch + P.partial_bytes + P.w_bytes);
    const bool vec = P.vec_ok && aligned16(a) && aligned16(b);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid = launch_grid(G.nblk), blk(ZS_THREADS);
    const float2 *tw = (const float2 *)twiddle;
#define ZS_LAUNCH(PAIR, VEC) \
    hipLaunchKernelGGL((zonal_spectrum_kernel<PAIR, VEC>), grid, blk, 0, s, G, a, b, w, tw, partial, part_w, part_skip, out, skipped)
    if (pair) { if (vec) ZS_LAUNCH(true, true); else ZS_LAUNCH(true, false); }
    else { if (vec) ZS_LAUNCH(false, true); else ZS_LAUNCH(false, false); }
#undef ZS_LAUNCH
    if (G.slabs > 1) {
        const int nq = pair ? 4 : 1;
        const int64_t n = (int64_t)nq * G.groups * G.K;
        hipLaunchKernelGGL(zonal_spectrum_finish_kernel, launch_grid((n + 255) / 256), dim3(256), 0, s, partial, part_w, part_skip,
                           G.groups, G.K, nq, G.slabs, out, skipped);
    }
    return check_launch("zonal_spectrum");
}
