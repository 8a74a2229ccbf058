// Small-face bf16 3x3 convolution (faces of <= 320 cells: the coarsest U-Net level): forward pass with the cube-sphere halo, and the
// data gradient on the padded grid.  NOT persistent and not wave-specialised: one workgroup of four waves per (sample, face, 32
// output channels), several resident per CU, so that one workgroup's loads hide behind another's MFMAs -- a face of 144 cells is a
// single tile, and the chunk pipeline of conv_ws.h (one workgroup per CU, a barrier per chunk) has nothing to overlap it with.
//   * the WHOLE haloed face, every input channel, goes to LDS once: straight-line buffer loads of all four waves (a cell outside
//     the face / the zero border: an out-of-range offset, the hardware returns zeros), one barrier;
//   * the waves split the face's 32-pixel M tiles round-robin (tiles w', w' + 4, ... where w' rotates with the workgroup); weight fragments come straight from
//     L2 into registers, one 16-channel operand group ahead of the MFMAs that use them;
//   * the arithmetic is conv_ws.h's to the bit: v_mfma_f32_32x32x16_bf16 as D[co][pixel], accumulators start at the bias, operand
//     groups in order with the nine taps inside, the same activation sequence, one rounding, whole-line stores through a
//     wave-private LDS patch; the data gradient writes interior cells to the source's gradient (times act'(source) where asked)
//     and the halo ring to the workspace, exactly where the padded-grid kernel puts them (tests/test_gpu_conv_small.py: bitwise).
// No workgroup waits for another one; cross-face dependencies stay at the kernel boundary.
#include "conv_ws.h"

namespace dlwpcs {

struct SmallParams {
    const void *src;            // (B,6,Ns,Ns,Cin) bf16: the layer's input (forward) / dz (data gradient)
    const void *wpk;            // packed operands [3][NT][CG][9][64 lanes][16 B]
    const float *bias;          // packed bias [3][NT*32] or nullptr
    const int32_t *table;       // forward: (6, Ns+2, Ns+2) halo table
    void *out;                  // forward: y (B,6,No,No,Cout); data gradient: the padded gradient (B,6,No,No,Cout), ring cells only
    void *d0;                   // data gradient: the source's gradient (B,6,No-2,No-2,Cout), interior cells
    const void *m0;             // data gradient: the source itself (act' operand of what goes to d0) or nullptr
    int B, Ns, No, W2;          // source face, output face, LDS tile width (No + 2)
    int Cin, Cout, CG, NT;      // CG = Cin / 16, NT = Cout / 32
    int Q;                      // 16-B vectors per cell = Cin / 8
    uint32_t magicQ, magicW2, magicNo, magicNT, magicB;
    int act;
    float alpha, vmax;
    float m_alpha;
    uint32_t m_thr1;
    int patch_base;             // LDS offset of the wave-private epilogue patches
};

constexpr int SM_THREADS = 256, SM_WAVES = 4;
constexpr int SM_PROW = 32 * 2 + 16;            // patch row: one pixel's 32 bf16 channels + pad
constexpr int SM_U = 16;                        // input vectors in flight per thread

// BWD = false: forward (halo table); true: data gradient (zero border of width 2).  MTW = M tiles per wave at most.
template <bool BWD, int MTW>
__global__ void __launch_bounds__(SM_THREADS, 2) conv_small_kernel(const SmallParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    // workgroup -> (face, sample, n tile): n tile fastest, then the sample; neighbours share an XCD's L2 (input tile, weights)
    const uint32_t t = xcd_remap(blockIdx.x, gridDim.x);
    const int bf = P.magicNT ? __umulhi(t, P.magicNT) : (int)t;
    const int nt = (int)t - bf * P.NT;
    const int f = P.magicB ? __umulhi((uint32_t)bf, P.magicB) : bf;
    const int b = bf - f * P.B;
    const int v = f < 4 ? 0 : (f == 4 ? 1 : 2);
    const int RB = P.Cin * 2 + 16;              // LDS bytes per cell
    const int face_pix = P.No * P.No;
    const int ncells = P.W2 * P.W2;
    const int nitems = ncells * P.Q;

    // weight fragments of this n tile: [operand group][tap][lane]; group 0 is requested before anything else
    const uint4 *wsrc = reinterpret_cast<const uint4 *>(P.wpk) + ((size_t)v * P.NT + nt) * P.CG * 576 + lane;
    auto load_w = [&](int cg, uint4 (&w)[9]) __attribute__((always_inline)) {
        const uint4 *p = wsrc + (size_t)min(cg, P.CG - 1) * 576;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) w[tap] = p[tap * 64];
    };
    uint4 wa[9], wb[9];
    load_w(0, wa);

    // ---- the haloed face -> LDS
    {
        const int spix = 6 * P.Ns * P.Ns;
        const rsrc_t rs = make_rsrc(reinterpret_cast<const bf16_t *>(P.src) + (size_t)b * spix * P.Cin, (uint32_t)(spix * P.Cin * 2));
#pragma unroll 1
        for (int e0 = 0; e0 < nitems; e0 += SM_THREADS * SM_U) {
            int sp[SM_U];
#pragma unroll
            for (int u = 0; u < SM_U; ++u) {
                const int e = e0 + tid + u * SM_THREADS;
                const bool live = e < nitems;
                const int cell = __umulhi((uint32_t)e, P.magicQ);
                if constexpr (!BWD) {
                    sp[u] = P.table[live ? f * ncells + cell : 0];
                    if (!live) sp[u] = -1;
                } else {
                    const int ty = __umulhi((uint32_t)cell, P.magicW2), tx = cell - ty * P.W2;
                    const int vy = ty - 2, vx = tx - 2;
                    const bool ok = live & ((uint32_t)vy < (uint32_t)P.Ns) & ((uint32_t)vx < (uint32_t)P.Ns);
                    sp[u] = ok ? (f * P.Ns + vy) * P.Ns + vx : -1;
                }
            }
            u32x4 val[SM_U];
#pragma unroll
            for (int u = 0; u < SM_U; ++u) {
                const int e = e0 + tid + u * SM_THREADS;
                const int cell = __umulhi((uint32_t)e, P.magicQ), qv = e - cell * P.Q;
                const uint32_t off = sp[u] >= 0 ? (uint32_t)(sp[u] * P.Cin + qv * 8) * 2u : ST_SKIP;
                val[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < SM_U; ++u) {
                const int e = e0 + tid + u * SM_THREADS;
                const int cell = __umulhi((uint32_t)e, P.magicQ), qv = e - cell * P.Q;
                if (e < nitems) *reinterpret_cast<uint4 *>(smem + cell * RB + qv * 16) = make_uint4(val[u].x, val[u].y, val[u].z, val[u].w);
            }
        }
    }

    // ---- this wave's M tiles: tile j = wv + 4 i, pixel j * 32 + l31 of the face (row-major)
    const int nmt = (face_pix + 31) >> 5;
    // (which wave takes the face's odd tiles rotates with the workgroup: waves of equal index share a SIMD, and with 5 tiles over 4
    // waves the one with two would be the same SIMD's in every workgroup of the CU)
    const int wv = (wave + (int)(blockIdx.x >> 3) + (int)(blockIdx.x >> 8)) & (SM_WAVES - 1);
    const int my_mt = max(0, min(MTW, (nmt - wv + SM_WAVES - 1) / SM_WAVES));
    int abase[MTW];
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
        const int m = (wv + SM_WAVES * i) * 32 + l31;
        int base = 0;
        if (m < face_pix) {
            const int oy = __umulhi((uint32_t)m, P.magicNo), ox = m - oy * P.No;
            base = (oy * P.W2 + ox) * RB;
        }
        abase[i] = base + half * 16;
    }
    // the bias quads the accumulators start at (row = output channel in the D[co][pixel] layout)
    float4 bq[4];
#pragma unroll
    for (int jq = 0; jq < 4; ++jq)
        bq[jq] = P.bias ? *reinterpret_cast<const float4 *>(P.bias + (size_t)v * P.NT * 32 + nt * 32 + 8 * jq + 4 * half)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
    f32x16 acc[MTW];            // (set by the matrix phase, for the M tiles the wave has: the others stay undefined and unused)

    load_w(1, wb);
    __syncthreads();            // the face is in LDS; nothing writes that part of LDS again
    if (my_mt == 0) return;     // (uniform per wave: faces of fewer than four M tiles)

    // ---- matrix phase: operand groups in order, the nine taps inside (two groups = 18 steps per trip of the loop).  A wave has one
    // to three MFMAs per step and an LDS read takes longer than those: the pixel fragments run SM_D steps ahead of the MFMAs through
    // a ring of SM_R register sets (18 % SM_R == 0: the ring position of a step is a compile-time constant), the weight fragments a
    // whole group ahead (group 0 was requested before the face was staged, group 1 before the barrier).
    auto matrix = [&](auto mta_tag) __attribute__((always_inline)) {
        constexpr int MTA = decltype(mta_tag)::value;
        constexpr int SM_R = MTA == 1 ? 6 : 3, SM_D = SM_R - 1;     // (one M tile: five steps = five MFMAs ahead; more: two steps)
        uint4 fa[SM_R][MTA];
#pragma unroll
        for (int i = 0; i < MTA; ++i)
#pragma unroll
            for (int jq = 0; jq < 4; ++jq) {
                acc[i][4 * jq] = bq[jq].x; acc[i][4 * jq + 1] = bq[jq].y; acc[i][4 * jq + 2] = bq[jq].z; acc[i][4 * jq + 3] = bq[jq].w;
            }
        auto rd = [&](int cg, int tap, uint4 (&a)[MTA]) __attribute__((always_inline)) {
            // (the last trip reads SM_D steps into a group that does not exist: at most 32 B past a cell's channels, inside the
            // workgroup's allocation, never used)
            const char *lds = smem + cg * 32 + ((tap / 3) * P.W2 + tap % 3) * RB;
#pragma unroll
            for (int i = 0; i < MTA; ++i) a[i] = *reinterpret_cast<const uint4 *>(lds + abase[i]);
        };
#pragma unroll
        for (int st = 0; st < SM_D; ++st) rd(0, st, fa[st % SM_R]);
        __builtin_amdgcn_sched_group_barrier(0x100, SM_D * MTA, 0);
#pragma unroll 1
        for (int cg = 0; cg < P.CG; cg += 2) {          // (CG is even: Cin is a multiple of 32)
#pragma unroll
            for (int st = 0; st < 18; ++st) {
                rd(cg + (st + SM_D) / 9, (st + SM_D) % 9, fa[(st + SM_D) % SM_R]);
#pragma unroll
                for (int i = 0; i < MTA; ++i) frag_mma<bf16_t>(acc[i], st < 9 ? wa[st] : wb[st - 9], fa[st % SM_R][i]);
                __builtin_amdgcn_sched_group_barrier(0x100, MTA, 0);        // the reads of step st + SM_D first
                __builtin_amdgcn_sched_group_barrier(0x008, MTA, 0);        // then the MFMAs of step st
                // (the compiler barrier keeps the requests here: hoisted above the MFMAs that still read the old fragments they would
                // need a third register set)
                if (st == 8) { asm volatile("" ::: "memory"); load_w(cg + 2, wa); }     // (past the end: the last group again, unused)
                if (st == 17) { asm volatile("" ::: "memory"); load_w(cg + 3, wb); }
            }
        }
    };
    if (MTW >= 3 && my_mt >= 3) matrix(std::integral_constant<int, (MTW >= 3 ? 3 : 1)>{});
    else if (MTW >= 2 && my_mt == 2) matrix(std::integral_constant<int, (MTW >= 2 ? 2 : 1)>{});
    else matrix(std::integral_constant<int, 1>{});

    // ---- epilogue set-up (behind the matrix phase, which has no registers to spare for it)
    // store pass (i, ps) of this lane: byte offset of its 16 B inside one sample of the destination and (data gradient) which one
    constexpr int NPS = 2;                      // bf16: 4 lanes per pixel, 16 pixels per pass
    uint32_t soff[MTW][NPS];
    uint32_t ssel = 0;
    const int c = nt * 32 + (lane & 3) * 8;
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int ps = 0; ps < NPS; ++ps) {
            const int m = (wv + SM_WAVES * i) * 32 + ps * 16 + (lane >> 2);
            const int oy = __umulhi((uint32_t)m, P.magicNo), ox = m - oy * P.No;
            int off = ((f * face_pix + m) * P.Cout + c) * 2;
            if constexpr (BWD) {
                const int Nd = P.No - 2;
                const bool interior = ((uint32_t)(oy - 1) < (uint32_t)Nd) & ((uint32_t)(ox - 1) < (uint32_t)Nd);
                if (interior && P.d0 != nullptr) {
                    off = (((f * Nd + (oy - 1)) * Nd + (ox - 1)) * P.Cout + c) * 2;
                    ssel |= 1u << (i * NPS + ps);
                }
            }
            soff[i][ps] = m < face_pix ? (uint32_t)off : ST_SKIP;
        }
    // the source's own values at the cells this lane sends to d0 (requested behind the matrix phase: 16 registers it has no room for;
    // other workgroups' MFMAs cover the round trip)
    uint4 ymq[BWD ? MTW : 1][NPS];
    if constexpr (BWD) {
        const int dpix = 6 * (P.No - 2) * (P.No - 2);
        const rsrc_t rm = make_rsrc(P.m0 ? reinterpret_cast<const bf16_t *>(P.m0) + (size_t)b * dpix * P.Cout : nullptr, (uint32_t)(dpix * P.Cout * 2));
#pragma unroll
        for (int i = 0; i < MTW; ++i)
#pragma unroll
            for (int ps = 0; ps < NPS; ++ps) {
                const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(rm, ((ssel >> (i * NPS + ps)) & 1u) ? soff[i][ps] : ST_SKIP, 0, 0);
                ymq[i][ps] = make_uint4(a.x, a.y, a.z, a.w);
            }
    }
    // ---- epilogue: activation, one rounding, whole lines out of the wave's patch (see conv_ws.h)
    const float e_alpha = P.act == DLWPCS_ACT_LEAKY_CLIP ? P.alpha : 1.f;
    const float e_vmax = P.act == DLWPCS_ACT_LEAKY_CLIP ? P.vmax : __builtin_inff();
    const bool fast_act = e_alpha >= 0.f && e_alpha <= 1.f && e_vmax >= 0.f;
    const int amode = (BWD || P.act != DLWPCS_ACT_LEAKY_CLIP) ? 2 : (fast_act ? 1 : 0);      // 2: identity, 1: max / minimum3, 0: select form
    auto quad = [&](const f32x16 &a, int jq) __attribute__((always_inline)) {
        float4 v4 = make_float4(a[4 * jq], a[4 * jq + 1], a[4 * jq + 2], a[4 * jq + 3]);
        if (amode == 2) return v4;
        if (amode == 1) {
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            auto lc = [&](float x, float ax) {
                float tt, y;
                asm("v_max_f32 %0, %1, %2" : "=v"(tt) : "v"(x), "v"(ax));
                asm("v_minimum3_f32 %0, %1, %2, %2" : "=v"(y) : "v"(tt), "v"(e_vmax));
                return y;
            };
            const f32x2 a01 = f32x2{v4.x, v4.y} * e_alpha, a23 = f32x2{v4.z, v4.w} * e_alpha;
            v4.x = lc(v4.x, a01.x); v4.y = lc(v4.y, a01.y); v4.z = lc(v4.z, a23.x); v4.w = lc(v4.w, a23.y);
        } else {
            v4.x = act_leaky_clip(v4.x, e_alpha, e_vmax); v4.y = act_leaky_clip(v4.y, e_alpha, e_vmax);
            v4.z = act_leaky_clip(v4.z, e_alpha, e_vmax); v4.w = act_leaky_clip(v4.w, e_alpha, e_vmax);
        }
        return v4;
    };
    const rsrc_t d_out = make_rsrc(reinterpret_cast<bf16_t *>(P.out) + (size_t)b * 6 * face_pix * P.Cout, (uint32_t)(6 * face_pix * P.Cout * 2));
    const int dpix = 6 * (P.No - 2) * (P.No - 2);
    const rsrc_t d_0 = BWD ? make_rsrc(P.d0 ? reinterpret_cast<bf16_t *>(P.d0) + (size_t)b * dpix * P.Cout : nullptr, (uint32_t)(dpix * P.Cout * 2))
                           : d_out;
    char *const patch = smem + P.patch_base + wave * (32 * SM_PROW);
    if constexpr (BWD) {
        // (every mask value is waited for here, before the first store: loads and stores share one counter)
#pragma unroll
        for (int i = 0; i < MTW; ++i)
#pragma unroll
            for (int ps = 0; ps < NPS; ++ps) asm volatile("" : "+v"(ymq[i][ps].x), "+v"(ymq[i][ps].y), "+v"(ymq[i][ps].z), "+v"(ymq[i][ps].w));
    }
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
        if (i < my_mt) {        // (uniform)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 v4 = quad(acc[i], k);
                *reinterpret_cast<uint2 *>(patch + l31 * SM_PROW + (8 * k + 4 * half) * 2) = make_uint2(f2bf2(v4.x, v4.y), f2bf2(v4.z, v4.w));
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int ps = 0; ps < NPS; ++ps) {
                uint4 o = *reinterpret_cast<const uint4 *>(patch + (ps * 16 + (lane >> 2)) * SM_PROW + (lane & 3) * 16);
                if constexpr (BWD) {
                    const bool to0 = ((ssel >> (i * NPS + ps)) & 1u) != 0;
                    uint4 om = o;
                    vmask_pk(om, ymq[i][ps], P.m_alpha, P.m_thr1);
                    const bool on = to0 && P.m0 != nullptr;
                    o.x = on ? om.x : o.x; o.y = on ? om.y : o.y; o.z = on ? om.z : o.z; o.w = on ? om.w : o.w;
                    bst128(o, d_out, to0 ? ST_SKIP : soff[i][ps]);
                    bst128(o, d_0, to0 ? soff[i][ps] : ST_SKIP);
                } else {
                    bst128(o, d_out, soff[i][ps]);
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// what the kernel serves (the callers have checked dtype, kernel size, halo, single source, no upsampling)
// (both directions of the layer: the data gradient stages (N + 4)^2 cells of C_out channels)
bool conv_small_serves(int B, int N, int Cin, int Cout) {
    const int cmax = Cin > Cout ? Cin : Cout;
    return N >= 2 && N * N <= 320 && Cin >= 32 && Cout >= 32 && Cin % 32 == 0 && Cout % 32 == 0 &&
           (size_t)(N + 4) * (N + 4) * (cmax * 2 + 16) + (size_t)SM_WAVES * 32 * SM_PROW <= 160 * 1024 && (long)B * 6 * (cmax / 32) < (1l << 16);
}

template <bool BWD>
static int launch_small_t(const SmallParams &P, int mtw, size_t lds, unsigned grid, hipStream_t s) {
    auto go = [&](auto kern) -> int {
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return fail(DLWPCS_E_LAUNCH, "conv_small: hipFuncSetAttribute: %s", hipGetErrorString(e));
        }
        hipLaunchKernelGGL(kern, dim3(grid), dim3(SM_THREADS), lds, s, P);
        return check_launch("conv_small");
    };
    if (mtw == 1) return go(conv_small_kernel<BWD, 1>);
    if (mtw == 2) return go(conv_small_kernel<BWD, 2>);
    return go(conv_small_kernel<BWD, 3>);
}

// K: the launch as conv_fwd_impl / conv_bwd_data_impl describe it to the persistent kernel (mode = MODE_HALO: forward, MODE_ZERO: data
// gradient on the padded grid).  Reports direct_done / mask_done like launch_conv_cfg; dry_run: reports only.
int launch_conv_small(const ConvKParams &K, hipStream_t s) {
    const bool bwd = K.mode == MODE_ZERO;
    if (K.mode != MODE_HALO && !bwd) return fail(DLWPCS_E_UNSUPPORTED, "conv_small: serves halo convolutions and their data gradients");
    const int N = K.Nin;                        // the layer's face (forward: input = output grid; data gradient: the dz grid)
    if (K.C1 != 0 || K.up0 || K.ymask || K.pool_out || K.head_w || K.edge)
        return fail(DLWPCS_E_UNSUPPORTED, "conv_small: one source, no upsampling, no mask on load, no pooled or folded second output");
    if (K.No != (bwd ? N + 2 : N) || !conv_small_serves(K.B, N, K.Cin, K.Cout))
        return fail(DLWPCS_E_UNSUPPORTED, "conv_small: N=%d Cin=%d Cout=%d outside faces of <= 320 cells with channel counts that are multiples of 32",
                    N, K.Cin, K.Cout);
    if (bwd && K.d1) return fail(DLWPCS_E_UNSUPPORTED, "conv_small: one source");
    if (bwd && K.d0 && K.dsplit != K.Cout) return fail(DLWPCS_E_UNSUPPORTED, "conv_small: one source");
    SmallParams P{};
    P.src = K.src0; P.wpk = K.wpk; P.bias = K.bias; P.table = K.table; P.out = K.out;
    P.d0 = bwd ? K.d0 : nullptr;
    P.m0 = (bwd && K.d0) ? K.m0 : nullptr;
    P.B = K.B; P.Ns = N; P.No = K.No; P.W2 = K.No + 2;
    P.Cin = K.Cin; P.Cout = K.Cout; P.CG = K.Cin / 16; P.NT = K.Cout / 32; P.Q = K.Cin / 8;
    P.magicQ = div_magic(P.Q); P.magicW2 = div_magic(P.W2); P.magicNo = div_magic(P.No);
    P.magicNT = P.NT > 1 ? div_magic(P.NT) : 0; P.magicB = P.B > 1 ? div_magic(P.B) : 0;
    P.act = K.act; P.alpha = K.alpha; P.vmax = K.vmax;
    P.m_alpha = K.m_alpha; P.m_thr1 = K.m_thr1;
    const size_t in_b = (size_t)P.W2 * P.W2 * (P.Cin * 2 + 16);
    P.patch_base = (int)in_b;
    const size_t lds = in_b + (size_t)SM_WAVES * 32 * SM_PROW;
    const int nmt = ceil_div(P.No * P.No, 32), mtw = ceil_div(nmt, SM_WAVES);
    const long nwg = (long)P.B * 6 * P.NT;
    // (the index arithmetic divides by multiplication: exact below 2^16)
    if (lds > 160 * 1024 || mtw > 3 || nwg >= (1l << 16) || P.W2 * P.W2 * P.Q >= (1 << 16))
        return fail(DLWPCS_E_UNSUPPORTED, "conv_small: B=%d N=%d Cin=%d beyond the kernel's LDS tile or index range", P.B, N, P.Cin);
    if (K.direct_done) *K.direct_done = (bwd && P.d0) ? 1 : 0;
    if (K.mask_done) *K.mask_done = P.m0 ? 1 : 0;
    if (K.pool_done) *K.pool_done = 0;
    if (K.head_done) *K.head_done = 0;
    if (K.dry_run || K.B == 0) return DLWPCS_OK;
    return bwd ? launch_small_t<true>(P, mtw, lds, (unsigned)nwg, s) : launch_small_t<false>(P, mtw, lds, (unsigned)nwg, s);
}

}  // namespace dlwpcs
