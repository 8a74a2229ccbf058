// The addressing layer the analysis kernels share: the launch grid for more workgroups than one grid dimension holds, the
// non-finite test, 16-byte chunk loads and stores, the walk from a flat index to one element offset per operand over ext[] /
// stride[], and the row-set geometry of dlwpcs_rows_desc.  Only what at least two translation units use lives here; a new
// analysis family starts from this file ("Shared addressing").
#pragma once
#include <type_traits>
#include "common.h"

namespace dlwpcs {

// ---- launch grid -------------------------------------------------------------------------------------------------------
// n workgroups: x at most 2^16 (so x * 256 work-items fits in 32 bits), the rest in y; the kernel tests flat_block() against n
constexpr int64_t MAX_BLOCKS = 65536ll * 65535ll;

inline dim3 launch_grid(int64_t n) {
    if (n <= 0) return dim3(0, 0);                      // (a zero extent: reported by the plan queries, never launched)
    const int64_t gx = n < 65536 ? n : 65536;
    return dim3((unsigned)gx, (unsigned)((n + gx - 1) / gx));
}

__device__ __forceinline__ int64_t flat_block() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }

// ---- values and pointers -----------------------------------------------------------------------------------------------
__device__ __forceinline__ bool nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ float pos_inf() { return __uint_as_float(0x7f800000u); }

__host__ __device__ inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

// ---- chunks: V = 4 elements in one 16-byte access, or V = 1 ------------------------------------------------------------
template <int V>
__device__ __forceinline__ void load_chunk(const float *__restrict__ p, float x[V]) {
    if constexpr (V == 4) {
        const float4 v = *reinterpret_cast<const float4 *>(p);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
        x[0] = *p;
    }
}

// wide: one 16-byte store (p is aligned, the elements are adjacent); else element by element, stride apart
template <int V, class T>
__device__ __forceinline__ void store_chunk(T *__restrict__ p, const T x[V], bool wide, int64_t stride) {
    if constexpr (V == 4) {
        if (wide) {
            *reinterpret_cast<HIP_vector_type<T, 4> *>(p) = HIP_vector_type<T, 4>(x[0], x[1], x[2], x[3]);
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) p[j * stride] = x[j];
}

// ---- flat index -> element offsets -------------------------------------------------------------------------------------
// one operand of the walk: its stride per dim, and where its element offset goes
struct Strided {
    const int64_t *stride;
    int64_t &off;
};

// q counts row-major over ext[0 .. n), whose last extent counts chunks of V elements; per operand off = sum of coordinate * stride.
// SMALL: 32-bit index arithmetic, for a caller that knows q and every extent to fit 31 bits.
template <int V, bool SMALL, class... Ops>
__device__ __forceinline__ void flat_offsets(int n, const int64_t *ext, int64_t q, Ops... ops) {
    static_assert(sizeof...(Ops) >= 1 && sizeof...(Ops) <= 3 && (V == 1 || V == 4), "one to three operands, chunks of 1 or 4");
    using index_t = typename std::conditional<SMALL, uint32_t, int64_t>::type;
    ((ops.off = 0), ...);
    index_t r = (index_t)q;
    for (int d = n - 1; d >= 0; --d) {
        const index_t e = (index_t)ext[d];
        index_t c = r % e;
        r /= e;
        if (d == n - 1) c *= V;
        ((ops.off += (int64_t)c * ops.stride[d]), ...);
    }
}

// the width chosen at run time (uniform over the launch)
template <int V, class... Ops>
__device__ __forceinline__ void flat_offsets_either(bool small, int n, const int64_t *ext, int64_t q, Ops... ops) {
    if (small) flat_offsets<V, true>(n, ext, q, ops...);
    else flat_offsets<V, false>(n, ext, q, ops...);
}

// ---- the row set of dlwpcs_rows_desc -----------------------------------------------------------------------------------
// What every kernel over a row set addresses with; a family's geometry struct begins with it.
struct RowsAddr {
    int32_t n_inner;
    int64_t ext[DLWPCS_SCORE_MAX_DIMS];                 // the last extent counts chunks (elements / V)
    int64_t sst[DLWPCS_SCORE_MAX_DIMS];
    int64_t ost[DLWPCS_SCORE_MAX_DIMS];
    int64_t src_row_stride, out_row_stride;
    int64_t ncol;                                       // chunks per row
    int64_t tiles;                                      // column tiles of a workgroup's lanes
    int64_t nblk;                                       // workgroups of the launch (the grid may round up)
    __device__ __forceinline__ int64_t last_out_stride() const { return n_inner ? ost[n_inner - 1] : 1; }
};

// chunk q of a row -> element offsets in the source and in the output
template <int V, bool SMALL>
__device__ __forceinline__ void rows_offsets(const RowsAddr &A, int64_t q, int64_t &soff, int64_t &ooff) {
    flat_offsets<V, SMALL>(A.n_inner, A.ext, q, Strided{A.sst, soff}, Strided{A.ost, ooff});
}

// validates the descriptor and copies extents (in elements) and strides; inner = elements per row.  ncol, tiles and nblk are the
// caller's, once it knows its chunk and workgroup sizes.
inline int rows_addr_init(const dlwpcs_rows_desc *d, const char *what, RowsAddr &A, int64_t &inner) {
    if (!d) return fail(DLWPCS_E_INVALID, "%s: null descriptor", what);
    if (d->n_inner < 0 || d->n_inner > DLWPCS_SCORE_MAX_DIMS) return fail(DLWPCS_E_INVALID, "%s: n_inner %d out of range", what, d->n_inner);
    A.n_inner = d->n_inner;
    A.src_row_stride = d->src_row_stride;
    A.out_row_stride = d->out_row_stride;
    inner = 1;
    for (int i = 0; i < d->n_inner; ++i) {
        if (d->inner_ext[i] < 0) return fail(DLWPCS_E_INVALID, "%s: inner extent %lld", what, (long long)d->inner_ext[i]);
        A.ext[i] = d->inner_ext[i];
        A.sst[i] = d->src_stride[i];
        A.ost[i] = d->out_stride[i];
        inner *= d->inner_ext[i];
    }
    return DLWPCS_OK;
}

// The stride and extent half of "may this layout use 16-byte loads (vec) and stores (ovec)": the last dim is contiguous and a
// multiple of 4, every other offset keeps a chunk on 16 bytes.  The pointers' alignment, and any limit of its own, is the caller's.
inline void rows_vector_ok(const dlwpcs_rows_desc *d, bool &vec, bool &ovec) {
    const int L = d->n_inner - 1;
    vec = L >= 0 && d->src_stride[L] == 1 && d->inner_ext[L] % 4 == 0 && d->src_row_stride % 4 == 0;
    for (int i = 0; i < L && vec; ++i) vec = d->src_stride[i] % 4 == 0;
    ovec = vec && d->out_stride[L] == 1 && d->out_row_stride % 4 == 0;
    for (int i = 0; i < L && ovec; ++i) ovec = d->out_stride[i] % 4 == 0;
}

}  // namespace dlwpcs
