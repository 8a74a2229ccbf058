// Areas of the intersections of lat-lon cells with equiangular cubed-sphere cells, closed form, fp64 (the numpy
// twin is DLWP/remap/overlap.py, which states the maths).  In (lambda, sin phi) a lat-lon cell is the rectangle
// [lc - w, lc + w] x [s1, s2] and area is d lambda * d sin phi.  A cube cell is four half-spaces n.p >= 0:
//     n_z != 0:  tan phi >= / <= c cos(lambda - l*),  c = -hypot(n_x, n_y) / n_z,  l* = atan2(n_y, n_x)   (lower: n_z > 0)
//                sin phi on the curve = u / sqrt(1 + u^2), u = c cos(lambda - l*); antiderivative asin(k sin(lambda - l*)),
//                k = c / sqrt(1 + c^2)
//     n_z == 0:  cos(lambda - l*) >= 0
//     A = integral over the cell's longitudes of [min(s2, uppers) - max(s1, lowers)]+
// cut at the interval's ends, the longitudes of the cube cell's corners, the crossings of every curve with the two latitude
// edges and the ends of every meridian constraint (<= 22 breakpoints, relative to lc and wrapped); on each piece the active
// bounds are chosen at its midpoint.
//
// One lane owns one lat-lon cell (a CSR row).  Per face, a cap about the cell's centre that reaches its corners gives an index
// range in each of the face's two equiangular coordinates; the exact routine returns 0 for the candidates that do not meet the
// cell.  A lane walks its candidates in ascending cube-cell order, so a row's entries ascend without a sort and no atomic decides
// an order: dlwpcs_overlap_count writes the number of entries above the dust threshold per row, the caller scans it, and
// dlwpcs_overlap_fill walks the same candidates again and writes each row's entries at its offset.  Same call, same bits.
//
// fp64 VALU and libm with lane-dependent trip counts: nothing here is bound by memory.  The breakpoints are the one
// runtime-indexed per-lane array, and they live in LDS (lane-strided: conflict free) instead of scratch; the four planes are
// walked by fully unrolled loops and the active bound is carried as values, not as an index, so they stay in registers.
#include "common.h"

namespace dlwpcs {

namespace {

constexpr int OV_THREADS = 64;
constexpr int OV_BREAKS = 22;                    // 2 ends + 4 corners + 4 planes x 4
constexpr double OV_PI = 3.14159265358979323846;
constexpr double OV_MERIDIAN_EPS = 1e-14;        // |n_z| <= eps * hypot(n_x, n_y): the plane holds the z axis
constexpr double OV_CAP_SLACK = 1e-9;
constexpr int OV_MAX_N = 16384;                  // 6 N^2 < 2^31

enum { OV_MERIDIAN = 0, OV_LOWER = 1, OV_UPPER = 2 };

struct OvPlane {
    double lam, cc, kk;
    int kind;
};

struct OvCell {                                  // a lat-lon cell
    double s1, s2, lc, w, t1, t2;                // t = tan of the latitude edges (+-inf at a pole)
};

__device__ __forceinline__ double ov_wrap(double x) { return x - (2.0 * OV_PI) * rint(x / (2.0 * OV_PI)); }

__device__ __forceinline__ double ov_line_tan(int k, int N) {
    if (k == 0) return -1.0;
    if (k == N) return 1.0;
    if (2 * k == N) return 0.0;
    return tan(-OV_PI / 4 + k * (OV_PI / (2 * N)));
}

__device__ __forceinline__ double ov_corner_area(double x, double y) { return atan(x * y / sqrt(1.0 + x * x + y * y)); }

// the half-space (a - t * b) . p >= 0 (sign = +1) or (t * b - a) . p >= 0 (sign = -1)
__device__ __forceinline__ OvPlane ov_plane(const double *a, const double *b, double t, double sign) {
    const double nx = sign * (a[0] - t * b[0]), ny = sign * (a[1] - t * b[1]), nz = sign * (a[2] - t * b[2]);
    const double hyp = hypot(nx, ny);
    OvPlane P;
    P.lam = atan2(ny, nx);
    if (fabs(nz) <= OV_MERIDIAN_EPS * hyp) {
        P.kind = OV_MERIDIAN;
        P.cc = 0.0;
        P.kk = 0.0;
    } else {
        P.kind = nz > 0.0 ? OV_LOWER : OV_UPPER;
        P.cc = -hyp / nz;
        P.kk = P.cc / sqrt(1.0 + P.cc * P.cc);
    }
    return P;
}

struct OvBreaks {                                // the lane's column of the workgroup's LDS table
    double *p;
    int n;
    __device__ __forceinline__ void push(double v, double w) {
        if (n < OV_BREAKS) {
            p[n * OV_THREADS] = fmin(fmax(v, -w), w);
            ++n;
        }
    }
    __device__ __forceinline__ double at(int k) const { return p[k * OV_THREADS]; }
    __device__ __forceinline__ void sort() {
        for (int i = 1; i < n; ++i) {
            const double v = p[i * OV_THREADS];
            int j = i - 1;
            while (j >= 0 && p[j * OV_THREADS] > v) {
                p[(j + 1) * OV_THREADS] = p[j * OV_THREADS];
                --j;
            }
            p[(j + 1) * OV_THREADS] = v;
        }
    }
};

__device__ __forceinline__ void ov_corner(OvBreaks &B, const OvCell &c, const double *e0, const double *eu, const double *ev,
                                          double x, double y) {
    const double px = e0[0] + x * eu[0] + y * ev[0], py = e0[1] + x * eu[1] + y * ev[1], pz = e0[2] + x * eu[2] + y * ev[2];
    const double h = hypot(px, py);
    if (h > OV_MERIDIAN_EPS * sqrt(h * h + pz * pz)) B.push(ov_wrap(atan2(py, px) - c.lc), c.w);
}

__device__ __forceinline__ double ov_pair_area(const OvCell &c, const OvPlane (&pl)[4], const double *e0, const double *eu, const double *ev,
                               double xa, double xb, double ya, double yb, double *lds_col) {
    OvBreaks B{lds_col, 0};
    B.push(-c.w, c.w);
    B.push(c.w, c.w);
    ov_corner(B, c, e0, eu, ev, xa, ya);
    ov_corner(B, c, e0, eu, ev, xb, ya);
    ov_corner(B, c, e0, eu, ev, xa, yb);
    ov_corner(B, c, e0, eu, ev, xb, yb);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        if (pl[p].kind == OV_MERIDIAN) {
            B.push(ov_wrap(pl[p].lam + OV_PI / 2 - c.lc), c.w);
            B.push(ov_wrap(pl[p].lam - OV_PI / 2 - c.lc), c.w);
        } else {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const double ratio = (e ? c.t2 : c.t1) / pl[p].cc;           // cc == 0: +-inf or NaN, no crossing
                if (fabs(ratio) <= 1.0) {
                    const double th = acos(ratio);
                    B.push(ov_wrap(pl[p].lam + th - c.lc), c.w);
                    B.push(ov_wrap(pl[p].lam - th - c.lc), c.w);
                }
            }
        }
    }
    B.sort();
    double A = 0.0;
    for (int k = 0; k + 1 < B.n; ++k) {
        const double a = B.at(k), b = B.at(k + 1);
        if (!(b > a)) continue;
        const double base = 0.5 * (a + b) + c.lc;
        double vu = INFINITY, ku = 0.0, lu = 0.0, vl = -INFINITY, kl = 0.0, ll = 0.0;
        bool out = false;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const double cm = cos(base - pl[p].lam);
            if (pl[p].kind == OV_MERIDIAN) {
                out = out || cm < 0.0;
            } else {
                const double u = pl[p].cc * cm;
                const double sv = u / sqrt(1.0 + u * u);
                if (pl[p].kind == OV_UPPER && sv < vu) { vu = sv; ku = pl[p].kk; lu = pl[p].lam; }
                if (pl[p].kind == OV_LOWER && sv > vl) { vl = sv; kl = pl[p].kk; ll = pl[p].lam; }
            }
        }
        if (out) continue;
        const bool cu = vu < c.s2, cl = vl > c.s1;
        if (!((cu ? vu : c.s2) > (cl ? vl : c.s1))) continue;
        const double iu = cu ? asin(ku * sin(b + c.lc - lu)) - asin(ku * sin(a + c.lc - lu)) : c.s2 * (b - a);
        const double il = cl ? asin(kl * sin(b + c.lc - ll)) - asin(kl * sin(a + c.lc - ll)) : c.s1 * (b - a);
        A += iu - il;
    }
    return A;
}

// inclusive index range [lo, hi] of the cap (centre q, radius rho) in the face coordinate atan2(p . along, p . e0)
__device__ __forceinline__ void ov_range(const double *q, double rho, double srho, const double *e0, const double *along,
                                         const double *across, int N, int &lo, int &hi) {
    const double qa = q[0] * along[0] + q[1] * along[1] + q[2] * along[2];
    const double q0 = q[0] * e0[0] + q[1] * e0[1] + q[2] * e0[2];
    const double qx = q[0] * across[0] + q[1] * across[1] + q[2] * across[2];
    const double cel = sqrt(fmax(0.0, 1.0 - qx * qx));
    if (rho >= OV_PI / 2 || srho >= cel * (1.0 - 1e-12)) {
        lo = 0;
        hi = N - 1;
        return;
    }
    const double a0 = atan2(qa, q0), dl = asin(fmin(1.0, srho / cel)) + OV_CAP_SLACK, h = OV_PI / (2 * N);
    lo = (int)fmin(fmax(floor((a0 - dl + OV_PI / 4) / h), 0.0), (double)N);
    hi = (int)fmin(fmax(floor((a0 + dl + OV_PI / 4) / h), -1.0), (double)(N - 1));
}

template <bool FILL>
__global__ void __launch_bounds__(OV_THREADS) overlap_kernel(const dlwpcs_overlap_desc d, const double *__restrict__ sin_lat_edges,
                                                             const double *__restrict__ lon_edges, int32_t *__restrict__ counts,
                                                             const int64_t *__restrict__ row_ptr, int32_t *__restrict__ col,
                                                             double *__restrict__ area, int64_t nnz) {
    __shared__ double s_breaks[OV_BREAKS * OV_THREADS];
    const int64_t r = (int64_t)blockIdx.x * OV_THREADS + threadIdx.x;
    const int64_t n_cells = (int64_t)d.n_lat * d.n_lon;
    if (r >= n_cells) return;                                        // (no barrier below: a lane's LDS column is its own)
    const int N = d.N;
    const int ir = (int)(r / d.n_lon), jr = (int)(r - (int64_t)ir * d.n_lon);
    OvCell c;
    {
        const double sa = sin_lat_edges[ir], sb = sin_lat_edges[ir + 1];
        c.s1 = fmin(sa, sb);
        c.s2 = fmax(sa, sb);
        const double l0 = lon_edges[jr], l1 = lon_edges[jr + 1];
        c.lc = 0.5 * (l0 + l1);
        c.w = 0.5 * (l1 - l0);
        c.t1 = c.s1 / sqrt(1.0 - c.s1 * c.s1);
        c.t2 = c.s2 / sqrt(1.0 - c.s2 * c.s2);
    }
    const double area_r = (c.s2 - c.s1) * (2.0 * c.w);
    // the cap about the cell's centre that reaches its corners (its farthest points: the cell is at most 180 degrees wide)
    double q[3], rho, srho;
    {
        const double p1 = asin(c.s1), p2 = asin(c.s2), pc = 0.5 * (p1 + p2);
        const double sp = sin(pc), cp = cos(pc), cw = cos(c.w);
        q[0] = cp * cos(c.lc);
        q[1] = cp * sin(c.lc);
        q[2] = sp;
        const double dmin = fmin(sp * c.s1 + cp * cos(p1) * cw, sp * c.s2 + cp * cos(p2) * cw);
        rho = acos(fmin(fmax(dmin, -1.0), 1.0)) + OV_CAP_SLACK;
        srho = sin(rho);
    }
    double *lds_col = s_breaks + threadIdx.x;
    int64_t at = 0, end = 0;
    if constexpr (FILL) {
        at = row_ptr[r];
        end = row_ptr[r + 1];
        if (end > nnz) end = nnz;                                    // a scan that does not belong to these counts writes nothing outside
        if (at < 0) at = end;
    }
    int32_t cnt = 0;
    for (int f = 0; f < 6; ++f) {
        double e0[3], eu[3], ev[3];                                  // (f is uniform: scalar loads from the kernel arguments)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            e0[k] = d.frames[f][0][k];
            eu[k] = d.frames[f][1][k];
            ev[k] = d.frames[f][2][k];
        }
        int j0, j1, i0, i1;
        ov_range(q, rho, srho, e0, eu, ev, N, j0, j1);
        ov_range(q, rho, srho, e0, ev, eu, N, i0, i1);
        if (j0 > j1) continue;
        for (int i = i0; i <= i1; ++i) {
            const double ya = ov_line_tan(i, N), yb = ov_line_tan(i + 1, N);
            OvPlane pl[4];
            pl[2] = ov_plane(ev, e0, ya, 1.0);
            pl[3] = ov_plane(ev, e0, yb, -1.0);
            for (int j = j0; j <= j1; ++j) {
                const double xa = ov_line_tan(j, N), xb = ov_line_tan(j + 1, N);
                pl[0] = ov_plane(eu, e0, xa, 1.0);
                pl[1] = ov_plane(eu, e0, xb, -1.0);
                const double A = ov_pair_area(c, pl, e0, eu, ev, xa, xb, ya, yb, lds_col);
                const double area_c = ov_corner_area(xb, yb) - ov_corner_area(xa, yb) - ov_corner_area(xb, ya) + ov_corner_area(xa, ya);
                if (A > d.dust * fmin(area_r, area_c)) {
                    if constexpr (FILL) {
                        if (at < end) {
                            col[at] = (f * N + i) * N + j;
                            area[at] = A;
                            ++at;
                        }
                    }
                    ++cnt;
                }
            }
        }
    }
    if constexpr (!FILL) counts[r] = cnt;
}

int ov_check(const dlwpcs_overlap_desc *d, const void *a, const void *b, const char *what) {
    if (!d || !a || !b) return fail(DLWPCS_E_INVALID, "%s: null pointer", what);
    if (d->N < 1 || d->N > OV_MAX_N) return fail(DLWPCS_E_INVALID, "%s: N = %d must lie in [1, %d]", what, d->N, OV_MAX_N);
    if (d->n_lat < 1 || d->n_lon < 2) return fail(DLWPCS_E_INVALID, "%s: n_lat = %d, n_lon = %d (>= 1, >= 2)", what, d->n_lat, d->n_lon);
    if (!(d->dust >= 0.0)) return fail(DLWPCS_E_INVALID, "%s: the dust factor must not be negative", what);
    if ((int64_t)d->n_lat * d->n_lon >= (1ll << 31) - OV_THREADS)
        return fail(DLWPCS_E_UNSUPPORTED, "%s: %lld lat-lon cells (< 2^31)", what, (long long)d->n_lat * d->n_lon);
    return DLWPCS_OK;
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" int dlwpcs_overlap_count(const dlwpcs_overlap_desc *d, const double *sin_lat_edges, const double *lon_edges,
                                    int32_t *counts, dlwpcs_stream_t stream) {
    const int rc = ov_check(d, sin_lat_edges, lon_edges, "overlap_count");
    if (rc != DLWPCS_OK) return rc;
    if (!counts) return fail(DLWPCS_E_INVALID, "overlap_count: null pointer");
    const int64_t n = (int64_t)d->n_lat * d->n_lon;
    hipLaunchKernelGGL(overlap_kernel<false>, dim3((unsigned)((n + OV_THREADS - 1) / OV_THREADS)), dim3(OV_THREADS), 0,
                       (hipStream_t)stream, *d, sin_lat_edges, lon_edges, counts, (const int64_t *)nullptr, (int32_t *)nullptr,
                       (double *)nullptr, (int64_t)0);
    return check_launch("overlap_count");
}

extern "C" int dlwpcs_overlap_fill(const dlwpcs_overlap_desc *d, const double *sin_lat_edges, const double *lon_edges,
                                   const int64_t *row_ptr, int32_t *col, double *area, int64_t nnz, dlwpcs_stream_t stream) {
    const int rc = ov_check(d, sin_lat_edges, lon_edges, "overlap_fill");
    if (rc != DLWPCS_OK) return rc;
    if (nnz < 0) return fail(DLWPCS_E_INVALID, "overlap_fill: nnz = %lld", (long long)nnz);
    if (nnz == 0) return DLWPCS_OK;
    if (!row_ptr || !col || !area) return fail(DLWPCS_E_INVALID, "overlap_fill: null pointer");
    const int64_t n = (int64_t)d->n_lat * d->n_lon;
    hipLaunchKernelGGL(overlap_kernel<true>, dim3((unsigned)((n + OV_THREADS - 1) / OV_THREADS)), dim3(OV_THREADS), 0,
                       (hipStream_t)stream, *d, sin_lat_edges, lon_edges, (int32_t *)nullptr, row_ptr, col, area, nnz);
    return check_launch("overlap_fill");
}
