// Bilinear sampling weights of points on the dual mesh of an equiangular cubed sphere, fp64 (the numpy twin is
// DLWP/remap/bilinear.py, which states the maths).  The dual mesh has the cell centres as vertices and great-circle arcs between
// them as sides: per cube face the (N-1)^2 quadrilaterals of neighbouring centres (coordinate rectangles of the face: a line of
// constant equiangular coordinate is a great circle), per cube edge a strip of N-1 quadrilaterals made of the border cells k, k+1
// and the cells facing them across the edge, per cube vertex the triangle of the three corner cells.
//     quadrilateral V0..V3:  (1-s)(1-t) V0 + s(1-t) V1 + s t V2 + (1-s) t V3 = lambda P, weights = the four bilinear factors
//     triangle V0..V2:       sum b_k V_k = lambda P, sum b_k = 1 (Cramer)
// Along a side the weights depend on the side's two ends only, so the interpolant is continuous over the sphere.
//
// One lane owns one point.  It takes the face whose centre is nearest.  Inside the rectangle of that face's centres the
// quadrilateral follows from the fractional cell coordinates.  Outside, the rungs of the edge strip (border cell -> facing cell)
// are not coordinate lines of either face: the lane walks the strip from the cell its along-edge coordinate names by the sign of
// P . (V_in x V_out), at most N + 1 steps and never back, and a point beyond the last rung of the strips it could belong to is in the corner
// triangle.  (s, t) come from a fixed number of Newton steps on the two components of the defining equation orthogonal to P.
//
// fp64 VALU and libm, nothing bound by memory: two loads and eight stores per lane.  The face frames and the edge table are read
// from the kernel arguments at a lane-dependent face; no per-lane array is indexed at run time, so nothing lives in scratch.
#include "common.h"

namespace dlwpcs {

namespace {

constexpr int BL_THREADS = 256;
constexpr int BL_NEWTON_STEPS = 12;              // DLWP/remap/bilinear.py NEWTON_STEPS
constexpr double BL_PI = 3.14159265358979323846;
constexpr int BL_MAX_N = 16384;                  // 6 N^2 < 2^31
constexpr double BL_FRAME_TOL = 1e-9;

struct BlVec {
    double x, y, z;
};

__device__ __forceinline__ BlVec bl_row(const dlwpcs_cube_bilinear_desc &d, int f, int r) {
    return BlVec{d.frames[f][r][0], d.frames[f][r][1], d.frames[f][r][2]};
}
__device__ __forceinline__ double bl_dot(const BlVec &a, const BlVec &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ BlVec bl_cross(const BlVec &a, const BlVec &b) {
    return BlVec{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double bl_det(const BlVec &a, const BlVec &b, const BlVec &c) { return bl_dot(a, bl_cross(b, c)); }
__device__ __forceinline__ BlVec bl_sub(const BlVec &a, const BlVec &b) { return BlVec{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ BlVec bl_scale(const BlVec &a, double s) { return BlVec{a.x * s, a.y * s, a.z * s}; }

// the centre of cell (i, j) of face f
__device__ __forceinline__ BlVec bl_centre(const dlwpcs_cube_bilinear_desc &d, int f, int i, int j, double h) {
    const double ta = tan(-BL_PI / 4 + (j + 0.5) * h), tb = tan(-BL_PI / 4 + (i + 0.5) * h);
    const BlVec e0 = bl_row(d, f, 0), eu = bl_row(d, f, 1), ev = bl_row(d, f, 2);
    const BlVec p{e0.x + ta * eu.x + tb * ev.x, e0.y + ta * eu.y + tb * ev.y, e0.z + ta * eu.z + tb * ev.z};
    const double nrm = sqrt(bl_dot(p, p));
    return BlVec{p.x / nrm, p.y / nrm, p.z / nrm};
}

// border cell k along a side (0 west: j = 0, 1 east: j = N - 1, 2 south: i = 0, 3 north: i = N - 1)
__device__ __forceinline__ void bl_border(int side, int k, int N, int &i, int &j) {
    i = side == 2 ? 0 : (side == 3 ? N - 1 : k);
    j = side == 0 ? 0 : (side == 1 ? N - 1 : k);
}

// the cell that faces border cell k of (f, side) across the cube edge
__device__ __forceinline__ void bl_facing(const dlwpcs_cube_bilinear_desc &d, int f, int side, int k, int N, int &g, int &i, int &j) {
    g = d.edge[f][side][0];
    const int t = d.edge[f][side][1], rev = d.edge[f][side][2];
    bl_border(t, rev ? N - 1 - k : k, N, i, j);
}

struct BlRung {
    BlVec vi, vo;
    int ci, co;
};

__device__ __forceinline__ BlRung bl_rung(const dlwpcs_cube_bilinear_desc &d, int f, int side, int m, int N, double h) {
    int i, j, g, io, jo;
    bl_border(side, m, N, i, j);
    bl_facing(d, f, side, m, N, g, io, jo);
    BlRung r;
    r.vi = bl_centre(d, f, i, j, h);
    r.vo = bl_centre(d, g, io, jo, h);
    r.ci = (f * N + i) * N + j;
    r.co = (g * N + io) * N + jo;
    return r;
}

__global__ void __launch_bounds__(BL_THREADS) cube_bilinear_kernel(const dlwpcs_cube_bilinear_desc d, const double *__restrict__ lat_deg,
                                                                   const double *__restrict__ lon_deg, int32_t *__restrict__ col,
                                                                   double *__restrict__ w) {
    const int64_t r = (int64_t)blockIdx.x * BL_THREADS + threadIdx.x;
    if (r >= d.n_points) return;
    const int N = d.N;
    const int n_cells = 6 * N * N;
    const double lat = lat_deg[r], lon = lon_deg[r];
    int32_t *cr = col + 4 * r;
    double *wr = w + 4 * r;
    if (!(isfinite(lat) && isfinite(lon))) {                        // a point that cannot be placed: cell 0, NaN weights
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cr[k] = 0;
            wr[k] = NAN;
        }
        return;
    }
    BlVec P;
    {
        double lo = fmod(lon, 360.0);
        if (lo < 0.0) lo += 360.0;
        const double la = lat * (BL_PI / 180), lr = lo * (BL_PI / 180);
        const double c = cos(la);
        P = BlVec{c * cos(lr), c * sin(lr), sin(la)};
    }
    const double h = BL_PI / (2 * N);
    int f = 0;
    {
        double best = -INFINITY;
        for (int g = 0; g < 6; ++g) {                               // (g is uniform: scalar loads)
            const double v = bl_dot(P, bl_row(d, g, 0));
            if (v > best) {
                best = v;
                f = g;
            }
        }
    }
    const BlVec e0 = bl_row(d, f, 0), eu = bl_row(d, f, 1), ev = bl_row(d, f, 2);
    const double p0 = bl_dot(P, e0);
    const double a = (atan2(bl_dot(P, eu), p0) + BL_PI / 4) / h - 0.5;      // width, in cells from the first centre
    const double b = (atan2(bl_dot(P, ev), p0) + BL_PI / 4) / h - 0.5;      // height
    const double top = (double)(N - 1);

    BlVec V0, V1, V2, V3;
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    double s = 0.0, t = 0.0;
    int kind = -1;                                                  // 0: quadrilateral, 1: triangle
    if (N >= 2 && a >= 0.0 && a <= top && b >= 0.0 && b <= top) {
        const int j0 = (int)fmin(fmax(floor(a), 0.0), (double)(N - 2)), i0 = (int)fmin(fmax(floor(b), 0.0), (double)(N - 2));
        V0 = bl_centre(d, f, i0, j0, h);
        V1 = bl_centre(d, f, i0, j0 + 1, h);
        V2 = bl_centre(d, f, i0 + 1, j0 + 1, h);
        V3 = bl_centre(d, f, i0 + 1, j0, h);
        c0 = (f * N + i0) * N + j0;
        c1 = c0 + 1;
        c2 = c0 + N + 1;
        c3 = c0 + N;
        s = a - j0;
        t = b - i0;
        kind = 0;
    } else if (N >= 2) {
        for (int side = 0; side < 4 && kind < 0; ++side) {
            const bool beyond = side == 0 ? a < 0.0 : (side == 1 ? a > top : (side == 2 ? b < 0.0 : b > top));
            if (!beyond) continue;
            const double c = side < 2 ? b : a;
            const BlVec along = side < 2 ? ev : eu;
            const BlVec outward = bl_scale(side < 2 ? eu : ev, (side & 1) ? 1.0 : -1.0);
            const double sgn = bl_det(along, e0, outward);          // orientation of a rung's triple product (mirrored grids)
            int k = (int)fmin(fmax(floor(c), 0.0), (double)(N - 2));
            bool ok = false;
            int dir = 0;                                            // the walk never turns back: a point on a rung, whose side
            for (int it = 0; it <= N; ++it) {                       // may read differently from below and from above, stays put
                const BlRung lo = bl_rung(d, f, side, k, N, h);
                if (dir <= 0 && sgn * bl_det(P, lo.vi, lo.vo) < 0.0) {
                    dir = -1;
                    if (--k < 0) break;
                    continue;
                }
                const BlRung hi = bl_rung(d, f, side, k + 1, N, h);
                if (dir >= 0 && sgn * bl_det(P, hi.vi, hi.vo) > 0.0) {
                    dir = 1;
                    if (++k > N - 2) break;
                    continue;
                }
                V0 = lo.vi;
                V1 = lo.vo;
                V2 = hi.vo;
                V3 = hi.vi;
                c0 = lo.ci;
                c1 = lo.co;
                c2 = hi.co;
                c3 = hi.ci;
                ok = true;
                break;
            }
            if (ok) {
                s = 0.25;
                t = fmin(fmax(c - k, 0.0), 1.0);
                kind = 0;
            }
        }
    }
    double w0, w1, w2, w3;
    if (kind == 0) {
        // two unit vectors that span the plane orthogonal to P: along P x (the axis of P's smallest component) and P x that
        int ax = 0;
        double small = fabs(P.x);
        if (fabs(P.y) < small) {
            small = fabs(P.y);
            ax = 1;
        }
        if (fabs(P.z) < small) ax = 2;
        BlVec u1 = ax == 0 ? BlVec{0.0, P.z, -P.y} : (ax == 1 ? BlVec{-P.z, 0.0, P.x} : BlVec{P.y, -P.x, 0.0});
        const double nrm = sqrt(bl_dot(u1, u1));
        u1 = BlVec{u1.x / nrm, u1.y / nrm, u1.z / nrm};
        const BlVec u2 = bl_cross(P, u1);
        const BlVec B = bl_sub(V1, V0), C = bl_sub(V3, V0);
        const BlVec D{V0.x - V1.x + V2.x - V3.x, V0.y - V1.y + V2.y - V3.y, V0.z - V1.z + V2.z - V3.z};
        const double a1 = bl_dot(V0, u1), b1 = bl_dot(B, u1), g1 = bl_dot(C, u1), d1 = bl_dot(D, u1);
        const double a2 = bl_dot(V0, u2), b2 = bl_dot(B, u2), g2 = bl_dot(C, u2), d2 = bl_dot(D, u2);
        for (int it = 0; it < BL_NEWTON_STEPS; ++it) {
            const double F1 = a1 + s * b1 + t * g1 + s * t * d1;
            const double F2 = a2 + s * b2 + t * g2 + s * t * d2;
            const double j11 = b1 + t * d1, j12 = g1 + s * d1, j21 = b2 + t * d2, j22 = g2 + s * d2;
            const double det = j11 * j22 - j12 * j21;
            const double ds = (F1 * j22 - F2 * j12) / det, dt = (F2 * j11 - F1 * j21) / det;
            s -= ds;
            t -= dt;
        }
        s = fmin(fmax(s, 0.0), 1.0);
        t = fmin(fmax(t, 0.0), 1.0);
        w0 = (1.0 - s) * (1.0 - t);
        w1 = s * (1.0 - t);
        w2 = s * t;
        w3 = (1.0 - s) * t;
    } else {
        // the corner of the face the point is nearest to: this face's corner cell and the two cells facing it
        const int sa = a < 0.5 * top ? 0 : 1, sb = b < 0.5 * top ? 2 : 3;
        const int ka = sa == 0 ? 0 : N - 1, kb = sb == 2 ? 0 : N - 1;
        int g2, i2, j2, g3, i3, j3;
        bl_facing(d, f, sa, kb, N, g2, i2, j2);
        bl_facing(d, f, sb, ka, N, g3, i3, j3);
        V0 = bl_centre(d, f, kb, ka, h);
        V1 = bl_centre(d, g2, i2, j2, h);
        V2 = bl_centre(d, g3, i3, j3, h);
        c0 = (f * N + kb) * N + ka;
        c1 = (g2 * N + i2) * N + j2;
        c2 = (g3 * N + i3) * N + j3;
        c3 = c2;
        const double vol = bl_det(V0, V1, V2);
        const double q0 = fmax(bl_det(P, V1, V2) / vol, 0.0), q1 = fmax(bl_det(V0, P, V2) / vol, 0.0),
                     q2 = fmax(bl_det(V0, V1, P) / vol, 0.0);
        const double sum = q0 + q1 + q2;
        w0 = q0 / sum;
        w1 = q1 / sum;
        w2 = q2 / sum;
        w3 = 0.0;
    }
    // whatever the descriptor's edge table holds, a cell index is written inside [0, 6 N^2)
    cr[0] = min(max(c0, 0), n_cells - 1);
    cr[1] = min(max(c1, 0), n_cells - 1);
    cr[2] = min(max(c2, 0), n_cells - 1);
    cr[3] = min(max(c3, 0), n_cells - 1);
    wr[0] = w0;
    wr[1] = w1;
    wr[2] = w2;
    wr[3] = w3;
}

}  // namespace

}  // namespace dlwpcs

using namespace dlwpcs;

extern "C" int dlwpcs_cube_bilinear(const dlwpcs_cube_bilinear_desc *d, const double *lat_deg, const double *lon_deg, int32_t *col,
                                    double *w, dlwpcs_stream_t stream) {
    if (!d) return fail(DLWPCS_E_INVALID, "cube_bilinear: null descriptor");
    if (d->N < 1 || d->N > BL_MAX_N) return fail(DLWPCS_E_INVALID, "cube_bilinear: N = %d must lie in [1, %d]", d->N, BL_MAX_N);
    if (d->n_points < 0) return fail(DLWPCS_E_INVALID, "cube_bilinear: n_points = %lld", (long long)d->n_points);
    for (int f = 0; f < 6; ++f)
        for (int p = 0; p < 3; ++p)
            for (int q = p; q < 3; ++q) {
                double dot = 0.0;
                for (int k = 0; k < 3; ++k) dot += d->frames[f][p][k] * d->frames[f][q][k];
                if (!(fabs(dot - (p == q ? 1.0 : 0.0)) <= BL_FRAME_TOL))
                    return fail(DLWPCS_E_INVALID, "cube_bilinear: the frame of face %d is not orthonormal", f);
            }
    for (int f = 0; f < 6; ++f)
        for (int s = 0; s < 4; ++s) {
            const int32_t *e = d->edge[f][s];
            if (e[0] < 0 || e[0] > 5 || e[1] < 0 || e[1] > 3 || e[2] < 0 || e[2] > 1)
                return fail(DLWPCS_E_INVALID, "cube_bilinear: edge[%d][%d] = {%d, %d, %d} is out of range", f, s, e[0], e[1], e[2]);
        }
    if (d->n_points == 0) return DLWPCS_OK;
    if (!lat_deg || !lon_deg || !col || !w) return fail(DLWPCS_E_INVALID, "cube_bilinear: null pointer");
    const int64_t blocks = (d->n_points + BL_THREADS - 1) / BL_THREADS;
    if (blocks >= (1ll << 31)) return fail(DLWPCS_E_UNSUPPORTED, "cube_bilinear: %lld points", (long long)d->n_points);
    hipLaunchKernelGGL(cube_bilinear_kernel, dim3((unsigned)blocks), dim3(BL_THREADS), 0, (hipStream_t)stream, *d, lat_deg, lon_deg,
                       col, w);
    return check_launch("cube_bilinear");
}
