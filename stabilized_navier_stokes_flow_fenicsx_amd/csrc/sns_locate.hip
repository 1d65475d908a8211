// Point location in a tet mesh and P1 evaluation at the located points (row a9: the device side of interpolate.locate_points,
// what DOLFINx' bounding-box tree + Function.eval / interpolate_nonmatching give the reference).
//
// The host function is the specification, ties included.  It is restated step by step so that both paths see the same candidate
// lists:
//   grid     lo / ext / res / h by the host's expression (interpolate.py), evaluated on the host from the exact min / max of the
//            points (k_loc_bounds: a min / max does not depend on the order)
//   build    every tet goes into each bucket its bounding box overlaps, floor((min - lo) / h - 1e-9) .. floor((max - lo) / h + 1e-9)
//            clipped to the grid: count with int32 atomics (k_loc_count), exclusive scan into int64 offsets (the three-launch
//            pattern of sns_aggregate.hip), fill with int32 atomics (k_loc_fill), then every bucket sorted by tet id (k_loc_sort).
//            The sorted lists are what the host's stable argsort gives, so the build is deterministic although the fill is not
//   locate   one lane per query point, its bucket floor((x - lo) / h) clipped to the grid, candidates in list order, barycentric
//            coordinates in fp64 by an explicit 3x3 solve (k_loc_find).  THE SELECTION RULE (interpolate.py's candidate loop):
//              - the chosen tet is the FIRST candidate whose smallest barycentric coordinate is >= -padding;
//              - if no candidate reaches that, the candidate with the LARGEST smallest coordinate, the first one on ties
//                (a strict `>` against the running best; a NaN never wins).
//   miss     a point whose bucket holds no candidate (or none with a comparable coordinate) takes the tet with the nearest
//            centroid over ALL tets, the lowest index on ties (np.argmin): one workgroup per missed point, an argmin reduction
//            ordered by (distance, index) (k_loc_nearest)
//   clamp    lambda clipped to [0, 1] and divided by its sum
// No fused multiply-adds in this file: the grid cells, bucket memberships and centroid distances are then the host's bit for bit
// (the barycentric solve differs from numpy's LU in the last bits, which moves a choice only where two candidates tie to ~1e-16).
// No float atomics.  The locate step is bound by gathers (16 B of connectivity + 96 B of corners per candidate, L2 hits).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "sns_internal.h"

#pragma clang fp contract(off)

namespace sns {

namespace {

constexpr int LOC_TPB = 256;
constexpr int SCAN_ITEMS = 4;                          // per thread: 1024 per block
constexpr int SCAN_BLOCK = LOC_TPB * SCAN_ITEMS;
constexpr int BOUNDS_BLOCKS = 256;
constexpr int SORT_LDS = 2048;                         // a bucket of up to this many entries is ranked from LDS
constexpr int SORT_GRID = 65536;

struct Grid {
    double lo[3], h[3];
    int32_t res[3];
};

inline unsigned loc_blocks(int64_t n) { return (unsigned)((n + LOC_TPB - 1) / LOC_TPB); }

// floor(v) clipped to [0, r - 1]; NaN -> 0 (what astype(int64) + clip gives on the host)
__device__ inline int32_t clip_cell(double v, int32_t r) {
    if (!(v >= 0.0)) return 0;
    if (v > (double)(r - 1)) return r - 1;
    return (int32_t)v;
}

__device__ inline void tet_corners(const double* __restrict__ pts, int4 v, double X[4][3]) {
    const int32_t id[4] = {v.x, v.y, v.z, v.w};
    for (int a = 0; a < 4; ++a)
        for (int d = 0; d < 3; ++d) X[a][d] = pts[3 * (int64_t)id[a] + d];
}

// cells [lo, hi] of the tet's bounding box (interpolate.py: tlo / thi)
__device__ inline void tet_box(const Grid& G, const double X[4][3], int32_t lo[3], int32_t hi[3]) {
    for (int d = 0; d < 3; ++d) {
        const double mn = fmin(fmin(X[0][d], X[1][d]), fmin(X[2][d], X[3][d]));
        const double mx = fmax(fmax(X[0][d], X[1][d]), fmax(X[2][d], X[3][d]));
        lo[d] = clip_cell(floor((mn - G.lo[d]) / G.h[d] - 1e-9), G.res[d]);
        hi[d] = clip_cell(floor((mx - G.lo[d]) / G.h[d] + 1e-9), G.res[d]);
    }
}

__device__ inline int64_t cell_of(const Grid& G, int32_t i, int32_t j, int32_t k) {
    return ((int64_t)i * G.res[1] + j) * G.res[2] + k;
}

// barycentric coordinates of x in the tet with corners X (T lambda_123 = x - X0, T = [X1-X0 | X2-X0 | X3-X0], Cramer's rule)
__device__ inline void bary(const double X[4][3], const double x[3], double lam[4]) {
    const double a0 = X[1][0] - X[0][0], a1 = X[1][1] - X[0][1], a2 = X[1][2] - X[0][2];
    const double b0 = X[2][0] - X[0][0], b1 = X[2][1] - X[0][1], b2 = X[2][2] - X[0][2];
    const double c0 = X[3][0] - X[0][0], c1 = X[3][1] - X[0][1], c2 = X[3][2] - X[0][2];
    const double r0 = x[0] - X[0][0], r1 = x[1] - X[0][1], r2 = x[2] - X[0][2];
    const double bc0 = b1 * c2 - b2 * c1, bc1 = b2 * c0 - b0 * c2, bc2 = b0 * c1 - b1 * c0;
    const double id = 1.0 / (a0 * bc0 + a1 * bc1 + a2 * bc2);
    const double ca0 = c1 * a2 - c2 * a1, ca1 = c2 * a0 - c0 * a2, ca2 = c0 * a1 - c1 * a0;
    const double ab0 = a1 * b2 - a2 * b1, ab1 = a2 * b0 - a0 * b2, ab2 = a0 * b1 - a1 * b0;
    lam[1] = (r0 * bc0 + r1 * bc1 + r2 * bc2) * id;
    lam[2] = (r0 * ca0 + r1 * ca1 + r2 * ca2) * id;
    lam[3] = (r0 * ab0 + r1 * ab1 + r2 * ab2) * id;
    lam[0] = 1.0 - ((lam[1] + lam[2]) + lam[3]);
}

// smallest coordinate, NaN if any is NaN (np.min)
__device__ inline double min4(const double l[4]) {
    if (l[0] != l[0] || l[1] != l[1] || l[2] != l[2] || l[3] != l[3]) return NAN;
    return fmin(fmin(l[0], l[1]), fmin(l[2], l[3]));
}

// clip to [0, 1], divide by the sum (interpolate.py: np.clip + lam /= lam.sum(axis=1))
__device__ inline void store_clamped(const double l[4], double* __restrict__ out) {
    double c[4];
    for (int a = 0; a < 4; ++a) c[a] = fmin(fmax(l[a], 0.0), 1.0);
    const double s = ((c[0] + c[1]) + c[2]) + c[3];
    for (int a = 0; a < 4; ++a) out[a] = c[a] / s;
}

// ---- grid ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LOC_TPB) void k_loc_bounds(int32_t n, const double* __restrict__ pts, double* __restrict__ part) {
    __shared__ double lds[6][LOC_TPB];
    double v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = (int64_t)blockIdx.x * LOC_TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * LOC_TPB)
        for (int d = 0; d < 3; ++d) {
            const double p = pts[3 * i + d];
            v[d] = fmin(v[d], p);
            v[3 + d] = fmax(v[3 + d], p);
        }
    for (int d = 0; d < 6; ++d) lds[d][threadIdx.x] = v[d];
    __syncthreads();
    for (int s = LOC_TPB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int d = 0; d < 6; ++d)
                lds[d][threadIdx.x] = d < 3 ? fmin(lds[d][threadIdx.x], lds[d][threadIdx.x + s])
                                            : fmax(lds[d][threadIdx.x], lds[d][threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x < 6) part[6 * (int64_t)blockIdx.x + threadIdx.x] = lds[threadIdx.x][0];
}

// ---- build -----------------------------------------------------------------------------------------------------------------------
// per bucket the number of tets whose box overlaps it; a node id outside [0, n_nodes) raises *bad and the tet is skipped
__global__ __launch_bounds__(LOC_TPB) void k_loc_count(int32_t n_tets, int32_t n_nodes, Grid G, const double* __restrict__ pts,
                                                       const int4* __restrict__ tets, int32_t* __restrict__ cnt,
                                                       int32_t* __restrict__ bad) {
    const int32_t t = blockIdx.x * LOC_TPB + threadIdx.x;
    if (t >= n_tets) return;
    const int4 v = tets[t];
    if (v.x < 0 || v.y < 0 || v.z < 0 || v.w < 0 || v.x >= n_nodes || v.y >= n_nodes || v.z >= n_nodes || v.w >= n_nodes) {
        atomicOr(bad, 1);
        return;
    }
    double X[4][3];
    tet_corners(pts, v, X);
    int32_t lo[3], hi[3];
    tet_box(G, X, lo, hi);
    for (int32_t i = lo[0]; i <= hi[0]; ++i)
        for (int32_t j = lo[1]; j <= hi[1]; ++j)
            for (int32_t k = lo[2]; k <= hi[2]; ++k) atomicAdd(cnt + cell_of(G, i, j, k), 1);
}

// each tet into its buckets at a slot from the bucket's cursor (any order; k_loc_sort orders the lists)
__global__ __launch_bounds__(LOC_TPB) void k_loc_fill(int32_t n_tets, Grid G, const double* __restrict__ pts,
                                                      const int4* __restrict__ tets, const int64_t* __restrict__ off,
                                                      int32_t* __restrict__ cursor, int32_t* __restrict__ raw) {
    const int32_t t = blockIdx.x * LOC_TPB + threadIdx.x;
    if (t >= n_tets) return;
    double X[4][3];
    tet_corners(pts, tets[t], X);
    int32_t lo[3], hi[3];
    tet_box(G, X, lo, hi);
    for (int32_t i = lo[0]; i <= hi[0]; ++i)
        for (int32_t j = lo[1]; j <= hi[1]; ++j)
            for (int32_t k = lo[2]; k <= hi[2]; ++k) {
                const int64_t c = cell_of(G, i, j, k);
                raw[off[c] + atomicAdd(cursor + c, 1)] = t;
            }
}

// one wave per bucket: every entry goes to its rank among the bucket's (distinct) tet ids -> ascending lists
__global__ __launch_bounds__(64) void k_loc_sort(int32_t ncell, const int64_t* __restrict__ off, const int32_t* __restrict__ raw,
                                                 int32_t* __restrict__ list) {
    __shared__ int32_t s[SORT_LDS];
    for (int32_t c = blockIdx.x; c < ncell; c += gridDim.x) {
        const int64_t b = off[c];
        const int32_t n = (int32_t)(off[c + 1] - b);
        if (n == 0) continue;
        const int32_t* src = raw + b;
        if (n <= SORT_LDS) {
            for (int32_t i = threadIdx.x; i < n; i += 64) s[i] = src[i];
            __syncthreads();
            src = s;
        }
        for (int32_t i = threadIdx.x; i < n; i += 64) {
            const int32_t v = src[i];
            int32_t r = 0;
            for (int32_t j = 0; j < n; ++j) r += src[j] < v;
            list[b + r] = v;
        }
        __syncthreads();
    }
}

// ---- exclusive scan of int32 counts into int64 offsets out[0..n] (out[n] = total), three launches (sns_aggregate.hip's pattern)
__device__ inline int64_t block_exclusive_scan(int64_t v, int64_t* lds, int64_t* total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int o = 1; o < LOC_TPB; o <<= 1) {
        const int64_t add = t >= o ? lds[t - o] : 0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const int64_t incl = lds[t];
    *total = lds[LOC_TPB - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(LOC_TPB) void k_loc_scan_sums(int32_t n, const int32_t* __restrict__ in, int64_t* __restrict__ bsum) {
    __shared__ int64_t lds[LOC_TPB];
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)threadIdx.x * SCAN_ITEMS;
    int64_t v = 0;
    for (int q = 0; q < SCAN_ITEMS; ++q)
        if (base + q < n) v += in[base + q];
    int64_t tot;
    block_exclusive_scan(v, lds, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(LOC_TPB) void k_loc_scan_top(int32_t nb, int64_t* __restrict__ bsum, int32_t n, int64_t* __restrict__ out) {
    __shared__ int64_t lds[LOC_TPB];
    int64_t carry = 0;
    for (int32_t b0 = 0; b0 < nb; b0 += LOC_TPB) {
        const int32_t b = b0 + (int32_t)threadIdx.x;
        const int64_t v = b < nb ? bsum[b] : 0;
        int64_t tot;
        const int64_t ex = block_exclusive_scan(v, lds, &tot);
        if (b < nb) bsum[b] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) out[n] = carry;
}

__global__ __launch_bounds__(LOC_TPB) void k_loc_scan_apply(int32_t n, const int32_t* __restrict__ in, const int64_t* __restrict__ bsum,
                                                            int64_t* __restrict__ out) {
    __shared__ int64_t lds[LOC_TPB];
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)threadIdx.x * SCAN_ITEMS;
    int32_t v[SCAN_ITEMS];
    int64_t sum = 0;
    for (int q = 0; q < SCAN_ITEMS; ++q) {
        v[q] = base + q < n ? in[base + q] : 0;
        sum += v[q];
    }
    int64_t tot;
    int64_t run = bsum[blockIdx.x] + block_exclusive_scan(sum, lds, &tot);
    for (int q = 0; q < SCAN_ITEMS; ++q)
        if (base + q < n) {
            out[base + q] = run;
            run += v[q];
        }
}

// ---- locate ----------------------------------------------------------------------------------------------------------------------
// the selection rule of the header comment; a point without a winner is appended to the miss list (tet -1 until k_loc_nearest)
__global__ __launch_bounds__(LOC_TPB) void k_loc_find(int32_t nq, Grid G, double padding, const double* __restrict__ pts,
                                                      const int4* __restrict__ tets, const int64_t* __restrict__ off,
                                                      const int32_t* __restrict__ list, const double* __restrict__ query,
                                                      int32_t* __restrict__ tet_out, double* __restrict__ lam_out,
                                                      int32_t* __restrict__ miss, int32_t* __restrict__ n_miss) {
    const int32_t q = blockIdx.x * LOC_TPB + threadIdx.x;
    if (q >= nq) return;
    const double x[3] = {query[3 * (int64_t)q], query[3 * (int64_t)q + 1], query[3 * (int64_t)q + 2]};
    int32_t ijk[3];
    for (int d = 0; d < 3; ++d) ijk[d] = clip_cell(floor((x[d] - G.lo[d]) / G.h[d]), G.res[d]);
    const int64_t c = cell_of(G, ijk[0], ijk[1], ijk[2]);
    const int64_t b1 = off[c + 1];
    int32_t best_t = -1;
    double best_m = -INFINITY, best_l[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t k = off[c]; k < b1; ++k) {
        const int32_t t = list[k];
        double X[4][3], lam[4];
        tet_corners(pts, tets[t], X);
        bary(X, x, lam);
        const double mn = min4(lam);
        if (mn > best_m) {
            best_t = t;
            best_m = mn;
            for (int a = 0; a < 4; ++a) best_l[a] = lam[a];
        }
        if (best_m >= -padding) break;
    }
    tet_out[q] = best_t;
    if (best_t < 0) {
        miss[atomicAdd(n_miss, 1)] = q;
        return;
    }
    store_clamped(best_l, lam_out + 4 * (int64_t)q);
}

// centroids as the host's X.mean(axis=1): ((x0 + x1) + x2) + x3, then / 4
__global__ __launch_bounds__(LOC_TPB) void k_loc_centroids(int32_t n_tets, const double* __restrict__ pts, const int4* __restrict__ tets,
                                                           double* __restrict__ cen) {
    const int32_t t = blockIdx.x * LOC_TPB + threadIdx.x;
    if (t >= n_tets) return;
    double X[4][3];
    tet_corners(pts, tets[t], X);
    for (int d = 0; d < 3; ++d) cen[3 * (int64_t)t + d] = (((X[0][d] + X[1][d]) + X[2][d]) + X[3][d]) / 4.0;
}

// one workgroup per missed point: argmin over all tets of ((dx^2 + dy^2) + dz^2), the lowest index on ties
__global__ __launch_bounds__(LOC_TPB) void k_loc_nearest(int32_t n_tets, const int32_t* __restrict__ miss, const double* __restrict__ cen,
                                                         const double* __restrict__ pts, const int4* __restrict__ tets,
                                                         const double* __restrict__ query, int32_t* __restrict__ tet_out,
                                                         double* __restrict__ lam_out) {
    __shared__ double sd[LOC_TPB];
    __shared__ int32_t st[LOC_TPB];
    const int32_t q = miss[blockIdx.x];
    const double x[3] = {query[3 * (int64_t)q], query[3 * (int64_t)q + 1], query[3 * (int64_t)q + 2]};
    double bd = INFINITY;
    int32_t bt = INT32_MAX;
    for (int32_t t = threadIdx.x; t < n_tets; t += LOC_TPB) {
        const double dx = cen[3 * (int64_t)t] - x[0], dy = cen[3 * (int64_t)t + 1] - x[1], dz = cen[3 * (int64_t)t + 2] - x[2];
        const double d = (dx * dx + dy * dy) + dz * dz;
        if (d < bd) { bd = d; bt = t; }                   // ascending t per thread: a strict < keeps the first
    }
    sd[threadIdx.x] = bd;
    st[threadIdx.x] = bt;
    __syncthreads();
    for (int s = LOC_TPB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double d2 = sd[threadIdx.x + s];
            const int32_t t2 = st[threadIdx.x + s];
            if (d2 < sd[threadIdx.x] || (d2 == sd[threadIdx.x] && t2 < st[threadIdx.x])) {
                sd[threadIdx.x] = d2;
                st[threadIdx.x] = t2;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int32_t t = st[0] == INT32_MAX ? 0 : st[0];        // every distance NaN: np.argmin would give 0 as well
        double X[4][3], lam[4];
        tet_corners(pts, tets[t], X);
        bary(X, x, lam);
        tet_out[q] = t;
        store_clamped(lam, lam_out + 4 * (int64_t)q);
    }
}

// ---- evaluate --------------------------------------------------------------------------------------------------------------------
template <int NC>
struct Rec { double v[NC]; };
template <>
struct alignas(32) Rec<4> { double v[4]; };            // [ux, uy, uz, p] of a node: one 32-byte record

// out[q, c] = sum_a lam[q, a] vals[tets[tet[q], a], c]; a tet id outside [0, n_tets) gives NaN
template <int NC>
__global__ __launch_bounds__(LOC_TPB) void k_eval_p1(int32_t nq, int32_t n_tets, const int4* __restrict__ tets,
                                                     const Rec<NC>* __restrict__ vals, const int32_t* __restrict__ tet,
                                                     const double4* __restrict__ lam, double* __restrict__ out) {
    const int32_t q = blockIdx.x * LOC_TPB + threadIdx.x;
    if (q >= nq) return;
    const int32_t t = tet[q];
    double acc[NC];
    if (t < 0 || t >= n_tets) {
        for (int c = 0; c < NC; ++c) acc[c] = NAN;
    } else {
        const int4 v = tets[t];
        const double4 l = lam[q];
        const Rec<NC> r0 = vals[v.x], r1 = vals[v.y], r2 = vals[v.z], r3 = vals[v.w];
        for (int c = 0; c < NC; ++c) acc[c] = ((l.x * r0.v[c] + l.y * r1.v[c]) + l.z * r2.v[c]) + l.w * r3.v[c];
    }
    for (int c = 0; c < NC; ++c) out[NC * (int64_t)q + c] = acc[c];
}

// the host's grid (interpolate.py): ext = max(hi - lo, 1e-300); res = max(1, round((E / 6) ** (1/3) * ext / ext.max() *
// (ext.max() ** 3 / ext.prod()) ** (1/3))); h = ext / res -- the same operations in the same order (numpy's pow is libm's pow)
void host_grid(const double lo[3], const double hi[3], int64_t n_tets, Grid& G, int64_t& ncell) {
    volatile double third = 1.0 / 3.0, three = 3.0;      // keep pow() a libm call
    double ext[3];
    for (int d = 0; d < 3; ++d) ext[d] = std::max(hi[d] - lo[d], 1e-300);
    const double emax = std::max(std::max(ext[0], ext[1]), ext[2]);
    const double a = std::pow((double)n_tets / 6.0, (double)third);
    const double b = std::pow(std::pow(emax, (double)three) / ((ext[0] * ext[1]) * ext[2]), (double)third);
    ncell = 1;
    for (int d = 0; d < 3; ++d) {
        const double r = std::max(1.0, std::nearbyint(a * ext[d] / emax * b));
        G.lo[d] = lo[d];
        G.res[d] = r < 2147483647.0 ? (int32_t)r : 2147483647;
        G.h[d] = ext[d] / (double)G.res[d];
        ncell *= G.res[d];
        if (ncell > 2147483646) ncell = 2147483647;
    }
}

}  // namespace

}  // namespace sns

#define LOC_TRY(expr)                                                                              \
    do {                                                                                           \
        const hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                                    \
            sns::set_error(std::string("sns_locate_points: ") + hipGetErrorString(e_));            \
            return SNS_E_HIP;                                                                      \
        }                                                                                          \
    } while (0)
#define LOC_ALLOC(buf, count)                                                                      \
    do {                                                                                           \
        if ((buf).alloc(count) != SNS_OK) return SNS_E_HIP;                                        \
    } while (0)

extern "C" int sns_locate_points(int32_t n_nodes, int64_t n_tets, const double* pts_dev, const int32_t* tets_dev,
                                 int64_t n_query, const double* query_dev, double padding, int32_t* tet_out_dev,
                                 double* lam_out_dev, int64_t* n_missed_out, void* hip_stream) {
    using namespace sns;
    if (n_tets < 0 || n_tets > INT32_MAX || n_nodes < 0 || n_query < 0 || n_query > INT32_MAX || !(padding >= 0.0)) {
        set_error("sns_locate_points: bad arguments (0 <= n_tets, n_query < 2^31, padding >= 0)");
        return SNS_E_ARG;
    }
    if (n_tets == 0 || n_nodes < 4) {
        set_error("sns_locate_points: the mesh has no tets");
        return SNS_E_MESH;
    }
    if (n_missed_out) *n_missed_out = 0;
    if (n_query == 0) return SNS_OK;
    if (!pts_dev || !tets_dev || !query_dev || !tet_out_dev || !lam_out_dev) {
        set_error("sns_locate_points: null pointer");
        return SNS_E_ARG;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    const int32_t E = (int32_t)n_tets, nq = (int32_t)n_query;
    const int4* tets4 = (const int4*)tets_dev;
    // grid: exact min / max per block on the device, the rest on the host
    const int nbb = (int)std::min<int64_t>(BOUNDS_BLOCKS, (n_nodes + LOC_TPB - 1) / LOC_TPB);
    DevBuf<double> d_part;                              // (device scratch of the call, freed on every return path)
    LOC_ALLOC(d_part, 6 * (size_t)nbb);
    hipLaunchKernelGGL(k_loc_bounds, dim3(nbb), dim3(LOC_TPB), 0, s, n_nodes, pts_dev, d_part);
    std::vector<double> part(6 * (size_t)nbb);
    LOC_TRY(hipMemcpyAsync(part.data(), d_part, part.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    LOC_TRY(hipStreamSynchronize(s));
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = 0; b < nbb; ++b)
        for (int d = 0; d < 3; ++d) {
            lo[d] = std::min(lo[d], part[6 * b + d]);
            hi[d] = std::max(hi[d], part[6 * b + 3 + d]);
        }
    if (!(std::isfinite(lo[0]) && std::isfinite(lo[1]) && std::isfinite(lo[2]) && std::isfinite(hi[0]) && std::isfinite(hi[1]) &&
          std::isfinite(hi[2]))) {
        set_error("sns_locate_points: the mesh has non-finite coordinates");
        return SNS_E_MESH;
    }
    Grid G;
    int64_t ncell;
    host_grid(lo, hi, n_tets, G, ncell);
    if (ncell >= INT32_MAX) {
        set_error("sns_locate_points: bucket grid too large");
        return SNS_E_ARG;
    }
    const int32_t nc = (int32_t)ncell;
    // build: count, scan, fill, sort
    DevBuf<int32_t> d_cnt, d_bad;
    DevBuf<int64_t> d_off, d_bsum;
    const int32_t nsb = (nc + SCAN_BLOCK - 1) / SCAN_BLOCK;
    LOC_ALLOC(d_cnt, (size_t)nc);
    LOC_ALLOC(d_bad, 1);
    LOC_ALLOC(d_off, (size_t)nc + 1);
    LOC_ALLOC(d_bsum, (size_t)nsb);
    LOC_TRY(hipMemsetAsync(d_cnt, 0, (size_t)nc * sizeof(int32_t), s));
    LOC_TRY(hipMemsetAsync(d_bad, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_loc_count, dim3(loc_blocks(E)), dim3(LOC_TPB), 0, s, E, n_nodes, G, pts_dev, tets4, d_cnt, d_bad);
    hipLaunchKernelGGL(k_loc_scan_sums, dim3(nsb), dim3(LOC_TPB), 0, s, nc, d_cnt, d_bsum);
    hipLaunchKernelGGL(k_loc_scan_top, dim3(1), dim3(LOC_TPB), 0, s, nsb, d_bsum, nc, d_off);
    hipLaunchKernelGGL(k_loc_scan_apply, dim3(nsb), dim3(LOC_TPB), 0, s, nc, d_cnt, d_bsum, d_off);
    LOC_TRY(hipGetLastError());
    int64_t total = 0;
    int32_t bad = 0;
    LOC_TRY(hipMemcpyAsync(&total, d_off + nc, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    LOC_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    LOC_TRY(hipStreamSynchronize(s));
    if (bad) {
        set_error("sns_locate_points: a tet names a node outside [0, n_nodes)");
        return SNS_E_MESH;
    }
    DevBuf<int32_t> d_raw, d_list, d_miss, d_nmiss;
    LOC_ALLOC(d_raw, (size_t)total);
    LOC_ALLOC(d_list, (size_t)total);
    LOC_ALLOC(d_miss, (size_t)nq);
    LOC_ALLOC(d_nmiss, 1);
    LOC_TRY(hipMemsetAsync(d_cnt, 0, (size_t)nc * sizeof(int32_t), s));
    LOC_TRY(hipMemsetAsync(d_nmiss, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_loc_fill, dim3(loc_blocks(E)), dim3(LOC_TPB), 0, s, E, G, pts_dev, tets4, d_off, d_cnt, d_raw);
    hipLaunchKernelGGL(k_loc_sort, dim3(std::min(nc, SORT_GRID)), dim3(64), 0, s, nc, d_off, d_raw, d_list);
    // locate
    hipLaunchKernelGGL(k_loc_find, dim3(loc_blocks(nq)), dim3(LOC_TPB), 0, s, nq, G, padding, pts_dev, tets4, d_off, d_list,
                       query_dev, tet_out_dev, lam_out_dev, d_miss, d_nmiss);
    LOC_TRY(hipGetLastError());
    int32_t n_miss = 0;
    LOC_TRY(hipMemcpyAsync(&n_miss, d_nmiss, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    LOC_TRY(hipStreamSynchronize(s));
    if (n_miss > 0) {
        DevBuf<double> d_cen;
        LOC_ALLOC(d_cen, 3 * (size_t)E);
        hipLaunchKernelGGL(k_loc_centroids, dim3(loc_blocks(E)), dim3(LOC_TPB), 0, s, E, pts_dev, tets4, d_cen);
        hipLaunchKernelGGL(k_loc_nearest, dim3(n_miss), dim3(LOC_TPB), 0, s, E, d_miss, d_cen, pts_dev, tets4, query_dev,
                           tet_out_dev, lam_out_dev);
        LOC_TRY(hipGetLastError());
        LOC_TRY(hipStreamSynchronize(s));
    }
    if (n_missed_out) *n_missed_out = n_miss;
    return SNS_OK;
}

extern "C" int sns_eval_p1(int64_t n_tets, const int32_t* tets_dev, int32_t ncomp, const double* vals_dev, int64_t n_query,
                           const int32_t* tet_dev, const double* lam_dev, double* out_dev, void* hip_stream) {
    using namespace sns;
    if (n_tets < 0 || n_tets > INT32_MAX || ncomp < 1 || ncomp > 4 || n_query < 0 || n_query > INT32_MAX) {
        set_error("sns_eval_p1: bad arguments (1 <= ncomp <= 4, 0 <= n_tets, n_query < 2^31)");
        return SNS_E_ARG;
    }
    if (n_tets == 0) {
        set_error("sns_eval_p1: the mesh has no tets");
        return SNS_E_MESH;
    }
    if (n_query == 0) return SNS_OK;
    if (!tets_dev || !vals_dev || !tet_dev || !lam_dev || !out_dev) {
        set_error("sns_eval_p1: null pointer");
        return SNS_E_ARG;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    const int32_t nq = (int32_t)n_query, E = (int32_t)n_tets;
    const int4* t4 = (const int4*)tets_dev;
    const double4* l4 = (const double4*)lam_dev;
    const dim3 g(loc_blocks(nq)), b(LOC_TPB);
    switch (ncomp) {
        case 1: hipLaunchKernelGGL(k_eval_p1<1>, g, b, 0, s, nq, E, t4, (const Rec<1>*)vals_dev, tet_dev, l4, out_dev); break;
        case 2: hipLaunchKernelGGL(k_eval_p1<2>, g, b, 0, s, nq, E, t4, (const Rec<2>*)vals_dev, tet_dev, l4, out_dev); break;
        case 3: hipLaunchKernelGGL(k_eval_p1<3>, g, b, 0, s, nq, E, t4, (const Rec<3>*)vals_dev, tet_dev, l4, out_dev); break;
        default: hipLaunchKernelGGL(k_eval_p1<4>, g, b, 0, s, nq, E, t4, (const Rec<4>*)vals_dev, tet_dev, l4, out_dev); break;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        set_error(std::string("sns_eval_p1: ") + hipGetErrorString(e));
        return SNS_E_HIP;
    }
    return SNS_OK;
}
