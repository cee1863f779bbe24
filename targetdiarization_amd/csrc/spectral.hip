// spectral.hip — the dense linear algebra of spectral clustering on MI355X: the part of clustering.spectral_labels that grows as
// n^3.  Two stateless entries, everything in fp64, no floating-point atomics, every reduction in a fixed order, so
// a call returns the same bits every time.  No kernel waits for another workgroup: what one step needs from all workgroups of the
// step before it crosses a launch boundary.
//
// tdx_spectral_laplacian      emb [n,d] f32 -> L [n,n] f64, five launches:
//     spec_aff_unit_kernel    one wave per row: u = x / max(|x|, 1e-12)
//     spec_aff_gemm_kernel    A = U U^T, 64 x 64 tiles, 4 x 4 per thread, k ascending (fma commutes: A is symmetric to the bit)
//     spec_prune_kernel       one workgroup per row, the row as order-preserving 64-bit keys in LDS; radix select (8 passes of
//                             8 bits, integer histogram) finds the key of rank drop - 1, equal keys go by column index: what
//                             np.argsort(kind="stable")[:, :drop] names is set to 0
//     spec_lap_sym_kernel     pairs of 32 x 32 tiles through LDS: L = -(A + A^T) / 2, diagonal 0, in place
//     spec_lap_diag_kernel    one workgroup per row: L[i][i] = -(sum of the row)
// tdx_symeig_lowest           M [n,n] symmetric -> the m lowest eigenpairs, about 2 n + 4 launches:
//     spec_tri_p_kernel       step k, launch (a): every workgroup rebuilds the reflector of row k (= column k: the trailing matrix is
//                             kept symmetric to the bit) and computes its rows of p = tau S v; workgroup 0 stores e_k, tau_k, the scale
//     spec_tri_update_kernel  step k, launch (b): every workgroup recomputes v.p, w = p - (tau v.p / 2) v, S -= v w^T + w v^T
//                             (LAPACK dsytd2, unblocked).  v stays where it was: row k right of the diagonal, times the stored scale
//     spec_tri_gather_kernel  d_i = M[i][i], e_i^2
//     spec_bis_kernel         one lane per eigenvalue: Gershgorin interval, bisection on Sturm counts with dstebz' pivmin rule
//     spec_inv_kernel         one workgroup: the m shifted tridiagonals are factored (partial pivoting, dgttrf) and solved in
//                             lock-step, one lane each; after every solve modified Gram-Schmidt against the earlier vectors
//     spec_back_kernel        one workgroup per eigenvector, the vector in LDS: reflectors n-3 .. 0
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <string>

#include "../../include/tdx.h"
#include "tdx_common.hpp"

using namespace tdx;

namespace {

constexpr int MAX_N = 8192, MAX_M = 16;
constexpr int NT = 256, NW = NT / 64;
constexpr int TRI_ROWS = 4;                  // rows of the trailing matrix per workgroup (one per wave)
constexpr int BIS_ITERS = 128;               // the interval halves each time: 2^-128 of Gershgorin's width is below any fp64 spacing that matters
constexpr int INV_ITERS = 5;
constexpr double EPS = 2.220446049250313e-16;        // LAPACK's ulp (dlamch('P'))

struct Ws {
    size_t U, d, e, e2, tau, scale, p, scal, fac, total;
};
// fac: 7 planes of [n][MAX_M] doubles — multipliers, three diagonals of U, the pivot flags, and two vectors
constexpr int FAC_PLANES = 7;
Ws ws_plan(int n, int d) {
    auto a = [](size_t b) { return (b + 255) / 256 * 256; };
    Ws w{};
    size_t o = 0;
    w.U = o; o += a((size_t)n * d * 8);
    w.d = o; o += a((size_t)n * 8);
    w.e = o; o += a((size_t)n * 8);
    w.e2 = o; o += a((size_t)n * 8);
    w.tau = o; o += a((size_t)n * 8);
    w.scale = o; o += a((size_t)n * 8);
    w.p = o; o += a((size_t)n * 8);
    w.scal = o; o += 256;                              // [0] |T| (Gershgorin), [1] pivmin
    w.fac = o; o += a((size_t)FAC_PLANES * n * MAX_M * 8);
    w.total = o;
    return w;
}

// the sum over the workgroup, the same bits in every thread and in every workgroup that sums the same values
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sh[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) s += sh[w];
    __syncthreads();
    return s;
}

// ---------------------------------------------------------------------------------------------------------------- affinity
__global__ __launch_bounds__(NT) void spec_aff_unit_kernel(const float* __restrict__ x, int n, int d, double* __restrict__ U) {
    const int row = blockIdx.x * NW + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    const float* xr = x + (size_t)row * d;
    double ss = 0.0;
    for (int j = lane; j < d; j += 64) { const double v = (double)xr[j]; ss = fma(v, v, ss); }
    ss = wave_sum(ss);
    const double nrm = fmax(sqrt(ss), 1e-12);
    for (int j = lane; j < d; j += 64) U[(size_t)row * d + j] = (double)xr[j] / nrm;
}

__global__ __launch_bounds__(NT) void spec_aff_gemm_kernel(const double* __restrict__ U, int n, int d, double* __restrict__ A, double* __restrict__ tap) {
    __shared__ double As[16][65], Bs[16][65];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    double acc[4][4] = {};
    for (int k0 = 0; k0 < d; k0 += 16) {
        for (int q = threadIdx.x; q < 64 * 16; q += NT) {
            const int r = q >> 4, k = q & 15;
            const bool kin = k0 + k < d;
            As[k][r] = (kin && i0 + r < n) ? U[(size_t)(i0 + r) * d + k0 + k] : 0.0;
            Bs[k][r] = (kin && j0 + r < n) ? U[(size_t)(j0 + r) * d + k0 + k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            double a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { a[r] = As[k][ty * 4 + r]; b[r] = Bs[k][tx * 4 + r]; }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fma(a[r], b[c], acc[r][c]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + ty * 4 + r;
        if (i >= n) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + tx * 4 + c;
            if (j >= n) continue;
            A[(size_t)i * n + j] = acc[r][c];
            if (tap) tap[(size_t)i * n + j] = acc[r][c];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- pruning
// ascending unsigned order of the keys = ascending order of the doubles; -0.0 counts as +0.0, as it does for numpy's sort
__device__ __forceinline__ unsigned long long order_key(double v) {
    if (v == 0.0) v = 0.0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ __launch_bounds__(NT) void spec_prune_kernel(double* __restrict__ A, int n, int drop) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long* keys = (unsigned long long*)smem;              // [n]
    unsigned int* hist = (unsigned int*)(keys + n);                    // [256]
    __shared__ unsigned int sh_bin, sh_rank, sh_eq;
    __shared__ int sh_cut;
    double* row = A + (size_t)blockIdx.x * n;
    for (int i = threadIdx.x; i < n; i += NT) keys[i] = order_key(row[i]);
    if (threadIdx.x == 0) { sh_rank = (unsigned)(drop - 1); sh_cut = n; }
    unsigned long long prefix = 0, mask = 0;
    for (int pass = 7; pass >= 0; --pass) {
        hist[threadIdx.x] = 0;                                         // NT == 256 bins
        __syncthreads();
        const int sh = pass * 8;
        for (int i = threadIdx.x; i < n; i += NT) {
            const unsigned long long k = keys[i];
            if ((k & mask) == prefix) atomicAdd(&hist[(unsigned)(k >> sh) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int rank = sh_rank, b = 0;
            while (b < 255 && rank >= hist[b]) { rank -= hist[b]; ++b; }
            sh_bin = b; sh_rank = rank; sh_eq = hist[b];
        }
        __syncthreads();
        prefix |= (unsigned long long)sh_bin << sh;
        mask |= 0xffull << sh;
        __syncthreads();                                               // sh_bin is read before the next pass rewrites it
    }
    // prefix is the key of rank drop - 1; sh_rank + 1 of the sh_eq keys equal to it go, those of the lowest column index
    const unsigned int need = sh_rank + 1;
    if (need < sh_eq && threadIdx.x < 64) {
        const int lane = threadIdx.x;
        unsigned int run = 0;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            const bool eq = i < n && keys[i] == prefix;
            const unsigned long long m = __ballot(eq);
            const unsigned int c = (unsigned)__popcll(m);
            if (run + c >= need) {
                const unsigned int before = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
                if (eq && run + before + 1 == need) sh_cut = i;
                break;
            }
            run += c;
        }
    }
    __syncthreads();
    const int cut = sh_cut;
    for (int i = threadIdx.x; i < n; i += NT) {
        const unsigned long long k = keys[i];
        if (k < prefix || (k == prefix && i <= cut)) row[i] = 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- Laplacian
__global__ __launch_bounds__(NT) void spec_lap_sym_kernel(double* __restrict__ A, int n) {
    __shared__ double T1[32][33], T2[32][33];
    const int bx = blockIdx.x, by = blockIdx.y;
    if (bx < by) return;
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    for (int r = r0; r < 32; r += 8) {
        const int i1 = by * 32 + r, j1 = bx * 32 + c, i2 = bx * 32 + r, j2 = by * 32 + c;
        T1[r][c] = (i1 < n && j1 < n) ? A[(size_t)i1 * n + j1] : 0.0;
        T2[r][c] = (i2 < n && j2 < n) ? A[(size_t)i2 * n + j2] : 0.0;
    }
    __syncthreads();
    for (int r = r0; r < 32; r += 8) {
        const int i1 = by * 32 + r, j1 = bx * 32 + c, i2 = bx * 32 + r, j2 = by * 32 + c;
        if (i1 < n && j1 < n) A[(size_t)i1 * n + j1] = i1 == j1 ? 0.0 : 0.0 - 0.5 * (T1[r][c] + T2[c][r]);
        if (i2 < n && j2 < n) A[(size_t)i2 * n + j2] = i2 == j2 ? 0.0 : 0.0 - 0.5 * (T2[r][c] + T1[c][r]);
    }
}

__global__ __launch_bounds__(NT) void spec_lap_diag_kernel(double* __restrict__ L, int n) {
    __shared__ double sh[NW];
    double* row = L + (size_t)blockIdx.x * n;
    double s = 0.0;
    for (int j = threadIdx.x; j < n; j += NT) s += row[j];            // the diagonal is 0 here
    s = block_sum(s, sh);
    if (threadIdx.x == 0) row[blockIdx.x] = 0.0 - s;
}

// ---------------------------------------------------------------------------------------------------------------- tridiagonalisation
// element j of the reflector of step k (v_0 = 1), x = row k from column k + 1 on
__device__ __forceinline__ double refl(const double* __restrict__ x, int j, double sc) { return j == 0 ? 1.0 : x[j] * sc; }

__global__ __launch_bounds__(NT) void spec_tri_p_kernel(const double* __restrict__ M, int n, int k, double* __restrict__ p, double* __restrict__ e,
                                                        double* __restrict__ tau, double* __restrict__ scale) {
    __shared__ double sh[NW];
    const double* x = M + (size_t)k * n + (k + 1);
    const int len = n - k - 1;
    double ss = 0.0;
    for (int j = 1 + threadIdx.x; j < len; j += NT) ss = fma(x[j], x[j], ss);
    ss = block_sum(ss, sh);
    const double alpha = x[0];
    double beta = alpha, t = 0.0, sc = 0.0;
    if (ss != 0.0) {                                   // nothing below the subdiagonal: H = I, the step is skipped
        beta = -copysign(sqrt(fma(alpha, alpha, ss)), alpha);
        t = (beta - alpha) / beta;
        sc = 1.0 / (alpha - beta);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { e[k] = beta; tau[k] = t; scale[k] = sc; }
    if (t == 0.0) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = 0; r < TRI_ROWS / NW; ++r) {
        const int ii = blockIdx.x * TRI_ROWS + wave * (TRI_ROWS / NW) + r;     // row of the trailing matrix
        if (ii >= len) break;
        const double* row = M + (size_t)(k + 1 + ii) * n + (k + 1);
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;      // four loads in flight per lane; the order is fixed all the same
        int j = lane;
        for (; j + 192 < len; j += 256) {
            a0 = fma(row[j], refl(x, j, sc), a0);
            a1 = fma(row[j + 64], refl(x, j + 64, sc), a1);
            a2 = fma(row[j + 128], refl(x, j + 128, sc), a2);
            a3 = fma(row[j + 192], refl(x, j + 192, sc), a3);
        }
        for (; j < len; j += 64) a0 = fma(row[j], refl(x, j, sc), a0);
        double acc = wave_sum((a0 + a1) + (a2 + a3));
        if (lane == 0) p[k + 1 + ii] = t * acc;
    }
}

// s - (vi wj + wi vj) with both products rounded on their own: the same bits for (i, j) and (j, i)
__device__ __forceinline__ double rank2(double s, double vi, double wi, double vj, double wj) {
#pragma clang fp contract(off)
    const double a = vi * wj, b = wi * vj;
    return s - (a + b);
}

__global__ __launch_bounds__(NT) void spec_tri_update_kernel(double* __restrict__ M, int n, int k, const double* __restrict__ p,
                                                             const double* __restrict__ tau, const double* __restrict__ scale) {
    __shared__ double sh[NW];
    const double t = tau[k];
    if (t == 0.0) return;
    const double sc = scale[k];
    const double* x = M + (size_t)k * n + (k + 1);
    const double* pp = p + (k + 1);
    const int len = n - k - 1;
    double vp = 0.0;
    for (int j = threadIdx.x; j < len; j += NT) vp = fma(refl(x, j, sc), pp[j], vp);
    vp = block_sum(vp, sh);
    const double a2 = -0.5 * t * vp;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = 0; r < TRI_ROWS / NW; ++r) {
        const int ii = blockIdx.x * TRI_ROWS + wave * (TRI_ROWS / NW) + r;
        if (ii >= len) break;
        double* row = M + (size_t)(k + 1 + ii) * n + (k + 1);
        const double vi = refl(x, ii, sc), wi = fma(a2, vi, pp[ii]);
#pragma unroll 4
        for (int j = lane; j < len; j += 64) {
            const double vj = refl(x, j, sc), wj = fma(a2, vj, pp[j]);
            row[j] = rank2(row[j], vi, wi, vj, wj);
        }
    }
}

__global__ __launch_bounds__(NT) void spec_tri_gather_kernel(const double* __restrict__ M, int n, double* __restrict__ d, double* __restrict__ e,
                                                             double* __restrict__ e2) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    d[i] = M[(size_t)i * n + i];
    if (i == n - 1) e[i] = 0.0;
    const double ei = i == n - 1 ? 0.0 : e[i];
    e2[i] = ei * ei;
}

// ---------------------------------------------------------------------------------------------------------------- bisection
// eigenvalues of T that are <= x (dstebz: a pivot within pivmin of 0 becomes -pivmin)
__device__ __forceinline__ int sturm_count(const double* __restrict__ d, const double* __restrict__ e2, int n, double x, double pivmin) {
    double q = d[0] - x;
    if (fabs(q) <= pivmin) q = -pivmin;
    int c = q <= 0.0 ? 1 : 0;
#pragma unroll 8
    for (int i = 1; i < n; ++i) {
        q = d[i] - e2[i - 1] / q - x;
        if (fabs(q) <= pivmin) q = -pivmin;
        c += q <= 0.0 ? 1 : 0;
    }
    return c;
}

__global__ __launch_bounds__(64) void spec_bis_kernel(const double* __restrict__ d, const double* __restrict__ e, const double* __restrict__ e2,
                                                      int n, int m, double* __restrict__ w, double* __restrict__ scal) {
    __shared__ double sw[MAX_M];
    double gl = d[0], gu = d[0], emax2 = 0.0;
    for (int i = 0; i < n; ++i) {
        const double r = (i > 0 ? fabs(e[i - 1]) : 0.0) + (i < n - 1 ? fabs(e[i]) : 0.0);
        gl = fmin(gl, d[i] - r);
        gu = fmax(gu, d[i] + r);
        emax2 = fmax(emax2, e2[i]);
    }
    const double tnorm = fmax(fabs(gl), fabs(gu));
    const double pivmin = DBL_MIN * fmax(1.0, emax2);
    if (threadIdx.x == 0) { scal[0] = tnorm; scal[1] = pivmin; }
    const int j = threadIdx.x;
    if (j < m) {
        double lo = 0.0, hi = 0.0;
        if (tnorm != 0.0) {
            const double slack = 2.1 * tnorm * EPS * n + 4.2 * pivmin;
            lo = gl - slack; hi = gu + slack;            // count(lo) = 0, count(hi) = n
            for (int it = 0; it < BIS_ITERS; ++it) {
                const double mid = 0.5 * (lo + hi);
                if (mid == lo || mid == hi) break;
                if (sturm_count(d, e2, n, mid, pivmin) >= j + 1) hi = mid; else lo = mid;
            }
        }
        sw[j] = 0.5 * (lo + hi);
    }
    __syncthreads();
    if (j == 0) {                                        // ascending, whatever the counts did at the last bit
        for (int a = 1; a < m; ++a) {
            const double v = sw[a];
            int b = a - 1;
            while (b >= 0 && sw[b] > v) { sw[b + 1] = sw[b]; --b; }
            sw[b + 1] = v;
        }
        for (int a = 0; a < m; ++a) w[a] = sw[a];
    }
}

// ---------------------------------------------------------------------------------------------------------------- inverse iteration
// start vector: a fixed function of (row, vector) in [-1, 1), never 0
__device__ __forceinline__ double start_value(int i, int j) {
    unsigned int h = (unsigned)i * 0x9E3779B1u + (unsigned)j * 0x85EBCA77u + 0x165667B1u;
    h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
    return ((double)(h | 1u) - 2147483648.0) / 2147483648.0;
}

__global__ __launch_bounds__(NT) void spec_inv_kernel(const double* __restrict__ d, const double* __restrict__ e, int n, int m,
                                                      const double* __restrict__ w, const double* __restrict__ scal, double* __restrict__ fac) {
    __shared__ double sh[NW];
    __shared__ double shift[MAX_M];
    const size_t plane = (size_t)n * MAX_M;
    double* Lm = fac;                 // multipliers
    double* U0 = fac + plane;         // diagonal of U
    double* U1 = fac + 2 * plane;
    double* U2 = fac + 3 * plane;
    double* Pv = fac + 4 * plane;     // 1.0: rows i and i + 1 were interchanged
    double* Z = fac + 5 * plane;      // right-hand side / result [n][MAX_M]
    double* Y = fac + 6 * plane;
    const double tnorm = scal[0];
    const int t = threadIdx.x;
    if (tnorm == 0.0) {               // M = 0: the first m unit vectors
        for (int q = t; q < n * MAX_M; q += NT) Z[q] = (q / MAX_M == q % MAX_M) ? 1.0 : 0.0;
        return;
    }
    const double tiny = EPS * tnorm, pertol = 10.0 * EPS * tnorm;
    if (t == 0) {
        for (int j = 0; j < m; ++j) {
            double xj = w[j];
            if (j > 0 && xj - shift[j - 1] < pertol) xj = shift[j - 1] + pertol;
            shift[j] = xj;
        }
    }
    for (int q = t; q < n * MAX_M; q += NT) Z[q] = start_value(q / MAX_M, q % MAX_M);
    __syncthreads();
    if (t < m) {                      // T - shift = L U with partial pivoting, a zero pivot becomes eps |T|
        const double x = shift[t];
        double dc = d[0] - x, uc = n > 1 ? e[0] : 0.0;
        for (int i = 0; i < n - 1; ++i) {
            const size_t o = (size_t)i * MAX_M + t;
            const double sub = e[i], nd = d[i + 1] - x, nu = i + 2 < n ? e[i + 1] : 0.0;
            if (fabs(dc) >= fabs(sub)) {
                const double mult = dc != 0.0 ? sub / dc : 0.0;
                Lm[o] = mult; Pv[o] = 0.0; U0[o] = dc != 0.0 ? dc : tiny; U1[o] = uc; U2[o] = 0.0;
                dc = nd - mult * uc; uc = nu;
            } else {
                const double mult = dc / sub;
                Lm[o] = mult; Pv[o] = 1.0; U0[o] = sub; U1[o] = nd; U2[o] = nu;
                dc = uc - mult * nd; uc = -mult * nu;
            }
        }
        U0[(size_t)(n - 1) * MAX_M + t] = dc != 0.0 ? dc : tiny;
    }
    __syncthreads();
    for (int it = 0; it < INV_ITERS; ++it) {
        if (t < m) {
            double yc = Z[t];
            for (int i = 0; i < n - 1; ++i) {
                const size_t o = (size_t)i * MAX_M + t;
                const double bn = Z[o + MAX_M], mult = Lm[o];
                if (Pv[o] == 0.0) { Y[o] = yc; yc = bn - mult * yc; }
                else { Y[o] = bn; yc = yc - mult * bn; }
            }
            Y[(size_t)(n - 1) * MAX_M + t] = yc;
            double z1 = 0.0, z2 = 0.0;                    // z[i + 1], z[i + 2]
            for (int i = n - 1; i >= 0; --i) {
                const size_t o = (size_t)i * MAX_M + t;
                double v = Y[o];
                if (i < n - 1) v -= U1[o] * z1 + U2[o] * z2;
                v /= U0[o];
                Z[o] = v;
                z2 = z1; z1 = v;
            }
        }
        __threadfence_block();
        __syncthreads();
        for (int j = 0; j < m; ++j) {                     // modified Gram-Schmidt: vector j against 0 .. j-1 of this sweep, then unit length
            for (int i = 0; i < j; ++i) {
                double s = 0.0;
                for (int r = t; r < n; r += NT) s = fma(Z[(size_t)r * MAX_M + i], Z[(size_t)r * MAX_M + j], s);
                s = block_sum(s, sh);
                for (int r = t; r < n; r += NT) Z[(size_t)r * MAX_M + j] -= s * Z[(size_t)r * MAX_M + i];
            }
            double s = 0.0;
            for (int r = t; r < n; r += NT) { const double v = Z[(size_t)r * MAX_M + j]; s = fma(v, v, s); }
            s = block_sum(s, sh);
            const double inv = s > 0.0 ? 1.0 / sqrt(s) : 0.0;
            for (int r = t; r < n; r += NT) Z[(size_t)r * MAX_M + j] *= inv;
        }
        __threadfence_block();
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- back-transformation
__global__ __launch_bounds__(NT) void spec_back_kernel(const double* __restrict__ M, int n, int m, const double* __restrict__ tau,
                                                       const double* __restrict__ scale, const double* __restrict__ Z, double* __restrict__ V) {
    extern __shared__ __align__(16) unsigned char smem[];
    double* z = (double*)smem;                            // [n]
    __shared__ double sh[NW];
    const int col = blockIdx.x, t = threadIdx.x;
    for (int i = t; i < n; i += NT) z[i] = Z[(size_t)i * MAX_M + col];
    __syncthreads();
    for (int k = n - 3; k >= 0; --k) {
        const double tk = tau[k];
        if (tk == 0.0) continue;
        const double sc = scale[k];
        const double* x = M + (size_t)k * n + (k + 1);
        // a thread keeps the rows i = t (mod NT) for every k, so only the sum crosses threads
        double s = 0.0;
        for (int i = t; i < n; i += NT)
            if (i > k) s = fma(refl(x, i - k - 1, sc), z[i], s);
        s = block_sum(s, sh);
        const double f = tk * s;
        for (int i = t; i < n; i += NT)
            if (i > k) z[i] -= f * refl(x, i - k - 1, sc);
    }
    for (int i = t; i < n; i += NT) V[(size_t)i * m + col] = z[i];
}

template <typename K>
int allow_lds(K kernel, size_t bytes) {
    if (bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return fail_hip(e, __FILE__, __LINE__);
    }
    return TDX_OK;
}

}  // namespace

extern "C" {

size_t tdx_spectral_workspace_bytes(int n, int d, int m) {
    if (n < 1 || n > MAX_N || d < 1 || d > 65536 || m < 1 || m > MAX_M || m > n) return 0;
    return ws_plan(n, d).total;
}

int tdx_spectral_laplacian(const float* emb_dev, int n, int d, int drop, double* L_dev, double* A_tap_dev, void* ws_, size_t ws_bytes, void* stream) {
    if (!emb_dev || !L_dev || !ws_) return fail(TDX_E_INVALID, "tdx_spectral_laplacian: null argument");
    if (n < 1 || n > MAX_N) return fail(TDX_E_INVALID, "tdx_spectral_laplacian: n must be in [1, 8192]");
    if (d < 1 || d > 65536) return fail(TDX_E_INVALID, "tdx_spectral_laplacian: d must be in [1, 65536]");
    if (drop < 0 || drop >= n) return fail(TDX_E_INVALID, "tdx_spectral_laplacian: drop must be in [0, n)");
    const Ws w = ws_plan(n, d);
    if (ws_bytes < w.total) return fail(TDX_E_WORKSPACE, "tdx_spectral_laplacian: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    double* U = (double*)((char*)ws_ + w.U);
    hipLaunchKernelGGL(spec_aff_unit_kernel, dim3((n + NW - 1) / NW), dim3(NT), 0, st, emb_dev, n, d, U);
    LAUNCH_CHECK();
    const int t64 = (n + 63) / 64, t32 = (n + 31) / 32;
    hipLaunchKernelGGL(spec_aff_gemm_kernel, dim3(t64, t64), dim3(NT), 0, st, U, n, d, L_dev, A_tap_dev);
    LAUNCH_CHECK();
    if (drop > 0) {
        const size_t lds = (size_t)n * 8 + 256 * 4;
        TRY(allow_lds(spec_prune_kernel, lds + 64));
        hipLaunchKernelGGL(spec_prune_kernel, dim3(n), dim3(NT), lds, st, L_dev, n, drop);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(spec_lap_sym_kernel, dim3(t32, t32), dim3(NT), 0, st, L_dev, n);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(spec_lap_diag_kernel, dim3(n), dim3(NT), 0, st, L_dev, n);
    LAUNCH_CHECK();
    return TDX_OK;
}

int tdx_symeig_lowest(double* M_dev, int n, int m, double* w_dev, double* V_dev, void* ws_, size_t ws_bytes, void* stream) {
    if (!M_dev || !w_dev || !V_dev || !ws_) return fail(TDX_E_INVALID, "tdx_symeig_lowest: null argument");
    if (n < 1 || n > MAX_N) return fail(TDX_E_INVALID, "tdx_symeig_lowest: n must be in [1, 8192]");
    if (m < 1 || m > MAX_M || m > n) return fail(TDX_E_INVALID, "tdx_symeig_lowest: m must be in [1, min(n, 16)]");
    const Ws w = ws_plan(n, 1);
    if (ws_bytes < w.total) return fail(TDX_E_WORKSPACE, "tdx_symeig_lowest: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws_;
    double *dd = (double*)(base + w.d), *ee = (double*)(base + w.e), *e2 = (double*)(base + w.e2), *tau = (double*)(base + w.tau);
    double *scale = (double*)(base + w.scale), *p = (double*)(base + w.p), *scal = (double*)(base + w.scal), *fac = (double*)(base + w.fac);
    for (int k = 0; k + 1 < n; ++k) {
        const int grid = (n - k - 1 + TRI_ROWS - 1) / TRI_ROWS;
        hipLaunchKernelGGL(spec_tri_p_kernel, dim3(grid), dim3(NT), 0, st, M_dev, n, k, p, ee, tau, scale);
        LAUNCH_CHECK();
        if (k + 2 < n) {
            hipLaunchKernelGGL(spec_tri_update_kernel, dim3(grid), dim3(NT), 0, st, M_dev, n, k, p, tau, scale);
            LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(spec_tri_gather_kernel, dim3((n + NT - 1) / NT), dim3(NT), 0, st, M_dev, n, dd, ee, e2);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(spec_bis_kernel, dim3(1), dim3(64), 0, st, dd, ee, e2, n, m, w_dev, scal);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(spec_inv_kernel, dim3(1), dim3(NT), 0, st, dd, ee, n, m, w_dev, scal, fac);
    LAUNCH_CHECK();
    const size_t lds = (size_t)n * 8;
    TRY(allow_lds(spec_back_kernel, lds + 64));
    hipLaunchKernelGGL(spec_back_kernel, dim3(m), dim3(NT), lds, st, M_dev, n, m, tau, scale, fac + 5 * (size_t)n * MAX_M, V_dev);
    LAUNCH_CHECK();
    return TDX_OK;
}

}  // extern "C"
