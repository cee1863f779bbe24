// fft.hpp — a complex / real FFT of any length on MI355X, and the band mix of AudioProcessor.mix_audio_by_freq on top of it
// (DESIGN 8.27).  Kernels, the pass planner and the drivers; the C-ABI entry points are in fft.hip, the small-tile test hook in
// diag.hip.  Layout: complex64, re / im interleaved, [batch][n].  numpy's conventions: forward unnormalised, inverse scaled 1 / n.
//
// Power of two, M = 2^m.  Stockham autosort over mixed large radices: M = R_1 R_2 .. R_p, one pass per factor.  Pass i, with
// Ns = R_1 .. R_(i-1) and column j < M / R_i:
//     v[r] = in[j + r M / R_i] W^((j mod Ns) r),  W = exp(-+ 2 pi i / (Ns R_i));   V = DFT_(R_i)(v);
//     out[(j / Ns) Ns R_i + (j mod Ns) + r Ns] = V[r].
// A workgroup takes a bundle of B adjacent columns: every global read is a run of B complex (128 bytes at B = 16), the R_i-point
// transforms of the bundle run in LDS (the same Stockham recursion with radix-4 butterflies in registers and a radix-2 step when
// log2 R_i is odd, in place: every thread holds its butterflies across a barrier), and the results leave LDS in the order of their
// global addresses, in runs of B complex or, while Ns < B, as one contiguous block of B R_i — the transposition of the four-step
// scheme goes through LDS, never through a strided global store.  M <= tile is one pass with B = 1, R = M.  For M = R_1 R_2 this is
// the four-step FFT (column transforms, transposition, twiddle, column transforms of the transposed array); more factors apply
// it again.  Every pass reads the data once and writes it once.
//
// Twiddles.  Exponents are reduced in 64-bit integers first.  Inside a tile the fraction e / (Ns rad) has a power-of-two
// denominator <= tile and is exact in fp32: sincospif of it.  Between passes the denominator D = Ns R_i goes up to 2^27: up to
// 2^24 e / D is still exact; beyond, e = eh 2^12 + el, both fractions are exact and the two roots are multiplied.
//
// Any other n: Bluestein.  c[k] = exp(i pi k^2 / n) with k^2 mod 2n in 64-bit integers, evaluated in fp64 (sincospi) and rounded
// once; X = conj(c) IFFT_M(FFT_M(x conj(c)) FFT_M(c wrapped)), M the power of two >= 2n - 1.  The chirp and its spectrum are built
// in the caller's workspace on every call: no handle, no allocation, nothing but kernel launches on the caller's stream.
// Up to DIRECT_MAX = 64 points such a length is the DFT sum itself, roots and sum in fp64, and the band mix of so short a clip runs
// in fp64 throughout (both rounded once at the end).
//
// No atomics; a workgroup never depends on the batch size, so row b of a batch equals a call with that row alone bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "tdx_common.hpp"

namespace tdx {
namespace fft {

constexpr int THREADS = 256;
constexpr int MAX_TILE_LOG2 = 12;         // the in-place LDS stages keep at most 2^12 / (4 * 256) radix-4 butterflies per thread
constexpr int MIN_TILE_LOG2 = 4;
constexpr long MAX_N = 1L << 26;          // so that Bluestein's M <= 2^27
constexpr int MAX_BATCH = 65535;
constexpr int MAX_PASSES = 12;

// ---------------------------------------------------------------------------------------------------------------- the planner
struct Plan {
    int m;                    // log2 M
    int npass;
    int logB;                 // log2 of the columns per workgroup (0 for the single pass)
    int logR[MAX_PASSES];     // log2 of the radix of every pass, sum = m
};

// B = min(16, tile / 8) columns per workgroup, so R <= tile / B; the bits are spread evenly over the fewest passes
inline Plan plan_pow2(int m, int tile_log2) {
    Plan p{};
    p.m = m;
    if (m <= tile_log2) {
        p.npass = 1; p.logB = 0; p.logR[0] = m;
        return p;
    }
    p.logB = std::min(4, tile_log2 - 3);
    const int rb = tile_log2 - p.logB;
    p.npass = (m + rb - 1) / rb;
    for (int i = 0; i < p.npass; ++i) p.logR[i] = m / p.npass + (i < m % p.npass ? 1 : 0);
    return p;
}

inline bool is_pow2(long n) { return n > 0 && (n & (n - 1)) == 0; }
inline int ilog2(long n) { int l = 0; while ((1L << l) < n) ++l; return l; }      // ceil(log2 n)
inline int bluestein_m(long n) { return ilog2(2 * n - 1); }                        // log2 of the power of two >= 2n - 1

// ---------------------------------------------------------------------------------------------------------------- device helpers
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cconj(float2 a) { return make_float2(a.x, -a.y); }

// exp(sign 2 pi i e / 2^logD), 0 <= e < 2^logD <= 2^27
__device__ __forceinline__ float2 root(long e, int logD, int sign) {
    float s, c;
    if (logD <= 24) {
        sincospif((float)sign * 2.0f * ((float)e / (float)(1L << logD)), &s, &c);
        return make_float2(c, s);
    }
    const long eh = e >> 12, el = e & 4095;
    float s2, c2;
    sincospif((float)sign * 2.0f * ((float)eh / (float)(1L << (logD - 12))), &s, &c);
    sincospif((float)sign * 2.0f * ((float)el / (float)(1L << logD)), &s2, &c2);
    return cmul(make_float2(c, s), make_float2(c2, s2));
}

// Where element i of a tile lives in LDS: one float2 of padding after every 32.  The stores of a pass read the tile with r
// fastest, a stride of B float2; without the padding 64 lanes would meet in two banks.
__device__ __forceinline__ int lds_at(int i) { return i + (i >> 5); }
inline size_t lds_bytes(int tile_log2) { return sizeof(float2) * ((size_t)(1 << tile_log2) + ((size_t)(1 << tile_log2) >> 5) + 1); }

// One Stockham stage of radix RAD over the R-point transforms of the B columns held in s[r * B + col], in place.
template <int RAD>
__device__ __forceinline__ void lds_stage(float2* s, int logR, int logB, int logNs, int sign) {
    constexpr int ITERS = (1 << MAX_TILE_LOG2) / RAD / THREADS;
    const int B = 1 << logB, Ns = 1 << logNs, cnt = (1 << (logR + logB)) / RAD, q4 = (1 << logR) / RAD;
    float2 v[ITERS][RAD];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int idx = (int)threadIdx.x + it * THREADS;
        if (idx < cnt) {
            const int col = idx & (B - 1), q = idx >> logB, k = q & (Ns - 1);
#pragma unroll
            for (int t = 0; t < RAD; ++t) v[it][t] = s[lds_at(((q + t * q4) << logB) + col)];
            if (k != 0) {
#pragma unroll
                for (int t = 1; t < RAD; ++t) {
                    float sn, cs;                // k t / (Ns RAD) < 1 with a power-of-two denominator <= tile: exact in fp32
                    sincospif((float)sign * 2.0f * ((float)(k * t) / (float)(Ns * RAD)), &sn, &cs);
                    v[it][t] = cmul(v[it][t], make_float2(cs, sn));
                }
            }
            if constexpr (RAD == 4) {
                const float2 t0 = make_float2(v[it][0].x + v[it][2].x, v[it][0].y + v[it][2].y);
                const float2 t1 = make_float2(v[it][0].x - v[it][2].x, v[it][0].y - v[it][2].y);
                const float2 t2 = make_float2(v[it][1].x + v[it][3].x, v[it][1].y + v[it][3].y);
                const float2 t3 = make_float2(v[it][1].x - v[it][3].x, v[it][1].y - v[it][3].y);
                // forward: X1 = t1 - i t3, X3 = t1 + i t3; inverse the other way round
                const float2 jt3 = sign < 0 ? make_float2(t3.y, -t3.x) : make_float2(-t3.y, t3.x);
                v[it][0] = make_float2(t0.x + t2.x, t0.y + t2.y);
                v[it][2] = make_float2(t0.x - t2.x, t0.y - t2.y);
                v[it][1] = make_float2(t1.x + jt3.x, t1.y + jt3.y);
                v[it][3] = make_float2(t1.x - jt3.x, t1.y - jt3.y);
            } else {
                const float2 a = v[it][0], b = v[it][RAD - 1];
                v[it][0] = make_float2(a.x + b.x, a.y + b.y);
                v[it][RAD - 1] = make_float2(a.x - b.x, a.y - b.y);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int idx = (int)threadIdx.x + it * THREADS;
        if (idx < cnt) {
            const int col = idx & (B - 1), q = idx >> logB, k = q & (Ns - 1);
            const int base = (q - k) * RAD + k;
#pragma unroll
            for (int t = 0; t < RAD; ++t) s[lds_at(((base + t * Ns) << logB) + col)] = v[it][t];
        }
    }
    __syncthreads();
}

// One pass (see the head of the file).  grid (M / R / B, batch), THREADS threads, lds_bytes(log2(B R)) of dynamic LDS.
// mul (or null): the input is multiplied by mul[index] first (the product of the two spectra in Bluestein's convolution; one row,
// shared by the batch) — only the first pass of a transform is given one.
__global__ __launch_bounds__(THREADS) void fft_pass_kernel(const float2* __restrict__ in, float2* __restrict__ out, const float2* __restrict__ mul,
                                                           int m, int logR, int logNs, int logB, int sign, float scale) {
    extern __shared__ float2 fft_lds[];
    float2* s = fft_lds;
    const long M = 1L << m, row = (long)blockIdx.y * M;
    const long j0 = (long)blockIdx.x << logB;
    const int B = 1 << logB, R = 1 << logR, tile = R << logB;
    const int logS = m - logR;                      // the stride between the elements of a column: M / R
    for (int e = (int)threadIdx.x; e < tile; e += THREADS) {
        const int col = e & (B - 1), r = e >> logB;
        const long j = j0 + col, at = j + ((long)r << logS);
        float2 v = in[row + at];
        if (mul) v = cmul(v, mul[at]);
        if (logNs > 0 && r != 0) {
            const long k = j & ((1L << logNs) - 1);
            if (k != 0) v = cmul(v, root(k * r, logNs + logR, sign));
        }
        s[lds_at(e)] = v;
    }
    __syncthreads();
    int ns = 0;
    for (; ns + 2 <= logR; ns += 2) lds_stage<4>(s, logR, logB, ns, sign);
    if (ns < logR) lds_stage<2>(s, logR, logB, ns, sign);
    // results in the order of their addresses: g = min(Ns, B) adjacent columns, then r, then the column groups
    const int logG = logNs < logB ? logNs : logB;
    for (int e = (int)threadIdx.x; e < tile; e += THREADS) {
        const int jl = e & ((1 << logG) - 1), r = (e >> logG) & (R - 1), jh = e >> (logG + logR);
        const int col = (jh << logG) + jl;
        const long j = j0 + col, k = j & ((1L << logNs) - 1);
        const float2 v = s[lds_at((r << logB) + col)];
        out[row + ((j - k) << logR) + k + ((long)r << logNs)] = make_float2(v.x * scale, v.y * scale);
    }
}

// ---- Bluestein
// c[k] = exp(i pi k^2 / n), k < n, and its wrapped form over M points: bw[j] = c[j] (j < n), c[M - j] (M - j < n), else 0
__global__ void chirp_kernel(long n, long M, float2* __restrict__ c, float2* __restrict__ bw) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    const long k = j < n ? j : (M - j < n ? M - j : -1);
    float2 v = make_float2(0.f, 0.f);
    if (k >= 0) {
        const long e = (k * k) % (2 * n);           // k < 2^26: k^2 < 2^52
        double sn, cs;
        sincospi((double)e / (double)n, &sn, &cs);
        v = make_float2((float)cs, (float)sn);
    }
    bw[j] = v;
    if (j < n) c[j] = v;
}

enum { SRC_CPLX = 0, SRC_REAL = 1, SRC_TWO_REAL = 2, SRC_HERM = 3 };
// what a transform reads: complex [batch][n]; real [batch][n]; a + i b of two real clips (batch 1); or the n / 2 + 1 bins of a
// Hermitian spectrum [batch][n / 2 + 1] extended to n bins, the imaginary part of bin 0 (and of bin n / 2, n even) dropped
struct Src { int mode; const float* a; const float* b; };
__device__ __forceinline__ float2 src_load(const Src& s, long n, long row, long k) {
    switch (s.mode) {
    case SRC_CPLX: return ((const float2*)s.a)[row * n + k];
    case SRC_REAL: return make_float2(s.a[row * n + k], 0.f);
    case SRC_TWO_REAL: return make_float2(s.a[k], s.b[k]);
    default: {
        const long nb = n / 2 + 1, kk = k < nb ? k : n - k;
        float2 v = ((const float2*)s.a)[row * nb + kk];
        if (kk == 0 || 2 * kk == n) v.y = 0.f;
        return k < nb ? v : cconj(v);
    }
    }
}

// a[k] = x[k] conj(c[k]) (inverse: conj(x[k]) conj(c[k])) for k < n, zero up to M
__global__ void bluestein_in_kernel(Src src, long n, long M, int inverse, const float2* __restrict__ c, float2* __restrict__ a) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x, row = blockIdx.y;
    if (k >= M) return;
    float2 v = make_float2(0.f, 0.f);
    if (k < n) {
        v = src_load(src, n, row, k);
        if (inverse) v.y = -v.y;
        v = cmul(v, cconj(c[k]));
    }
    a[row * M + k] = v;
}

// X[k] = conj(c[k]) conv[k], k < nout (inverse: its conjugate, times scale); real != 0 stores the real parts alone
__global__ void bluestein_out_kernel(const float2* __restrict__ conv, long n, long M, long nout, int inverse, float scale, const float2* __restrict__ c,
                                     float* __restrict__ out, int real) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x, row = blockIdx.y;
    if (k >= nout) return;
    float2 v = cmul(conv[row * M + k], cconj(c[k]));
    if (inverse) v.y = -v.y;
    if (real) out[row * nout + k] = v.x * scale;
    else ((float2*)out)[row * nout + k] = make_float2(v.x * scale, v.y * scale);
}

// Lengths up to DIRECT_MAX that are no power of two: the DFT sum itself, roots and sum in fp64, rounded once.  Three float32
// transforms of 2n - 1 .. 4n points would cost more there and lose to the exact small butterflies of a mixed-radix library.
constexpr long DIRECT_MAX = 64;
// cos and sin of 2 pi e / n, 0 <= e < n, in fp64; multiples of a quarter turn and the values +-1/2 (multiples of pi / 6) are exact,
// which e / n as a double cannot promise
__device__ __forceinline__ void root64(long e, long n, double* cs, double* sn) {
    if ((4 * e) % n == 0) {
        const long q = 4 * e / n;
        *cs = q == 0 ? 1.0 : q == 2 ? -1.0 : 0.0;
        *sn = q == 1 ? 1.0 : q == 3 ? -1.0 : 0.0;
        return;
    }
    sincospi(2.0 * (double)e / (double)n, sn, cs);
    if (fabs(fabs(*cs) - 0.5) < 1e-12) *cs = copysign(0.5, *cs);
    if (fabs(fabs(*sn) - 0.5) < 1e-12) *sn = copysign(0.5, *sn);
}
// bin k of the DFT of n <= DIRECT_MAX points of `src`, fp64.  The samples j and n - j share one root and its conjugate:
// x_j w + x_(n-j) conj(w) = (x_j + x_(n-j)) cos -+ i (x_j - x_(n-j)) sin, so what cancels in the input cancels exactly.
__device__ __forceinline__ void dft_bin64(const Src& src, long n, long row, long k, int inverse, double* ore, double* oim) {
    const float2 x0 = src_load(src, n, row, 0);
    double re = x0.x, im = x0.y;
    const double sg = inverse ? -1.0 : 1.0;
    for (long j = 1; 2 * j < n; ++j) {
        const float2 a = src_load(src, n, row, j), b = src_load(src, n, row, n - j);
        const double sr = (double)a.x + b.x, si = (double)a.y + b.y, dr = (double)a.x - b.x, di = (double)a.y - b.y;
        double cs, sn;
        root64((j * k) % n, n, &cs, &sn);
        re += sr * cs + sg * sn * di;                  // -i sg (dr + i di) sin = sg sin (di - i dr)
        im += si * cs - sg * sn * dr;
    }
    if (n % 2 == 0) {
        const float2 m = src_load(src, n, row, n / 2);
        const double s = (k & 1) ? -1.0 : 1.0;
        re += s * m.x; im += s * m.y;
    }
    *ore = re; *oim = im;
}
__global__ void direct_dft_kernel(Src src, long n, long nout, int inverse, double scale, float* __restrict__ out, int real) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x, row = blockIdx.y;
    if (k >= nout) return;
    double re, im;
    dft_bin64(src, n, row, k, inverse, &re, &im);
    if (real) out[row * nout + k] = (float)(re * scale);
    else ((float2*)out)[row * nout + k] = make_float2((float)(re * scale), (float)(im * scale));
}

__global__ void interleave_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, float2* __restrict__ z) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) z[k] = make_float2(a[k], b[k]);
}

// ---- real transforms of even n through h = n / 2 complex points
// after Z = DFT_h(x[2j] + i x[2j + 1]):  X[k] = (Z[k] + conj Z[h - k]) / 2 + exp(-2 pi i k / n) (Z[k] - conj Z[h - k]) / 2i, k <= h
__global__ void r2c_split_kernel(const float2* __restrict__ Z, long h, float2* __restrict__ X) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x, row = blockIdx.y;
    if (k > h) return;
    const float2 a = Z[row * h + (k == h ? 0 : k)], b = cconj(Z[row * h + (k == 0 ? 0 : h - k)]);
    const double er = 0.5 * ((double)a.x + b.x), ei = 0.5 * ((double)a.y + b.y);
    const double dr = 0.5 * ((double)a.x - b.x), di = 0.5 * ((double)a.y - b.y);      // O = d / i = (di, -dr)
    double sn, cs;
    sincospi(-(double)k / (double)h, &sn, &cs);
    X[row * (h + 1) + k] = make_float2((float)(er + (cs * di + sn * dr)), (float)(ei + (sn * di - cs * dr)));
}

// before z = IDFT_h(Z'):  Z'[k] = E[k] + i O[k],  E = (X[k] + conj X[h - k]) / 2,  O = exp(2 pi i k / n) (X[k] - conj X[h - k]) / 2
__device__ __forceinline__ float2 c2r_merge(float2 a, float2 xb, long k, long h) {
    const float2 b = cconj(xb);
    const double er = 0.5 * ((double)a.x + b.x), ei = 0.5 * ((double)a.y + b.y);
    const double dr = 0.5 * ((double)a.x - b.x), di = 0.5 * ((double)a.y - b.y);
    double sn, cs;
    sincospi((double)k / (double)h, &sn, &cs);
    const double o_r = cs * dr - sn * di, o_i = cs * di + sn * dr;
    return make_float2((float)(er - o_i), (float)(ei + o_r));
}
__global__ void c2r_merge_kernel(const float2* __restrict__ X, long h, float2* __restrict__ Zp) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x, row = blockIdx.y;
    if (k >= h) return;
    float2 a = X[row * (h + 1) + k], b = X[row * (h + 1) + h - k];
    if (k == 0) { a.y = 0.f; b.y = 0.f; }
    Zp[row * h + k] = c2r_merge(a, b, k, h);
}

// ---- the band mix (AudioProcessor.mix_audio_by_freq): from Z = DFT_n(main + i aux) to the input of the inverse of m = 2 (n / 2)
// points.  rg: main, aux, overlap bin ranges [lo, hi).  Written in the reference's order main, aux, overlap; a bin in no range is 0.
struct MixRanges { long lo[3], hi[3]; };
struct MixBin { float2 fm, fa, mix; };
// the mixed bin k from the two spectra's bins, in fp64
__device__ __forceinline__ void mix_select(long k, const MixRanges& rg, double fmr, double fmi, double far_, double fai, double* mr, double* mi) {
    *mr = 0.0; *mi = 0.0;
    if (k >= rg.lo[0] && k < rg.hi[0]) { *mr = fmr; *mi = fmi; }
    if (k >= rg.lo[1] && k < rg.hi[1]) { *mr = far_; *mi = fai; }
    if (k >= rg.lo[2] && k < rg.hi[2]) {
        const long cnt = rg.hi[2] - rg.lo[2], j = k - rg.lo[2];
        // np.linspace(1, 0, cnt): j * step + 1 with step = -1 / (cnt - 1) in fp64, the last one exactly 0; [1.0] for cnt == 1
        double w = 1.0;
        if (cnt > 1) w = j == cnt - 1 ? 0.0 : (double)j * (-1.0 / (double)(cnt - 1)) + 1.0;
        const double wa = 1.0 - w;
        *mr = fmr * w + far_ * wa;
        *mi = fmi * w + fai * wa;
    }
}
__device__ __forceinline__ MixBin mix_bin(const float2* __restrict__ Z, long n, long k, const MixRanges& rg) {
    const float2 a = Z[k], b = cconj(Z[k == 0 ? 0 : n - k]);
    MixBin r;
    r.fm = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y + b.y));
    r.fa = make_float2(0.5f * (a.y - b.y), -0.5f * (a.x - b.x));          // (a - b) / 2i
    double mr, mi;
    mix_select(k, rg, r.fm.x, r.fm.y, r.fa.x, r.fa.y, &mr, &mi);
    r.mix = make_float2((float)mr, (float)mi);
    return r;
}
__global__ void band_mix_kernel(const float2* __restrict__ Z, long n, MixRanges rg, float2* __restrict__ Zp, float2* __restrict__ tap_main,
                                float2* __restrict__ tap_aux, float2* __restrict__ tap_mix) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x, h = n / 2;
    if (k > h) return;
    const MixBin bk = mix_bin(Z, n, k, rg);
    if (tap_main) tap_main[k] = bk.fm;
    if (tap_aux) tap_aux[k] = bk.fa;
    if (tap_mix) tap_mix[k] = bk.mix;
    if (k == h) return;
    float2 a = bk.mix, b = mix_bin(Z, n, h - k, rg).mix;
    if (k == 0) { a.y = 0.f; b.y = 0.f; }           // irfft drops the imaginary parts of bin 0 and of the last bin
    Zp[k] = c2r_merge(a, b, k, h);
}

// Clips of up to DIRECT_MAX samples: the same mix with every step in fp64 and one rounding at the end.  The first kernel forms bin
// k <= n / 2 of both spectra as DFT sums, mixes and leaves the mixed bins as doubles (re [h + 1] | im [h + 1]); the second is the
// inverse real DFT sum of m = 2 h samples.
__global__ void mix_small_spec_kernel(const float* __restrict__ main_x, const float* __restrict__ aux_x, long n, MixRanges rg, double* __restrict__ mix64,
                                      float2* __restrict__ tap_main, float2* __restrict__ tap_aux, float2* __restrict__ tap_mix) {
    const long k = threadIdx.x, h = n / 2;
    if (k > h) return;
    double fmr, fmi, far_, fai, mr, mi;
    dft_bin64(Src{SRC_REAL, main_x, nullptr}, n, 0, k, 0, &fmr, &fmi);
    dft_bin64(Src{SRC_REAL, aux_x, nullptr}, n, 0, k, 0, &far_, &fai);
    mix_select(k, rg, fmr, fmi, far_, fai, &mr, &mi);
    if (tap_main) tap_main[k] = make_float2((float)fmr, (float)fmi);
    if (tap_aux) tap_aux[k] = make_float2((float)far_, (float)fai);
    if (tap_mix) tap_mix[k] = make_float2((float)mr, (float)mi);
    mix64[k] = mr;
    mix64[h + 1 + k] = mi;
}
__global__ void mix_small_out_kernel(const double* __restrict__ mix64, long h, float* __restrict__ y) {
    const long t = threadIdx.x, m = 2 * h;
    if (t >= m) return;
    double acc = mix64[0] + ((t & 1) ? -mix64[h] : mix64[h]);          // the imaginary parts of bin 0 and of bin h are dropped
    for (long k = 1; k < h; ++k) {
        double cs, sn;
        root64((k * t) % m, m, &cs, &sn);
        acc += 2.0 * (mix64[k] * cs - mix64[h + 1 + k] * sn);
    }
    y[t] = (float)(acc / (double)m);
}

// ---------------------------------------------------------------------------------------------------------------- drivers
inline size_t alf(size_t floats) { return tdx::al(floats); }

// The passes of a power-of-two transform of 2^m points: in -> A -> B -> A ..; returns where the result is (A after an odd number
// of passes, B after an even one) through *res.  `in` may be B (it is then overwritten).  mul: see fft_pass_kernel.
inline int run_passes(const float2* in, float2* A, float2* B, const float2* mul, int m, int batch, int inverse, float scale, int tile_log2,
                      hipStream_t st, float2** res) {
    const Plan p = plan_pow2(m, tile_log2);
    const float2* src = in;
    int logNs = 0;
    for (int i = 0; i < p.npass; ++i) {
        float2* dst = (i % 2 == 0) ? A : B;
        const int logR = p.logR[i];
        const dim3 grid((unsigned)(1L << (m - logR - p.logB)), (unsigned)batch);
        hipLaunchKernelGGL(fft_pass_kernel, grid, dim3(THREADS), lds_bytes(logR + p.logB), st, src, dst, i == 0 ? mul : nullptr, m, logR,
                           logNs, p.logB, inverse ? 1 : -1, i == p.npass - 1 ? scale : 1.0f);
        LAUNCH_CHECK();
        logNs += logR;
        src = dst;
    }
    *res = const_cast<float2*>(src);
    return 0;
}
inline int passes_of(int m, int tile_log2) { return plan_pow2(m, tile_log2).npass; }

// Bluestein's workspace, in floats: c [n] | spectrum of the wrapped chirp [M] | P [batch][M] | Q [batch][M], all complex
struct BlueWs { size_t c, bf, p, q, total; };
inline BlueWs blue_ws(long n, int batch) {
    const size_t M = (size_t)1 << bluestein_m(n);
    BlueWs w;
    w.c = 0;
    w.bf = w.c + alf(2 * (size_t)n);
    w.p = w.bf + alf(2 * M);
    w.q = w.p + alf(2 * M * batch);
    w.total = w.q + alf(2 * M * batch);
    return w;
}

// DFT_n of `src` (any n) -> the first nout bins, complex or (real != 0) their real parts, [batch][nout]; scale is applied to
// the result (1 / n for an inverse).  ws: blue_ws(n, batch).total floats.
inline int bluestein(Src src, long n, int batch, int inverse, double scale, float* out, long nout, int real, float* ws, int tile_log2, hipStream_t st) {
    if (n <= DIRECT_MAX) {
        hipLaunchKernelGGL(direct_dft_kernel, dim3(1, batch), dim3(64), 0, st, src, n, nout, inverse, scale, out, real);
        LAUNCH_CHECK();
        return 0;
    }
    const int m = bluestein_m(n);
    const long M = 1L << m;
    const BlueWs w = blue_ws(n, batch);
    float2 *c = (float2*)(ws + w.c), *bf = (float2*)(ws + w.bf), *P = (float2*)(ws + w.p), *Q = (float2*)(ws + w.q);
    const int np = passes_of(m, tile_log2);
    const unsigned gM = (unsigned)((M + 255) / 256);
    hipLaunchKernelGGL(chirp_kernel, dim3(gM), dim3(256), 0, st, n, M, c, P);
    LAUNCH_CHECK();
    float2* r;
    TRY(run_passes(P, np % 2 ? bf : Q, np % 2 ? Q : bf, nullptr, m, 1, 0, 1.0f, tile_log2, st, &r));      // ends in bf
    hipLaunchKernelGGL(bluestein_in_kernel, dim3(gM, batch), dim3(256), 0, st, src, n, M, inverse, c, P);
    LAUNCH_CHECK();
    TRY(run_passes(P, Q, P, nullptr, m, batch, 0, 1.0f, tile_log2, st, &r));
    float2* other = r == P ? Q : P;
    float2* conv;
    TRY(run_passes(r, other, r, bf, m, batch, 1, 1.0f / (float)M, tile_log2, st, &conv));
    hipLaunchKernelGGL(bluestein_out_kernel, dim3((unsigned)((nout + 255) / 256), batch), dim3(256), 0, st, conv, n, M, nout, inverse, (float)scale, c, out, real);
    LAUNCH_CHECK();
    return 0;
}

// complex [batch][n] -> complex [batch][n], in != out
inline size_t c2c_ws_floats(long n, int batch, int tile_log2) {
    if (is_pow2(n)) return passes_of(ilog2(n), tile_log2) > 1 ? alf(2 * (size_t)n * batch) : 0;
    return blue_ws(n, batch).total;
}
inline int c2c(const float* in, long n, int batch, int inverse, float* out, float* ws, int tile_log2, hipStream_t st) {
    const double scale = inverse ? 1.0 / (double)n : 1.0;
    if (is_pow2(n)) {
        const int m = ilog2(n), np = passes_of(m, tile_log2);
        float2 *o = (float2*)out, *w = (float2*)ws, *r;
        return run_passes((const float2*)in, np % 2 ? o : w, np % 2 ? w : o, nullptr, m, batch, inverse, (float)scale, tile_log2, st, &r);
    }
    return bluestein(Src{SRC_CPLX, in, nullptr}, n, batch, inverse, scale, out, n, 0, ws, tile_log2, st);
}

// real [batch][n] -> complex [batch][n / 2 + 1]
inline size_t r2c_ws_floats(long n, int batch, int tile_log2) {
    if (n % 2) return blue_ws(n, batch).total;
    return alf((size_t)n * batch) + c2c_ws_floats(n / 2, batch, tile_log2);
}
inline int r2c(const float* x, long n, int batch, float* X, float* ws, int tile_log2, hipStream_t st) {
    if (n % 2) return bluestein(Src{SRC_REAL, x, nullptr}, n, batch, 0, 1.0f, X, n / 2 + 1, 0, ws, tile_log2, st);
    const long h = n / 2;
    TRY(c2c(x, h, batch, 0, ws, ws + alf((size_t)n * batch), tile_log2, st));
    hipLaunchKernelGGL(r2c_split_kernel, dim3((unsigned)((h + 1 + 255) / 256), batch), dim3(256), 0, st, (const float2*)ws, h, (float2*)X);
    LAUNCH_CHECK();
    return 0;
}

// complex [batch][n / 2 + 1] -> real [batch][n]
inline size_t c2r_ws_floats(long n, int batch, int tile_log2) { return r2c_ws_floats(n, batch, tile_log2); }
inline int c2r(const float* X, long n, int batch, float* y, float* ws, int tile_log2, hipStream_t st) {
    if (n % 2) return bluestein(Src{SRC_HERM, X, nullptr}, n, batch, 1, 1.0 / (double)n, y, n, 1, ws, tile_log2, st);
    const long h = n / 2;
    hipLaunchKernelGGL(c2r_merge_kernel, dim3((unsigned)((h + 255) / 256), batch), dim3(256), 0, st, (const float2*)X, h, (float2*)ws);
    LAUNCH_CHECK();
    return c2c(ws, h, batch, 1, y, ws + alf((size_t)n * batch), tile_log2, st);
}

// the band mix: F [n] complex | Z' [n / 2] complex | the larger of the two transforms' workspaces (forward: + z [n] when n is a
// power of two)
struct MixWs { size_t f, zp, rest, total; };
inline MixWs mix_ws(long n, int tile_log2) {
    const long h = n / 2;
    MixWs w;
    w.f = 0;
    w.zp = w.f + alf(2 * (size_t)n);
    w.rest = w.zp + alf(2 * (size_t)h);
    const size_t fwd = is_pow2(n) ? alf(2 * (size_t)n) + c2c_ws_floats(n, 1, tile_log2) : blue_ws(n, 1).total;
    w.total = w.rest + std::max(fwd, c2c_ws_floats(h, 1, tile_log2));
    return w;
}
inline int band_mix(const float* main_dev, const float* aux_dev, long n, const MixRanges& rg, float* y, float* tap_main, float* tap_aux,
                    float* tap_mix, float* ws, int tile_log2, hipStream_t st) {
    const MixWs w = mix_ws(n, tile_log2);
    const long h = n / 2;
    float *F = ws + w.f, *Zp = ws + w.zp, *rest = ws + w.rest;
    if (n <= DIRECT_MAX) {                           // (2 (h + 1) doubles <= the 2 n + 2 h floats of F and Z', rounded up to 64 each)
        hipLaunchKernelGGL(mix_small_spec_kernel, dim3(1), dim3(64), 0, st, main_dev, aux_dev, n, rg, (double*)F, (float2*)tap_main, (float2*)tap_aux,
                           (float2*)tap_mix);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(mix_small_out_kernel, dim3(1), dim3(64), 0, st, (const double*)F, h, y);
        LAUNCH_CHECK();
        return 0;
    }
    if (is_pow2(n)) {
        hipLaunchKernelGGL(interleave_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, main_dev, aux_dev, n, (float2*)rest);
        LAUNCH_CHECK();
        TRY(c2c(rest, n, 1, 0, F, rest + alf(2 * (size_t)n), tile_log2, st));
    } else {
        TRY(bluestein(Src{SRC_TWO_REAL, main_dev, aux_dev}, n, 1, 0, 1.0f, F, n, 0, rest, tile_log2, st));
    }
    hipLaunchKernelGGL(band_mix_kernel, dim3((unsigned)((h + 1 + 255) / 256)), dim3(256), 0, st, (const float2*)F, n, rg, (float2*)Zp, (float2*)tap_main,
                       (float2*)tap_aux, (float2*)tap_mix);
    LAUNCH_CHECK();
    return c2c(Zp, h, 1, 1, y, rest, tile_log2, st);
}

// ---- the argument rules shared by the entry points and the test hook (nullptr = fine)
inline const char* size_error(long n, int batch) {
    if (n < 1 || n > MAX_N) return "need 1 <= n <= 2^26";
    if (batch < 1 || batch > MAX_BATCH) return "need 1 <= batch <= 65535";
    return nullptr;
}

}  // namespace fft
}  // namespace tdx
