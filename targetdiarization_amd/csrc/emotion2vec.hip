// emotion2vec.hip — funasr's emotion2vec (a data2vec 2.0 audio encoder + a linear head) on MI355X: the model behind the
// reference's ASRProcessor.emotion_detection (ASRProcessor.py:935-973, loaded at :277-283).  fp32 throughout, restated from
// upstream (parity with the published checkpoint is unpinned).
//
// A launch takes B clips of N samples each:
//     e2v_stat_kernel x 2     mean, then the centred squares of a clip, as 64 fp64 partial sums each
//     e2v_conv0_kernel        conv 0 (1 -> C) on the normalised samples + LayerNorm + GELU, one wave per frame
//     per conv 1..: gemm      the strided convolution as a GEMM over overlapping channel-last rows      EpiConvRows
//                   e2v_ln_rows_kernel   LayerNorm + GELU in place
//     e2v_ln_rows_kernel, gemm            projection: LayerNorm, Linear C -> D
//     per positional layer:   e2v_gconv_kernel (grouped convolution, fp32 MFMA), e2v_ln_rows_kernel (no affine, GELU; the
//                             last one adds the residual and writes rows E.. of the sequence [B][S][D])
//     e2v_extra_kernel        the E learned prefix rows
//     e2v_ln_rows_kernel      the context encoder's LayerNorm
//     per block:              gemm qkv, e2v_attn_kernel (streaming softmax + ALiBi), gemm proj + residual, LayerNorm,
//                             gemm fc1 + GELU, gemm fc2 + residual, LayerNorm
//     e2v_feats_kernel, e2v_head_kernel   frame features; mean over frames, head, softmax
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/tdx.h"
#include "epilogues.hpp"
#include "weight_pack.hpp"

using namespace tdx;

namespace {

constexpr int DK = 64;                   // head width of every published size
constexpr float LN_EPS = 1e-5f;
constexpr int NPART = 64;                // fp64 partial sums per clip and pass
constexpr int MAX_CONV = 8;
constexpr int MAX_K0 = 16;
constexpr int MAX_C = 1024;              // conv 0 keeps C / 64 channels per lane
constexpr int MAX_CLASSES = 64;
constexpr int GC_TILE = 64;              // frames per workgroup of the grouped convolution
constexpr int MAX_GW = 64;               // widest group: a tap's [64][64] slab is 4 float4 per thread

__device__ __forceinline__ float gelu_erf(float v) { return ActGelu::f(v); }

// ------------------------------------------------------------------------------------------------ clip statistics
// PASS 0: part[b][blk] = sum x.  PASS 1: part[B * NPART + ...] = sum (x - mean)^2, the mean from the partials of pass 0 added in
// a fixed order.  grid (NPART, B); a block owns a contiguous slice of the clip.
template <int PASS>
__global__ __launch_bounds__(256) void e2v_stat_kernel(const float* __restrict__ wav, long N, int B, double* __restrict__ part) {
    __shared__ double red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long per = (N + NPART - 1) / NPART, i0 = (long)blockIdx.x * per, i1 = min(i0 + per, N);
    double mean = 0.0;
    if (PASS == 1) {
        for (int j = 0; j < NPART; ++j) mean += part[(long)b * NPART + j];
        mean /= (double)N;
    }
    const float* x = wav + (long)b * N;
    double s = 0.0;
    for (long i = i0 + tid; i < i1; i += 256) { const double v = (double)x[i] - mean; s += PASS == 0 ? v : v * v; }
    s = wave_sum_d(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) part[(long)(PASS * B + b) * NPART + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ------------------------------------------------------------------------------------------------ conv 0
// out[b][t][c] = gelu(LN_c(sum_j w[c][j] (x[b][s t + j] - mean) rstd)): grid (ceil(L1 / 64), B), a wave takes frames
// w, w + 4, ... of the block's 64; lane l owns channels l, l + 64, ...; the weights sit tap-major in LDS.
__global__ __launch_bounds__(256) void e2v_conv0_kernel(const float* __restrict__ wav, long N, int B, const double* __restrict__ part,
                                                         const float* __restrict__ w0 /*[k][C]*/, const float* __restrict__ g, const float* __restrict__ be,
                                                         float* __restrict__ out, int L1, int Lp1, int C, int k0, int s0) {
    extern __shared__ __attribute__((aligned(16))) float e2v_lds[];
    float* ws = e2v_lds;
    __shared__ float stat[2];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < k0 * C; i += 256) ws[i] = w0[i];
    if (tid == 0) {
        double s = 0.0, q = 0.0;
        for (int j = 0; j < NPART; ++j) { s += part[(long)b * NPART + j]; q += part[(long)(B + b) * NPART + j]; }
        stat[0] = (float)(s / (double)N);
        stat[1] = (float)(1.0 / sqrt(q / (double)N + 1e-5));
    }
    __syncthreads();
    const float mean = stat[0], rstd = stat[1];
    const int nch = C >> 6;
    const float* x = wav + (long)b * N;
    for (int r = wave; r < 64; r += 4) {
        const int t = blockIdx.x * 64 + r;
        if (t >= L1) break;
        float xn[MAX_K0];
#pragma unroll
        for (int j = 0; j < MAX_K0; ++j) xn[j] = j < k0 ? (x[(long)t * s0 + j] - mean) * rstd : 0.f;
        float v[MAX_C / 64];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < MAX_C / 64; ++i) {
            v[i] = 0.f;
            if (i < nch) {
                float a = 0.f;
#pragma unroll
                for (int j = 0; j < MAX_K0; ++j) if (j < k0) a = fmaf(ws[j * C + lane + 64 * i], xn[j], a);
                v[i] = a; s += a;
            }
        }
        const float mu = wave_sum(s) / (float)C;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < MAX_C / 64; ++i) if (i < nch) { const float d = v[i] - mu; q = fmaf(d, d, q); }
        const float rs = 1.0f / sqrtf(wave_sum(q) / (float)C + LN_EPS);
        float* o = out + ((long)b * Lp1 + t) * C;
#pragma unroll
        for (int i = 0; i < MAX_C / 64; ++i)
            if (i < nch) { const int c = lane + 64 * i; o[c] = gelu_erf(fmaf((v[i] - mu) * rs, g[c], be[c])); }
    }
}

// conv 1..: GEMM row m = rows_in b + t reads k C floats from input row s m -> out row Lp_out b + t for t < L_out
struct EpiConvRows {
    float* out; int rows_in, L_out, Lp_out, C;
    __device__ EpiNone col(int, int) const { return EpiNone{}; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int, int m, int n, float v, EpiNone, EpiNone) const {
        const int bi = m / rows_in, t = m - bi * rows_in;
        if (t < L_out && n < C) out[((long)bi * Lp_out + t) * C + n] = v;
    }
};

// ------------------------------------------------------------------------------------------------ rows
// LayerNorm of rows of d floats (d % 4 == 0), one wave per row, two passes; then the affine part, GELU and a residual as
// asked.  Logical row m = rin b + t is read at row pin b + t of x, the residual at row m of res, and written to row
// pout b + ooff + t of y (y may be x: a lane rewrites only what it read).
template <bool AFFINE, bool GELU, bool RES>
__global__ __launch_bounds__(256) void e2v_ln_rows_kernel(const float* x, const float* __restrict__ g, const float* __restrict__ be,
                                                           const float* __restrict__ res, float* y, long M, int d, int rin, int pin, int pout, int ooff) {
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (m >= M) return;
    const long b = m / rin, t = m - b * rin;
    const float* xr = x + (b * pin + t) * d;
    float* yr = y + (b * pout + ooff + t) * d;
    float s = 0.f;
    for (int k = 4 * lane; k < d; k += 256) { const f32x4 v = ldg4(xr + k); s += (v[0] + v[1]) + (v[2] + v[3]); }
    const float mean = wave_sum(s) / (float)d;
    float q = 0.f;
    for (int k = 4 * lane; k < d; k += 256) {
        const f32x4 v = ldg4(xr + k);
        const float a0 = v[0] - mean, a1 = v[1] - mean, a2 = v[2] - mean, a3 = v[3] - mean;
        q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + LN_EPS);
    for (int k = 4 * lane; k < d; k += 256) {
        const f32x4 v = ldg4(xr + k);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (v[j] - mean) * rstd;
        if constexpr (AFFINE) {
            const f32x4 gv = ldg4(g + k), bv = ldg4(be + k);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = fmaf(o[j], gv[j], bv[j]);
        }
        if constexpr (GELU) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = gelu_erf(o[j]);
        }
        if constexpr (RES) {
            const f32x4 rv = ldg4(res + m * d + k);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = rv[j] + o[j];
        }
        *reinterpret_cast<f32x4*>(yr + k) = o;
    }
}

// ------------------------------------------------------------------------------------------------ grouped positional convolution
// y[b][f][g gw + co] = bias + sum_t sum_ci W[g gw + co][ci][t] x[b][f + t - KT / 2][g gw + ci], zero outside [0, T).
// Workgroup (time tile of 64 frames, group g, clip b), 4 waves as 2 (frames) x 2 (output channels) tiles of 32 x 32 on
// v_mfma_f32_32x32x2_f32.  The tile's 64 + KT - 1 input rows of the group's gw channels are staged in LDS once (rows outside
// the clip are zeros by predicate); a tap is then a [64] x [gw] x [NP] GEMM whose A rows are the staged rows shifted by the tap.
// The taps' weight slabs [NP][gw] (output channels zero-padded to NP = 32 or 64, K contiguous) stream through two LDS buffers:
// the loads of tap t + 1 are in flight during the MFMAs of tap t.  Both operands have a row pitch of gw + 4 floats and are read
// as 4 consecutive k per lane (ds_read_b128; the pitch / 4 is odd for gw % 8 == 0, so 16 consecutive rows hit distinct slots);
// register j of a fragment pairs k = 8 kc + j with k = 8 kc + 4 + j on both operands, a re-ordered but complete K sum (gemm.hpp).
// Lanes whose 4 k lie beyond gw (gw % 8 == 4, last step) feed zeros.
__global__ __launch_bounds__(256) void e2v_gconv_kernel(const float* __restrict__ x, const float* __restrict__ Wp, const float* __restrict__ bias,
                                                         float* __restrict__ y, int T, int D, int gw, int NP, int KT) {
    extern __shared__ __attribute__((aligned(16))) float e2v_lds[];
    const int PX = gw + 4, rows = GC_TILE + KT - 1;
    float* xs = e2v_lds;
    float* wsb = e2v_lds + rows * PX;                 // 2 x [NP][PX]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const int mt = wave & 1, nt = wave >> 1;
    const int f0 = blockIdx.x * GC_TILE, g = blockIdx.y, b = blockIdx.z;
    const int q4 = gw >> 2, n4 = NP * q4;             // float4 per row, per slab (<= 1024)
    const float* Wg = Wp + (long)g * KT * NP * gw;

    f32x4 wr[4];
#define E2V_LOAD_SLAB(t)                                                                        \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                             \
        const int e = tid + 256 * i;                                                            \
        wr[i] = ldg4(Wg + (long)(t) * NP * gw + 4 * min(e, n4 - 1));                            \
    }
#define E2V_WRITE_SLAB(buf)                                                                     \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                             \
        const int e = tid + 256 * i;                                                            \
        if (e < n4) { const int r = e / q4, c = e - r * q4; *reinterpret_cast<f32x4*>(wsb + (buf) * NP * PX + r * PX + 4 * c) = wr[i]; } \
    }
    E2V_LOAD_SLAB(0)
    for (int e = tid; e < rows * q4; e += 256) {
        const int r = e / q4, c = e - r * q4, t = f0 - KT / 2 + r;
        const bool ok = t >= 0 && t < T;
        const f32x4 v = ldg4(x + ((long)b * T + (ok ? t : 0)) * D + g * gw + 4 * c);
        *reinterpret_cast<f32x4*>(xs + r * PX + 4 * c) = sel4(ok, v);
    }
    E2V_WRITE_SLAB(0)
    __syncthreads();

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const bool active = nt * 32 < NP;
    const int nkc = (gw + 7) >> 3;
    for (int t = 0; t < KT; ++t) {
        if (t + 1 < KT) { E2V_LOAD_SLAB(t + 1) }
        if (active) {
            const float* ar = xs + (mt * 32 + l31 + t) * PX + 4 * hh;
            const float* br = wsb + (t & 1) * NP * PX + (nt * 32 + l31) * PX + 4 * hh;
            for (int kc = 0; kc < nkc; ++kc) {
                const bool ok = 8 * kc + 4 * hh < gw;
                const f32x4 a = sel4(ok, *reinterpret_cast<const f32x4*>(ar + (ok ? 8 * kc : 0)));
                const f32x4 w = sel4(ok, *reinterpret_cast<const f32x4*>(br + (ok ? 8 * kc : 0)));
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], w[j], acc, 0, 0, 0);
            }
        }
        if (t + 1 < KT) { E2V_WRITE_SLAB((t + 1) & 1) }
        __syncthreads();
    }
#undef E2V_LOAD_SLAB
#undef E2V_WRITE_SLAB
    const int co = nt * 32 + l31;
    if (active && co < gw) {
        const float bv = bias[g * gw + co];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = f0 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (f < T) y[((long)b * T + f) * D + g * gw + co] = acc[r] + bv;
        }
    }
}

// rows 0 .. E-1 of every clip of the sequence [B][S][D]
__global__ void e2v_extra_kernel(const float* __restrict__ extra, float* __restrict__ seq, int E, int S, int D) {
    const float* s = extra + (long)blockIdx.x * D;
    float* p = seq + ((long)blockIdx.y * S + blockIdx.x) * D;
    for (int i = threadIdx.x; i < D; i += blockDim.x) p[i] = s[i];
}

// ------------------------------------------------------------------------------------------------ attention
// Softmax attention over the S = E + T rows of a clip with the symmetric ALiBi bias: score(i, j) = (q_i / 8) . k_j +
// ns_h |i - j| where both i and j are frames (>= E), and no bias where either is a prefix token; ns_h = -slope_h max(scale_h, 0)
// is one register per workgroup.  q, k, v are the three column blocks of qkv [B][S][3 D].  Streaming softmax: workgroup
// (query tile, head, clip) holds 64 queries; thread (query t >> 2, part t & 3) owns 16 of the 64 dimensions of its query and of
// its output; a 64-key tile of K and V sits in LDS; the four parts of a score meet in two DPP quad exchanges; keys go in
// chunks of 8 with a running maximum, and no score is stored.
__global__ __launch_bounds__(256) void e2v_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ nslope, float* __restrict__ out,
                                                        int S, int E, int d) {
    __shared__ __attribute__((aligned(16))) float Ks[64 * DK];
    __shared__ __attribute__((aligned(16))) float Vs[64 * DK];
    const int tid = threadIdx.x, qi = tid >> 2, p = tid & 3;
    const int h = blockIdx.y, b = blockIdx.z;
    const int qg = blockIdx.x * 64 + qi;
    const long pitch = 3L * d;
    const long base = (long)b * S * pitch + (long)h * DK;
    const float ns = nslope[h];
    const bool qframe = qg >= E;
    float qv[16], acc[16];
    {
        const float* qr = qkv + base + (long)min(qg, S - 1) * pitch + 16 * p;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 t = ldg4(qr + 4 * i);
#pragma unroll
            for (int j = 0; j < 4; ++j) { qv[4 * i + j] = t[j] * 0.125f; acc[4 * i + j] = 0.f; }
        }
    }
    float mrun = -INFINITY, lrun = 0.f;
    for (int k0 = 0; k0 < S; k0 += 64) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, r = e >> 4, c = (e & 15) * 4;
            const long off = base + (long)min(k0 + r, S - 1) * pitch + c;
            *reinterpret_cast<f32x4*>(Ks + r * DK + c) = ldg4(qkv + off + d);
            *reinterpret_cast<f32x4*>(Vs + r * DK + c) = ldg4(qkv + off + 2 * d);
        }
        __syncthreads();
#pragma unroll 1
        for (int j0 = 0; j0 < 64 && k0 + j0 < S; j0 += 8) {
            float s[8];
            float cm = -INFINITY;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const float* kr = Ks + (j0 + jj) * DK + 16 * p;
                float a = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(kr + 4 * i);
#pragma unroll
                    for (int j = 0; j < 4; ++j) a = fmaf(qv[4 * i + j], t[j], a);
                }
                a += h3_dpp(a, 0);
                a += h3_dpp(a, 1);
                const int kg = k0 + j0 + jj;
                if (qframe && kg >= E) a = fmaf(ns, fabsf((float)(qg - kg)), a);
                s[jj] = kg < S ? a : -INFINITY;
                cm = fmaxf(cm, s[jj]);
            }
            if (cm > mrun) {
                const float sc = expf(mrun - cm);
                lrun *= sc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] *= sc;
                mrun = cm;
            }
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const float pj = expf(s[jj] - mrun);
                lrun += pj;
                const float* vr = Vs + (j0 + jj) * DK + 16 * p;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(vr + 4 * i);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[4 * i + j] = fmaf(pj, t[j], acc[4 * i + j]);
                }
            }
        }
    }
    if (qg < S) {
        float* o = out + ((long)b * S + qg) * d + (long)h * DK + 16 * p;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f32x4 t;
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = acc[4 * i + j] / lrun;
            *reinterpret_cast<f32x4*>(o + 4 * i) = t;
        }
    }
}

// ------------------------------------------------------------------------------------------------ outputs
// feats[b][t][:] = seq[b][E + t][:]      grid (T, B)
__global__ void e2v_feats_kernel(const float* __restrict__ seq, float* __restrict__ feats, int T, int E, int S, int D) {
    const float* s = seq + ((long)blockIdx.y * S + E + blockIdx.x) * D;
    float* p = feats + ((long)blockIdx.y * T + blockIdx.x) * D;
    for (int i = 4 * threadIdx.x; i < D; i += 4 * blockDim.x) *reinterpret_cast<f32x4*>(p + i) = ldg4(s + i);
}
// One workgroup per clip: the mean over the T frames (four running sums per column, frames t % 4, added as (0 + 1) + (2 + 3)),
// the head (a wave per class) and its softmax.  The order of every sum is fixed.
__global__ __launch_bounds__(256) void e2v_head_kernel(const float* __restrict__ seq, const float* __restrict__ Wh, const float* __restrict__ bh,
                                                        float* __restrict__ emb, float* __restrict__ scores, int T, int E, int S, int D, int NC) {
    extern __shared__ __attribute__((aligned(16))) float e2v_lds[];
    float* mean = e2v_lds;               // [D]
    __shared__ float logit[MAX_CLASSES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = seq + ((long)b * S + E) * D;
    for (int c = tid; c < D; c += 256) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int t = 0;
        for (; t + 3 < T; t += 4) { s0 += x[(long)t * D + c]; s1 += x[(long)(t + 1) * D + c]; s2 += x[(long)(t + 2) * D + c]; s3 += x[(long)(t + 3) * D + c]; }
        if (t < T) s0 += x[(long)t * D + c];
        if (t + 1 < T) s1 += x[(long)(t + 1) * D + c];
        if (t + 2 < T) s2 += x[(long)(t + 2) * D + c];
        const float m = ((s0 + s1) + (s2 + s3)) / (float)T;
        mean[c] = m;
        if (emb) emb[(long)b * D + c] = m;
    }
    __syncthreads();
    if (!scores) return;
    for (int c = wave; c < NC; c += 4) {
        float a = 0.f;
        for (int k = lane; k < D; k += 64) a = fmaf(mean[k], Wh[(long)c * D + k], a);
        a = wave_sum(a);
        if (lane == 0) logit[c] = a + bh[c];
    }
    __syncthreads();
    if (tid == 0) {
        float mx = -INFINITY, sum = 0.f;
        for (int c = 0; c < NC; ++c) mx = fmaxf(mx, logit[c]);
        for (int c = 0; c < NC; ++c) { const float e = expf(logit[c] - mx); logit[c] = e; sum += e; }
        for (int c = 0; c < NC; ++c) scores[(long)b * NC + c] = logit[c] / sum;
    }
}

struct Block {
    const float *Wqkv = nullptr, *bqkv = nullptr, *Wo = nullptr, *bo = nullptr, *g1 = nullptr, *b1n = nullptr, *W1 = nullptr, *b1 = nullptr,
        *W2 = nullptr, *b2 = nullptr, *g2 = nullptr, *b2n = nullptr;
};

// the standard ALiBi slopes (get_slopes): powers of 2^(-8 / n) for n a power of two, otherwise those of the power of two below
// followed by every other one of the next power of two
void alibi_slopes(int n, std::vector<double>& out) {
    auto pow2 = [](int m, std::vector<double>& o) {
        const double start = std::pow(2.0, -8.0 / m);
        double v = start;
        for (int i = 0; i < m; ++i) { o.push_back(v); v *= start; }
    };
    int c = 1;
    while (2 * c <= n) c *= 2;
    pow2(c, out);
    if (c != n) {
        std::vector<double> more;
        pow2(2 * c, more);
        for (int i = 0; i < 2 * c && (int)out.size() < n; i += 2) out.push_back(more[i]);
    }
}

}  // namespace

struct tdx_emo2v {
    int device = 0;
    tdx_emo2v_config c{};
    int gw = 0, NP = 0;
    tdx::DevBuf dev;
    const float *w0 = nullptr, *ln0g = nullptr, *ln0b = nullptr;
    const float *cw[MAX_CONV] = {}, *clg[MAX_CONV] = {}, *clb[MAX_CONV] = {};     // layers 1 .. n_conv - 1 (layer 0: w0, ln0g, ln0b)
    const float *plg = nullptr, *plb = nullptr, *pw = nullptr, *pb = nullptr;
    std::vector<const float*> gcw, gcb;
    const float *extra = nullptr, *nslope = nullptr, *eng = nullptr, *enb = nullptr, *hw = nullptr, *hb = nullptr;
    std::vector<Block> blocks;          // prenet blocks, then the main blocks
};

namespace {

// frames after every conv layer: L[0] = N samples, L[i + 1] = (L[i] - k_i) / s_i + 1; Lp[i] = the row pitch of a clip in the
// buffer that holds L[i] rows: L[i] rounded up to the stride of the layer that reads it (the last one is not padded)
struct Frames { long L[MAX_CONV + 1], Lp[MAX_CONV + 1]; bool ok; };
Frames frames_of(const tdx_emo2v_config& c, long N) {
    Frames f{};
    f.ok = true;
    f.L[0] = f.Lp[0] = N;
    for (int i = 0; i < c.n_conv; ++i) {
        if (f.L[i] < c.conv_k[i]) { f.ok = false; return f; }
        f.L[i + 1] = (f.L[i] - c.conv_k[i]) / c.conv_s[i] + 1;
        const long s = i + 1 < c.n_conv ? c.conv_s[i + 1] : 1;
        f.Lp[i + 1] = (f.L[i + 1] + s - 1) / s * s;
    }
    return f;
}

struct Ws { size_t part, a, bq, x, y0, y1, seq, qkv, ao, hb, total; };      // offsets in floats
Ws ws_plan(const tdx_emo2v* h, int B, const Frames& f) {
    const tdx_emo2v_config& c = h->c;
    const size_t T = f.L[c.n_conv], S = c.E + T, D = c.D;
    size_t ra = 0, rb = 0;                     // conv outputs alternate between two buffers: layers 0, 2, .. in a; 1, 3, .. in bq
    for (int i = 1; i <= c.n_conv; ++i) { size_t& r = (i & 1) ? ra : rb; r = std::max(r, (size_t)B * f.Lp[i] * c.C); }
    Ws w{}; size_t o = 0;
    w.part = o; o += al((size_t)2 * 2 * B * NPART);      // doubles
    w.a = o; o += al(ra); w.bq = o; o += al(rb);
    w.x = o; o += al(B * T * D); w.y0 = o; o += al(B * T * D); w.y1 = o; o += al(B * T * D);
    w.seq = o; o += al(B * S * D); w.qkv = o; o += al(B * S * 3 * D); w.ao = o; o += al(B * S * D); w.hb = o; o += al(B * S * 4 * D);
    w.total = o;
    return w;
}

template <bool AFFINE, bool GELU, bool RES>
int ln_rows(const float* x, const float* g, const float* be, const float* res, float* y, long M, int d, long rin, long pin, long pout, int ooff, hipStream_t st) {
    hipLaunchKernelGGL((e2v_ln_rows_kernel<AFFINE, GELU, RES>), dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, x, g, be, res, y, M, d, (int)rin, (int)pin,
                       (int)pout, ooff);
    LAUNCH_CHECK();
    return TDX_OK;
}

int forward_impl(tdx_emo2v* h, const float* wav, int B, long N, float* feats, float* emb, float* scores, float* tap_proj, float* tap_pos, float* tap_qkv,
                 float* tap_attn, void* ws_, size_t ws_bytes, hipStream_t st) {
    const tdx_emo2v_config& c = h->c;
    const Frames f = frames_of(c, N);
    const Ws w = ws_plan(h, B, f);
    if (ws_bytes < w.total * sizeof(float)) return tdx::fail(TDX_E_WORKSPACE, "tdx_emo2v_forward: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    float* fw = (float*)ws_;
    double* part = (double*)(fw + w.part);
    const int C = c.C, D = c.D, E = c.E, H = c.H, Cp = up(C, 128), Dp = up(D, 128);
    const long T = f.L[c.n_conv], S = E + T;

    hipLaunchKernelGGL(e2v_stat_kernel<0>, dim3(NPART, B), dim3(256), 0, st, wav, N, B, part);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(e2v_stat_kernel<1>, dim3(NPART, B), dim3(256), 0, st, wav, N, B, part);
    LAUNCH_CHECK();
    float* cur = fw + w.a;
    hipLaunchKernelGGL(e2v_conv0_kernel, dim3((unsigned)((f.L[1] + 63) / 64), B), dim3(256), (size_t)c.conv_k[0] * C * sizeof(float), st, wav, N, B,
                       (const double*)part, h->w0, h->ln0g, h->ln0b, cur, (int)f.L[1], (int)f.Lp[1], C, c.conv_k[0], c.conv_s[0]);
    LAUNCH_CHECK();
    for (int i = 1; i < c.n_conv; ++i) {
        float* nxt = (i & 1) ? fw + w.bq : fw + w.a;
        const int s = c.conv_s[i], k = c.conv_k[i];
        const long rows_in = f.Lp[i] / s;                                 // GEMM rows of a clip
        const long M = (long)(B - 1) * rows_in + f.L[i + 1];              // the last row computed is the last one kept: no read past the buffer
        TRY(linear_f32(cur, (long)s * C, h->cw[i], (int)M, Cp, k * C, EpiConvRows{nxt, (int)rows_in, (int)f.L[i + 1], (int)f.Lp[i + 1], C}, st));
        TRY((ln_rows<true, true, false>(nxt, h->clg[i], h->clb[i], nullptr, nxt, (long)B * f.L[i + 1], C, f.L[i + 1], f.Lp[i + 1], f.Lp[i + 1], 0, st)));
        cur = nxt;
    }
    // projection (the last conv buffer is not padded: rows b T + t)
    const long MT = (long)B * T;
    TRY((ln_rows<true, false, false>(cur, h->plg, h->plb, nullptr, cur, MT, C, T, T, T, 0, st)));
    float *x = fw + w.x, *y0 = fw + w.y0, *y1 = fw + w.y1, *seq = fw + w.seq, *qkv = fw + w.qkv, *ao = fw + w.ao, *hb = fw + w.hb;
    TRY(linear_f32(cur, C, h->pw, (int)MT, Dp, C, EpiBiasActN<>{h->pb, x, D, D}, st));
    if (tap_proj) {
        hipLaunchKernelGGL(e2v_feats_kernel, dim3((unsigned)T, B), dim3(256), 0, st, (const float*)x, tap_proj, (int)T, 0, (int)T, D);
        LAUNCH_CHECK();
    }
    // x + P(x) into rows E.. of the sequence
    const int np = (int)h->gcw.size();
    const size_t gc_lds = ((size_t)(GC_TILE + c.pos_k - 1) + 2 * h->NP) * (h->gw + 4) * sizeof(float);
    const float* in = x;
    for (int l = 0; l < np; ++l) {
        float* yo = (l & 1) ? y1 : y0;
        hipLaunchKernelGGL(e2v_gconv_kernel, dim3((unsigned)((T + GC_TILE - 1) / GC_TILE), c.pos_groups, B), dim3(256), gc_lds, st, in, h->gcw[l], h->gcb[l], yo,
                           (int)T, D, h->gw, h->NP, c.pos_k);
        LAUNCH_CHECK();
        if (l + 1 < np) TRY((ln_rows<false, true, false>(yo, nullptr, nullptr, nullptr, yo, MT, D, T, T, T, 0, st)));
        else TRY((ln_rows<false, true, true>(yo, nullptr, nullptr, x, seq, MT, D, T, T, S, E, st)));
        in = yo;
    }
    if (E > 0) {
        hipLaunchKernelGGL(e2v_extra_kernel, dim3(E, B), dim3(256), 0, st, h->extra, seq, E, (int)S, D);
        LAUNCH_CHECK();
    }
    if (tap_pos) {
        hipLaunchKernelGGL(e2v_feats_kernel, dim3((unsigned)T, B), dim3(256), 0, st, (const float*)seq, tap_pos, (int)T, E, (int)S, D);
        LAUNCH_CHECK();
    }
    const long MS = (long)B * S;
    TRY((ln_rows<true, false, false>(seq, h->eng, h->enb, nullptr, seq, MS, D, S, S, S, 0, st)));
    for (size_t l = 0; l < h->blocks.size(); ++l) {
        const Block& L = h->blocks[l];
        float* q = (l == 0 && tap_qkv) ? tap_qkv : qkv;
        float* a = (l == 0 && tap_attn) ? tap_attn : ao;
        TRY(linear_f32(seq, D, L.Wqkv, (int)MS, up(3 * D, 128), D, EpiBiasActN<>{L.bqkv, q, 3L * D, 3 * D}, st));
        hipLaunchKernelGGL(e2v_attn_kernel, dim3((unsigned)((S + 63) / 64), H, B), dim3(256), 0, st, (const float*)q, h->nslope, a, (int)S, E, D);
        LAUNCH_CHECK();
        TRY(linear_f32(a, D, L.Wo, (int)MS, Dp, D, EpiBiasResN<>{L.bo, seq, seq, D, D}, st));
        TRY((ln_rows<true, false, false>(seq, L.g1, L.b1n, nullptr, seq, MS, D, S, S, S, 0, st)));
        TRY(linear_f32(seq, D, L.W1, (int)MS, up(4 * D, 128), D, EpiBiasActN<ActGelu>{L.b1, hb, 4L * D, 4 * D}, st));
        TRY(linear_f32(hb, 4L * D, L.W2, (int)MS, Dp, 4 * D, EpiBiasResN<>{L.b2, seq, seq, D, D}, st));
        TRY((ln_rows<true, false, false>(seq, L.g2, L.b2n, nullptr, seq, MS, D, S, S, S, 0, st)));
    }
    if (feats) {
        hipLaunchKernelGGL(e2v_feats_kernel, dim3((unsigned)T, B), dim3(256), 0, st, (const float*)seq, feats, (int)T, E, (int)S, D);
        LAUNCH_CHECK();
    }
    if (emb || scores) {
        hipLaunchKernelGGL(e2v_head_kernel, dim3(B), dim3(256), (size_t)D * sizeof(float), st, (const float*)seq, h->hw, h->hb, emb, scores, (int)T, E, (int)S, D,
                           c.n_classes);
        LAUNCH_CHECK();
    }
    return TDX_OK;
}

int check_forward_args(const tdx_emo2v* h, const float* wav, int B, long N, const void* ws, const char* fn) {
    const std::string who = fn;
    if (!h || !wav || !ws) return tdx::fail(TDX_E_INVALID, who + ": null argument");
    if (B < 1 || B > 65535) return tdx::fail(TDX_E_INVALID, who + ": need 1 <= B <= 65535");
    const Frames f = frames_of(h->c, N);
    if (N < 1 || !f.ok || f.L[h->c.n_conv] < 1) return tdx::fail(TDX_E_INVALID, who + ": the clip is too short for one frame");
    // rows of the largest buffer: the GEMMs index rows with an int
    if ((long)B * f.Lp[1] > 0x7fffffffL) return tdx::fail(TDX_E_INVALID, who + ": B x N is too large for one launch");
    return TDX_OK;
}

}  // namespace

extern "C" {

int tdx_emo2v_create(const tdx_emo2v_config* cfg, const void* blob, size_t blob_bytes, int device, tdx_emo2v** out) {
    if (!cfg || !blob || !out) return tdx::fail(TDX_E_INVALID, "tdx_emo2v_create: null argument");
    if (device < 0) return tdx::fail(TDX_E_INVALID, "tdx_emo2v_create: device must be >= 0");
    const tdx_emo2v_config c = *cfg;
    if (c.H < 1 || c.D != DK * c.H) return tdx::fail(TDX_E_INVALID, "tdx_emo2v_create: D must be 64 x H (head width 64), got D = " + std::to_string(c.D) + ", H = " + std::to_string(c.H));
    if (c.pos_groups < 1 || c.D % c.pos_groups) return tdx::fail(TDX_E_INVALID, "tdx_emo2v_create: D must be divisible by the group count of the positional convolution");
    const int gw = c.D / c.pos_groups;
    if (gw % 4) return tdx::fail(TDX_E_INVALID, "tdx_emo2v_create: the group width D / groups must be a multiple of 4, got " + std::to_string(gw));
    if (gw > MAX_GW) return tdx::fail(TDX_E_INVALID, "tdx_emo2v_create: the group width D / groups must be at most 64, got " + std::to_string(gw));
    if (c.C < 64 || c.C % 64 || c.C > MAX_C) return tdx::fail(TDX_E_INVALID, "tdx_emo2v_create: the conv width C must be a multiple of 64 in [64, 1024]");
    if (c.n_conv < 1 || c.n_conv > MAX_CONV) return tdx::fail(TDX_E_INVALID, "tdx_emo2v_create: need 1 .. 8 conv layers");
    for (int i = 0; i < c.n_conv; ++i)
        if (c.conv_k[i] < 1 || c.conv_k[i] > MAX_K0 || c.conv_s[i] < 1 || c.conv_s[i] > c.conv_k[i])
            return tdx::fail(TDX_E_INVALID, "tdx_emo2v_create: conv layer " + std::to_string(i) + ": need 1 <= stride <= kernel <= 16");
    if (c.pos_layers < 1 || c.pos_layers > 16 || c.pos_k < 1 || c.pos_k > 31 || c.pos_k % 2 == 0)
        return tdx::fail(TDX_E_INVALID, "tdx_emo2v_create: need 1 .. 16 positional layers with an odd kernel of at most 31 taps");
    if (c.E < 0 || c.E > 4096) return tdx::fail(TDX_E_INVALID, "tdx_emo2v_create: need 0 <= extra tokens <= 4096");
    if (c.prenet_depth < 0 || c.depth < 0 || c.prenet_depth + c.depth < 1 || c.prenet_depth + c.depth > 256)
        return tdx::fail(TDX_E_INVALID, "tdx_emo2v_create: need 1 .. 256 transformer blocks");
    if (c.n_classes < 1 || c.n_classes > MAX_CLASSES) return tdx::fail(TDX_E_INVALID, "tdx_emo2v_create: need 1 .. 64 classes");
    tdx::Loader ld;
    if (!ld.parse(blob, blob_bytes)) return tdx::fail(TDX_E_BLOB, "tdx_emo2v_create: malformed TDXW blob");
    const int C = c.C, D = c.D, Cp = up(C, 128), Dp = up(D, 128), NP = up(gw, 32);
    const uint32_t uC = (uint32_t)C, uD = (uint32_t)D;
    std::unique_ptr<tdx_emo2v> h(new tdx_emo2v());
    h->device = device; h->c = c; h->gw = gw; h->NP = NP;

    const int nb = c.prenet_depth + c.depth;
    h->gcw.resize(c.pos_layers); h->gcb.resize(c.pos_layers); h->blocks.resize(nb);      // final sizes: their elements are bound below

    // conv 0 [C][1][k] -> tap-major [k][C]
    ld.push_tapmajor(h->w0, ld.get("conv.0.weight", {uC, 1u, (uint32_t)c.conv_k[0]}), C, c.conv_k[0]);
    for (int i = 0; i < c.n_conv; ++i) {
        const std::string p = "conv." + std::to_string(i) + ".";
        if (i > 0) ld.bind(h->cw[i], push_conv_gemm<float>(ld, ld.get(p + "weight", {uC, uC, (uint32_t)c.conv_k[i]}), nullptr, nullptr, C, C, c.conv_k[i], Cp, C).w);
        ld.push(i ? h->clg[i] : h->ln0g, ld.get(p + "ln.weight", {uC}), C);
        ld.push(i ? h->clb[i] : h->ln0b, ld.get(p + "ln.bias", {uC}), C);
    }
    ld.push(h->plg, ld.get("proj.ln.weight", {uC}), C); ld.push(h->plb, ld.get("proj.ln.bias", {uC}), C);
    bind(ld, h->pw, h->pb, push_linear(ld, ld.get("proj.weight", {uD, uC}), ld.get("proj.bias", {uD}), D, C, Dp, C));
    // positional conv [D][gw][k] -> [G][k][NP][gw]
    for (int l = 0; l < c.pos_layers; ++l) {
        const std::string p = "pos." + std::to_string(l) + ".";
        const float* W = ld.get(p + "weight", {uD, (uint32_t)gw, (uint32_t)c.pos_k});
        const size_t gcw = ld.room(h->gcw[l], (size_t)c.pos_groups * c.pos_k * NP * gw);
        if (W)
            for (int g = 0; g < c.pos_groups; ++g) for (int t = 0; t < c.pos_k; ++t) for (int n = 0; n < gw; ++n) for (int ci = 0; ci < gw; ++ci)
                ld.host[gcw + (((size_t)g * c.pos_k + t) * NP + n) * gw + ci] = W[((size_t)(g * gw + n) * gw + ci) * c.pos_k + t];
        ld.push(h->gcb[l], ld.get(p + "bias", {uD}), D);
    }
    ld.push(h->extra, c.E ? ld.get("extra_tokens", {1u, (uint32_t)c.E, uD}) : nullptr, (size_t)c.E * D, 64);
    // -slope_h max(scale_h, 0)
    const size_t nslope = ld.room(h->nslope, c.H);
    if (const float* sc = ld.get("alibi_scale", {1u, 1u, (uint32_t)c.H, 1u, 1u})) {
        std::vector<double> sl;
        alibi_slopes(c.H, sl);
        for (int i = 0; i < c.H; ++i) ld.host[nslope + i] = (float)(-sl[i] * std::max((double)sc[i], 0.0));
    }
    ld.push(h->eng, ld.get("prenet.norm.weight", {uD}), D); ld.push(h->enb, ld.get("prenet.norm.bias", {uD}), D);
    for (int l = 0; l < nb; ++l) {
        const std::string p = (l < c.prenet_depth ? "prenet.blocks." + std::to_string(l) : "blocks." + std::to_string(l - c.prenet_depth)) + ".";
        Block& w = h->blocks[l];
        bind(ld, w.Wqkv, w.bqkv, push_linear(ld, ld.get(p + "attn.qkv.weight", {3 * uD, uD}), ld.get(p + "attn.qkv.bias", {3 * uD}), 3 * D, D, up(3 * D, 128), D));
        bind(ld, w.Wo, w.bo, push_linear(ld, ld.get(p + "attn.proj.weight", {uD, uD}), ld.get(p + "attn.proj.bias", {uD}), D, D, Dp, D));
        ld.push(w.g1, ld.get(p + "norm1.weight", {uD}), D); ld.push(w.b1n, ld.get(p + "norm1.bias", {uD}), D);
        bind(ld, w.W1, w.b1, push_linear(ld, ld.get(p + "mlp.fc1.weight", {4 * uD, uD}), ld.get(p + "mlp.fc1.bias", {4 * uD}), 4 * D, D, up(4 * D, 128), D));
        bind(ld, w.W2, w.b2, push_linear(ld, ld.get(p + "mlp.fc2.weight", {uD, 4 * uD}), ld.get(p + "mlp.fc2.bias", {uD}), D, 4 * D, Dp, 4 * D));
        ld.push(w.g2, ld.get(p + "norm2.weight", {uD}), D); ld.push(w.b2n, ld.get(p + "norm2.bias", {uD}), D);
    }
    ld.push(h->hw, ld.get("head.weight", {(uint32_t)c.n_classes, uD}), (size_t)c.n_classes * D);
    ld.push(h->hb, ld.get("head.bias", {(uint32_t)c.n_classes}), c.n_classes);
    TRY(ld.finish("tdx_emo2v_create", true, device, h->dev));
    *out = h.release();
    return TDX_OK;
}

int tdx_emo2v_destroy(tdx_emo2v* h) {
    delete h;
    return TDX_OK;
}

long tdx_emo2v_frames(const tdx_emo2v* h, long N) {
    if (!h || N < 1) return 0;
    const Frames f = frames_of(h->c, N);
    return f.ok ? f.L[h->c.n_conv] : 0;
}

size_t tdx_emo2v_workspace_bytes(const tdx_emo2v* h, int B, long N) {
    if (!h || B < 1 || N < 1) return 0;
    const Frames f = frames_of(h->c, N);
    if (!f.ok || f.L[h->c.n_conv] < 1) return 0;
    return ws_plan(h, B, f).total * sizeof(float);
}

int tdx_emo2v_forward(tdx_emo2v* h, const float* wav_dev, int B, long N, float* feats_dev, float* emb_dev, float* scores_dev, void* ws, size_t ws_bytes,
                      void* stream) {
    TRY(check_forward_args(h, wav_dev, B, N, ws, "tdx_emo2v_forward"));
    return forward_impl(h, wav_dev, B, N, feats_dev, emb_dev, scores_dev, nullptr, nullptr, nullptr, nullptr, ws, ws_bytes, (hipStream_t)stream);
}

int tdx_emo2v_forward_taps(tdx_emo2v* h, const float* wav_dev, int B, long N, float* feats_dev, float* emb_dev, float* scores_dev, float* tap_proj_dev,
                           float* tap_pos_dev, float* tap_qkv_dev, float* tap_attn_dev, void* ws, size_t ws_bytes, void* stream) {
    TRY(check_forward_args(h, wav_dev, B, N, ws, "tdx_emo2v_forward_taps"));
    return forward_impl(h, wav_dev, B, N, feats_dev, emb_dev, scores_dev, tap_proj_dev, tap_pos_dev, tap_qkv_dev, tap_attn_dev, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
