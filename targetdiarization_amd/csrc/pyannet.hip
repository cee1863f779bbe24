// pyannet.hip — pyannote segmentation-3.0 ("PyanNet": SincNet front end, 4-layer bidirectional LSTM, two linears, a 7-class
// powerset classifier with log-softmax) on MI355X.  The network behind `self.od_pipeline` (TargetDiarization.py:84,132,143);
// third-party, parity unpinned [upstream-recall] — tests/pyannet_oracle.py restates it, DESIGN §8.12 governs.
// wav [B,T] (16 kHz, 1261 <= T <= 160000) -> logp [B,F,7]; taps: the SincNet output [B,F,60] and the LSTM output [B,F,256].
//
// 22 launches per forward, whatever B and T; everything fp32, activations channel-last:
//   wav_stats_kernel        per chunk, 64 slices: (mean, M2) of each slice                       (InstanceNorm1d(1), phase 1)
//   sinc_kernel             phase 2 of the waveform norm (two scalars per chunk) + the 80 x 251 sinc filters at stride 10
//                           + abs + MaxPool3, taps and waveform tile in LDS; only the pooled [B,p1,80] is written
//   3 x { norm_stats_kernel per chunk and channel, 32 slices of frames: (mean, M2) of the (pooled) input        (phase 1)
//         norm_apply_kernel phase 2 (Chan's combination in fp64, in slice order) + normalise + leaky_relu, pooling on the fly
//         GEMM              (stages 1, 2) the k5 convolution: frames t..t+4 of C channels are 5C contiguous floats, so
//                           it is the fp32 MFMA core with lda = C (overlapping rows), K = 5C padded with zero weight columns }
//   4 x { GEMM              input projection of both directions [B F, in] x [in, 1024] + (b_ih + b_hh)
//         lstm_rec_kernel   the recurrence: ONE launch per layer, grid (tiles of 2 chunks, direction) }
//   GEMM, GEMM, GEMM        linear 256->128, 128->128 (+ leaky_relu), classifier 128->7
//   logsoftmax_kernel       one thread per frame
// No statistic is accumulated with atomics, and every reduction has a fixed order that depends on the chunk alone: a chunk's
// result does not depend on its neighbours in the batch.
//
// The recurrence.  W_hh of one direction is [512 x 128] fp32 = 256 KB: more than the LDS, half of the CU's register file.  A
// workgroup of 512 threads owns one (direction, tile of chunks) and walks all F steps; thread (u, q) = (tid / 4, tid % 4)
// keeps rows {i,f,g,o} of unit u, columns 32q..32q+31, in 128 registers for the whole launch.  A step: each thread reads its
// quarter of h from LDS (8 x ds_read_b128, slice pitch 36 floats so the four quarters fall on different banks), 128 FMAs,
// two DPP quad exchanges give every lane of the quad the four gate sums, the cell update is computed redundantly in the
// quad, lane q = 0 writes h to the other LDS buffer and to the output: one barrier per step.  The projected input of step
// t + 2 is loaded at step t, one value per lane (the projection's columns are permuted to u*4 + gate at load time so a wave
// reads 256 contiguous bytes), and enters lane q's partial sum of gate q.  The 128 FMAs per thread run at the vector rate,
// which on this chip is the fp32 MFMA rate as well, so a [tile x 128].[128 x 512] MFMA form was not built; chunks of a
// tile (REC_TILE, reported by tdx_pyannet_chunk_tile) are walked one after the other by the same code, a tile with one chunk
// simply does half the work.  Neither choice has been timed; DESIGN §8.12 (Times) has the cycle bounds of both.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tdx.h"
#include "epilogues.hpp"
#include "weight_pack.hpp"

using namespace tdx;

namespace {

constexpr int T_MIN = 1261, T_MAX = 160000, B_MAX = 1024;
constexpr int NTAP = 251, SINC_STRIDE = 10, C0 = 80, C1 = 60, KCONV = 5;
constexpr int K1 = C0 * KCONV, K1P = 416, K2 = C1 * KCONV, K2P = 320;      // conv GEMM K, padded to the core's BK = 32
constexpr int HID = 128, GATES = 4 * HID, NDIR = 2, NLAYER = 4, LSTM_OUT = NDIR * HID, XP = NDIR * GATES;
constexpr int SIN = 64;                        // the SincNet output's row pitch: 60 channels + 4 zeros (K of layer 0's projection)
constexpr int NCLS = 7, LOGIT_LD = 8;
constexpr int WAV_PARTS = 64, NORM_PARTS = 32;
constexpr int SINC_HALF = C0 / 2, SINC_FRAMES = 48, SINC_CONV = 3 * SINC_FRAMES;     // per block: 40 channels x 48 pooled frames
constexpr int SINC_SAMPLES = (SINC_CONV - 1) * SINC_STRIDE + NTAP;                   // 1681
constexpr int APPLY_ROWS = 64;
#ifndef TDX_PYANNET_REC_TILE
#define TDX_PYANNET_REC_TILE 2                 // chunks per workgroup of the recurrence; -D overrides it for tools/pyannet_bench.py's comparison
#endif
constexpr int REC_TILE = TDX_PYANNET_REC_TILE, REC_THREADS = 512, H_PITCH = 4 * 36;
static_assert(REC_TILE >= 1 && REC_TILE * H_PITCH <= REC_THREADS, "one thread zeroes one float of the first h buffer");
constexpr int SLACK = 64;                      // floats after a conv input for the last rows' K-padding over-read (<= 20)
constexpr float EPS = 1e-5f, SLOPE = 0.01f;
static_assert(SLOPE == 1.0f / 100.0f, "dense() applies the slope as ActLeaky<1, 100>");

struct Dims { int n1, p1, n2, p2, n3, F; };
inline Dims dims_of(int T) {
    Dims d{};
    d.n1 = (T - NTAP) / SINC_STRIDE + 1; d.p1 = d.n1 / 3;
    d.n2 = d.p1 - (KCONV - 1); d.p2 = d.n2 / 3;
    d.n3 = d.p2 - (KCONV - 1); d.F = d.n3 / 3;
    return d;
}

// sum over the 256 threads of a block, the same value in every thread; s4: 4 floats of LDS
__device__ __forceinline__ float block_sum256(float v, float* s4) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    __syncthreads();
    return r;
}

// Phase 2 of a two-phase mean / biased variance: slices j = 0..nparts-1 of `per` items each (the last ones shorter or
// empty) carry (mean_j, M2_j) at part[j * stride]; combined in slice order in fp64 (Chan et al.).
__device__ __forceinline__ void combine_parts(const float2* part, int stride, int nparts, int total, int per, double& mean, double& var) {
    double n = 0.0, mu = 0.0, m2 = 0.0;
    for (int j = 0; j < nparts; ++j) {
        const int nj = min(per, total - j * per);
        if (nj <= 0) break;
        const float2 p = part[(size_t)j * stride];
        const double d = (double)p.x - mu, nn = n + nj;
        mu += d * nj / nn;
        m2 += (double)p.y + d * d * n * nj / nn;
        n = nn;
    }
    mean = mu; var = m2 / n;
}

// (a) waveform statistics, phase 1: block (j, b) owns samples [j*per, (j+1)*per) of chunk b
__global__ __launch_bounds__(256) void wav_stats_kernel(const float* __restrict__ wav, float2* __restrict__ part, int T) {
    __shared__ float s4[4];
    const int j = blockIdx.x, b = blockIdx.y, per = (T + WAV_PARTS - 1) / WAV_PARTS;
    const int s0 = j * per, s1 = min(T, s0 + per), n = s1 - s0;
    const float* x = wav + (size_t)b * T;
    float acc = 0.f;
    for (int i = s0 + (int)threadIdx.x; i < s1; i += 256) acc += x[i];
    const float mean = n > 0 ? block_sum256(acc, s4) / (float)n : 0.f;
    acc = 0.f;
    for (int i = s0 + (int)threadIdx.x; i < s1; i += 256) { const float d = x[i] - mean; acc = fmaf(d, d, acc); }
    const float m2 = n > 0 ? block_sum256(acc, s4) : 0.f;
    if (threadIdx.x == 0) part[(size_t)b * WAV_PARTS + j] = make_float2(mean, m2);
}

// (b) waveform norm + sinc filters (stride 10) + abs + MaxPool3.  Block (x, hc, b): pooled frames [48x, 48x+48) of channels
// [40hc, 40hc+40) of chunk b.  Thread (g, q) = (tid / 10, tid % 10), tid < 240: channels 4q..4q+3 of the half, pooled frames
// 2g, 2g+1 of the tile = 6 consecutive filter outputs.  taps: [251][80] (tap-major).
__global__ __launch_bounds__(256) void sinc_kernel(const float* __restrict__ wav, const float2* __restrict__ wpart, const float* __restrict__ wn,
                                                    const float* __restrict__ taps, float* __restrict__ out, int T, int p1) {
    __shared__ __attribute__((aligned(16))) float ts[NTAP * SINC_HALF];
    __shared__ float xs[SINC_SAMPLES + 3];
    __shared__ float s_ab[2];
    const int tid = threadIdx.x, hc = blockIdx.y, b = blockIdx.z, pf0 = blockIdx.x * SINC_FRAMES;
    if (tid == 0) {
        double mean, var;
        combine_parts(wpart + (size_t)b * WAV_PARTS, 1, WAV_PARTS, T, (T + WAV_PARTS - 1) / WAV_PARTS, mean, var);
        const float a = wn[0] * (float)(1.0 / sqrt(var + (double)EPS));
        s_ab[0] = a; s_ab[1] = wn[1] - (float)mean * a;
    }
    for (int i = tid; i < NTAP * (SINC_HALF / 4); i += 256) {
        const int k = i / (SINC_HALF / 4), c4 = (i - k * (SINC_HALF / 4)) * 4;
        *reinterpret_cast<f32x4*>(ts + k * SINC_HALF + c4) = ldg4(taps + k * C0 + hc * SINC_HALF + c4);
    }
    __syncthreads();
    {
        const float a = s_ab[0], c = s_ab[1];
        const float* x = wav + (size_t)b * T;
        const int s0 = pf0 * 3 * SINC_STRIDE;
        for (int i = tid; i < SINC_SAMPLES; i += 256) xs[i] = s0 + i < T ? fmaf(x[s0 + i], a, c) : 0.f;
    }
    __syncthreads();
    if (tid >= 240) return;
    const int g = tid / 10, q = tid - g * 10;
    f32x4 acc[6];
#pragma unroll
    for (int o = 0; o < 6; ++o) acc[o] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* xp = xs + g * 6 * SINC_STRIDE;
    const float* tp = ts + q * 4;
#pragma unroll 4
    for (int k = 0; k < NTAP; ++k) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(tp + k * SINC_HALF);
#pragma unroll
        for (int o = 0; o < 6; ++o) {
            const float xv = xp[o * SINC_STRIDE + k];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[o][c] = fmaf(w[c], xv, acc[o][c]);
        }
    }
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
        const int p = pf0 + 2 * g + pp;
        if (p >= p1) break;
        f32x4 v;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = fmaxf(fmaxf(fabsf(acc[3 * pp][c]), fabsf(acc[3 * pp + 1][c])), fabsf(acc[3 * pp + 2][c]));
        *reinterpret_cast<f32x4*>(out + ((size_t)b * p1 + p) * C0 + hc * SINC_HALF + q * 4) = v;
    }
}

// frame f, channel c of the normalised tensor's input: the value itself, or the max over input rows 3f..3f+2
template <int C, int POOL>
__device__ __forceinline__ float pooled(const float* __restrict__ in, int f, int c) {
    if constexpr (POOL == 1) return in[(size_t)f * C + c];
    const float* p = in + (size_t)f * 3 * C + c;
    return fmaxf(fmaxf(p[0], p[C]), p[2 * C]);
}

// (c) InstanceNorm statistics, phase 1: block (j, b) owns frames [j*per, (j+1)*per) of chunk b; thread (r, c) = (tid / C,
// tid % C) sums frames r, r+R, ...; the R partial sums of a channel are added in the order of r.
template <int C, int POOL>
__global__ __launch_bounds__(256) void norm_stats_kernel(const float* __restrict__ in, float2* __restrict__ part, int rows_in, int P) {
    constexpr int R = 256 / C;
    __shared__ float red[R * C], smean[C];
    const int j = blockIdx.x, b = blockIdx.y, per = (P + NORM_PARTS - 1) / NORM_PARTS;
    const int f0 = j * per, f1 = min(P, f0 + per), n = f1 - f0;
    const int r = threadIdx.x / C, c = threadIdx.x - r * C;
    const float* x = in + (size_t)b * rows_in * C;
    float acc = 0.f;
    if (r < R) { for (int f = f0 + r; f < f1; f += R) acc += pooled<C, POOL>(x, f, c); red[r * C + c] = acc; }
    __syncthreads();
    if (r == 0) {
        float s = red[c];
#pragma unroll
        for (int i = 1; i < R; ++i) s += red[i * C + c];
        smean[c] = n > 0 ? s / (float)n : 0.f;
    }
    __syncthreads();
    if (r < R) {
        const float mean = smean[c];
        acc = 0.f;
        for (int f = f0 + r; f < f1; f += R) { const float d = pooled<C, POOL>(x, f, c) - mean; acc = fmaf(d, d, acc); }
        red[r * C + c] = acc;
    }
    __syncthreads();
    if (r == 0) {
        float s = red[c];
#pragma unroll
        for (int i = 1; i < R; ++i) s += red[i * C + c];
        part[((size_t)b * NORM_PARTS + j) * C + c] = make_float2(smean[c], n > 0 ? s : 0.f);
    }
}

// (d) phase 2 + normalise + leaky_relu: out[b][f][0..ldo) = leaky((pooled - mean) * rsqrt(var + eps) * w + bias), columns
// C..ldo-1 zero; tap (or NULL) gets the same values at pitch C.  Block (x, b): APPLY_ROWS frames.  The very last block also
// zeroes `slack` floats behind the tensor (the next convolution's K padding reads them against zero weights).
template <int C, int POOL>
__global__ __launch_bounds__(256) void norm_apply_kernel(const float* in, const float2* __restrict__ part, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* out, float* __restrict__ tap,
                                                          int rows_in, int P, int ldo, int slack) {
    __shared__ float sa[C], sc[C];
    const int b = blockIdx.y, f0 = blockIdx.x * APPLY_ROWS, f1 = min(P, f0 + APPLY_ROWS), tid = threadIdx.x;
    if (tid < C) {
        double mean, var;
        combine_parts(part + (size_t)b * NORM_PARTS * C + tid, C, NORM_PARTS, P, (P + NORM_PARTS - 1) / NORM_PARTS, mean, var);
        const float a = w[tid] * (float)(1.0 / sqrt(var + (double)EPS));
        sa[tid] = a; sc[tid] = bias[tid] - (float)mean * a;
    }
    __syncthreads();
    const float* x = in + (size_t)b * rows_in * C;
    for (int i = tid; i < (f1 - f0) * ldo; i += 256) {
        const int fl = i / ldo, c = i - fl * ldo, f = f0 + fl;
        float v = 0.f;
        if (c < C) {
            v = leaky(fmaf(pooled<C, POOL>(x, f, c), sa[c], sc[c]), SLOPE);
            if (tap) tap[((size_t)b * P + f) * C + c] = v;
        }
        out[((size_t)b * P + f) * ldo + c] = v;
    }
    if (slack > 0 && blockIdx.y == gridDim.y - 1 && blockIdx.x == gridDim.x - 1 && tid < slack)
        out[(size_t)gridDim.y * P * ldo + tid] = 0.f;
}

// (e) the LSTM recurrence of one layer (file comment).  xp [B*F][1024]: column dir*512 + u*4 + gate (i, f, g, o);
// whh [2][512][128]: row u*4 + gate of each direction; y [B*F][256]: [h_fwd | h_bwd].
__global__ __launch_bounds__(REC_THREADS) void lstm_rec_kernel(const float* __restrict__ xp, const float* __restrict__ whh,
                                                                float* __restrict__ y, int B, int F) {
    __shared__ __attribute__((aligned(16))) float hs[2][REC_TILE][H_PITCH];
    const int tid = threadIdx.x, u = tid >> 2, q = tid & 3;
    const int dir = blockIdx.y, b0 = blockIdx.x * REC_TILE, nb = min(REC_TILE, B - b0);
    float w[4][32];
    {
        const float* wp = whh + ((size_t)dir * GATES + u * 4) * HID + q * 32;
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int k = 0; k < 32; k += 4) {
                const f32x4 v = ldg4(wp + g * HID + k);
                w[g][k] = v[0]; w[g][k + 1] = v[1]; w[g][k + 2] = v[2]; w[g][k + 3] = v[3];
            }
    }
    if (tid < REC_TILE * H_PITCH) (&hs[0][0][0])[tid] = 0.f;
    const int t0 = dir ? F - 1 : 0, dt = dir ? -1 : 1;
    const float* xcol = xp + dir * GATES + tid;
    float c[REC_TILE], xa[REC_TILE], xb[REC_TILE];
#pragma unroll
    for (int b = 0; b < REC_TILE; ++b) {
        c[b] = 0.f; xa[b] = 0.f; xb[b] = 0.f;
        if (b < nb) {
            const float* xr = xcol + (size_t)(b0 + b) * F * XP;
            xa[b] = xr[(size_t)t0 * XP];
            if (F > 1) xb[b] = xr[(size_t)(t0 + dt) * XP];
        }
    }
    const int hw = (u >> 5) * 36 + (u & 31);
    __syncthreads();
    for (int s = 0; s < F; ++s) {
        const int t = t0 + s * dt, cur = s & 1;
        float xc[REC_TILE];
#pragma unroll
        for (int b = 0; b < REC_TILE; ++b) {
            xc[b] = xa[b]; xa[b] = xb[b];
            if (b < nb && s + 2 < F) xb[b] = xcol[((size_t)(b0 + b) * F + (t + 2 * dt)) * XP];
        }
#pragma unroll
        for (int b = 0; b < REC_TILE; ++b) {
            if (b >= nb) break;
            float a0 = q == 0 ? xc[b] : 0.f, a1 = q == 1 ? xc[b] : 0.f, a2 = q == 2 ? xc[b] : 0.f, a3 = q == 3 ? xc[b] : 0.f;
            const f32x4* hp = reinterpret_cast<const f32x4*>(&hs[cur][b][q * 36]);
#pragma unroll
            for (int k4 = 0; k4 < 8; ++k4) {
                const f32x4 hv = hp[k4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a0 = fmaf(w[0][k4 * 4 + j], hv[j], a0); a1 = fmaf(w[1][k4 * 4 + j], hv[j], a1);
                    a2 = fmaf(w[2][k4 * 4 + j], hv[j], a2); a3 = fmaf(w[3][k4 * 4 + j], hv[j], a3);
                }
            }
            a0 += h3_dpp(a0, 0); a1 += h3_dpp(a1, 0); a2 += h3_dpp(a2, 0); a3 += h3_dpp(a3, 0);
            a0 += h3_dpp(a0, 1); a1 += h3_dpp(a1, 1); a2 += h3_dpp(a2, 1); a3 += h3_dpp(a3, 1);
            const float cn = fmaf(sigmoid_full(a1), c[b], sigmoid_full(a0) * tanhf(a2));
            const float h = sigmoid_full(a3) * tanhf(cn);
            c[b] = cn;
            if (q == 0) {
                hs[cur ^ 1][b][hw] = h;
                y[((size_t)(b0 + b) * F + t) * LSTM_OUT + dir * HID + u] = h;
            }
        }
        __syncthreads();
    }
}

// (f) log-softmax over the 7 classes, one thread per frame: logits [rows][8] -> logp [rows][7]
__global__ __launch_bounds__(256) void logsoftmax_kernel(const float* __restrict__ logits, float* __restrict__ logp, int rows) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const f32x4 lo = ldg4(logits + (size_t)r * LOGIT_LD), hi = ldg4(logits + (size_t)r * LOGIT_LD + 4);
    const float x[NCLS] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2]};
    float m = x[0];
#pragma unroll
    for (int i = 1; i < NCLS; ++i) m = fmaxf(m, x[i]);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NCLS; ++i) s += expf(x[i] - m);
    const float lse = m + logf(s);
#pragma unroll
    for (int i = 0; i < NCLS; ++i) logp[(size_t)r * NCLS + i] = x[i] - lse;
}

struct EpiConv {        // batch z = chunk: out[z][m][n] = v + b[n], n < 60
    const float* b; float* out; long rows;
    __device__ float col(int, int n) const { return b[n]; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int z, int m, int n, float v, EpiNone, float c) const {
        if (n < C1) out[((long)z * rows + m) * C1 + n] = v + c;
    }
};

using Lin = tdx::GemmW;

// columns < l.N: out[m][n] = v + b[n], optionally leaky_relu
int dense(const float* A, long lda, const float* dev, const Lin& l, int M, float* out, long ldo, bool act, hipStream_t st) {
    if (act) return linear_f32(A, lda, dev + l.w, M, l.Npad, l.Kp, EpiBiasActN<ActLeaky<1, 100>>{dev + l.b, out, ldo, l.N}, st, up(l.N, 32));
    return linear_f32(A, lda, dev + l.w, M, l.Npad, l.Kp, EpiBiasActN<>{dev + l.b, out, ldo, l.N}, st, up(l.N, 32));
}

// the k5 convolution of B chunks: in [B][rows_in][C] (normalised), out [B][rows_in - 4][60]
int conv5(const float* in, int C, int rows_in, const float* dev, const Lin& l, int B, float* out, hipStream_t st) {
    const int M = rows_in - (KCONV - 1);
    GemmArgs g = make_args(M, l.Npad, make_seg(in, C, dev + l.w, l.Kp, l.Kp, (long)rows_in * C));
    g.n_valid = up(l.N, 32);
    if (launch_gemm<false, false, false, false>(g, B, EpiConv{dev + l.b, out, (long)M}, st) != hipSuccess)
        return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
    return TDX_OK;
}

}  // namespace

struct tdx_pyannet {
    int device = 0;
    tdx::DevBuf dev;
    size_t wav_norm, taps, norm_w[3], norm_b[3];
    Lin conv[2], proj[NLAYER], lin[2], cls;
    size_t whh[NLAYER];
};

extern "C" {

int tdx_pyannet_create(const void* blob, size_t blob_bytes, int device, tdx_pyannet** out) {
    if (!blob || !out) return tdx::fail(TDX_E_INVALID, "tdx_pyannet_create: null argument");
    tdx::Loader ld;
    if (!ld.parse(blob, blob_bytes)) return tdx::fail(TDX_E_BLOB, "tdx_pyannet_create: malformed TDXW blob");
    std::unique_ptr<tdx_pyannet> h(new tdx_pyannet());
    {
        const float* w = ld.get("sincnet.wav_norm1d.weight", {1u});
        const float* b = ld.get("sincnet.wav_norm1d.bias", {1u});
        h->wav_norm = ld.room(2);
        if (w && b) { ld.host[h->wav_norm] = w[0]; ld.host[h->wav_norm + 1] = b[0]; }
    }
    {   // asteroid ParamSincFB: 40 cosine + 40 sine band-pass filters of 251 taps from (low_hz_, band_hz_), in fp64; tap-major
        const float* lo = ld.get("sincnet.conv1d.0.filterbank.low_hz_", {40u, 1u});
        const float* bw = ld.get("sincnet.conv1d.0.filterbank.band_hz_", {40u, 1u});
        h->taps = ld.room((size_t)NTAP * C0);
        if (lo && bw) {
            const double pi = 3.14159265358979323846;
            const int half = NTAP / 2;      // 125
            for (int f = 0; f < 40; ++f) {
                const double low = 50.0 + std::fabs((double)lo[f]);
                const double high = std::min(std::max(low + 50.0 + std::fabs((double)bw[f]), 50.0), 8000.0);
                const double band = high - low, norm = 2.0 * band;
                float* tc = ld.host.data() + h->taps + f;
                float* tsn = ld.host.data() + h->taps + 40 + f;
                for (int i = 0; i < half; ++i) {
                    const double n = 2.0 * pi * (double)(i - half) / 16000.0;
                    const double win = 0.54 - 0.46 * std::cos(2.0 * pi * ((double)i * 124.5 / 124.0) / (double)NTAP);
                    const double cl = (std::sin(high * n) - std::sin(low * n)) / (n / 2.0) * win / norm;
                    const double sl = (std::cos(low * n) - std::cos(high * n)) / (n / 2.0) * win / norm;
                    tc[(size_t)i * C0] = (float)cl;  tc[(size_t)(NTAP - 1 - i) * C0] = (float)cl;
                    tsn[(size_t)i * C0] = (float)sl; tsn[(size_t)(NTAP - 1 - i) * C0] = (float)-sl;
                }
                tc[(size_t)half * C0] = 1.0f; tsn[(size_t)half * C0] = 0.0f;
            }
        }
    }
    for (int i = 0; i < 3; ++i) {
        const uint32_t c = i == 0 ? C0 : C1;
        const std::string p = "sincnet.norm1d." + std::to_string(i) + ".";
        h->norm_w[i] = ld.push(ld.get(p + "weight", {c}), c);
        h->norm_b[i] = ld.push(ld.get(p + "bias", {c}), c);
    }
    // Conv1d weight [60][Cin][5] -> GEMM B [128][Kp], column k*Cin + c (the input is channel-last); rows 60.., columns 5Cin.. zero
    for (int i = 0; i < 2; ++i) {
        const int cin = i == 0 ? C0 : C1, Kp = i == 0 ? K1P : K2P;
        const std::string p = "sincnet.conv1d." + std::to_string(i + 1) + ".";
        const float* w = ld.get(p + "weight", {(uint32_t)C1, (uint32_t)cin, (uint32_t)KCONV});
        const float* b = ld.get(p + "bias", {(uint32_t)C1});
        h->conv[i] = tdx::push_conv_gemm(ld, w, nullptr, b, C1, cin, KCONV, GEMM_BN, cin, Kp);
    }
    // LSTM: both directions' W_ih as one [1024][Kp] matrix with rows permuted to dir*512 + u*4 + gate, bias b_ih + b_hh
    // likewise; W_hh [2][512][128] in the same row order
    for (int l = 0; l < NLAYER; ++l) {
        const int in = l == 0 ? C1 : LSTM_OUT, Kp = l == 0 ? SIN : LSTM_OUT;
        Lin& pj = h->proj[l];
        pj.N = XP; pj.Npad = XP; pj.Kp = Kp;
        pj.w = ld.room((size_t)XP * Kp); pj.b = ld.room(XP);
        h->whh[l] = ld.room((size_t)NDIR * GATES * HID);
        for (int d = 0; d < NDIR; ++d) {
            const std::string sfx = "_l" + std::to_string(l) + (d ? "_reverse" : "");
            const float* wih = ld.get("lstm.weight_ih" + sfx, {(uint32_t)GATES, (uint32_t)in});
            const float* whh = ld.get("lstm.weight_hh" + sfx, {(uint32_t)GATES, (uint32_t)HID});
            const float* bih = ld.get("lstm.bias_ih" + sfx, {(uint32_t)GATES});
            const float* bhh = ld.get("lstm.bias_hh" + sfx, {(uint32_t)GATES});
            tdx::push_lstm_gates(ld, wih, whh, bih, bhh, HID, in, pj, h->whh[l], d * GATES);
        }
    }
    auto linear = [&](const std::string& p, int N, int K) -> Lin {
        const float* w = ld.get(p + "weight", {(uint32_t)N, (uint32_t)K});
        const float* b = ld.get(p + "bias", {(uint32_t)N});
        return tdx::push_linear(ld, w, b, N, K, GEMM_BN, K);
    };
    h->lin[0] = linear("linear.0.", HID, LSTM_OUT);
    h->lin[1] = linear("linear.1.", HID, HID);
    h->cls = linear("classifier.", NCLS, HID);
    h->device = device;
    TRY(ld.finish("tdx_pyannet_create", true, device, h->dev));
    *out = h.release();
    return TDX_OK;
}

int tdx_pyannet_destroy(tdx_pyannet* h) {
    delete h;
    return TDX_OK;
}

int tdx_pyannet_chunk_tile(void) { return REC_TILE; }

int tdx_pyannet_frames(int T) {
    if (T < T_MIN || T > T_MAX) return 0;
    return dims_of(T).F;
}

namespace {
// `front` holds the SincNet stages' tensors; the projected LSTM input reuses it once they are dead (the SincNet output
// lives in `s`)
struct WsPlan { size_t wpart, npart, pool0, c1, a2, c2, front, s, y, hd, logits, total; };
inline WsPlan ws_plan(int B, int T) {
    const Dims d = dims_of(T);
    const size_t b = (size_t)B, rows = b * d.F;
    WsPlan w{};
    w.wpart = al(b * WAV_PARTS * 2); w.npart = al(b * NORM_PARTS * C0 * 2);
    w.pool0 = al(b * d.p1 * C0 + SLACK); w.c1 = al(b * d.n2 * C1); w.a2 = al(b * d.p2 * C1 + SLACK); w.c2 = al(b * d.n3 * C1);
    w.front = std::max(w.pool0 + w.c1 + w.a2 + w.c2, al(rows * XP));
    w.s = al(rows * SIN); w.y = al(rows * LSTM_OUT); w.hd = al(rows * HID); w.logits = al(rows * LOGIT_LD);
    w.total = w.wpart + w.npart + w.front + w.s + 2 * w.y + 2 * w.hd + w.logits;
    return w;
}
}  // namespace

size_t tdx_pyannet_workspace_bytes(const tdx_pyannet* h, int B, int T) {
    if (!h || B < 1 || B > B_MAX || T < T_MIN || T > T_MAX) return 0;
    return ws_plan(B, T).total * sizeof(float);
}

double tdx_pyannet_flops(const tdx_pyannet* h, int B, int T) {
    if (!h || B < 1 || T < T_MIN || T > T_MAX) return 0.0;
    const Dims d = dims_of(T);
    double per = 2.0 * d.n1 * C0 * NTAP + 2.0 * d.n2 * C1 * K1 + 2.0 * d.n3 * C1 * K2;
    double frame = 2.0 * C1 * XP + (NLAYER - 1) * 2.0 * LSTM_OUT * XP + NLAYER * 2.0 * NDIR * GATES * HID;
    frame += 2.0 * (LSTM_OUT * HID + HID * HID + HID * NCLS);
    return (per + frame * d.F) * B;
}

int tdx_pyannet_forward(tdx_pyannet* h, const float* wav, int B, int T, float* logp, float* tap_sincnet, float* tap_lstm,
                        void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !wav || !logp || !ws_) return tdx::fail(TDX_E_INVALID, "tdx_pyannet_forward: bad argument");
    if (B < 1 || B > B_MAX) return tdx::fail(TDX_E_INVALID, "tdx_pyannet_forward: B must be in [1, 1024]");
    if (T < T_MIN || T > T_MAX) return tdx::fail(TDX_E_INVALID, "tdx_pyannet_forward: T must be in [1261, 160000]");
    const WsPlan wp = ws_plan(B, T);
    if (ws_bytes < wp.total * sizeof(float)) return tdx::fail(TDX_E_WORKSPACE, "tdx_pyannet_forward: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    const Dims d = dims_of(T);
    const int rows = B * d.F;
    float* ws = (float*)ws_;
    float2* wpart = (float2*)ws;
    float2* npart = (float2*)(ws + wp.wpart);
    float* front = ws + wp.wpart + wp.npart;
    float* pool0 = front; float* c1 = pool0 + wp.pool0; float* a2 = c1 + wp.c1; float* c2 = a2 + wp.a2;
    float* xp = front;
    float* s = front + wp.front;
    float* y[2] = {s + wp.s, s + wp.s + wp.y};
    float* hd[2] = {y[1] + wp.y, y[1] + wp.y + wp.hd};
    float* logits = hd[1] + wp.hd;
    const float* dev = h->dev;
    auto blocks = [](int n, int per) { return (unsigned)((n + per - 1) / per); };

    hipLaunchKernelGGL(wav_stats_kernel, dim3(WAV_PARTS, B), dim3(256), 0, st, wav, wpart, T);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(sinc_kernel, dim3(blocks(d.p1, SINC_FRAMES), 2, B), dim3(256), 0, st, wav, (const float2*)wpart, dev + h->wav_norm,
                       dev + h->taps, pool0, T, d.p1);
    LAUNCH_CHECK();
    // stage 0: the pooled sinc output is normalised in place
    hipLaunchKernelGGL((norm_stats_kernel<C0, 1>), dim3(NORM_PARTS, B), dim3(256), 0, st, (const float*)pool0, npart, d.p1, d.p1);
    LAUNCH_CHECK();
    hipLaunchKernelGGL((norm_apply_kernel<C0, 1>), dim3(blocks(d.p1, APPLY_ROWS), B), dim3(256), 0, st, (const float*)pool0, (const float2*)npart,
                       dev + h->norm_w[0], dev + h->norm_b[0], pool0, (float*)nullptr, d.p1, d.p1, C0, SLACK);
    LAUNCH_CHECK();
    TRY(conv5(pool0, C0, d.p1, dev, h->conv[0], B, c1, st));
    hipLaunchKernelGGL((norm_stats_kernel<C1, 3>), dim3(NORM_PARTS, B), dim3(256), 0, st, (const float*)c1, npart, d.n2, d.p2);
    LAUNCH_CHECK();
    hipLaunchKernelGGL((norm_apply_kernel<C1, 3>), dim3(blocks(d.p2, APPLY_ROWS), B), dim3(256), 0, st, (const float*)c1, (const float2*)npart,
                       dev + h->norm_w[1], dev + h->norm_b[1], a2, (float*)nullptr, d.n2, d.p2, C1, SLACK);
    LAUNCH_CHECK();
    TRY(conv5(a2, C1, d.p2, dev, h->conv[1], B, c2, st));
    hipLaunchKernelGGL((norm_stats_kernel<C1, 3>), dim3(NORM_PARTS, B), dim3(256), 0, st, (const float*)c2, npart, d.n3, d.F);
    LAUNCH_CHECK();
    hipLaunchKernelGGL((norm_apply_kernel<C1, 3>), dim3(blocks(d.F, APPLY_ROWS), B), dim3(256), 0, st, (const float*)c2, (const float2*)npart,
                       dev + h->norm_w[2], dev + h->norm_b[2], s, tap_sincnet, d.n3, d.F, SIN, 0);
    LAUNCH_CHECK();

    const float* x = s;
    long ldx = SIN;
    for (int l = 0; l < NLAYER; ++l) {
        TRY(dense(x, ldx, dev, h->proj[l], rows, xp, XP, false, st));
        float* yo = (l == NLAYER - 1 && tap_lstm) ? tap_lstm : y[l & 1];
        hipLaunchKernelGGL(lstm_rec_kernel, dim3(blocks(B, REC_TILE), NDIR), dim3(REC_THREADS), 0, st, (const float*)xp, dev + h->whh[l], yo, B, d.F);
        LAUNCH_CHECK();
        x = yo; ldx = LSTM_OUT;
    }
    TRY(dense(x, LSTM_OUT, dev, h->lin[0], rows, hd[0], HID, true, st));
    TRY(dense(hd[0], HID, dev, h->lin[1], rows, hd[1], HID, true, st));
    TRY(dense(hd[1], HID, dev, h->cls, rows, logits, LOGIT_LD, false, st));
    hipLaunchKernelGGL(logsoftmax_kernel, dim3(blocks(rows, 256)), dim3(256), 0, st, (const float*)logits, logp, rows);
    LAUNCH_CHECK();
    return TDX_OK;
}

}  // extern "C"
