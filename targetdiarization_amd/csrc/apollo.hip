// apollo.hip — Apollo band-split RoFormer restorer on MI355X: the forward behind `AudioProcessor.restore_audio`
// (AudioProcessor.py:959-980; look2hear/models/apollo.py, built with sr=44100, win=20, feature_dim=256, layer=num_layers).
//
// One channel-last token layout for the whole net: X[frame][band][256] (frames of all items of a forward concatenated), so that
// the band attention of a frame reads 80 consecutive rows and the time conv of a band reads rows 80 apart — no permutes.
//   analysis   frames (reflect pad) -> DFT GEMM [F,896]x[896,896] (window folded into the basis) -> band features + RMSNorm + 1x1 conv
//   per layer  band Roformer: rms | QKV GEMM (norm gain folded, rsqrt in the epilogue) | RoPE + 80x80 softmax + PV per (frame, head)
//              | out GEMM + residual | rms | MLP GEMM, PAIRED epilogue silu(silu(gate)) * silu(z) | MLP_out GEMM + residual
//              seq ICB x3: depthwise conv7 + bias + row statistics in one kernel | 256->1024 GEMM + bias + SiLU | 1024->256 + bias + residual
//   synthesis  heads (RMSNorm, 1x1 conv, GLU) per (frame, band) -> C2R DFT GEMM (window / N folded) -> overlap-add / envelope
// Every 1x1 conv is the exact-fp32 MFMA core of gemm.hpp.  The model is local in time (receptive field +-54 frames): a forward
// item is a window of frames of one clip, so ragged batches and halo-cut long clips are the same call (include/tdx.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/tdx.h"
#include "dft_basis.hpp"
#include "epilogues.hpp"

using namespace tdx;

namespace {

constexpr int AD = 256, NB = 80, NFFT = 882, HOP = 441, NBIN = 442, KP = 896, HALO = 54, MAXI = 64;
constexpr int FEAT = 79 * 11 + 95;          // band-feature channels of all bands (2 bw + 1 each)
constexpr int HEADS = 79 * 20 + 188;        // head output channels of all bands (4 bw each)
constexpr float EPS_P = 1.1920928955078125e-07f;   // finfo(float32).eps
__host__ __device__ inline int band_w(int b) { return b < 79 ? 5 : 47; }

// the items of one forward (kernel argument, < 2 KB)
struct ApItems {
    int n;
    int f0[MAXI + 1];        // first workspace frame of item i (f0[n] = frames of the forward)
    int flo[MAXI];           // first clip frame of the window
    int len[MAXI];           // clip length in samples
    int slo[MAXI], shi[MAXI];   // output samples written
    long off[MAXI];          // sample offset of the clip in x / y
};

// frames of the reflect-padded clip, [F][896] (k >= 882 zero), and per frame (index in the window, window length)
__global__ __launch_bounds__(256) void ap_frames_kernel(const float* __restrict__ x, ApItems it, float* __restrict__ fr, int2* __restrict__ finfo) {
    const int g = blockIdx.x;
    int i = 0;
    while (i + 1 < it.n && g >= it.f0[i + 1]) ++i;
    const int tl = g - it.f0[i], t = it.flo[i] + tl, n = it.len[i];
    const float* xs = x + it.off[i];
    for (int k = threadIdx.x; k < KP; k += 256) {
        float v = 0.f;
        if (k < NFFT) {
            int s = t * HOP + k - HOP;
            s = s < 0 ? -s : s;
            s = s >= n ? 2 * (n - 1) - s : s;
            v = xs[min(max(s, 0), n - 1)];
        }
        fr[(long)g * KP + k] = v;
    }
    if (threadIdx.x == 0) finfo[g] = make_int2(tl, it.f0[i + 1] - it.f0[i]);
}

// band features of one frame: p = sqrt(sum |X|^2 + eps), [Re/p, Im/p, log p], RMSNorm (gain folded into Wt), 1x1 conv + bias
__global__ __launch_bounds__(256) void ap_band_in_kernel(const float* __restrict__ S, const float* __restrict__ Wt /* [FEAT][256] */,
                                                         const float* __restrict__ bias /* [80][256] */, float* __restrict__ X) {
    __shared__ float feat[FEAT];
    __shared__ float pw[NB], rr[NB];
    const int g = blockIdx.x, tid = threadIdx.x;
    const float* s = S + (long)g * KP;
    if (tid < NB) {
        const int lo = 5 * tid, bw = band_w(tid);
        float acc = 0.f;
        for (int k = 0; k < bw; ++k) { const float re = s[lo + k], im = s[NBIN + lo + k]; acc = fmaf(re, re, fmaf(im, im, acc)); }
        pw[tid] = sqrtf(acc + EPS_P);
    }
    __syncthreads();
    for (int idx = tid; idx < FEAT; idx += 256) {
        const int b = min(idx / 11, NB - 1), k = idx - 11 * b, bw = band_w(b), lo = 5 * b;
        const float p = pw[b];
        feat[idx] = k < bw ? s[lo + k] / p : (k < 2 * bw ? s[NBIN + lo + k - bw] / p : logf(p));
    }
    __syncthreads();
    if (tid < NB) {
        const int nk = 2 * band_w(tid) + 1;
        float ss = 0.f;
        for (int k = 0; k < nk; ++k) ss = fmaf(feat[11 * tid + k], feat[11 * tid + k], ss);
        rr[tid] = 1.0f / sqrtf(ss / (float)nk + 1e-5f);
    }
    __syncthreads();
    for (int b = 0; b < NB; ++b) {
        const int nk = 2 * band_w(b) + 1;
        const float* w = Wt + (long)11 * b * AD + tid;
        float acc = 0.f;
        for (int k = 0; k < nk; ++k) acc = fmaf(w[(long)k * AD], feat[11 * b + k], acc);
        X[((long)g * NB + b) * AD + tid] = fmaf(acc, rr[b], bias[b * AD + tid]);
    }
}

// rsqrt(mean(x^2) + 1e-5) of every 256-channel row, one wave per row
__global__ __launch_bounds__(256) void ap_rms_kernel(const float* __restrict__ X, float* __restrict__ r, long R) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const int lane = threadIdx.x & 63;
    const float4 v = *reinterpret_cast<const float4*>(X + row * AD + 4 * lane);
    const float ss = wave_sum(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w);
    if (lane == 0) r[row] = 1.0f / sqrtf(ss * (1.0f / AD) + 1e-5f);
}

// band attention of one (frame, head): RoPE on q / k at band positions 0..79, softmax(q k^T / sqrt(32)) v
__global__ __launch_bounds__(256) void ap_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ cosT, const float* __restrict__ sinT,
                                                      float* __restrict__ ctx) {
    __shared__ float q[NB][33], k[NB][33], v[NB][32], p[NB][NB + 1];
    const int g = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    const float scale = 0.17677669529663687f;
    for (int idx = tid; idx < NB * 32; idx += 256) {
        const int t = idx >> 5, d = idx & 31;
        const float* base = qkv + ((long)g * NB + t) * (3 * AD) + 96 * h;
        const float c = cosT[t * 32 + d], s = sinT[t * 32 + d];
        const float q0 = base[d], q1 = (d & 1) ? base[d - 1] : -base[d + 1];
        const float k0 = base[32 + d], k1 = (d & 1) ? base[32 + d - 1] : -base[32 + d + 1];
        q[t][d] = fmaf(q0, c, q1 * s) * scale;
        k[t][d] = fmaf(k0, c, k1 * s);
        v[t][d] = base[64 + d];
    }
    __syncthreads();
    for (int idx = tid; idx < NB * NB; idx += 256) {
        const int i = idx / NB, j = idx - i * NB;
        float acc = 0.f;
#pragma unroll
        for (int d = 0; d < 32; ++d) acc = fmaf(q[i][d], k[j][d], acc);
        p[i][j] = acc;
    }
    __syncthreads();
    {
        const int lane = tid & 63, w = tid >> 6;
        for (int i = w; i < NB; i += 4) {
            const float a = p[i][lane], b = lane < NB - 64 ? p[i][64 + lane] : -INFINITY;
            float mx = fmaxf(a, b);
            mx = wave_max(mx);
            const float ea = expf(a - mx), eb = lane < NB - 64 ? expf(b - mx) : 0.f;
            const float inv = 1.0f / wave_sum(ea + eb);
            p[i][lane] = ea * inv;
            if (lane < NB - 64) p[i][64 + lane] = eb * inv;
        }
    }
    __syncthreads();
    for (int idx = tid; idx < NB * 32; idx += 256) {
        const int i = idx >> 5, d = idx & 31;
        float acc = 0.f;
        for (int j = 0; j < NB; ++j) acc = fmaf(p[i][j], v[j][d], acc);
        ctx[((long)g * NB + i) * AD + 32 * h + d] = acc;
    }
}

// depthwise conv (k = 7, zero padded at the window's ends) + bias along the frames of one band, and the row statistic of the
// RMSNorm that follows; one wave per output row
__global__ __launch_bounds__(256) void ap_conv7_kernel(const float* __restrict__ X, const float* __restrict__ w7 /* [7][256] */, const float* __restrict__ b7,
                                                       const int2* __restrict__ finfo, float* __restrict__ Y, float* __restrict__ r, long R) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const int lane = threadIdx.x & 63;
    const long g = row / NB;
    const int2 fi = finfo[g];
    float4 acc = *reinterpret_cast<const float4*>(b7 + 4 * lane);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const int tt = fi.x + j - 3;
        if (tt >= 0 && tt < fi.y) {
            const float4 xv = *reinterpret_cast<const float4*>(X + (row + (long)(j - 3) * NB) * AD + 4 * lane);
            const float4 wv = *reinterpret_cast<const float4*>(w7 + j * AD + 4 * lane);
            acc.x = fmaf(wv.x, xv.x, acc.x); acc.y = fmaf(wv.y, xv.y, acc.y);
            acc.z = fmaf(wv.z, xv.z, acc.z); acc.w = fmaf(wv.w, xv.w, acc.w);
        }
    }
    *reinterpret_cast<float4*>(Y + row * AD + 4 * lane) = acc;
    const float ss = wave_sum(acc.x * acc.x + acc.y * acc.y + acc.z * acc.z + acc.w * acc.w);
    if (lane == 0) r[row] = 1.0f / sqrtf(ss * (1.0f / AD) + 1e-5f);
}

// output heads of one frame: per band RMSNorm (gain folded into Wh), 1x1 conv + bias to 4 bw, GLU -> Re | Im of the band's bins;
// writes the synthesis GEMM's A row [Re 0..441 | Im 0..441 | 12 zeros]
__global__ __launch_bounds__(256) void ap_head_kernel(const float* __restrict__ X, const float* __restrict__ Wh /* [HEADS][256] */,
                                                      const float* __restrict__ bh, float* __restrict__ E) {
    const int g = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float* e = E + (long)g * KP;
    for (int b = w; b < NB; b += 4) {
        const float4 xv = *reinterpret_cast<const float4*>(X + ((long)g * NB + b) * AD + 4 * lane);
        const float rr = 1.0f / sqrtf(wave_sum(xv.x * xv.x + xv.y * xv.y + xv.z * xv.z + xv.w * xv.w) * (1.0f / AD) + 1e-5f);
        const int bw = band_w(b), jo = 20 * b;
        for (int j = 0; j < 2 * bw; ++j) {
            const float4 wa = *reinterpret_cast<const float4*>(Wh + (long)(jo + j) * AD + 4 * lane);
            const float4 wg = *reinterpret_cast<const float4*>(Wh + (long)(jo + j + 2 * bw) * AD + 4 * lane);
            const float da = wave_sum(xv.x * wa.x + xv.y * wa.y + xv.z * wa.z + xv.w * wa.w);
            const float dg = wave_sum(xv.x * wg.x + xv.y * wg.y + xv.z * wg.z + xv.w * wg.w);
            const float o = fmaf(rr, da, bh[jo + j]) / (1.0f + expf(-fmaf(rr, dg, bh[jo + j + 2 * bw])));
            if (lane == 0) e[j < bw ? 5 * b + j : NBIN + 5 * b + j - bw] = o;
        }
    }
    if (threadIdx.x < KP - 2 * NBIN) e[2 * NBIN + threadIdx.x] = 0.f;
}

// overlap-add of the windowed C2R frames [F][896] and division by the squared-window envelope of the clip, samples [slo, shi)
__global__ __launch_bounds__(256) void ap_ola_kernel(const float* __restrict__ FO, ApItems it, const float* __restrict__ w2, float* __restrict__ y) {
    const int i = blockIdx.y;
    const int s = it.slo[i] + blockIdx.x * 256 + threadIdx.x;
    if (s >= it.shi[i]) return;
    const int T = 1 + it.len[i] / HOP, Tw = it.f0[i + 1] - it.f0[i];
    const int p = s + HOP, t2 = p / HOP, t1 = t2 - 1, k2 = p - t2 * HOP, k1 = k2 + HOP;
    const int l1 = t1 - it.flo[i], l2 = t2 - it.flo[i];
    float acc = 0.f, env = w2[k1];
    if (l1 >= 0 && l1 < Tw) acc += FO[(long)(it.f0[i] + l1) * KP + k1];
    if (t2 < T) {
        env += w2[k2];
        if (l2 >= 0 && l2 < Tw) acc += FO[(long)(it.f0[i] + l2) * KP + k2];
    }
    y[it.off[i] + s] = acc / env;
}

// ---- GEMM epilogues ----
struct EpiRow { const float* r; float* out; int ld;                    // out = v * r[m]          (RMSNorm rsqrt of the row)
    __device__ EpiNone col(int, int) const { return EpiNone{}; }
    __device__ float row(int, int m) const { return r[m]; }
    __device__ void store(int, int m, int n, float v, float rw, EpiNone) const { out[(long)m * ld + n] = v * rw; } };
struct EpiGate { const float* r; float* out;                           // out = silu(silu(v0 r)) * silu(v1 r)   (PAIRED, 1024 pairs)
    __device__ EpiNone col(int, int) const { return EpiNone{}; }
    __device__ float row(int, int m) const { return r[m]; }
    __device__ void store2(int, int m, int c, float v0, float v1, float rw, EpiNone) const {
        const float a = v0 * rw, z = v1 * rw;
        const float sa = a / (1.0f + expf(-a)), sz = z / (1.0f + expf(-z));
        out[(long)m * (4 * AD) + c] = sa / (1.0f + expf(-sa)) * sz;
    } };
struct EpiRowBiasSilu { const float* r; const float* b; float* out;     // out = silu(v r[m] + b[n])
    __device__ float col(int, int n) const { return b[n]; }
    __device__ float row(int, int m) const { return r[m]; }
    __device__ void store(int, int m, int n, float v, float rw, float c) const {
        const float a = fmaf(v, rw, c);
        out[(long)m * (4 * AD) + n] = a / (1.0f + expf(-a));
    } };
struct AIcb { size_t w7, b7, Wa, ba, Wb, bb; };
struct ALayer { size_t cosT, sinT, Wqkv, Wo, W1, W2; AIcb icb[3]; };

}  // namespace

struct tdx_apollo {
    int device = 0, L = 0;
    tdx::DevBuf dev;
    size_t bana = 0, bsyn = 0, w2 = 0, Wt = 0, bin = 0, Wh = 0, bh = 0;
    std::vector<ALayer> layers;
};

extern "C" {

int tdx_apollo_create(int num_layers, const void* blob, size_t blob_bytes, int device, tdx_apollo** out) {
    if (!blob || !out || num_layers < 1) return tdx::fail(TDX_E_INVALID, "tdx_apollo_create: bad argument");
    tdx::Loader ld;       // every tensor by exact shape (a strict load_state_dict compares shapes, not element counts)
    if (!ld.parse(blob, blob_bytes)) return tdx::fail(TDX_E_BLOB, "tdx_apollo_create: malformed TDXW blob");
    // W'[o][c] = W[o][c] * gain[c]  (the RMSNorm gain in front of a 1x1 conv, folded)
    auto push_folded = [&](const float* W, const float* gain, int O, int Cin) {
        size_t o = ld.room((size_t)O * Cin);
        if (W && gain) for (int i = 0; i < O; ++i) for (int c = 0; c < Cin; ++c) ld.host[o + (size_t)i * Cin + c] = W[(size_t)i * Cin + c] * gain[c];
        return o;
    };
    std::unique_ptr<tdx_apollo> h(new tdx_apollo());
    h->L = num_layers;
    // analysis / synthesis DFT bases (double, exact angle reduction), periodic hann window
    {
        const std::vector<double> w = tdx::hann_periodic(NFFT);
        h->bana = ld.room((size_t)KP * KP);
        h->bsyn = ld.room((size_t)KP * KP);
        h->w2 = ld.room(NFFT);
        for (int k = 0; k < NFFT; ++k) ld.host[h->w2 + k] = (float)(w[k] * w[k]);
        tdx::fill_dft_analysis(ld.host.data() + h->bana, NFFT, NBIN, NBIN, KP, w.data());      // im rows at NBIN + f
        // C2R with hann / NFFT; Im of bins 0 and 441 ignored: this image has always held -0 there (it was -0.0 * sin * w / NFFT)
        tdx::fill_dft_synthesis(ld.host.data() + h->bsyn, NFFT, NBIN, NBIN, KP, tdx::divided(w, NFFT).data(), -0.f);
    }
    // band-split input: Wt[11 b + k][c] = W_b[c][k] * gain_b[k], bias [80][256]
    h->Wt = ld.room((size_t)FEAT * AD);
    h->bin = ld.room((size_t)NB * AD);
    for (int b = 0; b < NB && ld.ok(); ++b) {
        const uint32_t nk = 2 * band_w(b) + 1;
        const float* gn = ld.get("BN." + std::to_string(b) + ".0.weight", {nk});
        const float* W = ld.get("BN." + std::to_string(b) + ".1.weight", {AD, nk, 1});
        const float* bb = ld.get("BN." + std::to_string(b) + ".1.bias", {AD});
        if (!ld.ok()) break;
        for (int c = 0; c < AD; ++c) {
            for (uint32_t k = 0; k < nk; ++k) ld.host[h->Wt + (size_t)(11 * b + k) * AD + c] = W[(size_t)c * nk + k] * gn[k];
            ld.host[h->bin + (size_t)b * AD + c] = bb[c];
        }
    }
    for (int l = 0; l < num_layers && ld.ok(); ++l) {
        const std::string p = "net." + std::to_string(l) + ".";
        ALayer w;
        w.cosT = ld.push(ld.get(p + "band_net.cos_freq", {100, 32}), 100 * 32);
        w.sinT = ld.push(ld.get(p + "band_net.sin_freq", {100, 32}), 100 * 32);
        w.Wqkv = push_folded(ld.get(p + "band_net.weight.weight", {3 * AD, AD, 1}), ld.get(p + "band_net.input_norm.weight", {AD}), 3 * AD, AD);
        w.Wo = ld.push(ld.get(p + "band_net.output.weight", {AD, AD, 1}), (size_t)AD * AD);
        w.W1 = push_folded(ld.get(p + "band_net.MLP.1.weight", {8 * AD, AD, 1}), ld.get(p + "band_net.MLP.0.weight", {AD}), 8 * AD, AD);
        w.W2 = ld.push(ld.get(p + "band_net.MLP_output.weight", {AD, 4 * AD, 1}), (size_t)AD * 4 * AD);
        for (int b = 0; b < 3; ++b) {
            const std::string q = p + "seq_net.blocks." + std::to_string(b) + ".conv.";
            AIcb& c = w.icb[b];
            c.w7 = ld.push_tapmajor(ld.get(q + "0.weight", {AD, 1, 7}), AD, 7);
            c.b7 = ld.push(ld.get(q + "0.bias", {AD}), AD);
            c.Wa = push_folded(ld.get(q + "2.weight", {4 * AD, AD, 1}), ld.get(q + "1.weight", {AD}), 4 * AD, AD);
            c.ba = ld.push(ld.get(q + "2.bias", {4 * AD}), 4 * AD);
            c.Wb = ld.push(ld.get(q + "4.weight", {AD, 4 * AD, 1}), (size_t)AD * 4 * AD);
            c.bb = ld.push(ld.get(q + "4.bias", {AD}), AD);
        }
        h->layers.push_back(w);
    }
    // heads: Wh[20 b + j][c] = W_b[j][c] * gain_b[c], bh[20 b + j]
    h->Wh = ld.room((size_t)HEADS * AD);
    h->bh = ld.room(HEADS);
    for (int b = 0; b < NB && ld.ok(); ++b) {
        const uint32_t no = 4 * band_w(b);
        const float* gn = ld.get("output." + std::to_string(b) + ".0.weight", {AD});
        const float* W = ld.get("output." + std::to_string(b) + ".1.weight", {no, AD, 1});
        const float* bb = ld.get("output." + std::to_string(b) + ".1.bias", {no});
        if (!ld.ok()) break;
        for (uint32_t j = 0; j < no; ++j) {
            for (int c = 0; c < AD; ++c) ld.host[h->Wh + (size_t)(20 * b + j) * AD + c] = W[(size_t)j * AD + c] * gn[c];
            ld.host[h->bh + 20 * b + j] = bb[j];
        }
    }
    h->device = device;
    TRY(ld.finish("tdx_apollo_create", true, device, h->dev));
    *out = h.release();
    return TDX_OK;
}

int tdx_apollo_destroy(tdx_apollo* h) {
    delete h;
    return TDX_OK;
}

size_t tdx_apollo_workspace_bytes(const tdx_apollo* h, int frames) {
    if (!h || frames < 1 || frames > (1 << 24)) return 0;
    const size_t F = (size_t)frames, R = F * NB;
    return (2 * al(F * KP) + 2 * al(R * AD) + al(R * 4 * AD) + al(R) + al(2 * F)) * sizeof(float);
}

double tdx_apollo_flops(const tdx_apollo* h, int frames) {
    if (!h || frames < 1) return 0.0;
    const double R = (double)NB;
    const double gemm = 2.0 * R * ((double)AD * 3 * AD + (double)AD * AD + (double)AD * 8 * AD + 4.0 * AD * AD + 3.0 * 2.0 * 4.0 * AD * AD);
    const double attn = 8.0 * 2.0 * 2.0 * R * R * 32.0, conv7 = 3.0 * 2.0 * 7.0 * R * AD;
    const double io = 2.0 * 2.0 * KP * KP + 2.0 * FEAT * AD + 2.0 * HEADS * AD;
    return (double)frames * (h->L * (gemm + attn + conv7) + io);
}

int tdx_apollo_forward(tdx_apollo* h, const float* x, const int64_t* lens, int nclips, const int32_t* items, int nitems, float* y,
                       void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !x || !lens || !y || !ws_ || nclips < 1) return tdx::fail(TDX_E_INVALID, "tdx_apollo_forward: null argument");
    if (!items) nitems = nclips;
    if (nitems < 1 || nitems > MAXI) return tdx::fail(TDX_E_INVALID, "tdx_apollo_forward: need 1 <= items <= 64");
    std::vector<long> off(nclips + 1, 0);
    for (int c = 0; c < nclips; ++c) {
        if (lens[c] < NBIN || lens[c] > (1L << 30)) return tdx::fail(TDX_E_INVALID, "tdx_apollo_forward: every clip needs 442 <= n < 2^30 samples");
        off[c + 1] = off[c] + lens[c];
    }
    ApItems it{};
    it.n = nitems;
    int F = 0, span = 0;
    for (int i = 0; i < nitems; ++i) {
        const int c = items ? items[5 * i] : i;
        if (c < 0 || c >= nclips) return tdx::fail(TDX_E_INVALID, "tdx_apollo_forward: item names no clip");
        const int n = (int)lens[c], T = 1 + n / HOP;
        const int lo = items ? items[5 * i + 1] : 0, hi = items ? items[5 * i + 2] : T;
        const int slo = items ? items[5 * i + 3] : 0, shi = items ? items[5 * i + 4] : n;
        if (lo < 0 || hi > T || lo >= hi || slo < 0 || shi > n || slo >= shi)
            return tdx::fail(TDX_E_INVALID, "tdx_apollo_forward: item window out of range");
        // every frame an output sample reads must be exact: >= HALO frames from an edge of the window that is not a clip edge
        const int tfirst = slo / HOP, tlast = min(T - 1, (shi - 1 + HOP) / HOP);
        if ((lo > 0 && tfirst < lo + HALO) || (hi < T && tlast > hi - 1 - HALO))
            return tdx::fail(TDX_E_INVALID, "tdx_apollo_forward: item samples depend on frames within 54 of a cut window edge");
        it.f0[i] = F; it.flo[i] = lo; it.len[i] = n; it.slo[i] = slo; it.shi[i] = shi; it.off[i] = off[c];
        F += hi - lo;
        span = max(span, shi - slo);
    }
    it.f0[nitems] = F;
    if (ws_bytes < tdx_apollo_workspace_bytes(h, F) || tdx_apollo_workspace_bytes(h, F) == 0)
        return tdx::fail(TDX_E_WORKSPACE, "tdx_apollo_forward: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    const long R = (long)F * NB;
    float* ws = (float*)ws_;
    float* fr = ws;                     // frames, later the head spectra
    float* S = fr + al((size_t)F * KP);  // spectrum, later the C2R frames
    float* X = S + al((size_t)F * KP);
    float* Y = X + al((size_t)R * AD);  // attention context / conv7 output
    float* U = Y + al((size_t)R * AD);  // qkv / MLP and ICB hidden
    float* r = U + al((size_t)R * 4 * AD);
    int2* finfo = reinterpret_cast<int2*>(r + al((size_t)R));
    const float* d = h->dev;
    const unsigned rows4 = (unsigned)((R + 3) / 4);

    hipLaunchKernelGGL(ap_frames_kernel, dim3(F), dim3(256), 0, st, x, it, fr, finfo);
    LAUNCH_CHECK();
    TRY(linear_f32(fr, KP, d + h->bana, F, KP, KP, EpiStoreZ{S, KP, 0}, st));
    hipLaunchKernelGGL(ap_band_in_kernel, dim3(F), dim3(256), 0, st, S, d + h->Wt, d + h->bin, X);
    LAUNCH_CHECK();
    for (const ALayer& w : h->layers) {
        hipLaunchKernelGGL(ap_rms_kernel, dim3(rows4), dim3(256), 0, st, X, r, R);
        LAUNCH_CHECK();
        TRY(linear_f32(X, AD, d + w.Wqkv, (int)R, 3 * AD, AD, EpiRow{r, U, 3 * AD}, st));
        hipLaunchKernelGGL(ap_attn_kernel, dim3(F, 8), dim3(256), 0, st, U, d + w.cosT, d + w.sinT, Y);
        LAUNCH_CHECK();
        TRY(linear_f32(Y, AD, d + w.Wo, (int)R, AD, AD, EpiBiasRes<>{nullptr, X, X, AD}, st));
        hipLaunchKernelGGL(ap_rms_kernel, dim3(rows4), dim3(256), 0, st, X, r, R);
        LAUNCH_CHECK();
        TRY(linear_f32<true>(X, AD, d + w.W1, (int)R, 4 * AD, AD, EpiGate{r, U}, st, 0, 4 * AD));
        TRY(linear_f32(U, 4 * AD, d + w.W2, (int)R, AD, 4 * AD, EpiBiasRes<>{nullptr, X, X, AD}, st));
        for (const AIcb& c : w.icb) {
            hipLaunchKernelGGL(ap_conv7_kernel, dim3(rows4), dim3(256), 0, st, X, d + c.w7, d + c.b7, finfo, Y, r, R);
            LAUNCH_CHECK();
            TRY(linear_f32(Y, AD, d + c.Wa, (int)R, 4 * AD, AD, EpiRowBiasSilu{r, d + c.ba, U}, st));
            TRY(linear_f32(U, 4 * AD, d + c.Wb, (int)R, AD, 4 * AD, EpiBiasRes<>{d + c.bb, X, X, AD}, st));
        }
    }
    hipLaunchKernelGGL(ap_head_kernel, dim3(F), dim3(256), 0, st, X, d + h->Wh, d + h->bh, fr);
    LAUNCH_CHECK();
    TRY(linear_f32(fr, KP, d + h->bsyn, F, KP, KP, EpiStoreZ{S, KP, 0}, st));
    hipLaunchKernelGGL(ap_ola_kernel, dim3((span + 255) / 256, nitems), dim3(256), 0, st, S, it, d + h->w2, y);
    LAUNCH_CHECK();
    return TDX_OK;
}

}  // extern "C"
