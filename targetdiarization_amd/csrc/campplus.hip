// campplus.hip — CAM++ (3D-Speaker speakerlab/models/campplus, FCM head + D-TDNN with context-aware masking) speaker-embedding
// extractor on MI355X.  Replaces the embedding model of modelscope's `speech_campplus_speaker-diarization_common` pipeline
// (TargetDiarization.py:73) and `self.embedding['campp']` (TargetASR.py:109); third-party, parity unpinned [upstream-recall] —
// tests/campplus_oracle.py restates the architecture.
// feat [B,F,80] (fbank minus utterance mean, tdx_fbank mode 0) -> embedding [B,192].
//
// Layout: channel-last fp32 everywhere.
//  * FCM head: NHWC rows = (b, freq, time), 32 channels.  The 3x3 / 1x1 convolutions are implicit GEMMs on the fp32-MFMA core
//    (gemm.hpp CONV mode with cv_stride_w = 1: the head strides the frequency axis only), N = 32 of the 128-wide tile
//    (n_valid skips the other column tiles).  Eval BatchNorm folded into the weights; ReLU / residual in the epilogues.
//    head.conv2 writes [b*T + t][f*32 + c] (the TDNN weights are permuted on the host to this channel order).
//  * D-TDNN: one [B*T'][ld] buffer per dense block (ld = 512 / 1024 / 1024); layer i reads columns [0, cin) and appends 32.
//      xa = relu(bn1(x[:, :cin]))                          bnrelu_kernel  (a BN+ReLU in FRONT of a convolution cannot fold)
//      h  = relu(bn2(W1 xa))                               fp32 GEMM, bn2 folded
//      mask = sigmoid(W2 relu(W1c (mean_t h + segmean h) + b1c) + b2)   cam_mask_kernel, one block per utterance
//      x[:, cin:cin+32] = (3-tap dilated conv of h) * mask cam_local_kernel: fp32 MFMA straight from global (h is L2-resident)
//    transits: bnrelu_kernel + GEMM into the next block's buffer; out_nonlinear's BN is folded into transit3, its ReLU fused.
//  * statistics pooling (mean | unbiased std over time) and dense (1024 -> 192, affine-free BN folded).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/tdx.h"
#include "epilogues.hpp"
#include "weight_pack.hpp"

using namespace tdx;

namespace {

constexpr int EMB = 192, HC = 32, GROWTH = 32, BNC = 128, SEG = 100, MIN_FRAMES = 9;
constexpr int NBLOCK = 3;
const int kLayers[NBLOCK] = {12, 24, 16};
const int kDil[NBLOCK] = {1, 2, 2};
const int kCin[NBLOCK] = {128, 256, 512};       // channels entering the block
const int kLd[NBLOCK] = {512, 1024, 1024};      // channels leaving it = buffer pitch



// head.conv1: conv3x3(1->32, pad 1) + BN + ReLU on x[b, h=freq, w=time] = feat[b, w, h]
__global__ __launch_bounds__(256) void stem_kernel(const float* __restrict__ feat, const float* __restrict__ w9,   // [9][32]
                                                    const float* __restrict__ bias, float* __restrict__ out, int F, long rows) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;     // (row, channel quad): 8 quads per row
    if (i >= rows * 8) return;
    const long m = i >> 3;
    const int c = (int)(i & 7) * 4;
    const int w = (int)(m % F), h = (int)((m / F) % 80);
    const long b = m / ((long)F * 80);
    float4 acc = *reinterpret_cast<const float4*>(bias + c);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int ih = h + t / 3 - 1, iw = w + t % 3 - 1;
        if (ih >= 0 && ih < 80 && iw >= 0 && iw < F) {
            const float x = feat[(b * F + iw) * 80 + ih];
            const float4 k = *reinterpret_cast<const float4*>(w9 + t * HC + c);
            acc.x = fmaf(k.x, x, acc.x); acc.y = fmaf(k.y, x, acc.y); acc.z = fmaf(k.z, x, acc.z); acc.w = fmaf(k.w, x, acc.w);
        }
    }
    acc.x = fmaxf(acc.x, 0.f); acc.y = fmaxf(acc.y, 0.f); acc.z = fmaxf(acc.z, 0.f); acc.w = fmaxf(acc.w, 0.f);
    *reinterpret_cast<float4*>(out + m * HC + c) = acc;
}

// TDNN input gather: im[(b,t')][j*320 + q] = x[(b, 2t' + j - 2)][q] (zero outside), j = 0..4
__global__ __launch_bounds__(256) void tdnn_gather_kernel(const float* __restrict__ x, float* __restrict__ im, int T, int Tp, long total4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;     // float4 index over [B*Tp][1600]
    if (i >= total4) return;
    const long row = i / 400;
    const int k = (int)(i - row * 400) * 4, j = k / 320, q = k - j * 320;
    const long b = row / Tp;
    const int tp = (int)(row - b * Tp), t = 2 * tp + j - 2;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (t >= 0 && t < T) v = ldg4(x + (b * T + t) * 320 + q);
    *reinterpret_cast<f32x4*>(im + row * 1600 + k) = v;
}

// xa[m][k] = max(0, x[m][k] * s[k] + sh[k]), k < C (C % 4 == 0); x and xa share the pitch ld
__global__ __launch_bounds__(256) void bnrelu_kernel(const float* __restrict__ x, const float* __restrict__ s, const float* __restrict__ sh,
                                                      float* __restrict__ xa, long M, int C, int ld) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int per = C / 4;
    if (i >= M * per) return;
    const long m = i / per;
    const int k = (int)(i - m * per) * 4;
    const f32x4 v = ldg4(x + m * ld + k), a = ldg4(s + k), b = ldg4(sh + k);
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = fmaxf(fmaf(v[j], a[j], b[j]), 0.f);
    *reinterpret_cast<f32x4*>(xa + m * ld + k) = r;
}

// context mask of one utterance: ctx = mean_t h + mean over the 100-frame segment; mask[b][seg] = sigmoid(W2 relu(W1 ctx + b1) + b2)
__global__ __launch_bounds__(128) void cam_mask_kernel(const float* __restrict__ h, const float* __restrict__ w1, const float* __restrict__ b1,
                                                        const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ mask,
                                                        int T, int nseg) {
    __shared__ float ctx[BNC];
    __shared__ float hid[64];
    const int b = blockIdx.x, c = threadIdx.x;
    const float* p = h + (long)b * T * BNC + c;
    float tot = 0.f;
    for (int t = 0; t < T; ++t) tot += p[(long)t * BNC];
    const float mean = tot / (float)T;
    for (int s = 0; s < nseg; ++s) {
        const int t0 = s * SEG, t1 = min(T, t0 + SEG);
        float acc = 0.f;
        for (int t = t0; t < t1; ++t) acc += p[(long)t * BNC];
        ctx[c] = mean + acc / (float)(t1 - t0);
        __syncthreads();
        if (c < 64) {
            float a = b1[c];
            for (int k = 0; k < BNC; ++k) a = fmaf(w1[c * BNC + k], ctx[k], a);
            hid[c] = fmaxf(a, 0.f);
        }
        __syncthreads();
        if (c < GROWTH) {
            float a = b2[c];
            for (int k = 0; k < 64; ++k) a = fmaf(w2[c * 64 + k], hid[k], a);
            mask[((long)b * nseg + s) * GROWTH + c] = 1.0f / (1.0f + expf(-a));
        }
        __syncthreads();
    }
}

// y = Conv1d(128 -> 32, k 3, dilation = pad = dil) over time, times the context mask, into columns [coff, coff + 32) of x.
// v_mfma_f32_32x32x2_f32 (exact fp32 products); a wave owns 32 rows, both operands come straight from global memory (h and the
// 48 KB of weights stay in L2; the GEMM that produced h dominates the layer).  Operand map as in gemm.hpp: lane l supplies
// A[row l&31][k] and B[k][col l&31] for the four k = 8 kc + 4 (l>>5) + j of one 16-byte load.
__global__ __launch_bounds__(256) void cam_local_kernel(const float* __restrict__ h, const float* __restrict__ w,      // w [32][3*128]
                                                         const float* __restrict__ mask, float* __restrict__ x, int ldx, int coff,
                                                         long M, int T, int nseg, int dil) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hh = lane >> 5;
    const long m0 = (long)blockIdx.x * 128 + wave * 32;
    if (m0 >= M) return;
    const long m = min(m0 + l31, M - 1);
    const int t = (int)(m % T);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int ts = t + (j - 1) * dil;
        const bool ok = ts >= 0 && ts < T;
        const float* ap = h + (ok ? m + (long)(j - 1) * dil : m) * BNC + 4 * hh;
        const float* bp = w + l31 * (3 * BNC) + j * BNC + 4 * hh;
#pragma unroll
        for (int kc = 0; kc < BNC / 8; ++kc) {
            const f32x4 av = sel4(ok, ldg4(ap + 8 * kc));
            const f32x4 bv = ldg4(bp + 8 * kc);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q], bv[q], acc, 0, 0, 0);
        }
    }
    // D: col = l31, row = (r&3) + 8*(r>>2) + 4*hh
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long mr = m0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        if (mr >= M) continue;
        const long b = mr / T;
        const int seg = (int)(mr - b * T) / SEG;
        x[mr * ldx + coff + l31] = acc[r] * mask[(b * nseg + seg) * GROWTH + l31];
    }
}

// statistics pooling: x [B*T][C] -> stats[b][c] = mean, stats[b][C + c] = unbiased std over time
__global__ __launch_bounds__(256) void stats_kernel(const float* __restrict__ x, float* __restrict__ stats, int T, int C) {
    const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float* p = x + (long)b * T * C + c;
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += p[(long)t * C];
    const double mean = s / T;
    double q = 0.0;
    for (int t = 0; t < T; ++t) { const double d = p[(long)t * C] - mean; q += d * d; }
    stats[(long)b * 2 * C + c] = (float)mean;
    stats[(long)b * 2 * C + C + c] = (float)sqrt(q / (T - 1));
}

// dense: emb[b][n] = bias[n] + stats[b] . W[n]      (K = 1024)
__global__ __launch_bounds__(256) void dense_kernel(const float* __restrict__ stats, const float* __restrict__ W,
                                                     const float* __restrict__ bias, float* __restrict__ emb, int K) {
    __shared__ float red[4];
    const int n = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* s = stats + (long)b * K;
    const float* w = W + (long)n * K;
    float acc = 0.f;
    for (int k = tid * 4; k < K; k += 1024) {
        const float4 a = *reinterpret_cast<const float4*>(s + k);
        const float4 c = *reinterpret_cast<const float4*>(w + k);
        acc = fmaf(a.x, c.x, acc); acc = fmaf(a.y, c.y, acc); acc = fmaf(a.z, c.z, acc); acc = fmaf(a.w, c.w, acc);
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) emb[(long)b * gridDim.x + n] = (red[0] + red[1]) + (red[2] + red[3]) + bias[n];
}

// ---------------------------------------------------------------- epilogues
struct EpiHeadOut {     // head.conv2: row (b, f, t) of [B, Hf, T], channel n -> out[(b*T + t)*(Hf*32) + f*32 + n], relu(v + b)
    const float* b; float* out; int Hf, T;
    __device__ float col(int, int n) const { return b[n]; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int, int m, int n, float v, EpiNone, float c) const {
        if (n >= HC) return;
        const int t = m % T, bf = m / T, f = bf % Hf, bb = bf / Hf;
        out[((long)bb * T + t) * (Hf * HC) + f * HC + n] = fmaxf(v + c, 0.f);
    }
};

using ConvW = tdx::GemmW;
struct LayerW { size_t s1, sh1; ConvW lin1; size_t wl, cw1, cb1, cw2, cb2; int cin; };
struct TransW { size_t s, sh; ConvW lin; int cin; };

// head convolution (3x3 or 1x1, stride (sh, 1)) as an implicit GEMM
template <class Epi>
int head_conv(const float* A, const float* dev, const ConvW& cw, int B, int Hin, int Hout, int W, int sh, Epi e, hipStream_t st) {
    const long M = (long)B * Hout * W;
    GemmArgs g = make_args((int)M, cw.Npad, make_seg(A, HC, dev + cw.w, (long)cw.taps * cw.cinp, cw.cinp));
    g.n_valid = up(cw.N, 32);
    g.cv_Hin = Hin; g.cv_Win = W; g.cv_Hout = Hout; g.cv_Wout = W; g.cv_stride = sh; g.cv_stride_w = 1; g.cv_ntaps = cw.taps; g.cv_cin = cw.cinp;
    if (launch_gemm<false, false, false, false, Epi, 0, true>(g, 1, e, st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
    return TDX_OK;
}
template <class Epi>
int plain_gemm(const float* A, long lda, const float* dev, const ConvW& cw, long M, Epi e, hipStream_t st) {
    return linear_f32(A, lda, dev + cw.w, (int)M, cw.Npad, cw.cinp, e, st, up(cw.N, 32));
}

}  // namespace

struct tdx_campp {
    int device = 0;
    tdx::DevBuf dev;
    size_t stem_w, stem_b;
    ConvW l_c1[4], l_c2[4], l_sc[2], head2, tdnn;      // head.layer{1,2}.{0,1} in order; shortcuts of the two .0 blocks
    std::vector<LayerW> layers;
    TransW trans[NBLOCK];
    size_t dense_w, dense_b;
};

extern "C" {

int tdx_campp_create(const void* blob, size_t blob_bytes, int device, tdx_campp** out) {
    if (!blob || !out) return tdx::fail(TDX_E_INVALID, "tdx_campp_create: null argument");
    tdx::Loader ld;
    if (!ld.parse(blob, blob_bytes)) return tdx::fail(TDX_E_BLOB, "tdx_campp_create: malformed TDXW blob");
    using tdx::BN;
    // eval BatchNorm `p` -> y = x*s + sh   (affine = false: running statistics only)
    auto bn = [&](const std::string& p, int N, bool affine = true) -> BN {
        const float *g = affine ? ld.get(p + "weight", N) : nullptr, *be = affine ? ld.get(p + "bias", N) : nullptr;
        const float *mu = ld.get(p + "running_mean", N), *var = ld.get(p + "running_var", N);
        return tdx::bn_fold(g, be, mu, var, N);
    };
    auto put = [&](const std::vector<double>& v) -> size_t {
        const size_t o = ld.room(v.size());
        for (size_t i = 0; i < v.size(); ++i) ld.host[o + i] = (float)v[i];
        return o;
    };
    // bias-free conv [N,cin,taps] followed by eval BatchNorm `bnp` ("" = none) -> [Npad][taps][cinp] + bias[Npad]
    auto fold = [&](const std::string& wname, const std::string& bnp, int N, int cin, int taps, bool affine = true) -> ConvW {
        const float* W = ld.get(wname, (size_t)N * cin * taps);
        if (bnp.empty()) return tdx::push_conv_gemm(ld, W, nullptr, (const double*)nullptr, N, cin, taps, up(N, 128), up(cin, 32));
        const BN b = bn(bnp, N, affine);
        return tdx::push_conv_gemm(ld, W, b.s.data(), b.sh.data(), N, cin, taps, up(N, 128), up(cin, 32));
    };
    std::unique_ptr<tdx_campp> h(new tdx_campp());
    {   // head.conv1 [32,1,3,3] + bn1 -> w9[9][32], bias[32]
        const float* W = ld.get("head.conv1.weight", HC * 9);
        tdx::push_stem9(ld, W, bn("head.bn1.", HC), HC, h->stem_w, h->stem_b);
    }
    for (int i = 0; i < 4; ++i) {
        const std::string p = "head.layer" + std::to_string(i / 2 + 1) + "." + std::to_string(i % 2) + ".";
        h->l_c1[i] = fold(p + "conv1.weight", p + "bn1.", HC, HC, 9);
        h->l_c2[i] = fold(p + "conv2.weight", p + "bn2.", HC, HC, 9);
        if (i % 2 == 0) h->l_sc[i / 2] = fold(p + "shortcut.0.weight", p + "shortcut.1.", HC, HC, 1);
    }
    h->head2 = fold("head.conv2.weight", "head.bn2.", HC, HC, 9);
    {   // xvector.tdnn.linear [128, 320 (c*10 + f), 5] + BN -> [128][j*320 + f*32 + c]
        const float* W = ld.get("xvector.tdnn.linear.weight", (size_t)BNC * 320 * 5);
        const BN b = bn("xvector.tdnn.nonlinear.batchnorm.", BNC);
        ConvW& cw = h->tdnn; cw.N = BNC; cw.Npad = BNC; cw.cinp = 1600; cw.taps = 1;
        cw.w = ld.room((size_t)BNC * 1600);
        cw.b = ld.room(BNC);
        if (ld.ok()) for (int n = 0; n < BNC; ++n) {
            ld.host[cw.b + n] = (float)b.sh[n];
            for (int c = 0; c < HC; ++c)
                for (int f = 0; f < 10; ++f)
                    for (int j = 0; j < 5; ++j)
                        ld.host[cw.w + (size_t)n * 1600 + j * 320 + f * HC + c] = (float)((double)W[((size_t)n * 320 + c * 10 + f) * 5 + j] * b.s[n]);
        }
    }
    for (int bi = 0; bi < NBLOCK && ld.ok(); ++bi) {
        for (int i = 0; i < kLayers[bi] && ld.ok(); ++i) {
            const std::string p = "xvector.block" + std::to_string(bi + 1) + ".tdnnd" + std::to_string(i + 1) + ".";
            LayerW L; L.cin = kCin[bi] + GROWTH * i;
            const BN b1 = bn(p + "nonlinear1.batchnorm.", L.cin);
            L.s1 = put(b1.s); L.sh1 = put(b1.sh);
            L.lin1 = fold(p + "linear1.weight", p + "nonlinear2.batchnorm.", BNC, L.cin, 1);
            {   // cam_layer.linear_local [32,128,3] -> [32][tap*128 + c]
                const float* W = ld.get(p + "cam_layer.linear_local.weight", (size_t)GROWTH * BNC * 3);
                L.wl = ld.room((size_t)GROWTH * 3 * BNC);
                if (W) for (int n = 0; n < GROWTH; ++n)
                    for (int c = 0; c < BNC; ++c)
                        for (int t = 0; t < 3; ++t) ld.host[L.wl + (size_t)n * 3 * BNC + t * BNC + c] = W[((size_t)n * BNC + c) * 3 + t];
            }
            L.cw1 = ld.push(ld.get(p + "cam_layer.linear1.weight", 64 * BNC), 64 * BNC); L.cb1 = ld.push(ld.get(p + "cam_layer.linear1.bias", 64), 64);
            L.cw2 = ld.push(ld.get(p + "cam_layer.linear2.weight", GROWTH * 64), GROWTH * 64); L.cb2 = ld.push(ld.get(p + "cam_layer.linear2.bias", GROWTH), GROWTH);
            h->layers.push_back(L);
        }
        const std::string p = "xvector.transit" + std::to_string(bi + 1) + ".";
        TransW& t = h->trans[bi]; t.cin = kLd[bi];
        const BN b = bn(p + "nonlinear.batchnorm.", t.cin);
        t.s = put(b.s); t.sh = put(b.sh);
        // the BN of out_nonlinear follows transit3's convolution: folded; its ReLU is the epilogue's
        t.lin = fold(p + "linear.weight", bi == NBLOCK - 1 ? "xvector.out_nonlinear.batchnorm." : "", t.cin / 2, t.cin, 1);
    }
    if (ld.ok()) {
        const ConvW d = fold("xvector.dense.linear.weight", "xvector.dense.nonlinear.batchnorm.", EMB, 1024, 1, false);
        h->dense_w = d.w; h->dense_b = d.b;
    }
    h->device = device;
    TRY(ld.finish("tdx_campp_create", true, device, h->dev));
    *out = h.release();
    return TDX_OK;
}

int tdx_campp_destroy(tdx_campp* h) {
    delete h;
    return TDX_OK;
}

namespace {
struct WsPlan { size_t p0, p, x320, im, xb[NBLOCK], xa, hb, mask, stats, total; int Tp, nseg; };
inline WsPlan ws_plan(int B, int F) {
    WsPlan w{};
    w.Tp = (F - 1) / 2 + 1; w.nseg = (w.Tp + SEG - 1) / SEG;
    const size_t M = (size_t)B * w.Tp;
    w.p0 = al((size_t)B * 80 * F * HC + 64); w.p = al((size_t)B * 40 * F * HC + 64);
    w.x320 = al((size_t)B * F * 320 + 64); w.im = al(M * 1600 + 64);
    for (int i = 0; i < NBLOCK; ++i) w.xb[i] = al(M * kLd[i] + 64);
    w.xa = al(M * 1024 + 64); w.hb = al(M * BNC + 64);
    w.mask = al((size_t)B * w.nseg * GROWTH); w.stats = al((size_t)B * 1024);
    w.total = w.p0 + 3 * w.p + w.x320 + w.im + w.xb[0] + w.xb[1] + w.xb[2] + w.xa + w.hb + w.mask + w.stats;
    return w;
}
}  // namespace

size_t tdx_campp_workspace_bytes(const tdx_campp* h, int B, int F) {
    if (!h || B < 1 || F < MIN_FRAMES || (long)B * 80 * F > 0x7fffffffL) return 0;
    return ws_plan(B, F).total * sizeof(float);
}

double tdx_campp_flops(const tdx_campp* h, int B, int F) {
    if (!h || F < 1) return 0.0;
    const double conv = 2.0 * 9 * HC * HC, Fd = F, Tp = (F - 1) / 2 + 1;
    double fl = 2.0 * 80 * Fd * 9 * HC;                                     // head.conv1
    fl += 40 * Fd * (4 * conv + 2.0 * HC * HC);                             // layer1: four 3x3 + shortcut at 40 bins
    fl += 20 * Fd * (4 * conv + 2.0 * HC * HC);                             // layer2
    fl += 10 * Fd * conv;                                                   // head.conv2
    fl += Tp * 2.0 * 1600 * BNC;                                            // tdnn
    for (int bi = 0; bi < NBLOCK; ++bi) {
        for (int i = 0; i < kLayers[bi]; ++i)
            fl += Tp * 2.0 * ((double)(kCin[bi] + GROWTH * i) * BNC + 3.0 * BNC * GROWTH);
        fl += Tp * 2.0 * kLd[bi] * (kLd[bi] / 2);
    }
    fl += 2.0 * 1024 * EMB;
    return fl * B;
}

int tdx_campp_forward(tdx_campp* h, const float* feat, int B, int F, float* emb, void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !feat || !emb || !ws_ || B < 1) return tdx::fail(TDX_E_INVALID, "tdx_campp_forward: bad argument");
    if (F < MIN_FRAMES) return tdx::fail(TDX_E_INVALID, "tdx_campp_forward: need >= 9 fbank frames");
    if ((long)B * 80 * F > 0x7fffffffL) return tdx::fail(TDX_E_INVALID, "tdx_campp_forward: B*F too large for one launch");
    const WsPlan wp = ws_plan(B, F);
    if (ws_bytes < wp.total * sizeof(float)) return tdx::fail(TDX_E_WORKSPACE, "tdx_campp_forward: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)ws_;
    float* P[4] = {ws, ws + wp.p0, ws + wp.p0 + wp.p, ws + wp.p0 + 2 * wp.p};
    float* x320 = P[3] + wp.p;
    float* im = x320 + wp.x320;
    float* xb[NBLOCK]; xb[0] = im + wp.im; xb[1] = xb[0] + wp.xb[0]; xb[2] = xb[1] + wp.xb[1];
    float* xa = xb[2] + wp.xb[2];
    float* hb = xa + wp.xa;
    float* mask = hb + wp.hb;
    float* stats = mask + wp.mask;
    const float* dev = h->dev;
    const int T = F, Tp = wp.Tp, nseg = wp.nseg;
    const long M = (long)B * Tp;

    // ---- FCM head
    const long rows0 = (long)B * 80 * F;
    hipLaunchKernelGGL(stem_kernel, dim3((unsigned)((rows0 * 8 + 255) / 256)), dim3(256), 0, st, feat, dev + h->stem_w, dev + h->stem_b, P[0], F, rows0);
    LAUNCH_CHECK();
    // layer1.0 (80 -> 40): x = P0
    TRY(head_conv(P[0], dev, h->l_c1[0], B, 80, 40, T, 2, EpiBiasActN<ActRelu>{dev + h->l_c1[0].b, P[1], HC, HC}, st));
    TRY(head_conv(P[0], dev, h->l_sc[0], B, 80, 40, T, 2, EpiBiasActN<>{dev + h->l_sc[0].b, P[2], HC, HC}, st));
    TRY(head_conv(P[1], dev, h->l_c2[0], B, 40, 40, T, 1, EpiBiasResN<ActRelu>{dev + h->l_c2[0].b, P[2], P[3], HC, HC}, st));
    // layer1.1: x = P3
    TRY(head_conv(P[3], dev, h->l_c1[1], B, 40, 40, T, 1, EpiBiasActN<ActRelu>{dev + h->l_c1[1].b, P[1], HC, HC}, st));
    TRY(head_conv(P[1], dev, h->l_c2[1], B, 40, 40, T, 1, EpiBiasResN<ActRelu>{dev + h->l_c2[1].b, P[3], P[2], HC, HC}, st));
    // layer2.0 (40 -> 20): x = P2
    TRY(head_conv(P[2], dev, h->l_c1[2], B, 40, 20, T, 2, EpiBiasActN<ActRelu>{dev + h->l_c1[2].b, P[1], HC, HC}, st));
    TRY(head_conv(P[2], dev, h->l_sc[1], B, 40, 20, T, 2, EpiBiasActN<>{dev + h->l_sc[1].b, P[3], HC, HC}, st));
    TRY(head_conv(P[1], dev, h->l_c2[2], B, 20, 20, T, 1, EpiBiasResN<ActRelu>{dev + h->l_c2[2].b, P[3], P[0], HC, HC}, st));
    // layer2.1: x = P0
    TRY(head_conv(P[0], dev, h->l_c1[3], B, 20, 20, T, 1, EpiBiasActN<ActRelu>{dev + h->l_c1[3].b, P[1], HC, HC}, st));
    TRY(head_conv(P[1], dev, h->l_c2[3], B, 20, 20, T, 1, EpiBiasResN<ActRelu>{dev + h->l_c2[3].b, P[0], P[2], HC, HC}, st));
    // head.conv2 (20 -> 10) -> x320 [B*T][f*32 + c]
    TRY(head_conv(P[2], dev, h->head2, B, 20, 10, T, 2, EpiHeadOut{dev + h->head2.b, x320, 10, T}, st));

    // ---- TDNN (k 5, stride 2, pad 2) -> columns [0, 128) of block 1's buffer
    {
        const long total4 = M * 400;
        hipLaunchKernelGGL(tdnn_gather_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, x320, im, T, Tp, total4);
        LAUNCH_CHECK();
        TRY(plain_gemm(im, 1600, dev, h->tdnn, M, EpiBiasActN<ActRelu>{dev + h->tdnn.b, xb[0], kLd[0], BNC}, st));
    }
    // ---- dense blocks
    size_t li = 0;
    for (int bi = 0; bi < NBLOCK; ++bi) {
        const int ld = kLd[bi];
        float* x = xb[bi];
        for (int i = 0; i < kLayers[bi]; ++i, ++li) {
            const LayerW& L = h->layers[li];
            hipLaunchKernelGGL(bnrelu_kernel, dim3((unsigned)((M * (L.cin / 4) + 255) / 256)), dim3(256), 0, st, x, dev + L.s1, dev + L.sh1, xa, M, L.cin, ld);
            LAUNCH_CHECK();
            TRY(plain_gemm(xa, ld, dev, L.lin1, M, EpiBiasActN<ActRelu>{dev + L.lin1.b, hb, BNC, BNC}, st));
            hipLaunchKernelGGL(cam_mask_kernel, dim3(B), dim3(128), 0, st, hb, dev + L.cw1, dev + L.cb1, dev + L.cw2, dev + L.cb2, mask, Tp, nseg);
            LAUNCH_CHECK();
            hipLaunchKernelGGL(cam_local_kernel, dim3((unsigned)((M + 127) / 128)), dim3(256), 0, st, hb, dev + L.wl, mask, x, ld, L.cin, M, Tp, nseg, kDil[bi]);
            LAUNCH_CHECK();
        }
        const TransW& t = h->trans[bi];
        hipLaunchKernelGGL(bnrelu_kernel, dim3((unsigned)((M * (t.cin / 4) + 255) / 256)), dim3(256), 0, st, x, dev + t.s, dev + t.sh, xa, M, t.cin, ld);
        LAUNCH_CHECK();
        if (bi + 1 < NBLOCK) TRY(plain_gemm(xa, ld, dev, t.lin, M, EpiBiasActN<>{nullptr, xb[bi + 1], kLd[bi + 1], t.cin / 2}, st));
        else TRY(plain_gemm(xa, ld, dev, t.lin, M, EpiBiasActN<ActRelu>{dev + t.lin.b, xb[0], 512, 512}, st));      // out_nonlinear -> xb[0] as [M][512]
    }
    // ---- statistics pooling + dense
    hipLaunchKernelGGL(stats_kernel, dim3(2, B), dim3(256), 0, st, xb[0], stats, Tp, 512);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(dense_kernel, dim3(EMB, B), dim3(256), 0, st, stats, dev + h->dense_w, dev + h->dense_b, emb, 1024);
    LAUNCH_CHECK();
    return TDX_OK;
}

}  // extern "C"
