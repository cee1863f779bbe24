// punc.hip — CT-Transformer punctuation restorer on MI355X: the neural forward behind
// `self.punc.inference(input=text)` (ASRProcessor.punctuation_restore, ASRProcessor.py:880-897; funasr CTTransformer: third-party,
// parity unpinned — oracle/punc_oracle.py restates the published punc_forward):
//     x = Embedding(ids) ; h = SANMEncoder(x) ; y = Linear(h)          (embed_unit = att_unit = 256, 8 heads, FFN 1024, 4 blocks,
//                                                                       FSMN memory k = 11, sinusoidal PE, pre-LN, eps 1e-12)
// The sequences are mini-sentences of <= a few hundred tokens (funasr splits the text in windows of 20 tokens and carries the
// unfinished sentence over), so every launch is tiny: the Linears run on the exact fp32 MFMA core (gemm.hpp), the rest are small
// one-purpose kernels.  ids_dev int32 [B,T] -> logits_dev [B,T,npunc] (argmax / the mini-sentence logic stay on the host: punctuation.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/tdx.h"
#include "epilogues.hpp"

using namespace tdx;

namespace {

constexpr int PD = 256, PH = 8, PDK = 32, PFFN = 1024, PKS = 11, PMAXT = 1024;

// x[b,t,:] = emb[id] * sqrt(256) + PE(t + 1)        (SinusoidalPositionEncoder: [sin | cos] halves, positions from 1)
__global__ __launch_bounds__(256) void punc_embed_kernel(const int* __restrict__ ids, const float* __restrict__ emb, int vocab, float* __restrict__ x, int T) {
    const int row = blockIdx.x, d = threadIdx.x;           // 256 threads = 256 channels
    int id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const int t = row % T;
    const int j = d & 127;
    const float inv = expf((float)j * (-logf(10000.0f) / (float)(PD / 2 - 1)));
    const float ang = (float)(t + 1) * inv;
    x[(long)row * PD + d] = emb[(long)id * PD + d] * 16.0f + (d < 128 ? sinf(ang) : cosf(ang));
}
// LayerNorm over 256 channels, one wave per row
__global__ __launch_bounds__(256) void punc_ln_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b, float* __restrict__ y,
                                                       long rows, float eps) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float4 v = *reinterpret_cast<const float4*>(x + row * PD + 4 * lane);
    const float mean = wave_sum(v.x + v.y + v.z + v.w) * (1.0f / PD);
    const float a0 = v.x - mean, a1 = v.y - mean, a2 = v.z - mean, a3 = v.w - mean;
    const float var = wave_sum(a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3) * (1.0f / PD);
    const float r = 1.0f / sqrtf(var + eps);
    const float4 gg = *reinterpret_cast<const float4*>(g + 4 * lane), bb = *reinterpret_cast<const float4*>(b + 4 * lane);
    *reinterpret_cast<float4*>(y + row * PD + 4 * lane) = make_float4(a0 * r * gg.x + bb.x, a1 * r * gg.y + bb.y, a2 * r * gg.z + bb.z, a3 * r * gg.w + bb.w);
}
// FSMN memory: mem[b,t,c] = v[b,t,c] + sum_j w[c][j] v[b,t + j - 5,c]   (depthwise over time, zero padded; v = qkv[:, 512:768])
__global__ __launch_bounds__(256) void punc_fsmn_kernel(const float* __restrict__ qkv, const float* __restrict__ wT /* [11][256] */, float* __restrict__ mem, int T,
                                                       const int* __restrict__ lens) {
    const int row = blockIdx.x, c = threadIdx.x;
    const int t = row % T;
    const int L = lens ? min(lens[row / T], T) : T;          // rows >= L of a batch entry are padding: they read as zero (funasr: inputs * mask)
    const long base = (long)(row - t) * (3 * PD) + 2 * PD + c;
    float acc = t < L ? qkv[base + (long)t * (3 * PD)] : 0.f;
#pragma unroll
    for (int j = 0; j < PKS; ++j) {
        const int tt = t + j - (PKS - 1) / 2;
        if (tt >= 0 && tt < L) acc = fmaf(wT[j * PD + c], qkv[base + (long)tt * (3 * PD)], acc);
    }
    mem[(long)row * PD + c] = acc;
}
// softmax(q k^T / sqrt(32)) v for 8 query rows of one (batch, head); T <= PMAXT
__global__ __launch_bounds__(256) void punc_attn_kernel(const float* __restrict__ qkv, float* __restrict__ ctx, int T, const int* __restrict__ lens) {
    __shared__ float qs[8][PDK];
    __shared__ float p[8][PMAXT];
    const int b = blockIdx.z, h = blockIdx.y, r0 = blockIdx.x * 8, tid = threadIdx.x;
    const float* base = qkv + (long)b * T * (3 * PD);
    const int L = lens ? min(lens[b], T) : T;                // keys >= L are padding (masked); L = 0: the context rows are written as zeros
    { const int r = tid >> 5, d = tid & 31; qs[r][d] = base[(long)min(r0 + r, T - 1) * (3 * PD) + h * PDK + d] * 0.17677669529663687f; }
    __syncthreads();
    for (int j = tid; j < L; j += 256) {
        const float* kp = base + (long)j * (3 * PD) + PD + h * PDK;
        float acc[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] = 0.f;
#pragma unroll
        for (int d = 0; d < PDK; ++d) {
            const float kv = kp[d];
#pragma unroll
            for (int r = 0; r < 8; ++r) acc[r] = fmaf(qs[r][d], kv, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) p[r][j] = acc[r];
    }
    __syncthreads();
    {
        const int lane = tid & 63, w = tid >> 6;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            float* row = p[2 * w + rr];
            float mx = -INFINITY;
            for (int c = lane; c < L; c += 64) mx = fmaxf(mx, row[c]);
            mx = wave_max(mx);
            float sum = 0.f;
            for (int c = lane; c < L; c += 64) { const float e = expf(row[c] - mx); row[c] = e; sum += e; }
            sum = wave_sum(sum);
            const float inv = L > 0 ? 1.0f / sum : 0.f;
            for (int c = lane; c < L; c += 64) row[c] *= inv;
        }
    }
    __syncthreads();
    {
        const int r = tid >> 5, d = tid & 31;
        const float* vp = base + 2 * PD + h * PDK + d;
        float acc = 0.f;
        for (int j = 0; j < L; ++j) acc = fmaf(p[r][j], vp[(long)j * (3 * PD)], acc);
        if (r0 + r < T) ctx[((long)b * T + r0 + r) * PD + h * PDK + d] = acc;
    }
}

struct PLayer { size_t Wqkv, bqkv, fsmnT, Wo, bo, W1, b1, W2, b2, n1g, n1b, n2g, n2b; };

}  // namespace

struct tdx_punc {
    int device = 0, L = 0, vocab = 0, npunc = 0;
    tdx::DevBuf dev;
    size_t emb = 0, ang = 0, anb = 0, Wd = 0, bd = 0;
    std::vector<PLayer> layers;
};

extern "C" {

int tdx_punc_create(int num_blocks, int vocab, int npunc, const void* blob, size_t blob_bytes, int device, tdx_punc** out) {
    if (!blob || !out || num_blocks < 1 || vocab < 1 || npunc < 1 || npunc > 128) return tdx::fail(TDX_E_INVALID, "tdx_punc_create: bad argument");
    tdx::Loader ld;
    if (!ld.parse(blob, blob_bytes)) return tdx::fail(TDX_E_BLOB, "tdx_punc_create: malformed TDXW blob");
    std::unique_ptr<tdx_punc> h(new tdx_punc());
    h->L = num_blocks; h->vocab = vocab; h->npunc = npunc;
    h->emb = ld.push(ld.get("embed.weight", (size_t)vocab * PD), (size_t)vocab * PD);
    for (int l = 0; l < num_blocks && ld.ok(); ++l) {
        const std::string p = l == 0 ? "encoder.encoders0.0." : "encoder.encoders." + std::to_string(l - 1) + ".";
        PLayer w;
        w.Wqkv = ld.push(ld.get(p + "self_attn.linear_q_k_v.weight", (size_t)3 * PD * PD), (size_t)3 * PD * PD);
        w.bqkv = ld.push(ld.get(p + "self_attn.linear_q_k_v.bias", 3 * PD), 3 * PD);
        w.fsmnT = ld.push_tapmajor(ld.get(p + "self_attn.fsmn_block.weight", (size_t)PD * PKS), PD, PKS);      // [256][1][11] -> [11][256]
        w.Wo = ld.push(ld.get(p + "self_attn.linear_out.weight", (size_t)PD * PD), (size_t)PD * PD);
        w.bo = ld.push(ld.get(p + "self_attn.linear_out.bias", PD), PD);
        w.W1 = ld.push(ld.get(p + "feed_forward.w_1.weight", (size_t)PFFN * PD), (size_t)PFFN * PD);
        w.b1 = ld.push(ld.get(p + "feed_forward.w_1.bias", PFFN), PFFN);
        w.W2 = ld.push(ld.get(p + "feed_forward.w_2.weight", (size_t)PD * PFFN), (size_t)PD * PFFN);
        w.b2 = ld.push(ld.get(p + "feed_forward.w_2.bias", PD), PD);
        w.n1g = ld.push(ld.get(p + "norm1.weight", PD), PD); w.n1b = ld.push(ld.get(p + "norm1.bias", PD), PD);
        w.n2g = ld.push(ld.get(p + "norm2.weight", PD), PD); w.n2b = ld.push(ld.get(p + "norm2.bias", PD), PD);
        h->layers.push_back(w);
    }
    h->ang = ld.push(ld.get("encoder.after_norm.weight", PD), PD);
    h->anb = ld.push(ld.get("encoder.after_norm.bias", PD), PD);
    h->Wd = ld.push(ld.get("decoder.weight", (size_t)npunc * PD), (size_t)npunc * PD, (size_t)128 * PD);       // rows read in 128-row tiles
    h->bd = ld.push(ld.get("decoder.bias", npunc), npunc, 128);
    h->device = device;
    TRY(ld.finish("tdx_punc_create", true, device, h->dev));
    *out = h.release();
    return TDX_OK;
}

int tdx_punc_destroy(tdx_punc* h) {
    delete h;
    return TDX_OK;
}

size_t tdx_punc_workspace_bytes(const tdx_punc* h, int B, int T) {
    if (!h || B < 1 || T < 1 || T > PMAXT) return 0;
    const size_t M = (size_t)B * T;
    return (al(M * PD) * 4 + al(M * 3 * PD) + al(M * PFFN) + 1024) * sizeof(float);
}

int tdx_punc_forward(tdx_punc* h, const int* ids, const int* lens, int B, int T, float* logits, void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !ids || !logits || !ws_) return tdx::fail(TDX_E_INVALID, "tdx_punc_forward: null argument");
    if (B < 1 || T < 1 || T > PMAXT) return tdx::fail(TDX_E_INVALID, "tdx_punc_forward: need 1 <= T <= 1024");
    if (ws_bytes < tdx_punc_workspace_bytes(h, B, T)) return tdx::fail(TDX_E_WORKSPACE, "tdx_punc_forward: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    const long M = (long)B * T;
    float* ws = (float*)ws_;
    float* x = ws; float* hn = x + al(M * PD); float* mem = hn + al(M * PD); float* ctx = mem + al(M * PD);
    float* qkv = ctx + al(M * PD); float* ffn = qkv + al(M * 3 * PD);
    const float* d = h->dev;
    hipLaunchKernelGGL(punc_embed_kernel, dim3((unsigned)M), dim3(256), 0, st, ids, d + h->emb, h->vocab, x, T);
    LAUNCH_CHECK();
    for (const PLayer& w : h->layers) {
        hipLaunchKernelGGL(punc_ln_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, x, d + w.n1g, d + w.n1b, hn, M, 1e-12f);
        LAUNCH_CHECK();
        TRY(linear_f32(hn, PD, d + w.Wqkv, (int)M, 3 * PD, PD, EpiBiasAct<>{d + w.bqkv, qkv, 3 * PD}, st));
        hipLaunchKernelGGL(punc_fsmn_kernel, dim3((unsigned)M), dim3(256), 0, st, qkv, d + w.fsmnT, mem, T, lens);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(punc_attn_kernel, dim3((T + 7) / 8, PH, B), dim3(256), 0, st, qkv, ctx, T, lens);
        LAUNCH_CHECK();
        TRY(linear_f32(ctx, PD, d + w.Wo, (int)M, PD, PD, EpiBiasRes2<>{d + w.bo, x, mem, x, PD}, st));                 // x += att W_o + b_o + mem
        hipLaunchKernelGGL(punc_ln_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, x, d + w.n2g, d + w.n2b, hn, M, 1e-12f);
        LAUNCH_CHECK();
        TRY(linear_f32(hn, PD, d + w.W1, (int)M, PFFN, PD, EpiBiasAct<ActRelu>{d + w.b1, ffn, PFFN}, st));
        TRY(linear_f32(ffn, PFFN, d + w.W2, (int)M, PD, PFFN, EpiBiasRes<>{d + w.b2, x, x, PD}, st));
    }
    hipLaunchKernelGGL(punc_ln_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, x, d + h->ang, d + h->anb, hn, M, 1e-12f);
    LAUNCH_CHECK();
    TRY(linear_f32(hn, PD, d + h->Wd, (int)M, 128, PD, EpiBiasActN<>{d + h->bd, logits, h->npunc, h->npunc}, st));
    return TDX_OK;
}

}  // extern "C"
