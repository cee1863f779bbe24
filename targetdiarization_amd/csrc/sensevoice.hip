// sensevoice.hip — SenseVoiceSmall on MI355X (include/tdx.h N9): the second local recogniser of the reference,
// `self.asr['sensevoice'].generate(...)` (ASRProcessor.py:398-402; funasr SenseVoiceSmall / SenseVoiceEncoderSmall —
// third-party, absent here, parity unpinned: tests/sensevoice_oracle.py restates it).
//   four prompt rows (language, event, emotion, text-norm embeddings) + LFR features -> x sqrt(512) + sinusoidal positions
//   -> encoders0, encoders, after_norm, tp_encoders, tp_norm (Paraformer's SANM layer: pf_sanm.hpp, paraformer.hip)
//   -> CTC head: log-softmax over the vocabulary, per frame (argmax id, log-prob at the argmax) -> greedy collapse.
// The head never holds the logits of a whole call: either the fused kernel below (running max / argmax / sum of exponentials
// per row while it sweeps the vocabulary), or row chunks through the x3 Linear into a logits buffer of a fixed cap.
#include <climits>
#include <cstdlib>

#include "pf_sanm.hpp"

using namespace tdx;

namespace {

constexpr int D = 512, DIN = 560, DINP = 576, FFN = 2048, H = 4, DK = 128, KS = 11;     // the SANM layer's sizes (paraformer.hip)
constexpr int SV_PROMPT = 4, SV_EMBED_ROWS = 16;
constexpr int SV_BM = 64, SV_SLICE = 512, SV_PA = D + 4;           // fused head: rows per workgroup, vocabulary columns per workgroup, LDS row pitch (4 mod 32 floats)
constexpr int SV_RP = 129;                                          // pitch of the reduction arrays (128 entries per row)
constexpr int SV_LDS = SV_BM * SV_PA * 4;                           // 132096 B: the row tile; reused for the reduction (3 x 64 x 129 x 4 = 99072 B)
static_assert(3 * SV_BM * SV_RP * 4 <= SV_LDS, "reduction arrays must fit the row tile");

// (max, argmax, sum of exp(v - max)) of a set of logits; the empty set is (-inf, INT_MAX, 0).  Ties: the lowest id, like torch.argmax.
struct SvTop { float m; int i; float s; };
__device__ inline void sv_merge(SvTop& a, const SvTop& b) {
    if (b.i == INT_MAX) return;
    if (a.i == INT_MAX) { a = b; return; }
    const float mx = fmaxf(a.m, b.m);
    a.s = a.s * expf(a.m - mx) + b.s * expf(b.m - mx);
    if (b.m > a.m || (b.m == a.m && b.i < a.i)) a.i = b.i;
    a.m = mx;
}

// FUSED HEAD.  Workgroup (bx, by): rows [64 bx, +64) x vocabulary columns [512 by, +512).  The 64 LN'd rows are staged ONCE in LDS
// (fp32, 2 KB each); wave w sweeps the 64-column blocks w and w + 4 of the slice with v_mfma_f32_32x32x2_f32 (exact fp32 products;
// operand map of gemm.hpp: lane l supplies A[row l&31][k] and B[k][col l&31] for the four k = 8 kc + 4 (l>>5) + j of one 16-byte
// load), W rows straight from global memory (the slice is 1 MB: L2-resident across the row tiles).  A lane keeps the running
// (max, argmax, sum exp) of the 32 (row, its column) streams it sees; the 128 streams of a row meet in LDS at the end and ONE
// triple per (row, slice) goes out.  Columns >= V (the tail of the last slice) read the last real row of W and enter nothing.
__global__ __launch_bounds__(256) void sv_head_fused_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                             float* __restrict__ pm, int* __restrict__ pi, float* __restrict__ ps, long M, int V, int nsl) {
    extern __shared__ __attribute__((aligned(16))) float ldsf[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const long m0 = (long)blockIdx.x * SV_BM;
    const int n0 = blockIdx.y * SV_SLICE;
    for (int idx = tid; idx < SV_BM * (D / 4); idx += 256) {
        const int r = idx >> 7, q = idx & 127;
        *reinterpret_cast<f32x4*>(ldsf + r * SV_PA + 4 * q) = ldg4(x + min(m0 + r, M - 1) * D + 4 * q);
    }
    __syncthreads();
    SvTop top[2][16];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) top[mt][r] = SvTop{-INFINITY, INT_MAX, 0.f};
#pragma unroll 1
    for (int cb = wave; cb < SV_SLICE / 64; cb += 4) {
        const int nb = n0 + cb * 64;
        if (nb >= V) break;                                     // (wave-uniform; the barriers below are outside this loop)
        f32x16 acc[2][2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
        const float* const Ab = ldsf + l31 * SV_PA + 4 * hh;
        const float* const B0 = W + (long)min(nb + l31, V - 1) * D + 4 * hh;
        const float* const B1 = W + (long)min(nb + 32 + l31, V - 1) * D + 4 * hh;
#pragma unroll 4
        for (int kc = 0; kc < D / 8; ++kc) {
            const f32x4 b0 = ldg4(B0 + 8 * kc), b1 = ldg4(B1 + 8 * kc);
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(Ab + 8 * kc), a1 = *reinterpret_cast<const f32x4*>(Ab + 32 * SV_PA + 8 * kc);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b0[j], acc[0][0], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b0[j], acc[1][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b1[j], acc[0][1], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b1[j], acc[1][1], 0, 0, 0);
            }
        }
        // D: col = l31, row = (r&3) + 8*(r>>2) + 4*hh.  The lane's columns ascend (nt, then cb): a strict > keeps the lowest id of equals.
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int n = nb + nt * 32 + l31;
            if (n >= V) continue;
            const float bn = bias[n];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = acc[mt][nt][r] + bn;
                    SvTop& t = top[mt][r];
                    if (t.i == INT_MAX) { t = SvTop{v, n, 1.f}; continue; }
                    if (v > t.m) { t.s = t.s * expf(t.m - v) + 1.f; t.m = v; t.i = n; }
                    else t.s += expf(v - t.m);
                }
        }
    }
    __syncthreads();                                            // the row tile is dead: its LDS becomes the reduction arrays [64][129]
    float* const rm = ldsf; float* const rs = ldsf + SV_BM * SV_RP; int* const ri = reinterpret_cast<int*>(ldsf + 2 * SV_BM * SV_RP);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh, e = row * SV_RP + wave * 32 + l31;
            rm[e] = top[mt][r].m; rs[e] = top[mt][r].s; ri[e] = top[mt][r].i;
        }
    __syncthreads();
    if (tid < SV_BM && m0 + tid < M) {
        SvTop t{-INFINITY, INT_MAX, 0.f};
        for (int e = 0; e < 128; ++e) sv_merge(t, SvTop{rm[tid * SV_RP + e], ri[tid * SV_RP + e], rs[tid * SV_RP + e]});
        const long o = (m0 + tid) * nsl + blockIdx.y;
        pm[o] = t.m; pi[o] = t.i; ps[o] = t.s;
    }
}
// the slices of a row -> (argmax id, log-softmax at the argmax = -log sum exp(v - max))
__global__ __launch_bounds__(256) void sv_head_combine_kernel(const float* __restrict__ pm, const int* __restrict__ pi, const float* __restrict__ ps, int nsl,
                                                               int* __restrict__ ids, float* __restrict__ score, long M) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    SvTop t{-INFINITY, INT_MAX, 0.f};
    for (int j = 0; j < nsl; ++j) sv_merge(t, SvTop{pm[m * nsl + j], pi[m * nsl + j], ps[m * nsl + j]});
    ids[m] = t.i; score[m] = -logf(t.s);
}

// greedy CTC decode of one utterance per workgroup: a frame is kept when its id is not blank and differs from the previous frame's
// (of the SAME utterance).  Kept ids and their frames are compacted in order (block scan, 256 frames per round); the rest of the
// row is (blank, -1).
__global__ __launch_bounds__(256) void ctc_collapse_kernel(const int* __restrict__ ids, int S, int blank, int* __restrict__ tok, int* __restrict__ frm,
                                                            int* __restrict__ counts) {
    __shared__ int sc[256];
    __shared__ int carry;
    const int tid = threadIdx.x;
    const long o = (long)blockIdx.x * S;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < S; base += 256) {
        const int i = base + tid;
        int id = blank, keep = 0;
        if (i < S) { id = ids[o + i]; keep = id != blank && (i == 0 || ids[o + i - 1] != id); }
        sc[tid] = keep;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int v = tid >= d ? sc[tid - d] : 0;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        const int pos = carry + sc[tid] - keep;
        if (keep) { tok[o + pos] = id; frm[o + pos] = i; }
        __syncthreads();
        if (tid == 255) carry += sc[255];
        __syncthreads();
    }
    const int total = carry;
    for (int i = total + tid; i < S; i += 256) { tok[o + i] = blank; frm[o + i] = -1; }
    if (tid == 0) counts[blockIdx.x] = total;
}
int launch_collapse(const int* ids, int B, int S, int blank, int* tok, int* frm, int* counts, hipStream_t st) {
    hipLaunchKernelGGL(ctc_collapse_kernel, dim3(B), dim3(256), 0, st, ids, S, blank, tok, frm, counts);
    LAUNCH_CHECK();
    return TDX_OK;
}

}  // namespace

struct tdx_sv {
    int device = 0;
    int L = 0, LT = 0, vocab = 0, vpad = 0, head = 1;
    tdx::DevBuf dev, dev_planes;
    std::vector<PfLayer> layers, tp;
    const float *embed = nullptr, *ang = nullptr, *anb = nullptr, *tng = nullptr, *tnb = nullptr, *Wctc = nullptr, *bctc = nullptr;
    H3W hctc;
};

extern "C" {

int tdx_sv_create(int num_blocks, int tp_blocks, int vocab, const void* blob, size_t blob_bytes, int device, tdx_sv** out) {
    if (!blob || !out || num_blocks < 1 || tp_blocks < 0 || vocab < 2) return tdx::fail(TDX_E_INVALID, "tdx_sv_create: bad argument");
    tdx::Loader ld;       // (not strict: the tensors are read out of the whole model's checkpoint)
    if (!ld.parse(blob, blob_bytes)) return tdx::fail(TDX_E_BLOB, "tdx_sv_create: malformed TDXW blob");
    const int vpad = tdx::up(vocab, 256);
    const int nl = num_blocks + tp_blocks;
    std::unique_ptr<tdx_sv> h(new tdx_sv());
    h->device = device; h->L = num_blocks; h->LT = tp_blocks; h->vocab = vocab; h->vpad = vpad;
    h->layers.resize(num_blocks); h->tp.resize(tp_blocks);
    auto layer = [&](int l) -> PfLayer& { return l < num_blocks ? h->layers[l] : h->tp[l - num_blocks]; };
    for (int l = 0; l < nl && ld.ok(); ++l)
        pf_stage_layer(ld, l == 0 ? std::string("encoder.encoders0.0.")
                           : l < num_blocks ? "encoder.encoders." + std::to_string(l - 1) + "." : "encoder.tp_encoders." + std::to_string(l - num_blocks) + ".",
                       l == 0, layer(l));
    if (ld.ok()) {
        ld.push(h->embed, ld.get("embed.weight", {(uint32_t)SV_EMBED_ROWS, (uint32_t)DIN}), (size_t)SV_EMBED_ROWS * DIN);
        ld.push(h->ang, ld.get("encoder.after_norm.weight", D), D); ld.push(h->anb, ld.get("encoder.after_norm.bias", D), D);
        ld.push(h->tng, ld.get("encoder.tp_norm.weight", D), D); ld.push(h->tnb, ld.get("encoder.tp_norm.bias", D), D);
        ld.push(h->Wctc, ld.get("ctc.ctc_lo.weight", {(uint32_t)vocab, (uint32_t)D}), (size_t)vocab * D, (size_t)vpad * D);     // rows vocab..vpad-1 zero (the x3 Linear's N)
        ld.push(h->bctc, ld.get("ctc.ctc_lo.bias", vocab), vocab, vpad);
    }
    const char* e = getenv("TDX_SV_HEAD");                // 1 = fused head kernel, 0 = row chunks through the x3 Linear; unset = the default
    h->head = e && *e ? (atoi(e) != 0) : 1;
    TRY(ld.finish("tdx_sv_create", false, device, h->dev));
    std::vector<tdx::PlaneJob> jobs;
    for (int l = 0; l < nl; ++l) pf_queue_planes(l == 0, layer(l), jobs);
    if (!h->head) jobs.push_back({h->Wctc, vpad, D, &h->hctc.p, &h->hctc.s});
    TRY(tdx::split_weight_planes(jobs, device, h->dev_planes));
    if (h->head) {        // the fused head's 129 KB of dynamic LDS: a per-device attribute, set on this handle's device
        tdx::DeviceGuard guard(device);
        if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
        const hipError_t rc = hipFuncSetAttribute((const void*)sv_head_fused_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SV_LDS);
        if (rc != hipSuccess) return tdx::fail_hip(rc, __FILE__, __LINE__);
    }
    *out = h.release();
    return TDX_OK;
}

int tdx_sv_destroy(tdx_sv* h) {
    delete h;
    return TDX_OK;
}

static size_t sv_head_floats(const tdx_sv* h, size_t M) {
    if (h->head) return 3 * al(M * (size_t)((h->vocab + SV_SLICE - 1) / SV_SLICE));
    return al(std::min(M, (size_t)TDX_SV_LOGITS_ROWS) * (size_t)h->vpad);
}

size_t tdx_sv_workspace_bytes(const tdx_sv* h, int B, int T) {
    if (!h || B < 1 || T < 1 || (long)B * (T + SV_PROMPT) >= (1L << 22)) return 0;
    const size_t S = (size_t)T + SV_PROMPT, M = (size_t)B * S;
    return (pf_work_floats(B, S) + 2 * al(M * D) + sv_head_floats(h, M)) * sizeof(float);      // + second residual stream, LN'd rows, the head's buffer
}

double tdx_sv_flops(const tdx_sv* h, int B, int T) {
    if (!h) return 0.0;
    const double S = T + SV_PROMPT, M = (double)B * S;
    const double per = 2.0 * M * (3.0 * D * D + D * D + 2.0 * D * FFN) + 2.0 * B * H * (2.0 * S * S * DK) + 2.0 * M * D * KS;
    return (h->L + h->LT) * per + 2.0 * M * 3.0 * D * (DIN - D) + 2.0 * M * D * (double)h->vocab;
}

int tdx_ctc_collapse(const int* frame_ids, int B, int S, int blank, int* tok_ids, int* tok_frames, int* counts, void* stream) {
    if (!frame_ids || !tok_ids || !tok_frames || !counts || B < 1 || S < 1) return tdx::fail(TDX_E_INVALID, "tdx_ctc_collapse: bad argument");
    return launch_collapse(frame_ids, B, S, blank, tok_ids, tok_frames, counts, (hipStream_t)stream);
}

int tdx_sv_forward(tdx_sv* h, const float* feats, int B, int T, const int* prompt_host, float* enc, int* frame_ids, float* frame_score,
                   int* tok_ids, int* tok_frames, int* counts, void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !feats || !prompt_host || !frame_ids || !frame_score || !tok_ids || !tok_frames || !counts || !ws_ || B < 1 || T < 1)
        return tdx::fail(TDX_E_INVALID, "tdx_sv_forward: bad argument");
    PfPrompt pr;
    for (int i = 0; i < SV_PROMPT; ++i) {
        if (prompt_host[i] < 0 || prompt_host[i] >= SV_EMBED_ROWS) return tdx::fail(TDX_E_INVALID, "tdx_sv_forward: prompt id outside the 16-row embedding");
        pr.id[i] = prompt_host[i];
    }
    const size_t need = tdx_sv_workspace_bytes(h, B, T);
    if (!need) return tdx::fail(TDX_E_INVALID, "tdx_sv_forward: B * (T + 4) must stay below 2^22 rows");
    if (ws_bytes < need) return tdx::fail(TDX_E_WORKSPACE, "tdx_sv_forward: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    const int S = T + SV_PROMPT;
    const long M = (long)B * S;
    const PfWork k = pf_carve((float*)ws_, M, B, S);
    float* x2 = (float*)ws_ + pf_work_floats(B, S);
    float* encb = x2 + al(M * D);
    float* headb = encb + al(M * D);
    if (enc) encb = enc;
    // rows [embed[lid], embed[1], embed[2], embed[textnorm], feats(0..T-1)] of every utterance; the scale and the positions 1..S apply to all
    TRY(pf_embed_rows(feats, h->embed, pr, SV_PROMPT, k.xin, B, T, st));
    TRY(pf_run_layers(h->layers.data(), h->L, true, k.x, k, B, S, st));
    TRY(pf_layernorm_rows(k.x, h->ang, h->anb, x2, M, st));
    TRY(pf_run_layers(h->tp.data(), h->LT, false, x2, k, B, S, st));
    TRY(pf_layernorm_rows(x2, h->tng, h->tnb, encb, M, st));
    if (h->head) {
        const int nsl = (h->vocab + SV_SLICE - 1) / SV_SLICE;
        float* pm = headb; int* pi = (int*)(pm + al(M * nsl)); float* ps = (float*)pi + al(M * nsl);
        hipLaunchKernelGGL(sv_head_fused_kernel, dim3((unsigned)((M + SV_BM - 1) / SV_BM), nsl), dim3(256), SV_LDS, st, encb, h->Wctc, h->bctc, pm, pi, ps, M,
                           h->vocab, nsl);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(sv_head_combine_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, pm, pi, ps, nsl, frame_ids, frame_score, M);
        LAUNCH_CHECK();
    } else {
        if (launch_h3_split_rows(encb, D, k.hp, k.hs, M, D, st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
        for (long r0 = 0; r0 < M; r0 += TDX_SV_LOGITS_ROWS) {
            const int mc = (int)std::min<long>(TDX_SV_LOGITS_ROWS, M - r0);
            TRY(linear_h3(k.hp + r0 * (4L * D), k.hs + r0, mc, h->hctc, h->vpad, D, EpiBiasAct<>{h->bctc, headb, h->vpad}, st));
            TRY(pf_argmax_rows(headb, (long)h->vpad, h->vocab, frame_ids + r0, frame_score + r0, (long)mc, st));
        }
    }
    return launch_collapse(frame_ids, B, S, 0, tok_ids, tok_frames, counts, st);
}

}  // extern "C"
