// mf2.hip — MossFormer2 separator on MI355X: weight import, workspace plan, launch sequence
// and the C-ABI entry points declared in include/tdx.h.
//
// Reference being replaced: MossFormer2.forward look2hear/models/mossformer2.py:563-589 and
// everything it calls.  Data layout: every activation is
// token-major fp32 [B*S, C]; the 24-layer stack runs as a fixed sequence of launches on
// the caller's stream (no allocation, no sync => hipGraph-capturable).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tdx.h"
#include "gemm.hpp"
#include "gemm_x6.hpp"
#include "gemm_h3.hpp"
#include "gemm_h3a.hpp"
#include "mf2_kernels.hpp"
#include "mf2_attention.hpp"
#include "tdx_common.hpp"
#include "weight_planes.hpp"
#include "epilogues.hpp"

using namespace tdx;

namespace {

constexpr int C = 512, HID = 2048, HQ = HID + QK, INNER = 256;      // (QK = 128: mf2_attention.hpp)

// ------------------------------------------------------------------ GEMM epilogues
// (concept in gemm.hpp: col()/row() fetch per-column / per-row constants once, store() writes)
template <bool ACT>
struct EpiHiddenT {  // silu(acc*rs[m]*g[n] + b[n])                      mossformer_block.py:89-102
    // ACT = false: the pre-activation is stored and the consuming depthwise convolution applies SiLU as it loads (Conv17Args::silu_in)
    const float* rs; const float* g; const float* b; float* out; long ld;
    __device__ static float f(float x) { return ACT ? siluf_acc(x) : x; }
    __device__ Col2 col(int, int n) const { return Col2{g[n], b[n]}; }
    __device__ float row(int, int m) const { return rs[m]; }
    __device__ void store(int, int m, int n, float v, float r, Col2 c) const { out[(long)m * (int)ld + n] = f(v * r * c.a + c.b); }
    __device__ float* ptr(int, int m, int n) const { return out + (long)m * (int)ld + n; }
    __device__ long ldm() const { return ld; }
    __device__ void put(float* p, float v, float r, Col2 c) const { *p = f(v * r * c.a + c.b); }
    __device__ float rowmul(float r) const { return r; }              // (folded into the kernel's row / column scales:
    __device__ float colmul(Col2 c) const { return c.a; }             //  put_scaled() gets v * r * c.a)
    __device__ void put_scaled(float* p, float v, float, Col2 c) const { *p = f(v + c.b); }
};
using EpiHidden = EpiHiddenT<true>;
// the same (pre-activation stored) with the ScaleNorm row factor formed from per-segment sums of squares that the producer of
// the planes left behind: rs = 1 / max(sqrt(sum_j ss[j]) * C^-1/2, 1e-5)   (mossformer_block.py:52-54).
//   SHIFT: the token-shifted row = [half 0 of token s-1 (nothing at s = 0) | half 1 of token s]
//   else : the NSEG 128-channel segments of the gated attention output
template <int NSEG, bool SHIFT>
struct EpiHiddenSN {
    const float* ss; long M; int S; float cinv; const float* g; const float* b; float* out; long ld;
    __device__ Col2 col(int, int n) const { return Col2{g[n], b[n]}; }
    __device__ float row(int, int m) const {
        float s = 0.f;
        if constexpr (SHIFT) { s = ss[M + m]; if (m % S) s += ss[m - 1]; }
        else {
#pragma unroll
            for (int j = 0; j < NSEG; ++j) s += ss[(long)j * M + m];
        }
        return 1.0f / fmaxf(sqrtf(s) * cinv, 1e-5f);
    }
    __device__ float* ptr(int, int m, int n) const { return out + (long)m * (int)ld + n; }
    __device__ long ldm() const { return ld; }
    __device__ void put(float* p, float v, float r, Col2 c) const { *p = v * r * c.a + c.b; }
    __device__ float rowmul(float r) const { return r; }
    __device__ float colmul(Col2 c) const { return c.a; }
    __device__ void put_scaled(float* p, float v, float, Col2 c) const { *p = v + c.b; }
    __device__ void store(int, int m, int n, float v, float r, Col2 c) const { out[(long)m * (int)ld + n] = v * r * c.a + c.b; }
};
// to_hidden + to_qk with the depthwise convolution of v|u FUSED into the epilogue (gemm_h3.hpp H3Conv): the v|u columns leave the
// launch as K-major planes (+ u in fp32) — y = silu(.) never goes through HBM and conv17<4> is gone; the to_qk columns leave as
// fp32 pre-activations for conv17<3>, like EpiHiddenSN<2, true>.                   mossformer_block.py:89-102, conv_module.py:180-220
struct EpiHiddenConv {
    const float* ss; long M; int S; float cinv; const float* g; const float* b; float* out; long ld;
    const float* cw; unsigned char* vuP; float sv; float* u32; int Sp;
    __device__ Col2 col(int, int n) const { return Col2{g[n], b[n]}; }
    __device__ float row(int, int m) const {
        float s = ss[M + m]; if (m % S) s += ss[m - 1];
        return 1.0f / fmaxf(sqrtf(s) * cinv, 1e-5f);
    }
    __device__ float* ptr(int, int m, int n) const { return out + (long)m * (int)ld + n; }
    __device__ long ldm() const { return ld; }
    __device__ float rowmul(float r) const { return r; }
    __device__ float colmul(Col2 c) const { return c.a; }
    __device__ void put_scaled(float* p, float v, float, Col2 c) const { *p = v + c.b; }
    __device__ void put(float* p, float v, float r, Col2 c) const { *p = v * r * c.a + c.b; }
    __device__ void store(int, int m, int n, float v, float r, Col2 c) const { out[(long)m * (int)ld + n] = v * r * c.a + c.b; }
    __device__ float act(float v, Col2 c) const { return siluf_acc(v + c.b); }
    __device__ tdx::H3Conv conv() const { return tdx::H3Conv{cw, HID, HID, vuP, 4L * HID, sv, u32, HID / 2, (long)(HID / 2), S, Sp}; }
};
// pad rows S .. Sp-1 of every sample of the K-major v|u planes = 0 (the split-K lin_k^T [v|u] launch and the attention launch read
// whole 256-token groups); once per forward when the planes come from the fused epilogue, which only writes the S real rows
__global__ void zero_pad_rows_kernel(unsigned char* __restrict__ planes, int S, int Sp, long pitch) {
    const int b = blockIdx.y, r = S + blockIdx.x;
    uint4* p = reinterpret_cast<uint4*>(planes + ((long)b * Sp + r) * pitch);
    for (int i = threadIdx.x; i < pitch / 16; i += blockDim.x) p[i] = make_uint4(0u, 0u, 0u, 0u);
}
struct EpiQuadSim {  // relu(acc/256)^2 with key mask                       mossformer_block.py:256-262
    float* A; int G; int S; float inv_g;
    __device__ bool col(int z, int n) const { return (z % G) * 256 + n < S; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int z, int m, int n, float v, EpiNone, bool keep) const {
        float s = fmaxf(v * inv_g, 0.f);
        A[((long)z * 256 + m) * 256 + n] = keep ? s * s : 0.f;
    }
};
struct EpiBiasPrelu { // prelu_scalar(acc + b[n])                            mossformer_block.py:405-408
    const float* b; const float* a; float* out; long ld;
    __device__ Col2 col(int, int n) const { return Col2{b[n], a[0]}; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int, int m, int n, float v, EpiNone, Col2 c) const {
        v += c.a;
        out[(long)m * (int)ld + n] = v >= 0.f ? v : c.b * v;
    }
    __device__ float* ptr(int, int m, int n) const { return out + (long)m * (int)ld + n; }
    __device__ long ldm() const { return ld; }
    __device__ void put(float* p, float v, EpiNone, Col2 c) const { v += c.a; *p = v >= 0.f ? v : c.b * v; }
};
struct EpiBiasReluPl { const float* b; unsigned char* P; float* sc;   // relu(acc + b) as row-major planes (N = 256 = one tile: whole rows)
    __device__ float col(int, int n) const { return b[n]; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ float val(int, int, int, float v, EpiNone, float c) const { return fmaxf(v + c, 0.f); }
    __device__ tdx::H3PlOut plout(int) const { return tdx::H3PlOut{P, 1024, sc, nullptr, 0}; }
    __device__ long prow(int, int m) const { return m; } };
struct EpiBiasHalves { const float* b; float* out; long M;   // [M][2C] written as [2][M][C] (the two mask branches)
    __device__ float col(int, int n) const { return b[n]; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int, int m, int n, float v, EpiNone, float c) const { out[(long)(n >> 9) * M * C + (long)m * C + (n & 511)] = v + c; } };
struct EpiBiasResidualPl {   // the same, and the new x rows also as planes with one scale + sum of squares per (row, 256-channel half):
    // the A operand and the ScaleNorm statistics of the next layer's to_hidden (PLOUT; N = 512 = two tiles = the two halves)
    const float* b; float* x; long ld; unsigned char* xp; float* xs; float* xss; long M;
    __device__ float col(int, int n) const { return b[n]; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ float aux(int, int m, int n, EpiNone) const { return x[(long)m * (int)ld + n]; }
    __device__ float val(int, int, int, float v, EpiNone, float c, float xo) const { return xo + (v + c); }
    __device__ float* rowout(int, long m, int n0) const { return x + m * ld + n0; }          // the fp32 x rows, from phase 2 (full lines)
    // (the launch moves 1.7 GB and sits at ~82 % of the streaming kernels' HBM rate: see epi_has_rowout in gemm_h3.hpp)
    __device__ tdx::H3PlOut plout(int) const { return tdx::H3PlOut{xp, 2048, xs, xss, M}; }
    __device__ long prow(int, int m) const { return m; } };
struct EpiPosEnc {   // z = acc + pe[s][n]*scale ; x = z                     mossformer2.py:490-496
    const float* pe; const float* scale; float* zout; float* x; int S;
    __device__ float col(int, int) const { return scale[0]; }
    __device__ int row(int, int m) const { return m % S; }
    __device__ float aux(int, int, int n, int s) const { return pe[(long)s * C + n]; }
    __device__ void store(int, int m, int n, float v, int, float sc, float pv) const {
        const float r = v + pv * sc;
        zout[(long)m * C + n] = r; x[(long)m * C + n] = r;
    }
};
struct EpiTanhSig {  // tanh(a+bt)*sigmoid(g+bg)                             mossformer2.py:510
    const float* bias; float* out; long strideZ;
    __device__ Col2 col(int, int c) const { return Col2{bias[c], bias[C + c]}; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store2(int z, int m, int c, float a, float g, EpiNone, Col2 k) const {
        out[(long)z * strideZ + (long)m * C + c] = tanhf(a + k.a) * sigmoidf_acc(g + k.b);
    }
};
struct EpiMaskMul {  // mask = relu(acc); EM = E*mask                        mossformer2.py:513-518, :576
    const float* E; float* EM; float* mask; long strideZ;
    __device__ EpiNone col(int, int) const { return EpiNone{}; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ float aux(int, int m, int n, EpiNone) const { return E[(long)m * C + n]; }
    __device__ void store(int z, int m, int n, float v, EpiNone, EpiNone, float e) const {
        v = fmaxf(v, 0.f);
        if (mask) mask[(long)z * strideZ + (long)m * C + n] = v;
        EM[(long)z * strideZ + (long)m * C + n] = v * e;
    }
};

// positional tables, fp32 angle product then sin/cos of the ROUNDED angle:
//   pe[s][c]  = sin(s*inv_freq[c]) c<256 ; cos(s*inv_freq[c-256])           mossformer_block.py:68-73
//   rot[s][i] = cos/sin(s*freqs[i])                                         rotary_embedding_torch
__global__ void tables_kernel(const float* __restrict__ inv_freq, const float* __restrict__ freqs, float* __restrict__ pe,
                              float* __restrict__ rc, float* __restrict__ rsn, int S) {
    const int s = blockIdx.x;
    const float t = (float)s;
    for (int c = threadIdx.x; c < 256; c += blockDim.x) {
        const float ang = __fmul_rn(t, inv_freq[c]);
        pe[(long)s * C + c] = sinf(ang);
        pe[(long)s * C + 256 + c] = cosf(ang);
    }
    if (threadIdx.x < 16) {
        const float ang = __fmul_rn(t, freqs[threadIdx.x]);
        rc[s * 16 + threadIdx.x] = cosf(ang);
        rsn[s * 16 + threadIdx.x] = sinf(ang);
    }
}


// diagnostics (taps): largest |f16| of a planes buffer — how close the values written under a layer's STATIC scale come to the
// f16 range (2^15 after scaling = the bound derived from the weights).  out holds the bits of a non-negative float (atomicMax on
// the bit pattern is then the float maximum).
__global__ void planes_absmax_kernel(const _Float16* __restrict__ p, long n, unsigned* __restrict__ out) {
    float m = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) m = fmaxf(m, fabsf((float)p[i]));
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));
}
__global__ void zero_words_kernel(unsigned* __restrict__ p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0u;
}

// ------------------------------------------------------------------ model
struct LayerW {
    // FLASH
    const float *Whq = nullptr, *ghq = nullptr, *bhq = nullptr, *cw_h = nullptr, *cw_qk = nullptr, *gamma = nullptr, *beta = nullptr,
        *Wo = nullptr, *go = nullptr, *bo = nullptr, *cw_o = nullptr;
    // FSMN
    const float *W1 = nullptr, *b1 = nullptr, *a1 = nullptr, *ln1g = nullptr, *ln1b = nullptr, *Wuv = nullptr, *buv = nullptr,
        *cw_uv = nullptr, *Wl = nullptr, *bl = nullptr, *Wp = nullptr, *w1T = nullptr, *w2T = nullptr, *ing = nullptr, *inb = nullptr,
        *pre = nullptr, *ln2g = nullptr, *ln2b = nullptr, *W2 = nullptr, *b2 = nullptr;
    // nn.Linear weights as split-f16 planes + row scales (gemm_h3.hpp), made once at create
    H3W hWhq, hWo, hW1, hWuv, hWl, hWp, hW2;
    // static power-of-two scales of the K-major planes of v|u and lin_k (bounds from the weights, see tdx_mf2_create):
    // sv_* multiplies the value before the f16 split, st points at the device copy of {1/sv_vu, 1/sv_lk}
    float sv_vu, sv_lk;
    const float* st = nullptr;
};

}  // namespace

constexpr long FORK_ROWS = 1L << 40;    // token rows up to which a FLASH layer forks its q/k-head branch onto the side stream (env TDX_FORK_ROWS):
                                        // −5.7 % at one window per call, −0.6 % at 30 windows (the branches fill each other's tile tails), so: always

struct tdx_mf2 {
    int device;
    int L;
    tdx::DevBuf dev_weights;
    tdx::DevBuf dev_planes;         // split-f16 planes + scales of every nn.Linear weight
    tdx::DevBuf dev_static;         // [L][2] inverse static scales
    H3W hWenc, hWout, hWtg, hWdec1;
    std::vector<LayerW> layers;
    const float *encT = nullptr, *gn1g = nullptr, *gn1b = nullptr, *Wenc = nullptr, *pe_scale = nullptr, *inv_freq = nullptr,
        *rot_freqs = nullptr, *lnfg = nullptr, *lnfb = nullptr, *gn2g = nullptr, *gn2b = nullptr, *prelu = nullptr, *Wout = nullptr,
        *bout = nullptr, *Wtg = nullptr, *btg = nullptr, *Wdec1 = nullptr, *decT = nullptr;
    int taps;
    // optional live profiling of the dominant kernel (to_hidden GEMM): event pairs recorded on
    // the forward's stream, read back by tdx_mf2_profile_collect after the caller synchronised.
    std::vector<hipEvent_t> ev0, ev1;
    size_t ev_used;
    // The q/k-head branch of a FLASH layer (conv17<3> -> similarity GEMM) runs on a side stream next to the v|u branch
    // (conv17<4> -> lin_k^T[v|u]); fork / join by events, so the pair is capturable in a HIP graph.  The side stream and its three
    // events belong to the CALLER'S stream, not to the handle: one context per caller stream (created on first use, kept for the
    // handle's life), so that forwards issued concurrently on different (workspace, stream) pairs share nothing mutable
    // (include/tdx.h threading contract).  `mu` guards the map and the profile event vectors.
    struct SideCtx { hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr, ev_heads = nullptr, ev_sim = nullptr; };
    std::mutex mu;
    std::map<hipStream_t, SideCtx> side_ctx;
    static constexpr size_t MAX_SIDE_CTX = 64;    // beyond this many distinct caller streams a forward runs unforked (same results)
    // returns nullptr when no context can be had (stream under capture without one, creation failure, cap reached): the forward then
    // issues both branches on the caller's stream — slower at one window per call, never wrong
    SideCtx* side_for(hipStream_t st) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = side_ctx.find(st);
        if (it != side_ctx.end()) return &it->second;
        if (side_ctx.size() >= MAX_SIDE_CTX) return nullptr;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        if (cs != hipStreamCaptureStatusNone) return nullptr;      // no stream / event creation inside a capture: capture after one eager call on that stream
        SideCtx c;
        if (hipStreamCreateWithFlags(&c.side, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c.ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c.ev_heads, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c.ev_sim, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            if (c.ev_sim) hipEventDestroy(c.ev_sim);
            if (c.ev_heads) hipEventDestroy(c.ev_heads);
            if (c.ev_fork) hipEventDestroy(c.ev_fork);
            if (c.side) hipStreamDestroy(c.side);
            return nullptr;
        }
        return &(side_ctx[st] = c);      // (std::map: the address stays valid while other streams are added)
    }
};

namespace {

struct Plan {
    int B, T, S, G, Sp, splits, kchunk, nblk_enc, nblk_gn, nchunk1, nchunk2;
    long M;
    // offsets in floats
    size_t fs, xp, xs, xss, os, oss, zrow, E, z, x, rs, hid, vu, qk4, Abuf, slab, kvu, o, t, hraw, h, hp, hs, vuP, AbufP, Asc, qks, KvuP, kvus, uvpre, uv, f, p, c1, c2, pe, rc, rsn, stat,
        part, tap0, tap1, mask, hdr, total;
};


bool make_plan(const tdx_mf2* h, int B, int T, Plan& P) {
    if (B < 1 || T < 16) return false;
    P.B = B; P.T = T; P.S = (T - 16) / 8 + 1; P.G = (P.S + 255) / 256; P.Sp = P.G * 256; P.M = (long)B * P.S;
    // split-K for the linear-attention K^T[v|u] GEMM (16 N-tiles per sample, 3 blocks per CU
    // resident): aim for >= 1536 workgroups so that the 256 CUs stay full (slabs are 1 MB each)
    int sp = (1536 + 16 * B - 1) / (16 * B); if (sp < 1) sp = 1;
    int maxsp = (P.S + 511) / 512; if (sp > maxsp) sp = maxsp;
    P.splits = sp;
    P.kchunk = ((P.S + sp - 1) / sp + 31) / 32 * 32;
    P.splits = (P.S + P.kchunk - 1) / P.kchunk;
    P.nblk_enc = (P.S + ENC_TOK - 1) / ENC_TOK;
    P.nblk_gn = (P.S + 63) / 64;
    const int ts = ddn_ts(B, P.S);
    P.nchunk1 = (P.S + ts - 1) / ts;
    P.nchunk2 = 2 * ((P.S + 2 * ts - 1) / (2 * ts));
    const size_t M = (size_t)P.M;
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += al(n); return o; };
    P.E = take(M * C); P.z = take(M * C); P.x = take(M * C); P.rs = take(M);
    P.hid = take(M * HQ); P.vu = take(M * HID);
    P.qk4 = take((size_t)4 * B * P.Sp * QK);
    P.Abuf = take((size_t)B * P.G * 65536);
    P.slab = take((size_t)B * P.splits * QK * HID);
    P.kvu = take((size_t)B * QK * HID);
    P.o = take(M * 1024); P.t = take(M * C);
    P.hraw = take(M * INNER); P.h = take(M * INNER);
    P.hp = take(M * 1024);      // split-f16 planes of the current GEMM's A operand (<= 1024 channels: 4 KB per row)
    P.hs = take(2 * M);         // and its row scales (2M rows of 512 in the output head)
    // attention on the x3 core: K-major planes of v|u (pad rows zero), row-major planes + row scales of the
    // relu^2 similarity, row scales of quad_q / lin_q / quad_k (their planes live in the qk4 slots), K-major
    // planes of Kvu with one scale per sample (+ its atomicMax word)
    P.vuP = take((size_t)B * P.Sp * HID);
    P.AbufP = take((size_t)B * P.G * 65536);
    P.Asc = take((size_t)B * P.Sp);
    P.qks = take((size_t)3 * B * P.Sp);
    P.KvuP = take((size_t)B * QK * HID);
    P.kvus = take((size_t)B + (size_t)B * (QK * HID / 1024) + 64);
    P.uvpre = take(M * C); P.uv = take(M * C); P.f = take(M * INNER); P.fs = take(M); P.p = take(M * INNER);
    P.xp = take(M * C);          // x as planes (2 KB per row) with per-half scales / sums of squares
    P.xs = take(2 * M); P.xss = take(2 * M);
    P.os = take(8 * M); P.oss = take(8 * M);      // per-(token, 128-channel segment) scales / sums of squares of the gated attention output
    P.zrow = take(1024);         // zero planes row (token shift at the first token of a sample)
    P.c1 = take(M * INNER); P.c2 = take(M * INNER);
    P.pe = take((size_t)P.S * C); P.rc = take((size_t)P.S * 16); P.rsn = take((size_t)P.S * 16);
    P.stat = take((size_t)B * 2 + (size_t)2 * B * 256 * 2 + 64);
    size_t npart = (size_t)B * (P.nblk_enc > P.nblk_gn ? P.nblk_enc : P.nblk_gn) * 2;
    size_t npart_in = (size_t)B * (P.nchunk1 > P.nchunk2 ? P.nchunk1 : P.nchunk2) * 256 * 2;
    if (npart_in > npart) npart = npart_in;
    P.part = take(npart * 2);   // doubles
    if (h->taps) { P.tap0 = take(M * C); P.tap1 = take(M * C); P.mask = take(2 * M * C); P.hdr = take((size_t)h->L * 2 + 64); }
    else { P.tap0 = P.tap1 = P.mask = P.hdr = 0; }
    P.total = off;
    return true;
}


inline dim3 rows4(long M) { return dim3((unsigned)((M + 3) / 4)); }

// conv17 launch helper
template <int MODE>
int launch_conv17(Conv17Args a, int B, hipStream_t st) {
    constexpr int TPT = (MODE == 2 || MODE == 3) ? 32 : 128;      // tokens per thread
    constexpr int TPT_SMALL = TPT / 4;                             // small problems: 4x the blocks (one window per call: 68-136 blocks otherwise)
    const int quads = a.C / 4;
    const int qb = quads >= 256 ? 256 : quads;      // 256, 128 or 32
    const int ty = 256 / qb;
    dim3 block(qb, ty);
    const int s_lim = MODE >= 2 ? a.Sp : a.S;
    const long nblk = (long)(quads / qb) * ((s_lim + ty * TPT - 1) / (ty * TPT)) * B;
    if (nblk < 512) {
        dim3 grid(quads / qb, (s_lim + ty * TPT_SMALL - 1) / (ty * TPT_SMALL), B);
        hipLaunchKernelGGL((conv17_kernel<MODE, TPT_SMALL>), grid, block, 0, st, a);
    } else {
        dim3 grid(quads / qb, (s_lim + ty * TPT - 1) / (ty * TPT), B);
        hipLaunchKernelGGL((conv17_kernel<MODE, TPT>), grid, block, 0, st, a);
    }
    LAUNCH_CHECK();
    return TDX_OK;
}

// quadratic + linear attention on the fp32-MFMA / x6 cores: tdx_cal_attention at E % 128 != 0 (the model's path, and
// tdx_cal_attention otherwise, is attention_core_h3 in mf2_attention.hpp).
// qk4: [4][B][Sp][128] (quad_q, lin_q, quad_k, lin_k; rotary applied, pad rows zero);
// vu: [B*S][2E].  Produces o (gated) or att_v/att_u.
int attention_core(const float* qk4, const float* vu, int B, int S, int E, int splits, int kchunk, float* Abuf, float* slab,
                   float* kvu, float* o, float* att_v, float* att_u, hipStream_t st) {
    const int G = (S + 255) / 256, Sp = G * 256;
    const long hs = (long)B * Sp * QK;
    const float *quad_q = qk4, *lin_q = qk4 + hs, *quad_k = qk4 + 2 * hs, *lin_k = qk4 + 3 * hs;
    {   // A = relu(q k^T / 256)^2 per group                          mossformer_block.py:256-262
        GemmArgs g = make_args(256, 256, make_seg(quad_q, QK, quad_k, QK, QK, 256L * QK, 256L * QK));
        g.seg[0].zdiv = 1;
        EpiQuadSim e{Abuf, G, S, 1.0f / 256.0f};
        if (launch_gemm<false, false, false, false>(g, B * G, e, st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
    }
    {   // slab[b][sp] = lin_k^T [v|u] over the split's token range      mossformer_block.py:286,289
        GemmSeg s = make_seg(lin_k, QK, vu, 2L * E, kchunk, (long)Sp * QK, (long)S * 2 * E);
        s.zdiv = splits; s.strideA2 = (long)kchunk * QK; s.strideB2 = (long)kchunk * 2 * E; s.kchunk = kchunk; s.ktotal = S;
        GemmArgs g = make_args(QK, 2 * E, s);
        EpiStoreZ e{slab, 2L * E, (long)QK * 2 * E};
        if (launch_gemm<true, true, false, false>(g, B * splits, e, st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
        const long per = (long)QK * 2 * E;
        hipLaunchKernelGGL(kvu_reduce_kernel, dim3((unsigned)((per / 4 + 255) / 256), B), dim3(256), 0, st, slab, kvu, splits, per, (float)S);
        LAUNCH_CHECK();
    }
    {   // [A | lin_q] x [VU ; Kvu] with the gate epilogue              mossformer_block.py:269-294, :217
        GemmSeg s0 = make_seg(Abuf, 256, vu, 2L * E, 256, (long)G * 65536, (long)S * 2 * E);
        s0.zdiv = G; s0.strideA2 = 65536; s0.strideB2 = 256L * 2 * E; s0.kchunk = 256; s0.ktotal = S;
        GemmSeg s1 = make_seg(lin_q, QK, kvu, 2L * E, QK, (long)Sp * QK, (long)QK * 2 * E);
        s1.zdiv = G; s1.strideA2 = 256L * QK; s1.strideB2 = 0; s1.kchunk = 0; s1.ktotal = QK;
        GemmArgs g = make_args(256, E, s0);
        g.seg[1] = s1; g.nseg = 2; g.pair_off = E;
        EpiAttnGate e{vu, o, att_v, att_u, G, S, E};
        hipError_t r;
        if (E % 128 == 0) r = launch_gemm_x6<true, true, false>(g, B * G, e, st);       // split-bf16 x6 core (256-row group = one M tile)
        else r = launch_gemm<false, true, true, false>(g, B * G, e, st);                // fp32-MFMA core (test shapes with E % 128 != 0)
        if (r != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
    }
    return TDX_OK;
}

// A/B switch for the half-height two-blocks-per-CU attention kernel (gemm_h3a.hpp; bit-identical to the wide kernel).
// TDX_H3A=0 selects the wide 256-row kernel.
inline bool use_h3a() {
    static const bool on = [] { const char* e = getenv("TDX_H3A"); return e ? atoi(e) != 0 : true; }();
    return on;
}
// A/B switch for the order of the attention launch's two segments on that kernel (attention_core_h3 in mf2_attention.hpp):
// TDX_H3A_SWAP=0 restores the wide kernel's order.
inline bool h3a_swap() {
    static const bool on = [] { const char* e = getenv("TDX_H3A_SWAP"); return e ? atoi(e) != 0 : true; }();
    return on;
}


int ddn_core(const float* p, int B, int S, const float* w1T, const float* w2T, const float* ing, const float* inb,
             const float* pre, float* c1, float* c2, float* stat1, float* stat2, double* part, hipStream_t st) {
    const int ts = ddn_ts(B, S);
    const int nchunk1 = (S + ts - 1) / ts, nchunk2 = 2 * ((S + 2 * ts - 1) / (2 * ts));
    hipLaunchKernelGGL(ddn_conv1_kernel, dim3(nchunk1, B), dim3(256), 0, st, p, w1T, c1, part, S, nchunk1, ts);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(in_finalize_kernel, dim3(B, 16), dim3(256), 0, st, part, stat1, nchunk1, S);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(ddn_conv2_kernel, dim3(nchunk2, B), dim3(256), 0, st, c1, p, stat1, ing, inb, pre, w2T, c2, part, S, nchunk2, ts);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(in_finalize_kernel, dim3(B, 16), dim3(256), 0, st, part, stat2, nchunk2, S);
    LAUNCH_CHECK();
    return TDX_OK;
}

// nn.Linear on the split-f16 x3 core with A in fp32: split pass first (rows whose producer does not own whole rows)
template <class Epi>
int split_linear_h3(const float* A, long lda, unsigned char* hp, float* hs, int M, const H3W& W, int N, int K, Epi e, hipStream_t st) {
    if (tdx::launch_h3_split_rows(A, lda, hp, hs, M, K, st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
    return linear_h3(hp, hs, M, W, N, K, e, st);
}

// A/B switch: the depthwise convolution of v|u fused into the to_hidden epilogue (gemm_h3.hpp H3Conv).  TDX_FUSE_CONV=0 restores the
// separate conv17<4> pass (same arithmetic in the same order: bit-identical results).
inline bool fuse_conv() {
    static const bool on = [] { const char* e = getenv("TDX_FUSE_CONV"); return e ? atoi(e) != 0 : true; }();
    return on;
}
template <bool TWOSEG, class Epi>
hipError_t launch_linear_x3(tdx::H3Args g, Epi e, hipStream_t st) {
    return tdx::launch_gemm_h3x<false, false, false, TWOSEG>(g, 1, e, st);
}

}  // namespace

// =====================================================================================
extern "C" {

const char* tdx_version(void) { return "tdx 0.1.0 gfx950"; }
const char* tdx_last_error(void) { return tdx::last_error().c_str(); }

int tdx_mf2_create(const tdx_mf2_config* cfg, const void* blob, size_t blob_bytes, int device, tdx_mf2** out) {
    if (!cfg || !blob || !out) return tdx::fail(TDX_E_INVALID, "tdx_mf2_create: null argument");
    if (cfg->channels != C || cfg->num_spks != 2 || cfg->kernel_size != 16 || cfg->group_size != 256 || cfg->num_blocks < 1)
        return tdx::fail(TDX_E_INVALID, "tdx_mf2_create: unsupported config (need channels=512, spks=2, kernel=16, group=256)");
    tdx::Loader ld;       // strict both ways, like load_state_dict(strict=True) at base_model.py:63
    if (!ld.parse(blob, blob_bytes)) return tdx::fail(TDX_E_BLOB, "tdx_mf2_create: malformed TDXW blob");
    const int L = cfg->num_blocks;
    ld.host.reserve(60u * 1000 * 1000);
    std::vector<float> stat_host((size_t)L * 2, 1.f);
    std::vector<float> sv_host((size_t)L * 2, 1.f);
    std::unique_ptr<tdx_mf2> h(new tdx_mf2());
    h->device = device; h->L = L; h->taps = 0; h->ev_used = 0;
    h->layers.resize(L);
    const std::string PFX = "mask_net.mdl.intra_mdl.mossformerM.";
    for (int l = 0; l < L && ld.ok(); ++l) {
        LayerW& w = h->layers[l];
        const std::string p = PFX + "layers." + std::to_string(l) + ".";
        const float* Wh = ld.get(p + "to_hidden.mdl.1.weight", (size_t)HID * C);
        const float* Wq = ld.get(p + "to_qk.mdl.1.weight", (size_t)QK * C);
        const float* bh = ld.get(p + "to_hidden.mdl.1.bias", HID);
        const float* bq = ld.get(p + "to_qk.mdl.1.bias", QK);
        const float* gh = ld.get(p + "to_hidden.mdl.0.g", 1);
        const float* gq = ld.get(p + "to_qk.mdl.0.g", 1);
        const float* cwh = ld.get(p + "to_hidden.mdl.3.sequential.1.conv.weight", (size_t)HID * 17);
        const float* cwq = ld.get(p + "to_qk.mdl.3.sequential.1.conv.weight", (size_t)QK * 17);
        if (!ld.ok()) break;
        ld.push(w.Whq, Wh, (size_t)HID * C); ld.push(Wq, (size_t)QK * C);       // contiguous [2176][512] (HID*C is 64-aligned)
        ld.host.resize(ld.host.size() + (size_t)128 * C, 0.f);                     // zero rows up to 2304: the x6 GEMM reads W in 256-row tiles
        const size_t ghq = ld.room(w.ghq, HQ);
        for (int i = 0; i < HQ; ++i) ld.host[ghq + i] = i < HID ? gh[0] : gq[0];
        const size_t bhq = ld.room(w.bhq, HQ);
        for (int i = 0; i < HQ; ++i) ld.host[bhq + i] = i < HID ? bh[i] : bq[i - HID];
        ld.push_tapmajor(w.cw_h, cwh, HID, 17);
        ld.push_tapmajor(w.cw_qk, cwq, QK, 17);
        (void)ld.get(p + "rotary_pos_emb.freqs", 16);      // one RotaryEmbedding object shared by all layers (mossformer_block.py:453): layer 0's copy is used
        const float* gam = ld.get(p + "qk_offset_scale.gamma", 4 * QK);
        const float* bet = ld.get(p + "qk_offset_scale.beta", 4 * QK);
        ld.push(w.gamma, gam, 4 * QK);
        ld.push(w.beta, bet, 4 * QK);
        if (!ld.ok()) break;
        {
            // Static bounds for the K-major planes (gemm_h3.hpp).  After ScaleNorm the (shifted) row has norm
            // <= sqrt(512), so |x_hat . W_n| <= sqrt(512) |g| ||W_n|| (Cauchy-Schwarz) and |silu(p)| <= |p|;
            // the depthwise conv + identity multiplies by at most 1 + sum_t |w_ct|; OffsetScale by |gamma|,
            // + |beta|; the rotary pair rotation by sqrt(2).
            auto ybound = [&](const float* W, const float* bias, int rows, float gs) {
                double best = 0;
                for (int n = 0; n < rows; ++n) {
                    double q2 = 0;
                    for (int k = 0; k < C; ++k) q2 += (double)W[(size_t)n * C + k] * W[(size_t)n * C + k];
                    best = std::max(best, std::sqrt(512.0) * std::fabs(gs) * std::sqrt(q2) + std::fabs(bias[n]));
                }
                return best;
            };
            auto wsum = [&](const float* cw, int rows) {
                double best = 0;
                for (int c = 0; c < rows; ++c) {
                    double a = 1.0;
                    for (int t = 0; t < 17; ++t) a += std::fabs(cw[(size_t)c * 17 + t]);
                    best = std::max(best, a);
                }
                return best;
            };
            const double vub = wsum(cwh, HID) * ybound(Wh, bh, HID, gh[0]);
            double gmax = 0, bmax = 0;
            for (int i = 0; i < QK; ++i) { gmax = std::max(gmax, (double)std::fabs(gam[3 * QK + i])); bmax = std::max(bmax, (double)std::fabs(bet[3 * QK + i])); }
            const double lkb = (wsum(cwq, QK) * ybound(Wq, bq, QK, gq[0]) * gmax + bmax) * std::sqrt(2.0);
            auto pow2scale = [](double bound) { int e = (int)std::floor(std::log2(std::max(bound, 1e-30))); e = std::max(-100, std::min(100, e)); return std::ldexp(1.0, 14 - e); };
            sv_host[l * 2] = (float)pow2scale(vub); sv_host[l * 2 + 1] = (float)pow2scale(lkb);
            stat_host[l * 2] = 1.0f / sv_host[l * 2]; stat_host[l * 2 + 1] = 1.0f / sv_host[l * 2 + 1];
        }
        ld.push(w.Wo, ld.get(p + "to_out.mdl.1.weight", (size_t)C * 1024), (size_t)C * 1024);
        const float* go = ld.get(p + "to_out.mdl.0.g", 1);
        const size_t go_off = ld.room(w.go, C);
        if (go) for (int i = 0; i < C; ++i) ld.host[go_off + i] = go[0];
        ld.push(w.bo, ld.get(p + "to_out.mdl.1.bias", C), C);
        ld.push_tapmajor(w.cw_o, ld.get(p + "to_out.mdl.3.sequential.1.conv.weight", (size_t)C * 17), C, 17);
        // FSMN
        const std::string q = PFX + "fsmn." + std::to_string(l) + ".";
        ld.push(w.W1, ld.get(q + "conv1.0.weight", (size_t)INNER * C), (size_t)INNER * C);
        ld.push(w.b1, ld.get(q + "conv1.0.bias", INNER), INNER);
        ld.push(w.a1, ld.get(q + "conv1.1.weight", 1), 1);
        ld.push(w.ln1g, ld.get(q + "norm1.weight", INNER), INNER);
        ld.push(w.ln1b, ld.get(q + "norm1.bias", INNER), INNER);
        // fold the FFConvM LayerNorm affine into its Linear:  LN(h)W^T+b = hhat (W diag(g))^T + (b + W beta)
        const size_t Wuv = ld.room(w.Wuv, (size_t)C * INNER);
        const size_t buv = ld.room(w.buv, C);
        for (int br = 0; br < 2 && ld.ok(); ++br) {
            const std::string r = q + "gated_fsmn." + (br == 0 ? "to_u" : "to_v") + ".mdl.";
            const float* lg = ld.get(r + "0.weight", INNER);
            const float* lb = ld.get(r + "0.bias", INNER);
            const float* W = ld.get(r + "1.weight", (size_t)INNER * INNER);
            const float* bb = ld.get(r + "1.bias", INNER);
            if (!ld.ok()) break;
            for (int n = 0; n < INNER; ++n) {
                double acc = bb[n];
                for (int k = 0; k < INNER; ++k) {
                    ld.host[Wuv + ((size_t)br * INNER + n) * INNER + k] = W[(size_t)n * INNER + k] * lg[k];
                    acc += (double)W[(size_t)n * INNER + k] * (double)lb[k];
                }
                ld.host[buv + br * INNER + n] = (float)acc;
            }
        }
        if (!ld.ok()) break;
        {
            const float* cu = ld.get(q + "gated_fsmn.to_u.mdl.3.sequential.1.conv.weight", (size_t)INNER * 17);
            const float* cv = ld.get(q + "gated_fsmn.to_v.mdl.3.sequential.1.conv.weight", (size_t)INNER * 17);
            const size_t cw_uv = ld.room(w.cw_uv, (size_t)17 * C);
            if (cu && cv) for (int c = 0; c < INNER; ++c) for (int t = 0; t < 17; ++t) {
                ld.host[cw_uv + (size_t)t * C + c] = cu[c * 17 + t];
                ld.host[cw_uv + (size_t)t * C + INNER + c] = cv[c * 17 + t];
            }
        }
        const std::string f = q + "gated_fsmn.fsmn.";
        ld.push(w.Wl, ld.get(f + "linear.weight", (size_t)INNER * INNER), (size_t)INNER * INNER);
        ld.push(w.bl, ld.get(f + "linear.bias", INNER), INNER);
        ld.push(w.Wp, ld.get(f + "project.weight", (size_t)INNER * INNER), (size_t)INNER * INNER);
        ld.push_tapmajor(w.w1T, ld.get(f + "conv.conv1.weight", (size_t)INNER * 39), INNER, 39);
        {   // conv2.weight [256][2][39] -> [39][2][256]
            const float* w2 = ld.get(f + "conv.conv2.weight", (size_t)INNER * 2 * 39);
            const size_t w2T = ld.room(w.w2T, (size_t)39 * 2 * INNER);
            if (w2) for (int j = 0; j < INNER; ++j) for (int ic = 0; ic < 2; ++ic) for (int t = 0; t < 39; ++t)
                ld.host[w2T + ((size_t)t * 2 + ic) * INNER + j] = w2[((size_t)j * 2 + ic) * 39 + t];
        }
        ld.push(w.ing, ld.get(f + "conv.norm1.weight", INNER), INNER); ld.push(ld.get(f + "conv.norm2.weight", INNER), INNER);
        ld.push(w.inb, ld.get(f + "conv.norm1.bias", INNER), INNER); ld.push(ld.get(f + "conv.norm2.bias", INNER), INNER);
        ld.push(w.pre, ld.get(f + "conv.prelu1.weight", INNER), INNER); ld.push(ld.get(f + "conv.prelu2.weight", INNER), INNER);
        ld.push(w.ln2g, ld.get(q + "norm2.weight", INNER), INNER);
        ld.push(w.ln2b, ld.get(q + "norm2.bias", INNER), INNER);
        ld.push(w.W2, ld.get(q + "conv2.weight", (size_t)C * INNER), (size_t)C * INNER);
        ld.push(w.b2, ld.get(q + "conv2.bias", C), C);
    }
    if (ld.ok()) {
        ld.push_tapmajor(h->encT, ld.get("enc.conv1d.weight", (size_t)C * 16), C, 16);
        ld.push(h->gn1g, ld.get("mask_net.norm.weight", C), C);
        ld.push(h->gn1b, ld.get("mask_net.norm.bias", C), C);
        ld.push(h->Wenc, ld.get("mask_net.conv1d_encoder.weight", (size_t)C * C), (size_t)C * C);
        ld.push(h->pe_scale, ld.get("mask_net.pos_enc.scale", 1), 1);
        ld.push(h->inv_freq, ld.get("mask_net.pos_enc.inv_freq", 256), 256);
        ld.push(h->rot_freqs, ld.get(PFX + "layers.0.rotary_pos_emb.freqs", 16), 16);
        ld.push(h->lnfg, ld.get("mask_net.mdl.intra_mdl.norm.weight", C), C);
        ld.push(h->lnfb, ld.get("mask_net.mdl.intra_mdl.norm.bias", C), C);
        ld.push(h->gn2g, ld.get("mask_net.mdl.intra_norm.weight", C), C);
        ld.push(h->gn2b, ld.get("mask_net.mdl.intra_norm.bias", C), C);
        ld.push(h->prelu, ld.get("mask_net.prelu.weight", 1), 1);
        ld.push(h->Wout, ld.get("mask_net.conv1d_out.weight", (size_t)2 * C * C), (size_t)2 * C * C);
        ld.push(h->bout, ld.get("mask_net.conv1d_out.bias", 2 * C), 2 * C);
        ld.push(h->Wtg, ld.get("mask_net.output.0.weight", (size_t)C * C), (size_t)C * C);
        ld.push(ld.get("mask_net.output_gate.0.weight", (size_t)C * C), (size_t)C * C);
        ld.push(h->btg, ld.get("mask_net.output.0.bias", C), C);
        ld.push(ld.get("mask_net.output_gate.0.bias", C), C);
        ld.push(h->Wdec1, ld.get("mask_net.conv1_decoder.weight", (size_t)C * C), (size_t)C * C);
        ld.push_tapmajor(h->decT, ld.get("dec.weight", (size_t)C * 16), C, 16);
    }
    TRY(ld.finish("tdx_mf2_create", true, device, h->dev_weights));
    {
        tdx::DeviceGuard guard(device);
        const hipError_t e = guard.err != hipSuccess ? guard.err : h->dev_static.upload(stat_host.data(), stat_host.size() * sizeof(float));
        if (e != hipSuccess) return tdx::fail_hip(e, __FILE__, __LINE__);
    }
    for (int l = 0; l < L; ++l) { h->layers[l].sv_vu = sv_host[l * 2]; h->layers[l].sv_lk = sv_host[l * 2 + 1]; h->layers[l].st = h->dev_static + l * 2; }
    // ---- split every nn.Linear weight [N][K] into f16 planes + row scales, once
    {
        std::vector<tdx::PlaneJob> jobs;
        auto job = [&](const float* w, int N, int K, H3W& dst) { jobs.push_back({w, N, K, &dst.p, &dst.s}); };
        for (int l = 0; l < L; ++l) {
            LayerW& w = h->layers[l];
            job(w.Whq, HQ, C, w.hWhq); job(w.Wo, C, 1024, w.hWo); job(w.W1, INNER, C, w.hW1);
            job(w.Wuv, C, INNER, w.hWuv); job(w.Wl, INNER, INNER, w.hWl);
            job(w.Wp, INNER, INNER, w.hWp); job(w.W2, C, INNER, w.hW2);
        }
        job(h->Wenc, C, C, h->hWenc); job(h->Wout, 2 * C, C, h->hWout);
        job(h->Wtg, 2 * C, C, h->hWtg); job(h->Wdec1, C, C, h->hWdec1);
        TRY(tdx::split_weight_planes(jobs, device, h->dev_planes));
    }
    *out = h.release();
    return TDX_OK;
}

int tdx_mf2_destroy(tdx_mf2* h) {
    if (!h) return TDX_OK;
    for (auto e : h->ev0) hipEventDestroy(e);
    for (auto e : h->ev1) hipEventDestroy(e);
    for (auto& kv : h->side_ctx) {
        hipEventDestroy(kv.second.ev_fork); hipEventDestroy(kv.second.ev_heads); hipEventDestroy(kv.second.ev_sim);
        hipStreamDestroy(kv.second.side);
    }
    delete h;
    return TDX_OK;
}

int tdx_mf2_enable_taps(tdx_mf2* h, int on) {
    if (!h) return tdx::fail(TDX_E_INVALID, "null handle");
    h->taps = on ? 1 : 0;
    return TDX_OK;
}

int tdx_mf2_profile_enable(tdx_mf2* h, int max_records) {
    if (!h || max_records < 0) return tdx::fail(TDX_E_INVALID, "tdx_mf2_profile_enable: bad argument");
    std::lock_guard<std::mutex> lk(h->mu);
    for (auto e : h->ev0) hipEventDestroy(e);
    for (auto e : h->ev1) hipEventDestroy(e);
    h->ev0.assign(max_records, nullptr); h->ev1.assign(max_records, nullptr); h->ev_used = 0;
    for (int i = 0; i < max_records; ++i) {
        if (hipEventCreate(&h->ev0[i]) != hipSuccess || hipEventCreate(&h->ev1[i]) != hipSuccess)
            return tdx::fail(TDX_E_HIP, "tdx_mf2_profile_enable: hipEventCreate failed");
    }
    return TDX_OK;
}

int tdx_mf2_profile_collect(tdx_mf2* h, double* total_ms, int* launches) {
    if (!h || !total_ms || !launches) return tdx::fail(TDX_E_INVALID, "tdx_mf2_profile_collect: null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    double tot = 0;
    for (size_t i = 0; i < h->ev_used; ++i) {
        float ms = 0.f;
        hipError_t e = hipEventElapsedTime(&ms, h->ev0[i], h->ev1[i]);
        if (e != hipSuccess) return tdx::fail_hip(e, __FILE__, __LINE__);
        tot += ms;
    }
    *total_ms = tot; *launches = (int)h->ev_used; h->ev_used = 0;
    return TDX_OK;
}

size_t tdx_mf2_workspace_bytes(const tdx_mf2* h, int B, int T) {
    Plan P;
    if (!h || !make_plan(h, B, T, P)) return 0;
    return P.total * sizeof(float);
}

double tdx_mf2_flops(const tdx_mf2* h, int B, int T) {
    Plan P;
    if (!h || !make_plan(h, B, T, P)) return 0.0;
    const double S = P.S, Sp = P.Sp, Bd = B;
    // 2*MAC accounting, same terms as SURVEY.md Appendix D (torch FlopCounter convention)
    double per_layer = 2.0 * S * C * HQ                       // to_hidden + to_qk
                       + 2.0 * Sp * 256 * QK                   // quad sim
                       + 2.0 * Sp * 256 * HID                  // A [v|u]
                       + 2.0 * Sp * QK * HID * 2               // lin K^T[v|u] and lin_q K
                       + 2.0 * S * 1024 * C                    // to_out
                       + 2.0 * S * (HQ + C + C) * 17           // depthwise k=17
                       + 2.0 * S * (C * INNER * 2 + 4.0 * INNER * INNER)   // fsmn 1x1 + 4 linears
                       + 2.0 * S * INNER * 39 * 3;             // depthwise k=39 (conv1: 1 tap set, conv2: 2)
    double head = 2.0 * S * (C * C + C * 2 * C + 2.0 * (2 * C * C) + 2.0 * C * C) + 2.0 * S * C * 16 * 3;
    return Bd * (h->L * per_layer + head);
}

int tdx_mf2_forward(tdx_mf2* h, const float* wav, int B, int T, float* out, void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !wav || !out || !ws_) return tdx::fail(TDX_E_INVALID, "tdx_mf2_forward: null argument");
    Plan P;
    if (!make_plan(h, B, T, P)) return tdx::fail(TDX_E_INVALID, "tdx_mf2_forward: need B>=1 and T>=16");
    if (ws_bytes < P.total * sizeof(float)) return tdx::fail(TDX_E_WORKSPACE, "tdx_mf2_forward: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)ws_;
    const int S = P.S, G = P.G, Sp = P.Sp;
    const long M = P.M;
    float *E = ws + P.E, *z = ws + P.z, *x = ws + P.x, *rs = ws + P.rs, *hid = ws + P.hid, *vu = ws + P.vu, *qk4 = ws + P.qk4,
          *Abuf = ws + P.Abuf, *slab = ws + P.slab, *kvu = ws + P.kvu, *o = ws + P.o, *t = ws + P.t, *hraw = ws + P.hraw,
          *hh = ws + P.h, *hs = ws + P.hs, *uvpre = ws + P.uvpre, *uv = ws + P.uv, *f = ws + P.f, *p = ws + P.p,
          *c1 = ws + P.c1, *c2 = ws + P.c2, *pe = ws + P.pe, *rc = ws + P.rc, *rsn = ws + P.rsn, *stat = ws + P.stat;
    double* part = (double*)(ws + P.part);
    unsigned char* hp = (unsigned char*)(ws + P.hp);
    unsigned char *vuP = (unsigned char*)(ws + P.vuP), *AbufP = (unsigned char*)(ws + P.AbufP), *KvuP = (unsigned char*)(ws + P.KvuP);
    float *Asc = ws + P.Asc, *qks = ws + P.qks, *kvus = ws + P.kvus;
    unsigned char *xp = (unsigned char*)(ws + P.xp), *oP = (unsigned char*)(ws + P.o), *zrow = (unsigned char*)(ws + P.zrow);
    float *xs = ws + P.xs, *xss = ws + P.xss, *os = ws + P.os, *oss = ws + P.oss;
    unsigned char* fP = (unsigned char*)(ws + P.f);     // f = relu(linear(x_u)) lives as planes only (1 KB per row, like the fp32 row)
    float* fs = ws + P.fs;
    float* gnstat = stat;               // [B][2]
    float* stat1 = stat + al(2 * B);    // [B][256][2]
    float* stat2 = stat1 + (size_t)B * 512;
    (void)G;

    // fork / join context of THIS caller stream (nullptr: run unforked)
    static const long fork_rows = [] { const char* e = getenv("TDX_FORK_ROWS"); return e ? atol(e) : FORK_ROWS; }();
    tdx_mf2::SideCtx* sc = M <= fork_rows ? h->side_for(st) : nullptr;

    hipLaunchKernelGGL(tables_kernel, dim3(S), dim3(256), 0, st, h->inv_freq, h->rot_freqs, pe, rc, rsn, S);
    LAUNCH_CHECK();
    if (fuse_conv() && Sp > S) {      // the fused epilogue writes the S real rows of the v|u planes only
        hipLaunchKernelGGL(zero_pad_rows_kernel, dim3(Sp - S, B), dim3(256), 0, st, vuP, S, Sp, 4L * HID);
        LAUNCH_CHECK();
    }
    unsigned* hdr = h->taps ? reinterpret_cast<unsigned*>(ws + P.hdr) : nullptr;       // [L][2] largest scaled |f16| of v|u and lin_k (tap "headroom")
    if (hdr) { hipLaunchKernelGGL(zero_words_kernel, dim3((2 * h->L + 255) / 256), dim3(256), 0, st, hdr, 2 * h->L); LAUNCH_CHECK(); }
    // ---- encoder + GroupNorm + 1x1 conv + positional encoding   (mossformer2.py:573, :487-496)
    hipLaunchKernelGGL(encoder_kernel, dim3(P.nblk_enc, B), dim3(128), 0, st, wav, h->encT, E, part, T, S, P.nblk_enc);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(B), dim3(64), 0, st, part, gnstat, P.nblk_enc, (double)S * C, 1e-8);
    LAUNCH_CHECK();
    hipLaunchKernelGGL((gn_apply_kernel<0>), dim3((unsigned)((M * 128 + 255) / 256)), dim3(256), 0, st, E, gnstat, h->gn1g, h->gn1b,
                       (const float*)nullptr, (const float*)nullptr, t, M, S);
    LAUNCH_CHECK();
    TRY(split_linear_h3(t, C, hp, hs, (int)M, h->hWenc, C, C, EpiPosEnc{pe, h->pe_scale, z, x, S}, st));
    // x as planes with per-half scales and sums of squares: inside the stack the producers of x keep them up to date
    hipLaunchKernelGGL(xplanes_kernel, dim3((unsigned)((2 * M + 3) / 4)), dim3(256), 0, st, x, xp, xs, xss, M, reinterpret_cast<float*>(zrow));
    LAUNCH_CHECK();

    for (int l = 0; l < h->L; ++l) {
        const LayerW& w = h->layers[l];
        // ================= FLASH_ShareA_FFConvM  (mossformer_block.py:191-220)
        // token shift + ScaleNorm: the GEMM reads the planes of x as TWO K segments — channels 0..255 from the row above
        // (zero row at the first token of a sample), channels 256..511 from the row itself — each with its own row scale;
        // the ScaleNorm factor comes from the halves' sums of squares (no pass over x)
        {
            // (live profiling is a single-caller diagnostic: the slot is claimed under the lock, the events are recorded on this stream)
            hipEvent_t pe0 = nullptr, pe1 = nullptr;
            {
                std::lock_guard<std::mutex> lk(h->mu);
                if (h->ev_used < h->ev0.size()) { pe0 = h->ev0[h->ev_used]; pe1 = h->ev1[h->ev_used]; h->ev_used++; }
            }
            const bool prof = pe0 != nullptr;
            if (prof) hipEventRecord(pe0, st);
            tdx::H3Args g{};
            g.seg[0] = tdx::h3_seg(xp, xs, 4L * C, w.hWhq.p, w.hWhq.s, 4L * C, C / 2);
            g.seg[0].a_shift = -1; g.seg[0].a_period = S; g.seg[0].a_zero = zrow;
            g.seg[1] = tdx::h3_seg(xp + 2 * C, xs + M, 4L * C, w.hWhq.p + 2 * C, w.hWhq.s, 4L * C, C / 2);
            g.nseg = 2; g.M = (int)M; g.N = HQ;
            if (fuse_conv()) {      // SiLU + depthwise conv of v|u in the epilogue: planes + fp32 u straight from the GEMM (H3Conv)
                EpiHiddenConv e{xss, M, S, 0.044194173824159216f, w.ghq, w.bhq, hid, HQ, w.cw_h, vuP, w.sv_vu, vu, Sp};
                const hipError_t rc = tdx::launch_gemm_h3x<false, false, false, true>(g, 1, e, st);
                if (rc != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
            } else {
                EpiHiddenSN<2, true> e{xss, M, S, 0.044194173824159216f, w.ghq, w.bhq, hid, HQ};       // (SiLU in conv17)
                if (launch_linear_x3<true>(g, e, st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
            }
            if (prof) hipEventRecord(pe1, st);
        }
        // small forwards: the q/k-head branch (conv17<3> -> similarity) on the side stream, next to the v|u branch
        const bool fork = sc != nullptr;
        hipStream_t sq = fork ? sc->side : st;
        if (fork && (hipEventRecord(sc->ev_fork, st) != hipSuccess || hipStreamWaitEvent(sc->side, sc->ev_fork, 0) != hipSuccess))
            return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
        {
            Conv17Args a{};
            a.in = hid; a.ld_in = HQ; a.col0 = 0; a.wT = w.cw_h; a.C = HID; a.out = vu; a.out_c0 = HID / 2; a.ld_out = HID / 2; a.S = S; a.Sp = Sp;
            a.hp = vuP; a.sv = w.sv_vu; a.silu_in = 1;
            if (!fuse_conv())
                TRY(launch_conv17<4>(a, B, st));      // v|u as K-major planes (GEMM operands; v also as the gate's operand) + u in fp32 (the gate's sigmoid)
            Conv17Args q{};
            q.in = hid; q.ld_in = HQ; q.col0 = HID; q.wT = w.cw_qk; q.C = QK; q.S = S; q.Sp = Sp; q.gamma = w.gamma; q.beta = w.beta;
            q.rot_cos = rc; q.rot_sin = rsn; q.head_stride = (long)B * Sp * QK;
            q.hp = (unsigned char*)qk4; q.hs = qks; q.sv = w.sv_lk; q.silu_in = 1;
            TRY(launch_conv17<3>(q, B, sq));          // the four heads as planes
            if (hdr) {
                hipLaunchKernelGGL(planes_absmax_kernel, dim3(1024), dim3(256), 0, st, reinterpret_cast<const _Float16*>(vuP), (long)B * Sp * HID * 2, hdr + 2 * l);
                LAUNCH_CHECK();
                hipLaunchKernelGGL(planes_absmax_kernel, dim3(256), dim3(256), 0, sq, reinterpret_cast<const _Float16*>(qk4) + 3L * B * Sp * 256, (long)B * Sp * 256,
                                   hdr + 2 * l + 1);
                LAUNCH_CHECK();
            }
            if (fork && hipEventRecord(sc->ev_heads, sc->side) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
        }
        TRY(attention_core_h3((const unsigned char*)qk4, qks, vuP, nullptr, w.st, B, S, 1024, P.splits, P.kchunk, Abuf, AbufP, Asc, slab, kvu, KvuP,
                              kvus, nullptr, nullptr, nullptr, st, use_h3a(), h3a_swap(), oP, os, oss, fork ? sc->side : nullptr, fork ? sc->ev_heads : nullptr, fork ? sc->ev_sim : nullptr, vu));
        {   // to_out: A = the planes of o with one row scale per 128-channel segment; ScaleNorm from the segments' sums of squares
            tdx::H3Args g{};
            g.seg[0] = tdx::h3_seg(oP, os, 4L * 1024, w.hWo.p, w.hWo.s, 4L * 1024, 1024);
            g.seg[0].segk = 128; g.seg[0].strideSeg = M;
            g.nseg = 1; g.M = (int)M; g.N = C;
            EpiHiddenSN<8, false> e{oss, M, S, 0.03125f, w.go, w.bo, t, C};
            if (launch_linear_x3<false>(g, e, st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
        }
        {
            Conv17Args a{};
            a.in = t; a.ld_in = C; a.col0 = 0; a.wT = w.cw_o; a.C = C; a.out = x; a.ld_out = C; a.S = S; a.Sp = Sp; a.silu_in = 1;
            a.xp = xp; a.xs = xs; a.xs_stride = M;       // the new x also as planes (per-half scales): W1's A operand
            TRY(launch_conv17<1>(a, B, st));
        }
        if (h->taps && l == 0) hipMemcpyAsync(ws + P.tap0, x, M * C * sizeof(float), hipMemcpyDeviceToDevice, st);
        // ================= GatedFSMNBlockDilated  (mossformer_block.py:419-425)
        {
            tdx::H3Args g{};
            g.seg[0] = tdx::h3_seg(xp, xs, 4L * C, w.hW1.p, w.hW1.s, 4L * C, C);
            g.seg[0].segk = 256; g.seg[0].strideSeg = M;
            g.nseg = 1; g.M = (int)M; g.N = INNER;
            if (tdx::launch_gemm_h3x<false, false, false, false>(g, 1, EpiBiasPrelu{w.b1, w.a1, hraw, INNER}, st) != hipSuccess)
                return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
        }
        hipLaunchKernelGGL((layernorm_kernel<INNER, true>), rows4(M), dim3(256), 0, st, hraw, w.ln1g, w.ln1b, hh, (float*)nullptr, M, 1e-5f,
                           hp, hs);
        LAUNCH_CHECK();
        TRY(linear_h3(hp, hs, (int)M, w.hWuv, C, INNER, EpiBiasAct<ActSilu>{w.buv, uvpre, C}, st));
        {
            Conv17Args a{};
            a.in = uvpre; a.ld_in = C; a.col0 = 0; a.wT = w.cw_uv; a.C = C; a.out = uv; a.ld_out = C; a.S = S; a.Sp = Sp;
            a.xp = hp; a.xs = hs;                          // x_u (channels 0..255) also as planes: the A operand of fsmn.linear
            TRY(launch_conv17<0>(a, B, st));
        }
        TRY(linear_h3(hp, hs, (int)M, w.hWl, INNER, INNER, EpiBiasReluPl{w.bl, fP, fs}, st));       // f = relu(.) as planes
        TRY(linear_h3(fP, fs, (int)M, w.hWp, INNER, INNER, EpiBiasAct<>{nullptr, p, INNER}, st));
        TRY(ddn_core(p, B, S, w.w1T, w.w2T, w.ing, w.inb, w.pre, c1, c2, stat1, stat2, part, st));
        hipLaunchKernelGGL(fsmn_tail_kernel, rows4(M), dim3(256), 0, st, c2, stat2, w.ing + INNER, w.inb + INNER, w.pre + INNER, uv, hh,
                           w.ln2g, w.ln2b, hp, hs, M, S);
        LAUNCH_CHECK();
        TRY(linear_h3(hp, hs, (int)M, w.hW2, C, INNER, EpiBiasResidualPl{w.b2, x, C, xp, xs, xss, M}, st));    // x += ..., and its planes / statistics
        if (h->taps && l == 0) hipMemcpyAsync(ws + P.tap1, x, M * C * sizeof(float), hipMemcpyDeviceToDevice, st);
    }

    // ---- LayerNorm, GroupNorm + skip, PReLU, output head   (mossformer2.py:320, :389-396, :500-521)
    hipLaunchKernelGGL((layernorm_kernel<C, false>), rows4(M), dim3(256), 0, st, x, h->lnfg, h->lnfb, t, (float*)nullptr, M, 1e-6f);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(rowblock_stats_kernel, dim3(P.nblk_gn, B), dim3(256), 0, st, t, part, S, 64, P.nblk_gn);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(B), dim3(64), 0, st, part, gnstat, P.nblk_gn, (double)S * C, 1e-8);
    LAUNCH_CHECK();
    float* r = uvpre;    // [M,512] scratch
    hipLaunchKernelGGL((gn_apply_kernel<1>), dim3((unsigned)((M * 128 + 255) / 256)), dim3(256), 0, st, t, gnstat, h->gn2g, h->gn2b, z,
                       h->prelu, r, M, S);
    LAUNCH_CHECK();
    float* r2 = o;       // [2][M][512]: the conv1d_out rows of the two speakers
    TRY(split_linear_h3(r, C, hp, hs, (int)M, h->hWout, 2 * C, C, EpiBiasHalves{h->bout, r2, M}, st));
    float* gate = vu;    // [2][M][512]
    {
        if (tdx::launch_h3_split_rows(r2, C, hp, hs, 2 * M, C, st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
        tdx::H3Args g{};
        g.seg[0] = tdx::h3_seg(hp, hs, 4L * C, h->hWtg.p, h->hWtg.s, 4L * C, C);
        g.seg[0].strideA = M * 4L * C; g.seg[0].strideSA = M;
        g.nseg = 1; g.M = (int)M; g.N = C; g.pair_off = C;
        if (tdx::launch_gemm_h3<true>(g, 2, EpiTanhSig{h->btg, gate, M * C}, st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
    }
    float* EM = hid;     // [2][M][512]
    {
        if (tdx::launch_h3_split_rows(gate, C, hp, hs, 2 * M, C, st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
        tdx::H3Args g{};
        g.seg[0] = tdx::h3_seg(hp, hs, 4L * C, h->hWdec1.p, h->hWdec1.s, 4L * C, C);
        g.seg[0].strideA = M * 4L * C; g.seg[0].strideSA = M;
        g.nseg = 1; g.M = (int)M; g.N = C;
        EpiMaskMul e{E, EM, h->taps ? ws + P.mask : nullptr, M * C};
        if (tdx::launch_gemm_h3<false>(g, 2, e, st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
    }
    float* D = t;        // [2][M][16]
    hipLaunchKernelGGL(decoder_dot_kernel, dim3((unsigned)((2 * M + 4 * DEC_ROWS - 1) / (4 * DEC_ROWS))), dim3(256), 0, st, EM, h->decT, D, 2 * M);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(decoder_ola_kernel, dim3((unsigned)(((long)B * 2 * T + 255) / 256)), dim3(256), 0, st, D, out, B, S, T);
    LAUNCH_CHECK();
    return TDX_OK;
}

int tdx_mf2_tap(tdx_mf2* h, const char* name, int B, int T, void* ws_, float* dst, size_t dst_elems, size_t* n, void* stream) {
    if (!h || !name || !ws_ || !dst) return tdx::fail(TDX_E_INVALID, "tdx_mf2_tap: null argument");
    Plan P;
    if (!make_plan(h, B, T, P)) return tdx::fail(TDX_E_INVALID, "tdx_mf2_tap: bad shape");
    float* ws = (float*)ws_;
    const size_t MC = (size_t)P.M * C;
    size_t off, cnt = MC;
    std::string s(name);
    if (s == "enc") off = P.E;
    else if (s == "z") off = P.z;
    else if (s == "after_stack") off = P.x;
    else if (!h->taps) return tdx::fail(TDX_E_INVALID, "tdx_mf2_tap: enable taps before forward for this tap");
    else if (s == "after_flash0") off = P.tap0;
    else if (s == "after_fsmn0") off = P.tap1;
    else if (s == "mask") { off = P.mask; cnt = 2 * MC; }
    else if (s == "headroom") { off = P.hdr; cnt = (size_t)h->L * 2; }     // per layer: largest |f16| written under the static scales of v|u, lin_k
    else return tdx::fail(TDX_E_INVALID, "tdx_mf2_tap: unknown tap " + s);
    if (n) *n = cnt;
    if (dst_elems < cnt) return tdx::fail(TDX_E_INVALID, "tdx_mf2_tap: destination too small");
    hipError_t e = hipMemcpyAsync(dst, ws + off, cnt * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return tdx::fail_hip(e, __FILE__, __LINE__);
    return TDX_OK;
}

// ------------------------------------------------------------------ stand-alone ops
size_t tdx_cal_attention_workspace_bytes(int B, int S, int E) {
    if (B < 1 || S < 1 || E < 64 || E % 64) return 0;
    int sp, kc; size_t a, b, c, d, e, tot;
    attn_plan(B, S, E, sp, kc, a, b, c, d, e, tot);
    return tot * sizeof(float);
}

int tdx_cal_attention(const float* quad_q, const float* lin_q, const float* quad_k, const float* lin_k, const float* v, const float* u,
                      const float* freqs, int B, int S, int E, float* att_v, float* att_u, void* ws_, size_t ws_bytes, void* stream) {
    if (!quad_q || !lin_q || !quad_k || !lin_k || !v || !u || !freqs || !att_v || !att_u || !ws_)
        return tdx::fail(TDX_E_INVALID, "tdx_cal_attention: null argument");
    if (B < 1 || S < 1 || E < 64 || E % 64) return tdx::fail(TDX_E_INVALID, "tdx_cal_attention: need E % 64 == 0");
    int splits, kchunk; size_t oq, ovu, oA, oslab, okvu, tot;
    attn_plan(B, S, E, splits, kchunk, oq, ovu, oA, oslab, okvu, tot);
    if (ws_bytes < tot * sizeof(float)) return tdx::fail(TDX_E_WORKSPACE, "tdx_cal_attention: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)ws_;
    TRY(attn_pack_inputs(quad_q, lin_q, quad_k, lin_k, v, u, freqs, B, S, E, ws, oq, ovu, st));
    if (E % 128) return attention_core(ws + oq, ws + ovu, B, S, E, splits, kchunk, ws + oA, ws + oslab, ws + okvu, nullptr, att_v, att_u, st);
    // ---- the model's path (split-f16 x3 core)
    AttnPlanes P;
    TRY(attn_prepare_planes(ws, oq, ovu, okvu, B, S, E, P, st));
    return attention_core_h3(P.qkP, P.qks, P.vuP, ws + ovu, P.stt, B, S, E, splits, kchunk, ws + oA, P.AbufP, P.Asc, ws + oslab, ws + okvu, P.KvuP, P.kvus,
                             nullptr, att_v, att_u, st, use_h3a(), h3a_swap());
}

size_t tdx_dilated_dense_net_workspace_bytes(int B, int S) {
    if (B < 1 || S < 1) return 0;
    const size_t M = (size_t)B * S;
    const int ts = ddn_ts(B, S);
    const int nchunk1 = (S + ts - 1) / ts, nchunk2 = 2 * ((S + 2 * ts - 1) / (2 * ts));
    const int nc = nchunk1 > nchunk2 ? nchunk1 : nchunk2;
    return (al(M * 256) * 2 + al((size_t)B * 512) * 2 + al(39 * 256) + al(39 * 512) + al((size_t)B * nc * 256 * 2 * 2)) * sizeof(float);
}

// weights arrive in the reference's native layouts here (w1[256][39], w2[256][2][39]); the
// tap-major transposition is done on the device side of this test hook by tiny kernels.
__global__ void transpose_w_kernel(const float* __restrict__ w, float* __restrict__ wT, int Cc, int inner, int k) {
    // w[c][i][t] -> wT[t][i][c]
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Cc * inner * k) return;
    const int t = idx % k, i = (idx / k) % inner, c = idx / (k * inner);
    wT[((long)t * inner + i) * Cc + c] = w[idx];
}

int tdx_dilated_dense_net(const float* p, int B, int S, const float* w1, const float* w2, const float* in_g, const float* in_b,
                          const float* prelu, float* out, void* ws_, size_t ws_bytes, void* stream) {
    if (!p || !w1 || !w2 || !in_g || !in_b || !prelu || !out || !ws_) return tdx::fail(TDX_E_INVALID, "tdx_dilated_dense_net: null argument");
    if (ws_bytes < tdx_dilated_dense_net_workspace_bytes(B, S)) return tdx::fail(TDX_E_WORKSPACE, "tdx_dilated_dense_net: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)ws_;
    const size_t M = (size_t)B * S;
    float* c1 = ws; float* c2 = c1 + al(M * 256);
    float* stat1 = c2 + al(M * 256); float* stat2 = stat1 + al((size_t)B * 512);
    float* w1T = stat2 + al((size_t)B * 512); float* w2T = w1T + al(39 * 256);
    double* part = (double*)(w2T + al(39 * 512));
    hipLaunchKernelGGL(transpose_w_kernel, dim3((256 * 39 + 255) / 256), dim3(256), 0, st, w1, w1T, 256, 1, 39);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(transpose_w_kernel, dim3((256 * 78 + 255) / 256), dim3(256), 0, st, w2, w2T, 256, 2, 39);
    LAUNCH_CHECK();
    TRY(ddn_core(p, B, S, w1T, w2T, in_g, in_b, prelu, c1, c2, stat1, stat2, part, st));
    hipLaunchKernelGGL(ddn_out_kernel, dim3((unsigned)((M * 256 + 255) / 256)), dim3(256), 0, st, c2, stat2, in_g + 256, in_b + 256,
                       prelu + 256, out, (long)M, S);
    LAUNCH_CHECK();
    return TDX_OK;
}

int tdx_linear(const float* a, const float* w, const float* bias, int M, int N, int K, float* c, void* stream) {
    if (!a || !w || !c) return tdx::fail(TDX_E_INVALID, "tdx_linear: null argument");
    if (M < 1 || N % 128 || K % 32 || N < 128 || K < 32) return tdx::fail(TDX_E_INVALID, "tdx_linear: need N%128==0, K%32==0");
    if (N % 256 == 0) return linear_x6(a, K, w, M, N, K, EpiBiasAct<>{bias, c, N}, (hipStream_t)stream);     // split-bf16 x6 core
    return linear_f32(a, K, w, M, N, K, EpiBiasAct<>{bias, c, N}, (hipStream_t)stream);                   // fp32-MFMA core
}

int tdx_cosine_scores(const float* emb, const float* ref, int N, int D, float* scores, void* stream) {
    if (!emb || !ref || !scores || N < 0 || D < 1) return tdx::fail(TDX_E_INVALID, "tdx_cosine_scores: bad argument");
    if (N == 0) return TDX_OK;
    hipLaunchKernelGGL(cosine_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, emb, ref, N, D, scores);
    LAUNCH_CHECK();
    return TDX_OK;
}

}  // extern "C"
