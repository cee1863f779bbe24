// mf2_attention.hpp — the quadratic + linear attention of a FLASH layer on the split-f16 x3 core (mossformer_block.py:222-294, :217):
// its GEMM epilogues, the launch sequence attention_core_h3, and the stand-alone input packing / plane preparation around it.
// Included by mf2.hip (the model's forward and tdx_cal_attention) and by diag.hip (the test hook tdx_attn_gate_planes, which
// calls attention_core_h3 with the planes-out gate exactly as the model does).  Everything sits in the unnamed namespace, as it
// did inside mf2.hip.  The kernels kmajor_to_rows / kvu_reduce_t / kvu_planes it launches are in mf2_kernels.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "../../include/tdx.h"
#include "gemm.hpp"
#include "gemm_h3.hpp"
#include "gemm_h3a.hpp"
#include "mf2_kernels.hpp"
#include "tdx_common.hpp"
#include "epilogues.hpp"

namespace {

constexpr int QK = 128;       // width of the four q/k heads

// ------------------------------------------------------------------ GEMM epilogues of the attention
struct EpiQuadSimPl {  // relu(acc/256)^2 with key mask (mossformer_block.py:256-262), written as row-major planes + row scales (PLOUT): the A operand of the attention GEMM's quadratic segment
    unsigned char* P; float* sc; int G; int S; float inv_g;
    __device__ bool col(int z, int n) const { return (z % G) * 256 + n < S; }
    __device__ tdx::EpiNone row(int, int) const { return tdx::EpiNone{}; }
    __device__ float val(int, int, int, float v, tdx::EpiNone, bool keep) const { const float s = fmaxf(v * inv_g, 0.f); return keep ? s * s : 0.f; }
    __device__ tdx::H3PlOut plout(int) const { return tdx::H3PlOut{P, 1024, sc, nullptr, 0}; }
    __device__ long prow(int z, int m) const { return (long)z * 256 + m; }
};
struct EpiAttnGate { // o = (att_u*v)*sigmoid(att_v*u)                       mossformer_block.py:217
    const float* vu; float* o; float* att_v; float* att_u; int G; int S; int E;
    __device__ tdx::EpiNone col(int, int) const { return tdx::EpiNone{}; }
    __device__ long row(int z, int m) const {     // global token row, or -1 for group padding
        const int b = z / G, s = (z % G) * 256 + m;
        return s < S ? (long)b * S + s : -1L;
    }
    __device__ bool full(int z, int m0) const { return (z % G) * 256 + m0 + 256 <= S; }
    __device__ float2 aux(int, int, int c, long rw) const {       // the gate's v, u operands
        if (rw < 0 || att_v) return make_float2(0.f, 0.f);
        return make_float2(vu[rw * (2 * E) + c], vu[rw * (2 * E) + E + c]);
    }
    __device__ void store2(int, int, int c, float av, float au, long rw, tdx::EpiNone, float2 vu2) const {
        if (rw < 0) return;
        if (att_v) {  // stand-alone cal_attention: return the two attention outputs
            att_v[rw * E + c] = av;
            att_u[rw * E + c] = au;
        } else {
            o[rw * E + c] = (au * vu2.x) * tdx::sigmoidf_acc(av * vu2.y);
        }
    }
};
struct EpiAttnGatePlOut { // the gate o = (att_u*v)*sigmoid(att_v*u) with o written as ROW-major planes (PLOUT): one scale and one sum of
    // squares per (token, 128-channel segment) — the A operand of to_out with segmented row scales and its ScaleNorm statistics.
    // Gate operands:
    //   v  from the K-major split-f16 planes ((hi + lo) * inv; hi and lo of 32 columns share one 128-B line: lanes 2j / 2j+1
    //      (adjacent columns) share the loads — the even lane fetches the 4-byte (c, c+1) word of hi, the odd lane that of lo — and
    //      swap by DPP quad_perm [1,0,3,2] in val2_scaled()).  v enters the product linearly: the planes' ABSOLUTE precision
    //      (2^-40 of the layer's static bound) is an error 2^-40 * bound * |att_u| against |att_u| * |v|_typical — harmless.
    //   u  in fp32 (`u32`, written by conv17<4> next to the planes).  u sits INSIDE the sigmoid, multiplied by att_v: an absolute
    //      error du becomes an error att_v * du of the argument.  With large attention values (heavy-tailed checkpoints: outlier
    //      rows in to_hidden AND to_qk give att_v ~ 1e8) the planes' 2^-40 * bound flipped the gate of the 0.3 % of the elements
    //      whose argument is O(1): 6e-4 rel-L2 on the layer output where fp32 arithmetic has 2e-6
    //      (tests/test_gpu_mossformer2.py::test_static_scales_under_heavy_tailed_weights).  fp32's relative precision is what the
    //      reference has; the bytes read per output element are the same (one 4-byte word of v, one of u).
    // aux() returns the RAW words (the kernel issues it ahead of the stores: anything that consumed the loads there would wait for
    // them there); the lane swap and the unpacking happen in val2_scaled().
    const unsigned char* vuP; const float* inv; const float* u32; unsigned char* oP; float* os; float* oss; long M; int G; int S; int Sp; int E;
    __device__ float col(int, int) const { return inv[0]; }
    __device__ long row(int z, int m) const { const int b = z / G, s = (z % G) * 256 + m; return s < S ? (long)b * S + s : -1L; }
    __device__ bool full(int z, int m0) const { return (z % G) * 256 + m0 + 256 <= S; }
    __device__ int2 aux(int z, int m, int c, long) const {
        const int b = z / G, s = min((z % G) * 256 + m, S - 1);
        const int c2 = c & ~1;
        const unsigned char* p = vuP + (long)b * Sp * (8L * E) + (long)s * (8 * E) + (c2 >> 5) * 128 + (c2 & 31) * 2 + (c & 1) * 64;
        return make_int2(*reinterpret_cast<const int*>(p), __float_as_int(u32[((long)b * S + s) * E + c]));
    }
    // the plane scale k folded into the kernel's column scale of att_u, the sigmoid's -log2(e) into that of att_v:
    // val2_scaled() gets av' = -log2(e) * att_v and au' = k * att_u
    __device__ float2 pairmul(float k) const { return make_float2(-1.4426950408889634f, k); }
    __device__ float val2_scaled(int, int, int c, float av, float au, long rw, float, int2 w) const {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        // even lane: own = (hi[c], hi[c+1]), partner = (lo[c], lo[c+1]); odd lane: own = (lo[c-1], lo[c]), partner = (hi[c-1], hi[c]).
        // One byte permute builds (hi[c], lo[c]) as a packed f16 pair.
        const unsigned ov = (unsigned)__builtin_amdgcn_mov_dpp(w.x, 0xB1, 0xF, 0xF, true);
        const unsigned sel = (c & 1) ? 0x03020706u : 0x05040100u;        // v_perm_b32: bytes 0-3 = own word, 4-7 = partner word
        const h2 pv = __builtin_bit_cast(h2, __builtin_amdgcn_perm(ov, (unsigned)w.x, sel));
        const float vs = (float)pv[0] + (float)pv[1];                    // v / k
        const float t0 = au * vs;                                        // att_u * v
        const float t1 = av * __int_as_float(w.y);                       // -log2(e) * att_v * u
        const float o = t0 * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t1));
        return rw < 0 ? 0.f : o;
    }
    __device__ tdx::H3PlOut plout(int) const { return tdx::H3PlOut{oP, 4L * E, os, oss, M}; }
    __device__ long prow(int z, int m) const { return row(z, m); }
};

// stand-alone cal_attention input packing: rotary on the four heads, zero group padding,
// v|u concatenation.
__global__ void pack_heads_kernel(const float* __restrict__ src, const float* __restrict__ freqs, float* __restrict__ dst,
                                  int S, int Sp) {
    const int s = blockIdx.x, b = blockIdx.y, c = threadIdx.x;   // 128 threads
    float v = 0.f;
    if (s < S) {
        const float* row = src + ((long)b * S + s) * 128;
        v = row[c];
        if (c < 32) {
            const float ang = __fmul_rn((float)s, freqs[c >> 1]);
            const float cs = cosf(ang), sn = sinf(ang);
            const float other = row[c ^ 1];
            v = (c & 1) ? v * cs + other * sn : v * cs - other * sn;
        }
    }
    dst[((long)b * Sp + s) * 128 + c] = v;
}
__global__ void concat_vu_kernel(const float* __restrict__ v, const float* __restrict__ u, float* __restrict__ vu, long M, int E) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * 2 * E) return;
    const long m = i / (2 * E);
    const int c = (int)(i % (2 * E));
    vu[i] = c < E ? v[m * E + c] : u[m * E + c - E];
}

// The quadratic + linear attention on the split-f16 x3 core (gemm_h3.hpp), E % 128 == 0 (the model: E = 1024):
//   qkP : the four heads as planes in [4][B][Sp] x 512 B slots (conv17 MODE 3): quad_q, lin_q, quad_k row-major
//         with row scales qks[3][B*Sp]; lin_k K-major with the static scale st[1]
//   vuP : K-major planes [B][Sp][64][2][32] of v|u with the static scale st[0] (pad rows zero); vu: fp32 (gate)
//   h3a : the half-height two-blocks-per-CU kernel (gemm_h3a.hpp) where it fits, else the wide 256-row kernel; swap: with h3a and
//         oP, the lin_q x Kvu segment first.  The model and tdx_cal_attention pass the environment's TDX_H3A / TDX_H3A_SWAP
//         (mf2.hip use_h3a(), h3a_swap()), the test hook tdx_attn_gate_planes (diag.hip) its arguments.
int attention_core_h3(const unsigned char* qkP, const float* qks, const unsigned char* vuP, const float* vu, const float* st,
                      int B, int S, int E, int splits, int kchunk, float* Abuf, unsigned char* AbufP, float* Asc, float* slab, float* kvu,
                      unsigned char* KvuP, float* kvus, float* o, float* att_v, float* att_u, hipStream_t st_, bool h3a, bool swap,
                      unsigned char* oP = nullptr, float* os = nullptr, float* oss = nullptr,
                      hipStream_t side = nullptr, hipEvent_t ev_heads = nullptr, hipEvent_t ev_sim = nullptr, const float* u32 = nullptr) {
    // side != nullptr: the similarity GEMM runs on `side` (which already holds the conv17<3> that wrote the heads; `ev_heads` was
    // recorded behind it), next to lin_k^T[v|u] on st_; st_ waits for the heads before it reads lin_k and for the similarity
    // (`ev_sim`) before the attention launch
    const int G = (S + 255) / 256, Sp = G * 256;
    const long hs = (long)B * Sp;                 // rows per head
    const unsigned char *quad_q = qkP, *lin_q = qkP + hs * 512, *quad_k = qkP + 2 * hs * 512, *lin_k = qkP + 3 * hs * 512;
    const float *sq = qks, *slq = qks + hs, *sk = qks + 2 * hs;
    {   // A = relu(q k^T / 256)^2 per group, then its rows as planes                 mossformer_block.py:256-262
        tdx::H3Args g{};
        g.seg[0] = tdx::h3_seg(quad_q, sq, 512, quad_k, sk, 512, QK);
        g.seg[0].strideA = 256L * 512; g.seg[0].strideB = 256L * 512; g.seg[0].strideSA = 256; g.seg[0].strideSB = 256;
        g.nseg = 1; g.M = 256; g.N = 256;
        EpiQuadSimPl e{AbufP, Asc, G, S, 1.0f / 256.0f};         // (planes straight from the epilogue: no fp32 similarity, no split pass)
        if (tdx::launch_gemm_h3x<false, false, false, false>(g, B * G, e, side ? side : st_) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
        if (side) {
            if (hipEventRecord(ev_sim, side) != hipSuccess || hipStreamWaitEvent(st_, ev_heads, 0) != hipSuccess)
                return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
        }
    }
    {   // Kvu[b][d][ch] = (1/S) sum_t lin_k[t][d] vu[t][ch], split over token chunks         mossformer_block.py:286,289
        // M = 128 (d): the 128 rows of waves 4-7 do not exist and those waves only feed the ring; lin_k is the A operand — once
        // more as ROW-major planes (kmajor_to_rows_kernel; in the fp32 similarity buffer, which is dead after its split): the
        // transposing LDS reads of a K-major A operand bound this launch — v|u the K-major B operand with full 256-column tiles
        unsigned char* lin_kR = reinterpret_cast<unsigned char*>(Abuf);
        hipLaunchKernelGGL(tdx::kmajor_to_rows_kernel, dim3(Sp / 64, B), dim3(256), 0, st_, lin_k, lin_kR, Sp);
        LAUNCH_CHECK();
        tdx::H3Args g{};
        g.seg[0] = tdx::h3_seg(lin_kR, st + 1, 4L * Sp, vuP, st, 4L * 2 * E, kchunk);
        g.seg[0].sa_mul = 0; g.seg[0].sb_mul = 0;
        g.seg[0].zdiv = splits;
        g.seg[0].strideA = (long)Sp * 512; g.seg[0].strideA2 = (long)kchunk * 4;
        g.seg[0].strideB = (long)Sp * 4 * 2 * E; g.seg[0].strideB2 = (long)kchunk * 4 * 2 * E;
        g.seg[0].kchunk = kchunk; g.seg[0].ktotal = Sp;
        g.nseg = 1; g.M = QK; g.N = 2 * E;
        tdx::EpiStoreZ e{slab, 2L * E, (long)QK * 2 * E};
        if (h3a && tdx::h3a_fits<false>(g, false)) {      // 128-row tiles, two blocks per CU: every wave has rows
            if (tdx::launch_gemm_h3a<false>(g, B * splits, e, st_) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
        } else if (tdx::launch_gemm_h3x<false, true, false, false>(g, B * splits, e, st_) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
        const long per = (long)QK * 2 * E;
        const int nb = (int)((per / 4 + 255) / 256);
        float* bmax = kvus + B;          // [B][nb] block maxima
        hipLaunchKernelGGL(tdx::kvu_reduce_t_kernel, dim3(nb, B), dim3(256), 0, st_, slab, kvu, splits, per, (float)S, bmax);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(tdx::kvu_planes_kernel, dim3((unsigned)((128 * (2 * E / 8) + 255) / 256), B), dim3(256), 0, st_, kvu, bmax, nb, KvuP, kvus, 2 * E);
        LAUNCH_CHECK();
    }
    {   // [A | lin_q] x [VU ; Kvu] with the gate epilogue                                mossformer_block.py:269-294, :217
        tdx::H3Args g{};
        g.seg[0] = tdx::h3_seg(AbufP, Asc, 1024, vuP, st, 4L * 2 * E, 256);
        g.seg[0].sb_mul = 0; g.seg[0].zdiv = G;
        g.seg[0].strideA = (long)G * 256 * 1024; g.seg[0].strideA2 = 256L * 1024;
        g.seg[0].strideSA = (long)G * 256; g.seg[0].strideSA2 = 256;
        g.seg[0].strideB = (long)Sp * 4 * 2 * E; g.seg[0].strideB2 = 256L * 4 * 2 * E;
        g.seg[1] = tdx::h3_seg(lin_q, slq, 512, KvuP, kvus, 4L * 2 * E, QK);
        g.seg[1].sb_mul = 0; g.seg[1].zdiv = G;
        g.seg[1].strideA = (long)Sp * 512; g.seg[1].strideA2 = 256L * 512;
        g.seg[1].strideSA = Sp; g.seg[1].strideSA2 = 256;
        g.seg[1].strideB = (long)QK * 4 * 2 * E; g.seg[1].strideB2 = 0;
        g.seg[1].strideSB = 1; g.seg[1].strideSB2 = 0;
        g.nseg = 2; g.M = 256; g.N = E; g.pair_off = E;
        if (side && hipStreamWaitEvent(st_, ev_sim, 0) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
        {   // (diagnostic, timing only, wrong results: TDX_H3_DEBUG & 2 = every group reads the first group's v|u rows — an L2-resident B operand)
            static const int dbg = [] { const char* e = getenv("TDX_H3_DEBUG"); return e ? atoi(e) : 0; }();
            if (dbg & 2) { g.seg[0].strideB = 0; g.seg[0].strideB2 = 0; }
        }
#ifdef TDX_H3_STAMPS
        // diagnostic build: the 4th config-2-sized attention launch records per-block time stamps into $TDX_H3_STAMPS (a file)
        static int stamp_calls = 0;
        static unsigned long long* stamp_buf = nullptr;
        const long stamp_blocks = 8L * ((B * G + 7) / 8) * (h3a ? 16 : 8);
        const bool stamp_now = oP && getenv("TDX_H3_STAMPS") && B * G >= 900 && ++stamp_calls == 4;
        if (stamp_now) {
            hipMalloc((void**)&stamp_buf, stamp_blocks * 64);
            hipMemsetAsync(stamp_buf, 0, stamp_blocks * 64, st_);
            g.stamps = stamp_buf;
        }
        struct StampDump { bool on; long nb; unsigned long long* buf; hipStream_t s;
            ~StampDump() { if (!on) return; hipStreamSynchronize(s); std::vector<unsigned long long> h(nb * 8);
                hipMemcpy(h.data(), buf, nb * 64, hipMemcpyDeviceToHost); FILE* f = fopen(getenv("TDX_H3_STAMPS"), "wb");
                if (f) { fwrite(h.data(), 8, h.size(), f); fclose(f); } } } stamp_dump{stamp_now, stamp_blocks, stamp_buf, st_};
#endif
        if (oP) {             // the model: gate operands from the planes, o written as planes with per-segment scales / sums of squares
            if (h3a) {  // half-height tiles, two blocks per CU (gemm_h3a.hpp): one block's epilogue under the other's MFMAs
                // the L2-resident lin_q x Kvu segment FIRST: the ring fills from cache hits while the first v|u rows (HBM) are on their way
                // (ring fill 5.1 -> 4.9 us, k loop 27.1 -> 26.1 us per half tile; config 2: 203.3 vs 205.2 ms).  Only the accumulation
                // order changes; swap = false (TDX_H3A_SWAP=0) restores the wide kernel's order (then the results are bit-identical to it)
                if (swap) std::swap(g.seg[0], g.seg[1]);
                if (tdx::launch_gemm_h3a<true>(g, B * G, EpiAttnGatePlOut{vuP, st, u32, oP, os, oss, (long)B * S, G, S, Sp, E}, st_) != hipSuccess)
                    return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
                return TDX_OK;
            }
            if (tdx::launch_gemm_h3x<false, true, true, true>(g, B * G, EpiAttnGatePlOut{vuP, st, u32, oP, os, oss, (long)B * S, G, S, Sp, E}, st_) != hipSuccess)
                return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
            return TDX_OK;
        }
        EpiAttnGate e{vu, o, att_v, att_u, G, S, E};
        if (tdx::launch_gemm_h3x<false, true, true, true>(g, B * G, e, st_) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
    }
    return TDX_OK;
}

// ------------------------------------------------------------------ stand-alone attention: workspace plan and operand preparation
inline void attn_plan(int B, int S, int E, int& splits, int& kchunk, size_t& qk4, size_t& vu, size_t& Abuf, size_t& slab, size_t& kvu,
                      size_t& total) {
    const int G = (S + 255) / 256, Sp = G * 256;
    int sp = (1536 + (2 * E / 128) * B - 1) / ((2 * E / 128) * B); if (sp < 1) sp = 1;
    int maxsp = (S + 511) / 512; if (sp > maxsp) sp = maxsp;
    kchunk = ((S + sp - 1) / sp + 31) / 32 * 32;
    splits = (S + kchunk - 1) / kchunk;
    size_t off = 0;
    auto take = [&](size_t nn) { size_t o = off; off += tdx::al(nn); return o; };
    qk4 = take((size_t)4 * B * Sp * QK); vu = take((size_t)B * S * 2 * E); Abuf = take((size_t)B * G * 65536);
    slab = take((size_t)B * splits * QK * 2 * E); kvu = take((size_t)B * QK * 2 * E);
    if (E % 128 == 0) {   // split-f16 x3 path (as the model): planes of the heads, of v|u, of the similarity and of Kvu, and scales
        take((size_t)4 * B * Sp * QK); take((size_t)B * Sp * 2 * E); take((size_t)B * G * 65536); take((size_t)B * QK * 2 * E);
        take((size_t)4 * B * Sp); take((size_t)B + (size_t)B * (QK * 2 * E / 1024) + 64); take(64);
    }
    total = off;
}

// rotary on the four fp32 heads [B][S][128] into ws + qk4 ([4][B][Sp][128], pad rows zero) and v|u into ws + vu ([B*S][2E])
inline int attn_pack_inputs(const float* quad_q, const float* lin_q, const float* quad_k, const float* lin_k, const float* v, const float* u,
                            const float* freqs, int B, int S, int E, float* ws, size_t oq, size_t ovu, hipStream_t st) {
    const int G = (S + 255) / 256, Sp = G * 256;
    const long hs = (long)B * Sp * QK;
    const float* heads[4] = {quad_q, lin_q, quad_k, lin_k};
    for (int i = 0; i < 4; ++i) {
        hipLaunchKernelGGL(pack_heads_kernel, dim3(Sp, B), dim3(128), 0, st, heads[i], freqs, ws + oq + i * hs, S, Sp);
        LAUNCH_CHECK();
    }
    const long M = (long)B * S;
    hipLaunchKernelGGL(concat_vu_kernel, dim3((unsigned)((M * 2 * E + 255) / 256)), dim3(256), 0, st, v, u, ws + ovu, M, E);
    LAUNCH_CHECK();
    return TDX_OK;
}

// The operands of attention_core_h3 from the packed fp32 inputs (E % 128 == 0), in the planes part of an attn_plan workspace
// (behind kvu): planes made by the generic producers, with the exact maxima of lin_k and v|u standing in for the model's static bounds
struct AttnPlanes { unsigned char *qkP, *vuP, *AbufP, *KvuP; float *qks, *kvus, *stt, *Asc; };
inline int attn_prepare_planes(float* ws, size_t oq, size_t ovu, size_t okvu, int B, int S, int E, AttnPlanes& P, hipStream_t st) {
    const int G = (S + 255) / 256, Sp = G * 256;
    const long hs = (long)B * Sp * QK;
    const long M = (long)B * S;
    float* p = ws + okvu + tdx::al((size_t)B * QK * 2 * E);
    P.qkP = (unsigned char*)p; p += tdx::al((size_t)4 * B * Sp * QK);
    P.vuP = (unsigned char*)p; p += tdx::al((size_t)B * Sp * 2 * E);
    P.AbufP = (unsigned char*)p; p += tdx::al((size_t)B * G * 65536);
    P.KvuP = (unsigned char*)p; p += tdx::al((size_t)B * QK * 2 * E);
    P.qks = p; p += tdx::al((size_t)4 * B * Sp);
    P.kvus = p; p += tdx::al((size_t)B + (size_t)B * (QK * 2 * E / 1024) + 64);
    P.stt = p;                            // [0..1] inverse scales of v|u, lin_k ; [2..3] their maxima (bits)
    P.Asc = P.qks + 3L * B * Sp;
    unsigned* mx = reinterpret_cast<unsigned*>(P.stt + 2);
    if (hipMemsetAsync(mx, 0, 2 * sizeof(unsigned), st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
    hipLaunchKernelGGL(tdx::h3_absmax_kernel<0>, dim3(1024), dim3(256), 0, st, ws + ovu, M * 2 * E, mx);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(tdx::h3_absmax_kernel<0>, dim3(1024), dim3(256), 0, st, ws + oq + 3 * hs, hs, mx + 1);
    LAUNCH_CHECK();
    for (int i = 0; i < 3; ++i)
        if (tdx::launch_h3_split_rows(ws + oq + i * hs, QK, P.qkP + (size_t)i * hs * 4, P.qks + (long)i * B * Sp, (long)B * Sp, QK, st) != hipSuccess)
            return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
    {
        const long K = (long)B * Sp;
        long n = K * (QK / 8);
        hipLaunchKernelGGL(tdx::h3_split_kmajor_kernel<0>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ws + oq + 3 * hs, (long)QK,
                           P.qkP + (size_t)3 * hs * 4, K, QK, 1.0f, mx + 1, P.stt + 1, 0, 0);
        LAUNCH_CHECK();
        n = K * (2 * E / 8);
        hipLaunchKernelGGL(tdx::h3_split_kmajor_kernel<0>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ws + ovu, 2L * E, P.vuP, K, 2 * E, 1.0f,
                           mx, P.stt, S, Sp);
        LAUNCH_CHECK();
    }
    return TDX_OK;
}

}  // namespace
