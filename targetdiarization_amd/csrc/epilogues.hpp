// epilogues.hpp — the GEMM epilogues that more than one model needs, and the nn.Linear launchers of the three cores.
//
// Epilogue concept: gemm.hpp.  One family instead of a copy per model:
//   EpiBiasAct<Act>    out[m][n] = act(v + b[n])                          every column of the (padded) width is stored
//   EpiBiasActN<Act>   the same, columns n < nreal only
//   EpiBiasRes<Act>    out[m][n] = act((v + b[n]) + res[m][n])           res may alias out (x += ...)
//   EpiBiasResN<Act>   the same, columns n < nreal only (the residual is not read beyond them either)
//   EpiBiasRes2<Act>   out[m][n] = act((v + b[n]) + (res[m][n] + res2[m][n])), res2 may be null
//   EpiStoreZ          out[z][m][n] = v
//   EpiSpecMag         PAIRED: spec[m][c] = re, spec[m][im_off + c] = im, mag[m][c] = sqrt(re^2 + im^2), columns c < nreal
// A null b is a zero bias in all of them.  The order of the additions is fixed — bias first, then the residual (itself summed
// first where there are two), then the activation — so that the results do not depend on which struct a call site picks.
// The column guard is a struct of its own rather than nreal = INT_MAX in the unguarded one: the compare would sit in every
// store of the hot x6 / x3 kernels, whose outputs are never padded.  Rows are addressed as (long)m * (int)ld + n: every
// pitch of the project fits an int, and the 32-bit multiply is what the hot kernels were tuned with.
//
// Not here, on purpose: epilogues with model-specific indexing or arithmetic stay next to their model (mf2.hip EpiHidden*,
// EpiQuadSim*, EpiAttnGate*, EpiBiasPrelu, EpiBiasHalves, EpiPosEnc, EpiTanhSig, EpiMaskMul and the *Pl* plane writers;
// paraformer.hip EpiScores*, EpiCtx, EpiCifConv; mdx.hip EpiTdf1/2, EpiUp; campplus.hip EpiHeadOut; eres2net.hip EpiChain,
// EpiAffGate; apollo.hip EpiRow, EpiGate, EpiRowBiasSilu; pyannet.hip EpiConv; frontend.hip EpiPower, EpiLogMel, EpiSpec,
// EpiWinFrame), and so do the one-wave LayerNorms and softmaxes: they look alike but sum in different orders, and merging
// them moves the last bit of everything downstream.
//
// The host side of a GEMM's B operand lives elsewhere: weight_pack.hpp repacks the conv, BatchNorm, Linear and LSTM weights a create
// fetched, dft_basis.hpp builds the window x DFT bases of the spectral front ends.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tdx.h"
#include "devutil.hpp"
#include "gemm.hpp"
#include "gemm_x6.hpp"
#include "gemm_h3.hpp"
#include "tdx_common.hpp"

namespace tdx {

// ---- activations (applied last)
struct ActNone { __device__ static float f(float v) { return v; } };
struct ActRelu { __device__ static float f(float v) { return fmaxf(v, 0.f); } };
struct ActRelu20 { __device__ static float f(float v) { return relu20(v); } };
struct ActSilu { __device__ static float f(float v) { return siluf_acc(v); } };
struct ActGelu { __device__ static float f(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); } };      // exact (erf) GELU, nn.GELU()
template <int NUM = 1, int DEN = 100>      // slope NUM / DEN as a compile-time constant (a float cannot be a template argument)
struct ActLeaky { __device__ static float f(float v) { return leaky(v, (float)NUM / (float)DEN); } };

// ---- bias + activation.  ptr / ldm / put: the single row-major output form the x6 and x3 cores use (gemm_h3.hpp epi_has_ptr)
template <class Act = ActNone>
struct EpiBiasAct {
    const float* b; float* out; long ld;
    __device__ float col(int, int n) const { return b ? b[n] : 0.f; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int, int m, int n, float v, EpiNone, float c) const { out[(long)m * (int)ld + n] = Act::f(v + c); }
    __device__ float* ptr(int, int m, int n) const { return out + (long)m * (int)ld + n; }
    __device__ long ldm() const { return ld; }
    __device__ void put(float* p, float v, EpiNone, float c) const { *p = Act::f(v + c); }
};
template <class Act = ActNone>
struct EpiBiasActN {
    const float* b; float* out; long ld; int nreal;
    __device__ float col(int, int n) const { return b ? b[n] : 0.f; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int, int m, int n, float v, EpiNone, float c) const { if (n < nreal) out[(long)m * (int)ld + n] = Act::f(v + c); }
};

// ---- bias + residual + activation; the residual is an aux() value: loaded ahead of the stores (gemm.hpp)
template <class Act = ActNone>
struct EpiBiasRes {
    const float* b; const float* res; float* out; long ld;
    __device__ float col(int, int n) const { return b ? b[n] : 0.f; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ float aux(int, int m, int n, EpiNone) const { return res[(long)m * (int)ld + n]; }
    __device__ void store(int, int m, int n, float v, EpiNone, float c, float r) const { out[(long)m * (int)ld + n] = Act::f((v + c) + r); }
};
template <class Act = ActNone>
struct EpiBiasResN {
    const float* b; const float* res; float* out; long ld; int nreal;
    __device__ float col(int, int n) const { return b ? b[n] : 0.f; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ float aux(int, int m, int n, EpiNone) const { return n < nreal ? res[(long)m * (int)ld + n] : 0.f; }
    __device__ void store(int, int m, int n, float v, EpiNone, float c, float r) const { if (n < nreal) out[(long)m * (int)ld + n] = Act::f((v + c) + r); }
};
template <class Act = ActNone>
struct EpiBiasRes2 {
    const float* b; const float* res; const float* res2; float* out; long ld;
    __device__ float col(int, int n) const { return b ? b[n] : 0.f; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ float aux(int, int m, int n, EpiNone) const { const long i = (long)m * (int)ld + n; return res2 ? res[i] + res2[i] : res[i]; }
    __device__ void store(int, int m, int n, float v, EpiNone, float c, float r) const { out[(long)m * (int)ld + n] = Act::f((v + c) + r); }
};

// ---- plain store with a per-batch stride (split-K / split-tap slabs, batched GEMMs)
struct EpiStoreZ {
    float* out; long ld; long strideZ;
    __device__ EpiNone col(int, int) const { return EpiNone{}; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int z, int m, int n, float v, EpiNone, EpiNone) const { out[(long)z * strideZ + (long)m * (int)ld + n] = v; }
};

// ---- PAIRED (re, im) columns of a DFT: the spectrum as two half rows [re 0..nreal | im 0..nreal] and its magnitude
struct EpiSpecMag {
    float* spec; float* mag; long lds; long ldm; int im_off; int nreal;
    __device__ EpiNone col(int, int) const { return EpiNone{}; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store2(int, int m, int c, float re, float im, EpiNone, EpiNone) const {
        if (c < nreal) {
            float* s = spec + (long)m * (int)lds + c;
            s[0] = re; s[im_off] = im;
            // an explicit fma: left to -ffp-contract the guarded and the unguarded epilogue of the core fused re^2 + im^2
            // differently, and a row's last bit then depended on whether its tile was the last one
            mag[(long)m * (int)ldm + c] = sqrtf(fmaf(re, re, im * im));
        }
    }
};

// ---- nn.Linear / 1x1 convolution: out = epi(A [M][K] (row pitch lda) x W[N][K]^T), one launch, a TDX status back
// exact-fp32 MFMA core (gemm.hpp).  n_valid: columns from there on are never stored, so their MFMA tiles are skipped
// (0 = all N).  PAIRED: the epilogue gets columns c and pair_off + c together (store2).
template <bool PAIRED = false, class Epi>
inline int linear_f32(const float* A, long lda, const float* W, int M, int N, int K, Epi epi, hipStream_t st, int n_valid = 0, int pair_off = 0) {
    GemmArgs g = make_args(M, N, make_seg(A, lda, W, K, K));
    if (n_valid) g.n_valid = n_valid;
    g.pair_off = pair_off;
    const hipError_t e = launch_gemm<false, false, PAIRED, false>(g, 1, epi, st);
    return e == hipSuccess ? TDX_OK : fail_hip(e, __FILE__, __LINE__);
}
// split-bf16 x6 core (gemm_x6.hpp); W must be readable up to the next multiple of 256 rows
template <class Epi>
inline int linear_x6(const float* A, long lda, const float* W, int M, int N, int K, Epi epi, hipStream_t st) {
    GemmArgs g = make_args(M, N, make_seg(A, lda, W, K, K));
    const hipError_t e = launch_gemm_x6<false>(g, epi, st);
    return e == hipSuccess ? TDX_OK : fail_hip(e, __FILE__, __LINE__);
}
// split-f16 x3 core (gemm_h3.hpp): A already as planes (row pitch 4 * K bytes) + row scales, W as made by split_weight_planes
struct H3W { const unsigned char* p; const float* s; };      // one nn.Linear weight as planes [N][K] x 4 bytes + row scales
template <class Epi>
inline int linear_h3(const unsigned char* Ap, const float* As, int M, const H3W& W, int N, int K, Epi epi, hipStream_t st) {
    H3Args g{};
    g.seg[0] = h3_seg(Ap, As, 4L * K, W.p, W.s, 4L * K, K);
    g.nseg = 1; g.M = M; g.N = N;
    const hipError_t e = launch_gemm_h3<false>(g, 1, epi, st);
    return e == hipSuccess ? TDX_OK : fail_hip(e, __FILE__, __LINE__);
}

}  // namespace tdx
