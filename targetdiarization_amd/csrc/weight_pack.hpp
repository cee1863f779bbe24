// weight_pack.hpp — what a tdx_*_create does with the tensors it fetched: the host-side repacking of convolution, BatchNorm,
// Linear and LSTM weights into the Loader's image (tdx_common.hpp).  Host code only.  The helpers take pointers, not tensor
// names: the caller does its own ld.get(...) calls (by size or by shape, in its own order, with its own error text) and may
// hand over nullptr for a tensor the Loader reported missing; the room is then reserved and left zero, and finish() fails.
// (GEMM operands that come from no checkpoint — the window x DFT bases of the STFT front ends — are built by dft_basis.hpp.)
#pragma once
#include <cmath>
#include <vector>

#include "tdx_common.hpp"

namespace tdx {

// a packed GEMM B matrix [Npad][Kp] at `w` and its bias [Npad] at `b` (offsets into the image); N real rows.  A convolution's row
// is `taps` groups of `cinp` channels.
struct GemmW { size_t w = 0, b = 0; int N = 0, Npad = 0, Kp = 0, taps = 1, cinp = 0; };
// a handle that keeps pointers binds the pair (Loader::bind) after push_linear / push_conv_gemm
inline void bind(Loader& ld, const float*& W, const float*& b, const GemmW& g) { ld.bind(W, g.w); ld.bind(b, g.b); }

// eval BatchNorm -> y = x * s + sh, in fp64 (g / be null: no affine part; mu / var null: identity)
struct BN { std::vector<double> s, sh; };
inline BN bn_fold(const float* g, const float* be, const float* mu, const float* var, int N) {
    BN r; r.s.assign(N, 1.0); r.sh.assign(N, 0.0);
    if (!mu || !var) return r;
    for (int n = 0; n < N; ++n) {
        r.s[n] = (g ? (double)g[n] : 1.0) / std::sqrt((double)var[n] + 1e-5);
        r.sh[n] = (be ? (double)be[n] : 0.0) - (double)mu[n] * r.s[n];
    }
    return r;
}

// conv weight W [N][cin][taps] (times scale[n], in fp64) -> GEMM B [Npad][Kp], column (t - k0) * cinp + c for the taps
// k0 .. k0 + nk - 1 (all of them by default; Kp = nk * cinp by default), then bias [Npad].  scale / bias null: 1 / 0.
template <class TB>
GemmW push_conv_gemm(Loader& ld, const float* W, const double* scale, const TB* bias, int N, int cin, int taps, int Npad, int cinp,
                     int Kp = 0, int k0 = 0, int nk = 0) {
    GemmW g; g.N = N; g.Npad = Npad; g.taps = nk ? nk : taps; g.cinp = cinp; g.Kp = Kp ? Kp : g.taps * cinp;
    g.w = ld.room((size_t)Npad * g.Kp);
    g.b = ld.room(Npad);
    for (int n = 0; n < N; ++n) {
        if (bias) ld.host[g.b + n] = (float)bias[n];
        if (W) for (int c = 0; c < cin; ++c)
            for (int t = 0; t < g.taps; ++t)
                ld.host[g.w + (size_t)n * g.Kp + t * cinp + c] = (float)((double)W[((size_t)n * cin + c) * taps + k0 + t] * (scale ? scale[n] : 1.0));
    }
    return g;
}

// the one-channel 3x3 stem W [C][1][3][3] + BatchNorm -> w9 [9][C] at `w`, bias [C] at `b`
inline void push_stem9(Loader& ld, const float* W, const BN& bn, int C, size_t& w, size_t& b) {
    w = ld.room(9 * C);
    b = ld.room(C);
    if (W) for (int n = 0; n < C; ++n) {
        ld.host[b + n] = (float)bn.sh[n];
        for (int t = 0; t < 9; ++t) ld.host[w + t * C + n] = (float)((double)W[n * 9 + t] * bn.s[n]);
    }
}

// W [N][K] (+ b [N], or null) -> zero-padded [Npad][Kp] + bias [Npad]; fp32 or fp64 sources
template <class TW, class TB>
GemmW push_linear(Loader& ld, const TW* W, const TB* b, int N, int K, int Npad, int Kp) {
    GemmW g; g.N = N; g.Npad = Npad; g.Kp = Kp;
    g.w = ld.room((size_t)Npad * Kp);
    g.b = ld.room(Npad);
    for (int n = 0; n < N; ++n) {
        if (W) for (int k = 0; k < K; ++k) ld.host[g.w + (size_t)n * Kp + k] = (float)W[(size_t)n * K + k];
        if (b) ld.host[g.b + n] = (float)b[n];
    }
    return g;
}

// one LSTM direction (PyTorch rows gate * H + u, gates i, f, g, o) into rows row0 + u * 4 + gate of matrices reserved by the
// caller: W_ih [.][in] -> proj.w (pitch proj.Kp), b_ih + b_hh -> proj.b, and W_hh [.][H] -> `whh` in the same row order, or,
// with `transposed`, as [row0 / 4 + k][u * 4 + gate]
inline void push_lstm_gates(Loader& ld, const float* wih, const float* whh_src, const float* bih, const float* bhh, int H, int in,
                            const GemmW& proj, size_t whh, int row0, bool transposed = false) {
    if (!wih || !whh_src || !bih || !bhh) return;
    float* hh = ld.host.data() + whh + (size_t)row0 * H;
    for (int g = 0; g < 4; ++g)
        for (int u = 0; u < H; ++u) {
            const size_t src = (size_t)g * H + u, r = (size_t)u * 4 + g;
            memcpy(ld.host.data() + proj.w + (row0 + r) * proj.Kp, wih + src * in, in * sizeof(float));
            ld.host[proj.b + row0 + r] = bih[src] + bhh[src];
            if (!transposed) memcpy(hh + r * H, whh_src + src * H, H * sizeof(float));
            else for (int k = 0; k < H; ++k) hh[(size_t)k * 4 * H + r] = whh_src[src * H + k];
        }
}

}  // namespace tdx
