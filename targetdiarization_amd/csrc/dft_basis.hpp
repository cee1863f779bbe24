// dft_basis.hpp — the "window x DFT" matrices a tdx_*_create hands to the fp32 MFMA GEMM as its B operand: the analysis basis of
// every STFT front end (fbank, MDX, Whisper, Apollo, the spectral gate, the phase vocoder) and the synthesis basis of those that
// go back to samples.  Host code only, next to weight_pack.hpp: the tables are computed in double, once per handle, into room of
// the Loader's image (tdx_common.hpp).  What every site needs and none may get wrong lives here: the angle of entry (k, n) is
// reduced exactly, as (k * n) % N in integers, before cos / sin see it; the imaginary part of the DC and Nyquist bins of a
// synthesis basis is 0; every other bin counts twice (Hermitian symmetry); padding rows and columns are never written.
#pragma once
#include <cmath>
#include <vector>

#include "tdx_common.hpp"

namespace tdx {

inline std::vector<double> hann_periodic(int N) {
    std::vector<double> w(N);
    for (int i = 0; i < N; ++i) w[i] = 0.5 - 0.5 * cos(2.0 * M_PI * i / N);
    return w;
}
// w[n] / d: a window as the `gain` of fill_dft_synthesis (a division, as the sites have always written it: w * (1 / d) rounds twice)
inline std::vector<double> divided(std::vector<double> w, double d) {
    for (double& v : w) v /= d;
    return w;
}

struct DftTable {      // cos / sin of 2 pi i / N, i < N
    std::vector<double> cs, sn;
    explicit DftTable(int N) : cs(N), sn(N) {
        for (int i = 0; i < N; ++i) { cs[i] = cos(2.0 * M_PI * i / N); sn[i] = sin(2.0 * M_PI * i / N); }
    }
};

// analysis: frames [.][N] x dst^T gives re X_k in column k and im X_k in column im_row0 + k, k < nbin.
//   dst[k][n] = win[n] cos(2 pi k n / N),  dst[im_row0 + k][n] = -win[n] sin(2 pi k n / N);  rows of pitch ld, win null: no window.
// `dst` is zeroed room; nothing else is written, so the rows nbin .. and the columns N .. ld stay zero.
inline void fill_dft_analysis(float* dst, int N, int nbin, size_t im_row0, size_t ld, const double* win) {
    const DftTable t(N);
    for (int k = 0; k < nbin; ++k)
        for (int n = 0; n < N; ++n) {
            const int idx = (int)(((long)k * n) % N);
            const double w = win ? win[n] : 1.0;
            dst[(size_t)k * ld + n] = (float)(w * t.cs[idx]);
            dst[(im_row0 + k) * ld + n] = (float)(-w * t.sn[idx]);
        }
}

// synthesis (c2r of the bins k < nbin, the others taken as zero): spectrum rows [re 0 .. | im at im_off ..] x dst^T gives frames [.][N].
//   dst[n][k] = gain[n] w_k cos(2 pi k n / N),  dst[n][im_off + k] = -gain[n] w_k sin(2 pi k n / N),  w = 1 at DC and Nyquist, else 2;
// the imaginary parts of DC and Nyquist are ignored (`edge_im`, a zero).  gain[n] is whatever the caller folds in: 1 / N, a synthesis
// window.  The order (gain[n] * w_k) * trig is part of the result's last bit.  edge_im is +0 unless a site's image has always held
// -0 there (Apollo): no sum can tell the two apart, but the uploaded bytes stay what they were.
inline void fill_dft_synthesis(float* dst, int N, int nbin, size_t im_off, size_t ld, const double* gain, float edge_im = 0.f) {
    const DftTable t(N);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < nbin; ++k) {
            const int idx = (int)(((long)k * n) % N);
            const bool edge = k == 0 || 2 * k == N;
            const double coef = gain[n] * (edge ? 1.0 : 2.0);
            dst[(size_t)n * ld + k] = (float)(coef * t.cs[idx]);
            dst[(size_t)n * ld + im_off + k] = edge ? edge_im : (float)(-coef * t.sn[idx]);
        }
}

// The STFT round trip of the spectral gate and the phase vocoder: the analysis GEMM is PAIRED over NPAIR columns (64-column tiles)
// and stores spectrum rows [re 0 .. BP | im 0 .. BP]; the same row is the K = KS operand of the synthesis GEMM (a multiple of 32).
struct StftGeo { int n_fft, nbin, BP, NPAIR, KS; };
constexpr StftGeo stft_geo(int n_fft) { return StftGeo{n_fft, n_fft / 2 + 1, n_fft / 2 + 16, n_fft / 2 + 64, 2 * (n_fft / 2 + 16)}; }

// analysis [2 * NPAIR][n_fft] at Wa (window `win`), synthesis [n_fft][KS] at Ws (gain `syn_gain`)
inline void push_stft_basis(Loader& ld, const StftGeo& g, const double* win, const double* syn_gain, const float*& Wa, const float*& Ws) {
    const size_t oA = ld.room(Wa, (size_t)2 * g.NPAIR * g.n_fft);
    const size_t oS = ld.room(Ws, (size_t)g.n_fft * g.KS);
    fill_dft_analysis(ld.host.data() + oA, g.n_fft, g.nbin, g.NPAIR, g.n_fft, win);
    fill_dft_synthesis(ld.host.data() + oS, g.n_fft, g.nbin, g.BP, g.KS, syn_gain);
}

}  // namespace tdx
