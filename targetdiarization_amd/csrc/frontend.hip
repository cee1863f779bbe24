// frontend.hip — spectral front-ends of the path on MI355X:
//   * Kaldi-compatible 80-bin log-mel fbank (25 ms / 10 ms, 512-point) for the speaker
//     embedding (povey window, per-utterance mean removal) and the ASR front-end
//     (hamming, x32768, LFR 7/6 + CMVN)            [third-party torchaudio/funasr algorithm]
//   * the MDX block STFT / iSTFT pair: torch.stft(n_fft=6144, hop, hann periodic, center)
//     with the reference's (L-re, L-im, R-re, R-im) x dim_f x dim_t packing
//                                                   AudioProcessor.py:82-120
// Both transforms are evaluated as DFT-matrix GEMMs on the fp32 MFMA core (gemm.hpp):
// n_fft = 6144 = 3*2^11 would need a mixed-radix FFT, the whole STFT stage is ~2 % of the
// path's FLOPs even in matrix form, and the matrix form reuses the one tuned kernel and has
// FFT-grade error (each output is a single fp32 FMA chain over exactly-rounded twiddles).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/tdx.h"
#include "gemm.hpp"
#include "devutil.hpp"
#include "dft_basis.hpp"

using namespace tdx;

namespace {

constexpr int NF = 512, NBIN_PAD = 320, NMEL = 80, FLEN = 400, FSHIFT = 160;
constexpr float LOG_EPS = 1.1920928955078125e-07f;



// one block (256 threads) per frame: scale, DC removal, pre-emphasis 0.97 (replicate-left),
// window, zero-pad 400 -> 512     [kaldi.fbank _get_window]
__global__ __launch_bounds__(256) void fbank_frame_kernel(const float* __restrict__ wav, const float* __restrict__ win,
                                                           float* __restrict__ frames, int N, int F, float scale) {
    __shared__ float x[FLEN];
    __shared__ float red[4];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* src = wav + (long)b * N + (long)f * FSHIFT;
    float s = 0.f;
    for (int i = tid; i < FLEN; i += 256) { const float v = src[i] * scale; x[i] = v; s += v; }
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    const float mean = ((red[0] + red[1]) + (red[2] + red[3])) * (1.0f / FLEN);
    float* dst = frames + ((long)b * F + f) * NF;
    for (int i = tid; i < NF; i += 256) {
        float v = 0.f;
        if (i < FLEN) {
            const float cur = x[i] - mean, prev = x[i > 0 ? i - 1 : 0] - mean;
            v = (cur - 0.97f * prev) * win[i];
        }
        dst[i] = v;
    }
}

struct EpiPower {   // |X_k|^2 from the (cos, -sin) column pair
    float* P;
    __device__ EpiNone col(int, int) const { return EpiNone{}; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store2(int, int m, int c, float re, float im, EpiNone, EpiNone) const { P[(long)m * NBIN_PAD + c] = re * re + im * im; }
};
struct EpiLogMel {  // log(max(mel energy, eps)), 80 of the 128 padded columns kept
    float* out;
    __device__ EpiNone col(int, int) const { return EpiNone{}; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int, int m, int n, float v, EpiNone, EpiNone) const {
        if (n < NMEL) out[(long)m * NMEL + n] = logf(fmaxf(v, LOG_EPS));
    }
};

// SV / WeSpeaker: feat -= mean over frames (per utterance, per bin).  one block per utterance.
__global__ __launch_bounds__(320) void fbank_submean_kernel(float* __restrict__ feat, int F) {
    __shared__ double part[4][NMEL];
    const int b = blockIdx.x, d = threadIdx.x % NMEL, g = threadIdx.x / NMEL;
    float* p = feat + (long)b * F * NMEL;
    double s = 0.0;
    for (int f = g; f < F; f += 4) s += (double)p[(long)f * NMEL + d];
    part[g][d] = s;
    __syncthreads();
    const float mean = (float)((part[0][d] + part[1][d] + part[2][d] + part[3][d]) / (double)F);
    for (int f = g; f < F; f += 4) p[(long)f * NMEL + d] -= mean;
}

// ASR: LFR (stack 7, stride 6, 3 left copies of frame 0, repeat last frame) + CMVN
__global__ void lfr_cmvn_kernel(const float* __restrict__ feat, const float* __restrict__ shift, const float* __restrict__ scl,
                                float* __restrict__ out, int F, int Fl) {
    const int i = blockIdx.x, b = blockIdx.y;
    for (int c = threadIdx.x; c < 7 * NMEL; c += blockDim.x) {
        const int j = c / NMEL, d = c - j * NMEL;
        int src = i * 6 + j - 3;
        src = src < 0 ? 0 : (src > F - 1 ? F - 1 : src);
        out[((long)b * Fl + i) * 560 + c] = (feat[((long)b * F + src) * NMEL + d] + shift[c]) * scl[c];
    }
}

// ---------------------------------------------------------------- STFT / iSTFT (MDX geometry)
__global__ __launch_bounds__(256) void stft_frame_kernel(const float* __restrict__ x, const float* __restrict__ win,
                                                          float* __restrict__ frames, int chunk, int nfft, int hop, int T) {
    const int t = blockIdx.x, r = blockIdx.y;
    const float* src = x + (long)r * chunk;
    float* dst = frames + ((long)r * T + t) * nfft;
    for (int n = threadIdx.x; n < nfft; n += 256) {
        int p = t * hop + n - nfft / 2;                 // torch.stft(center=True): reflect padding
        if (p < 0) p = -p;
        if (p >= chunk) p = 2 * (chunk - 1) - p;
        dst[n] = src[p] * win[n];
    }
}
struct EpiSpec {   // C[m=(ri,f)][n=(r,t)] -> spec[r][ri][f][t]      AudioProcessor.py:93-98
    float* spec; int dimf; int T;
    __device__ EpiNone col(int, int) const { return EpiNone{}; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int, int m, int n, float v, EpiNone, EpiNone) const {
        const int ri = m / dimf, f = m - ri * dimf, r = n / T, t = n - r * T;
        spec[(((long)r * 2 + ri) * dimf + f) * T + t] = v;
    }
};
struct EpiWinFrame {  // irfft frame * window
    const float* win; float* out; int nfft; long strideZ;
    __device__ float col(int, int n) const { return win[n]; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int z, int m, int n, float v, EpiNone, float w) const { out[(long)z * strideZ + (long)m * nfft + n] = v * w; }
};
// overlap-add / window envelope, centre trim   (torch.istft, center=True)
__global__ __launch_bounds__(256) void istft_ola_kernel(const float* __restrict__ frames, const float* __restrict__ env,
                                                         float* __restrict__ y, int chunk, int nfft, int hop, int T) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y;
    if (i >= chunk) return;
    const int p = (int)i + nfft / 2;
    int t1 = p / hop; if (t1 > T - 1) t1 = T - 1;
    const int t0 = p >= nfft ? (p - nfft) / hop : 0;      // conservative lower bound; exact test below
    float acc = 0.f;
    for (int t = t0; t <= t1; ++t) {
        const int n = p - t * hop;
        if (n >= 0 && n < nfft) acc += frames[((long)r * T + t) * nfft + n];
    }
    y[(long)r * chunk + i] = acc / env[p];
}

}  // namespace

struct tdx_fbank {
    int device = 0;
    int mode = 0; float scale = 1.0f;
    tdx::DevBuf dev; const float *Wdft = nullptr, *mel = nullptr, *win = nullptr;
};
struct tdx_stft {
    int device = 0;
    int nfft = 0, hop = 0, dimf = 0, T = 0, chunk = 0;
    tdx::DevBuf dev; const float *Wf = nullptr, *Wi = nullptr, *win = nullptr, *env = nullptr;
};

extern "C" {

int tdx_fbank_create(int mode, int device, tdx_fbank** out) {
    if (!out || mode < 0 || mode > 2) return tdx::fail(TDX_E_INVALID, "tdx_fbank_create: mode must be 0 (SV), 1 (ASR) or 2 (WeSpeaker)");
    tdx::Loader ld;       // (no blob: the tables are computed here, then staged and uploaded like weights)
    std::vector<float>& host = ld.host;
    std::unique_ptr<tdx_fbank> h(new tdx_fbank());
    h->device = device; h->mode = mode; h->scale = mode != 0 ? 32768.0f : 1.0f;
    const size_t oW = ld.room(h->Wdft, (size_t)2 * NBIN_PAD * NF);      // DFT [2 * 320][512]: re rows k, im rows 320 + k, no window
    tdx::fill_dft_analysis(host.data() + oW, NF, NF / 2 + 1, NBIN_PAD, NF, nullptr);
    // mel banks [128][320] (torchaudio get_mel_banks; last FFT bin column is zero)
    const size_t oM = ld.room(h->mel, (size_t)128 * NBIN_PAD);
    {
        auto mel = [](double f) { return 1127.0 * log(1.0 + f / 700.0); };
        const double mlow = mel(20.0), mhigh = mel(8000.0), delta = (mhigh - mlow) / (NMEL + 1);
        for (int b = 0; b < NMEL; ++b) {
            const double left = mlow + b * delta, center = left + delta, right = center + delta;
            for (int k = 0; k < NF / 2; ++k) {
                const double m = mel(31.25 * k);
                const double up = (m - left) / (center - left), down = (right - m) / (right - center);
                const double v = fmax(0.0, fmin(up, down));
                host[oM + (size_t)b * NBIN_PAD + k] = (float)v;
            }
        }
    }
    const size_t oWin = ld.room(h->win, FLEN);
    for (int i = 0; i < FLEN; ++i) {
        if (mode == 0) host[oWin + i] = (float)pow(0.5 - 0.5 * cos(2.0 * M_PI * i / (FLEN - 1)), 0.85);   // povey
        else host[oWin + i] = (float)(0.54 - 0.46 * cos(2.0 * M_PI * i / (FLEN - 1)));                     // hamming
    }
    TRY(ld.finish("tdx_fbank_create", false, device, h->dev));
    *out = h.release();
    return TDX_OK;
}

int tdx_fbank_destroy(tdx_fbank* h) {
    delete h;
    return TDX_OK;
}

int tdx_fbank_frames(int N) { return N < FLEN ? 0 : 1 + (N - FLEN) / FSHIFT; }

size_t tdx_fbank_workspace_bytes(int B, int N) {
    const int F = tdx_fbank_frames(N);
    if (B < 1 || F < 1) return 0;
    return (al((size_t)B * F * NF) + al((size_t)B * F * NBIN_PAD)) * sizeof(float);
}

int tdx_fbank_forward(tdx_fbank* h, const float* wav, int B, int N, float* feat, void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !wav || !feat || !ws_) return tdx::fail(TDX_E_INVALID, "tdx_fbank_forward: null argument");
    const int F = tdx_fbank_frames(N);
    if (B < 1 || F < 1) return tdx::fail(TDX_E_INVALID, "tdx_fbank_forward: need N >= 400 samples");
    if (ws_bytes < tdx_fbank_workspace_bytes(B, N)) return tdx::fail(TDX_E_WORKSPACE, "tdx_fbank_forward: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    float* frames = (float*)ws_;
    float* P = frames + al((size_t)B * F * NF);
    const int M = B * F;
    hipLaunchKernelGGL(fbank_frame_kernel, dim3(F, B), dim3(256), 0, st, wav, h->win, frames, N, F, h->scale);
    LAUNCH_CHECK();
    {
        GemmArgs g = make_args(M, NBIN_PAD, make_seg(frames, NF, h->Wdft, NF, NF));
        g.pair_off = NBIN_PAD;
        if (launch_gemm<false, false, true, false>(g, 1, EpiPower{P}, st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
    }
    {
        GemmArgs g = make_args(M, 128, make_seg(P, NBIN_PAD, h->mel, NBIN_PAD, NBIN_PAD));
        if (launch_gemm<false, false, false, false>(g, 1, EpiLogMel{feat}, st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
    }
    if (h->mode != 1) {
        hipLaunchKernelGGL(fbank_submean_kernel, dim3(B), dim3(320), 0, st, feat, F);
        LAUNCH_CHECK();
    }
    return TDX_OK;
}

int tdx_lfr_cmvn(const float* feat, int B, int F, const float* shift, const float* scale, float* out, void* stream) {
    if (!feat || !shift || !scale || !out || B < 1 || F < 1) return tdx::fail(TDX_E_INVALID, "tdx_lfr_cmvn: bad argument");
    const int Fl = (F + 5) / 6;
    hipLaunchKernelGGL(lfr_cmvn_kernel, dim3(Fl, B), dim3(256), 0, (hipStream_t)stream, feat, shift, scale, out, F, Fl);
    LAUNCH_CHECK();
    return TDX_OK;
}

// ------------------------------------------------------------------------------ STFT
int tdx_stft_create(int n_fft, int hop, int dim_f, int dim_t, int device, tdx_stft** out) {
    if (!out || n_fft < 256 || n_fft % 128 || hop < 1 || dim_f < 128 || dim_f % 64 || dim_f > n_fft / 2 + 1 || dim_t < 128 ||
        dim_t % 128 || (long)hop * (dim_t - 1) <= n_fft / 2)
        return tdx::fail(TDX_E_INVALID, "tdx_stft_create: unsupported geometry (need n_fft%128==0, dim_f%64==0, dim_t%128==0)");
    const int N = n_fft, T = dim_t, chunk = hop * (dim_t - 1);
    tdx::Loader ld;       // (no blob: the tables are computed here, then staged and uploaded like weights)
    std::vector<float>& host = ld.host;
    std::unique_ptr<tdx_stft> h(new tdx_stft());
    h->device = device;
    h->nfft = N; h->hop = hop; h->dimf = dim_f; h->T = T; h->chunk = chunk;
    // forward: rows m = ri*dim_f + f over k=n (time):  re: cos, im: -sin
    const size_t oWf = ld.room(h->Wf, (size_t)2 * dim_f * N);
    tdx::fill_dft_analysis(host.data() + oWf, N, dim_f, dim_f, N, nullptr);
    // inverse (c2r, bins >= dim_f are zero): rows n (time) over k = ri*dim_f + f
    //   y[n] = 1/N [X0.re + 2 sum_{f>=1} (X_f.re cos - X_f.im sin)] (+ Nyquist term if dim_f covers it)
    const size_t oWi = ld.room(h->Wi, (size_t)N * 2 * dim_f);
    tdx::fill_dft_synthesis(host.data() + oWi, N, dim_f, dim_f, (size_t)2 * dim_f, std::vector<double>(N, 1.0 / N).data());
    const size_t oWin = ld.room(h->win, N);
    const std::vector<double> w = tdx::hann_periodic(N);
    for (int i = 0; i < N; ++i) host[oWin + i] = (float)w[i];
    const int L = N + hop * (T - 1);
    const size_t oEnv = ld.room(h->env, L);
    for (int t = 0; t < T; ++t)
        for (int n = 0; n < N; ++n) host[oEnv + (size_t)t * hop + n] += (float)((double)host[oWin + n] * (double)host[oWin + n]);
    TRY(ld.finish("tdx_stft_create", false, device, h->dev));
    *out = h.release();
    return TDX_OK;
}

int tdx_stft_destroy(tdx_stft* h) {
    delete h;
    return TDX_OK;
}

int tdx_stft_chunk_size(const tdx_stft* h) { return h ? h->chunk : 0; }

size_t tdx_stft_workspace_bytes(const tdx_stft* h, int R) {
    if (!h || R < 1) return 0;
    return al((size_t)R * h->T * h->nfft) * sizeof(float);
}

// x_dev [R, chunk] -> spec_dev [R, 2, dim_f, dim_t]  (R = n_blocks*2 channels; viewed by the
// caller as [n_blocks, 4, dim_f, dim_t] = (L-re, L-im, R-re, R-im))
int tdx_stft_forward(tdx_stft* h, const float* x, int R, float* spec, void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !x || !spec || !ws_ || R < 1) return tdx::fail(TDX_E_INVALID, "tdx_stft_forward: bad argument");
    if (ws_bytes < tdx_stft_workspace_bytes(h, R)) return tdx::fail(TDX_E_WORKSPACE, "tdx_stft_forward: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    float* frames = (float*)ws_;
    hipLaunchKernelGGL(stft_frame_kernel, dim3(h->T, R), dim3(256), 0, st, x, h->win, frames, h->chunk, h->nfft, h->hop, h->T);
    LAUNCH_CHECK();
    GemmArgs g = make_args(2 * h->dimf, R * h->T, make_seg(h->Wf, h->nfft, frames, h->nfft, h->nfft));
    if (launch_gemm<false, false, false, false>(g, 1, EpiSpec{spec, h->dimf, h->T}, st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
    return TDX_OK;
}

// spec_dev [R, 2, dim_f, dim_t] -> y_dev [R, chunk]   (bins >= dim_f taken as zero: freq_pad)
int tdx_stft_inverse(tdx_stft* h, const float* spec, int R, float* y, void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !spec || !y || !ws_ || R < 1) return tdx::fail(TDX_E_INVALID, "tdx_stft_inverse: bad argument");
    if (ws_bytes < tdx_stft_workspace_bytes(h, R)) return tdx::fail(TDX_E_WORKSPACE, "tdx_stft_inverse: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    float* frames = (float*)ws_;
    const int K = 2 * h->dimf;
    GemmArgs g = make_args(h->T, h->nfft, make_seg(spec, h->T, h->Wi, K, K, (long)K * h->T, 0));
    if (launch_gemm<true, false, false, false>(g, R, EpiWinFrame{h->win, frames, h->nfft, (long)h->T * h->nfft}, st) != hipSuccess)
        return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
    hipLaunchKernelGGL(istft_ola_kernel, dim3((h->chunk + 255) / 256, R), dim3(256), 0, st, frames, h->env, y, h->chunk, h->nfft, h->hop, h->T);
    LAUNCH_CHECK();
    return TDX_OK;
}


// ------------------------------------------------------------------------------------------------
// N3  integrated loudness (ITU-R BS.1770-4) of B mono clips — AudioProcessor.meter_loudness
// (AudioProcessor.py:1123-1127 -> pyloudnorm.Meter(rate).integrated_loudness, third-party; restated
// from the published algorithm, see targetdiarization_amd/loudness.py).  K-weighting (two biquads,
// direct form II transposed like scipy.lfilter, fp64) in 1024-sample chunks with a 0.25 s zero-state
// warm-up, all chunks of all clips in parallel; one wave per 400 ms / 75 % overlap gating block for
// its mean square; one thread per clip for the -70 LUFS absolute and -10 LU relative gates.
// ------------------------------------------------------------------------------------------------
}  // extern "C"   (kernels below)
namespace {
struct Biq { double b0, b1, b2, a1, a2; };
inline Biq make_biquad(bool shelf, double G, double Q, double fc, double rate) {
    const double A = pow(10.0, G / 40.0), w0 = 2.0 * M_PI * (fc / rate), alpha = sin(w0) / (2.0 * Q), c = cos(w0);
    double b0, b1, b2, a0, a1, a2;
    if (shelf) {
        b0 = A * ((A + 1) + (A - 1) * c + 2 * sqrt(A) * alpha); b1 = -2 * A * ((A - 1) + (A + 1) * c); b2 = A * ((A + 1) + (A - 1) * c - 2 * sqrt(A) * alpha);
        a0 = (A + 1) - (A - 1) * c + 2 * sqrt(A) * alpha; a1 = 2 * ((A - 1) - (A + 1) * c); a2 = (A + 1) - (A - 1) * c - 2 * sqrt(A) * alpha;
    } else {
        b0 = (1 + c) / 2; b1 = -(1 + c); b2 = (1 + c) / 2; a0 = 1 + alpha; a1 = -2 * c; a2 = 1 - alpha;
    }
    return Biq{b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0};
}
// block j covers samples [ (long)(Tg*(j*step)*rate), (long)(Tg*(j*step+1)*rate) ) — the same double arithmetic as the host meter
__device__ __forceinline__ long blk_lo(int j, double rate) { return (long)(__dmul_rn(__dmul_rn(0.4, __dmul_rn((double)j, 0.25)), rate)); }
__device__ __forceinline__ long blk_hi(int j, double rate) { return (long)(__dmul_rn(__dmul_rn(0.4, __dadd_rn(__dmul_rn((double)j, 0.25), 1.0)), rate)); }

// K-weighting of samples [c*CH, (c+1)*CH) of clip b by one thread.  The recurrence is sequential, but both biquads
// forget their past quickly (pole radius 0.985 at 38 Hz / 16 kHz: r^(0.25 s) ~ 1e-27), so a chunk started from zero
// state 0.25 s early is exact to far below fp64 rounding: all chunks of all clips run in parallel.
constexpr int LOUD_CH = 1024;
__global__ __launch_bounds__(64) void loud_filter_kernel(const float* __restrict__ wav, int B, long N, int warm, Biq f1, Biq f2, int nch,
                                                         double* __restrict__ y) {
    const long id = (long)blockIdx.x * 64 + threadIdx.x;
    if (id >= (long)B * nch) return;
    const int b = (int)(id / nch), c = (int)(id - (long)b * nch);
    const float* x = wav + (long)b * N;
    double* yo = y + (long)b * N;
    const long n0 = (long)c * LOUD_CH, n1 = min(n0 + LOUD_CH, N);
    double s1a = 0, s1b = 0, s2a = 0, s2b = 0;
    for (long n = max(0L, n0 - warm); n < n1; ++n) {
        const double xv = (double)x[n];
        const double y1 = __dadd_rn(__dmul_rn(f1.b0, xv), s1a);
        s1a = __dadd_rn(__dadd_rn(__dmul_rn(f1.b1, xv), -__dmul_rn(f1.a1, y1)), s1b);
        s1b = __dadd_rn(__dmul_rn(f1.b2, xv), -__dmul_rn(f1.a2, y1));
        const double y2 = __dadd_rn(__dmul_rn(f2.b0, y1), s2a);
        s2a = __dadd_rn(__dadd_rn(__dmul_rn(f2.b1, y1), -__dmul_rn(f2.a1, y2)), s2b);
        s2b = __dadd_rn(__dmul_rn(f2.b2, y1), -__dmul_rn(f2.a2, y2));
        if (n >= n0) yo[n] = y2;
    }
}
// z[b][j] = mean square of the filtered samples of gating block j; one wave per (clip, block)
__global__ __launch_bounds__(256) void loud_block_kernel(const double* __restrict__ y, int B, long N, double rate, int nblk, double* __restrict__ z) {
    const long id = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (id >= (long)B * nblk) return;
    const int b = (int)(id / nblk), j = (int)(id - (long)b * nblk);
    const int lane = threadIdx.x & 63;
    const long lo = blk_lo(j, rate), hi = min(blk_hi(j, rate), N);
    const double* yb = y + (long)b * N;
    double s = 0.0;
    for (long n = lo + lane; n < hi; n += 64) s = fma(yb[n], yb[n], s);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) z[(long)b * nblk + j] = s / __dmul_rn(0.4, rate);
}

// the two gates of BS.1770 over the block energies of one clip: one WAVE per clip (a 30 min recording has 18 000 blocks; one
// thread per clip took 10 ms), lanes stride over the blocks, double-precision partial sums reduced across the wave
__global__ __launch_bounds__(64) void loud_gate_kernel(const double* __restrict__ z, int B, int nblk, double* __restrict__ lufs) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    const double* zb = z + (long)b * nblk;
    auto wsum = [](double v) { for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64); return v; };
    double s = 0, c = 0;
    for (int j = lane; j < nblk; j += 64) { const double l = -0.691 + 10.0 * log10(zb[j]); if (l >= -70.0) { s += zb[j]; c += 1.0; } }
    s = wsum(s); c = wsum(c);
    if (c == 0) { if (lane == 0) lufs[b] = -INFINITY; return; }
    const double gamma_r = -0.691 + 10.0 * log10(s / c) - 10.0;
    s = 0; c = 0;
    for (int j = lane; j < nblk; j += 64) { const double l = -0.691 + 10.0 * log10(zb[j]); if (l > gamma_r && l > -70.0) { s += zb[j]; c += 1.0; } }
    s = wsum(s); c = wsum(c);
    if (lane == 0) lufs[b] = c == 0 ? -INFINITY : -0.691 + 10.0 * log10(s / c);
}
// Rational polyphase resampler (N3: AudioProcessor.audio_resample, AudioProcessor.py:549-569): y[c][m] = sum_i x[c][i] * h[m*down - i*up + half]
// — zero-stuffing by `up`, FIR h (2*half+1 taps, DC gain `up`), keep every `down`-th sample, the filter delay removed — as
// one gather per output sample: only the ~(2*half+1)/up input samples whose taps are non-zero are touched.
__global__ __launch_bounds__(256) void resample_poly_kernel(const float* __restrict__ x, long n_in, int C, int up, int down,
                                                             const float* __restrict__ h, int half, float* __restrict__ y, long n_out) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    if (m >= n_out) return;
    const long t = m * down + half;                       // h index = t - i*up, 0 <= . <= 2*half
    long i_hi = t / up;                                   // largest i with t - i*up >= 0
    long i_lo = (t - 2L * half + up - 1) / up;            // smallest i with t - i*up <= 2*half
    if (t - 2L * half < 0) i_lo = 0;
    if (i_hi > n_in - 1) i_hi = n_in - 1;
    const float* xc = x + (long)c * n_in;
    double acc = 0.0;
    for (long i = i_lo; i <= i_hi; ++i) acc = fma((double)xc[i], (double)h[t - i * up], acc);
    y[(long)c * n_out + m] = (float)acc;
}

inline int loud_nblk(long N, int rate) {
    const double T = (double)N / rate;
    return (int)(nearbyint((T - 0.4) / (0.4 * 0.25)) + 1);
}
}  // namespace
extern "C" {

size_t tdx_loudness_workspace_bytes(int B, long N, int rate) {
    if (B < 1 || rate < 1 || N < (long)(0.4 * rate)) return 0;
    return ((size_t)B * loud_nblk(N, rate) + (size_t)B * N) * sizeof(double) + 256;      // block energies + filtered signal
}

// wav_dev [B,N] f32 mono -> lufs_dev [B] f64 (-inf for silence).  Needs N >= 0.4 s.
int tdx_loudness(const float* wav, int B, long N, int rate, double* lufs, void* ws, size_t ws_bytes, void* stream) {
    if (!wav || !lufs || !ws || B < 1 || rate < 1) return tdx::fail(TDX_E_INVALID, "tdx_loudness: bad argument");
    if (N < (long)(0.4 * rate)) return tdx::fail(TDX_E_INVALID, "tdx_loudness: audio must be longer than the 400 ms block");
    if (ws_bytes < tdx_loudness_workspace_bytes(B, N, rate)) return tdx::fail(TDX_E_WORKSPACE, "tdx_loudness: workspace too small");
    const int nblk = loud_nblk(N, rate);
    const Biq f1 = make_biquad(true, 4.0, 1.0 / sqrt(2.0), 1500.0, rate), f2 = make_biquad(false, 0.0, 0.5, 38.0, rate);
    hipStream_t st = (hipStream_t)stream;
    double* z = (double*)ws;
    double* y = z + (size_t)B * nblk;
    const int nch = (int)((N + LOUD_CH - 1) / LOUD_CH);
    const int warm = (int)ceil(0.25 * rate);
    hipLaunchKernelGGL(loud_filter_kernel, dim3((unsigned)(((long)B * nch + 63) / 64)), dim3(64), 0, st, wav, B, N, warm, f1, f2, nch, y);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(loud_block_kernel, dim3((unsigned)(((long)B * nblk + 3) / 4)), dim3(256), 0, st, y, B, N, (double)rate, nblk, z);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(loud_gate_kernel, dim3(B), dim3(64), 0, st, z, B, nblk, lufs);
    LAUNCH_CHECK();
    return TDX_OK;
}


// x_dev [C][n_in] -> y_dev [C][n_out], n_out = ceil(n_in*up/down); h_dev: 2*half+1 taps (DC gain up)
int tdx_resample_poly(const float* x, long n_in, int C, int up, int down, const float* h, int half, float* y, long n_out, void* stream) {
    if (!x || !h || !y || n_in < 1 || C < 1 || up < 1 || down < 1 || half < 0 || n_out < 1) return tdx::fail(TDX_E_INVALID, "tdx_resample_poly: bad argument");
    if (n_out != (n_in * up + down - 1) / down) return tdx::fail(TDX_E_INVALID, "tdx_resample_poly: n_out must be ceil(n_in*up/down)");
    hipLaunchKernelGGL(resample_poly_kernel, dim3((unsigned)((n_out + 255) / 256), C), dim3(256), 0, (hipStream_t)stream, x, n_in, C, up, down, h, half, y, n_out);
    LAUNCH_CHECK();
    return TDX_OK;
}

}  // extern "C"
