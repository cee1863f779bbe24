// pvoc.hip — librosa's phase-vocoder time stretch, pitch shift and the reference's EQ match on MI355X: the bodies of
// AudioProcessor.audio_stretch (AudioProcessor.py:468-499, the librosa branch), audio_pitch (:452-465) and eq_match (:502-546).
// Third-party algorithms restated from upstream (librosa 0.10 stft / phase_vocoder / istft defaults).
//
// A clip of C channels x n samples and a transform (n_fft, hop), T = 1 + n / hop frames:
//     pv_pad_kernel     every channel zero-padded by n_fft / 2 on both sides, as R = T - 1 + ceil(n_fft / hop) rows of hop floats,
//                       so that frame f of a channel is the n_fft floats from its row f on (overlapping GEMM rows, pitch hop)
//     gemm (PAIRED)     S = frame x (hann * DFT) as rows [re 0 .. BP | im 0 .. BP], BP = n_fft / 2 + 16     EpiSpec
//     pv_kernel         the phase vocoder: T' output frames from the columns idx[t], idx[t] + 1 and alpha[t] of the host plan
//     gemm              frames = S' x (Hermitian weights * inverse DFT / n_fft * hann)
//     pv_gather_kernel  sample j = (the frame entries that cover it, summed in frame order) / (the hann^2 of the same frames)
// EQ match replaces pv_kernel by pv_mean_kernel (source and target), pv_gain_kernel and pv_scale_kernel.
// The rows between two channels give frames that straddle them: the analysis GEMM computes them and nothing reads them.
//
// Phases are fp64 (atan2, the wrap, the running sum, sincos): the sum reaches 1e8 rad on a 30-minute clip, where a float
// carries no phase at all.  Magnitudes and the stored spectra are fp32.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <mutex>
#include <vector>

#include "../../include/tdx.h"
#include "dft_basis.hpp"
#include "epilogues.hpp"

using namespace tdx;

namespace {

constexpr int SEG = TDX_PVOC_SEG;        // frames per scan segment: fixed, so that the summation order depends on the clip alone
constexpr int SC_BINS = 16, SC_SLOTS = TDX_PVOC_SLOTS, SC_THREADS = SC_BINS * SC_SLOTS;
constexpr int SWEEP = SEG * SC_SLOTS;    // frames one sweep of the segment slots covers
constexpr int MAX_NFFT = 4096, MAX_CH = 65535;
constexpr long MAX_N = 1L << 36;
constexpr int MAX_GRID_Y = 32768;

struct Geo : tdx::StftGeo { int hop, cover; };      // cover = ceil(n_fft / hop): frames over one sample, at most
inline Geo geo(int n_fft, int hop) { return Geo{tdx::stft_geo(n_fft), hop, (n_fft + hop - 1) / hop}; }
// The rule of include/tdx.h: the synthesis GEMM's N is n_fft (tiles of 128), its K is n_fft + 32; the analysis GEMM's row pitch
// is hop (16-byte loads); the gather sums at most 16 frames per sample.
inline const char* geo_error(int n_fft, int hop) {
    if (n_fft < 128 || n_fft > MAX_NFFT || n_fft % 128 != 0) return "n_fft must be a multiple of 128 in [128, 4096]";
    if (hop < 4 || hop % 4 != 0 || hop > n_fft || (long)hop * 16 < n_fft) return "hop_length must be a multiple of 4 in [n_fft / 16, n_fft]";
    return nullptr;
}

// a spectrum in memory: re at p[c * ch + f * ld + k * es], im `imo` floats further
struct SpecView { float* p; long ch, ld; int es, imo; };
inline SpecView rows_view(float* p, long rows_per_ch, const Geo& g) { return SpecView{p, rows_per_ch * g.KS, g.KS, 1, g.BP}; }
inline SpecView cplx_view(float* p, long T, const Geo& g) { return SpecView{p, T * 2L * g.nbin, 2L * g.nbin, 2, 1}; }

struct EpiSpec {      // PAIRED: spec[m][c] = re, spec[m][im_off + c] = im, columns c < nreal
    float* spec; long lds; int im_off; int nreal;
    __device__ EpiNone col(int, int) const { return EpiNone{}; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store2(int, int m, int c, float re, float im, EpiNone, EpiNone) const {
        if (c < nreal) { float* s = spec + (long)m * (int)lds + c; s[0] = re; s[im_off] = im; }
    }
};

// grid (R, C)
__global__ __launch_bounds__(256) void pv_pad_kernel(const float* __restrict__ x, long n, int n_fft, int hop, long R, float* __restrict__ pad) {
    const long row = blockIdx.x, c = blockIdx.y;
    for (int o = threadIdx.x; o < hop; o += 256) {
        const long i = row * hop + o - n_fft / 2;
        pad[(c * R + row) * hop + o] = (i >= 0 && i < n) ? x[c * n + i] : 0.f;
    }
}

// copy T rows of `nbin` bins from one view to another; bins nbin .. nstore of the destination become zero.
// grid (x, min(T, 32768), C): a block takes the rows blockIdx.y, blockIdx.y + gridDim.y, ...
__global__ __launch_bounds__(256) void pv_relayout_kernel(SpecView s, SpecView d, int nbin, int nstore, long T) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nstore) return;
    const long c = blockIdx.z;
    const bool in = k < nbin;
    for (long f = blockIdx.y; f < T; f += gridDim.y) {
        const float* sp = s.p + c * s.ch + f * s.ld + (long)k * s.es;
        float* dp = d.p + c * d.ch + f * d.ld + (long)k * d.es;
        dp[0] = in ? sp[0] : 0.f; dp[d.imo] = in ? sp[s.imo] : 0.f;
    }
}

// librosa.phase_vocoder.  acc[t] = angle(D[0]) + sum_{s < t} (phi + wrap(angle(D[i_s + 1]) - angle(D[i_s]) - phi)) is a prefix sum
// along time per bin.  A workgroup owns 16 bins of one channel over all output frames: 32 segment slots x 16 bins, and time goes
// by in sweeps of 32 segments of SEG = 16 frames:
//   1. every slot sums the increments of its segment (SEG dependent adds; the 32 segments of a sweep run side by side),
//   2. one thread per bin hands the carry on through LDS: the carry into segment s, then += its sum (32 dependent adds),
//   3. every slot walks its segment again from its carry and writes mag * (cos acc, sin acc).
// The increments are computed twice (two atan2 each) instead of being stored: a plane of doubles would be the largest buffer
// of the call.  Columns >= T are exact zeros (upstream pads two zero columns): they are never read.
// Layout [frame][bin]: the 16 lanes of a slot read neighbouring bins.
struct PvArgs {
    SpecView D, O;
    const int* idx; const double* alpha;
    int T, Tout, nbin, nstore, hop, n_fft;
};
struct PvCols { float r0, i0, r1, i1; };
__device__ __forceinline__ PvCols pv_cols(const float* __restrict__ D, long ld, int imo, int i, int T) {
    PvCols c{0.f, 0.f, 0.f, 0.f};
    if (i < T) { const float* p = D + (long)i * ld; c.r0 = p[0]; c.i0 = p[imo]; }
    if (i + 1 < T) { const float* p = D + (long)(i + 1) * ld; c.r1 = p[0]; c.i1 = p[imo]; }
    return c;
}
__device__ __forceinline__ double pv_inc(const PvCols& c, double phi) {
    double d = atan2((double)c.i1, (double)c.r1) - atan2((double)c.i0, (double)c.r0) - phi;
    d = d - 2.0 * M_PI * rint(d / (2.0 * M_PI));
    return phi + d;
}
__global__ __launch_bounds__(SC_THREADS) void pv_kernel(PvArgs p) {
    __shared__ double endv[SC_SLOTS][SC_BINS];
    __shared__ double carry[SC_BINS];
    const int tid = threadIdx.x, bl = tid & (SC_BINS - 1), slot = tid / SC_BINS;
    const int bin = blockIdx.x * SC_BINS + bl;
    const bool act = bin < p.nbin, zero = !act && bin < p.nstore;
    const long c = blockIdx.y;
    const float* __restrict__ D = p.D.p + c * p.D.ch + (long)(act ? bin : 0) * p.D.es;
    float* __restrict__ O = p.O.p + c * p.O.ch + (long)(act || zero ? bin : 0) * p.O.es;
    const double phi = 2.0 * M_PI * (double)bin * (double)p.hop / (double)p.n_fft;
    if (tid < SC_BINS) carry[tid] = act ? atan2((double)D[p.D.imo], (double)D[0]) : 0.0;
    const int nsweep = (p.Tout + SWEEP - 1) / SWEEP;
    for (int sw = 0; sw < nsweep; ++sw) {
        const int t0 = min(sw * SWEEP + slot * SEG, p.Tout), t1 = min(t0 + SEG, p.Tout);
        double s = 0.0;
        if (act)
            for (int t = t0; t < t1; ++t) s += pv_inc(pv_cols(D, p.D.ld, p.D.imo, p.idx[t], p.T), phi);
        endv[slot][bl] = s;
        __syncthreads();
        if (tid < SC_BINS) {
            double cr = carry[tid];
            for (int q = 0; q < SC_SLOTS; ++q) { const double e = endv[q][tid]; endv[q][tid] = cr; cr += e; }
            carry[tid] = cr;
        }
        __syncthreads();
        if (act) {
            double acc = endv[slot][bl];
            for (int t = t0; t < t1; ++t) {
                const PvCols cl = pv_cols(D, p.D.ld, p.D.imo, p.idx[t], p.T);
                const float a = (float)p.alpha[t];
                const float mag = (1.f - a) * hypotf(cl.r0, cl.i0) + a * hypotf(cl.r1, cl.i1);
                double sn, cs;
                sincos(acc, &sn, &cs);
                float* o = O + (long)t * p.O.ld;
                o[0] = mag * (float)cs; o[p.O.imo] = mag * (float)sn;
                acc += pv_inc(cl, phi);
            }
        } else if (zero) {
            for (int t = t0; t < t1; ++t) { float* o = O + (long)t * p.O.ld; o[0] = 0.f; o[p.O.imo] = 0.f; }
        }
        __syncthreads();
    }
}

// every output sample sums the entries of the frames that cover it, first frame first, and divides by the hann^2 of the same
// frames unless that is <= float32 tiny (librosa's rule).  Sample j is padded position j + n_fft / 2.  grid (length / 256, C)
__global__ __launch_bounds__(256) void pv_gather_kernel(const float* __restrict__ fr, long chF, int nF, int n_fft, int hop,
                                                        const float* __restrict__ win2, long length, float* __restrict__ y) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (j >= length) return;
    const long q = j + n_fft / 2;
    const long f_hi = min(q / hop, (long)nF - 1);
    const long f_lo = q - n_fft + 1 <= 0 ? 0 : (q - n_fft + hop) / hop;
    float v = 0.f, w = 0.f;
    for (long f = f_lo; f <= f_hi; ++f) {
        const int o = (int)(q - f * hop);
        v += fr[c * chF + f * n_fft + o];
        w += win2[o];
    }
    y[c * length + j] = w > FLT_MIN ? v / w : v;
}

// mean over frames of |S| per bin: fp64 sums in a fixed order — a segment's frames in order, a slot's segments in order, the
// slots in order.  grid (ceil(nbin / 16))
__global__ __launch_bounds__(SC_THREADS) void pv_mean_kernel(SpecView S, int T, int nbin, double* __restrict__ mean) {
    __shared__ double part[SC_SLOTS][SC_BINS];
    const int tid = threadIdx.x, bl = tid & (SC_BINS - 1), slot = tid / SC_BINS;
    const int bin = blockIdx.x * SC_BINS + bl;
    const bool act = bin < nbin;
    const float* __restrict__ D = S.p + (long)(act ? bin : 0) * S.es;
    const int nseg = (T + SEG - 1) / SEG;
    double tot = 0.0;
    if (act)
        for (int s = slot; s < nseg; s += SC_SLOTS) {
            const int f1 = min((s + 1) * SEG, T);
            double a = 0.0;
            for (int f = s * SEG; f < f1; ++f) { const float* p = D + (long)f * S.ld; a += (double)hypotf(p[0], p[S.imo]); }
            tot += a;
        }
    part[slot][bl] = tot;
    __syncthreads();
    if (tid < SC_BINS && act) {
        double a = 0.0;
        for (int q = 0; q < SC_SLOTS; ++q) a += part[q][tid];
        mean[bin] = a / (double)T;
    }
}

// gain = clip(mean_t / mean_s, 0.1, 10); a source mean of exactly 0 gives 10 (upstream: 0 / 0 -> NaN through the whole clip)
__global__ __launch_bounds__(256) void pv_gain_kernel(const double* __restrict__ ms, const double* __restrict__ mt, int nbin, float* __restrict__ gain,
                                                      double* __restrict__ tap_ms, double* __restrict__ tap_mt, float* __restrict__ tap_gain) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nbin) return;
    const double s = ms[k], t = mt[k];
    const float g = s == 0.0 ? 10.f : (float)fmin(fmax(t / s, 0.1), 10.0);
    gain[k] = g;
    if (tap_ms) tap_ms[k] = s;
    if (tap_mt) tap_mt[k] = t;
    if (tap_gain) tap_gain[k] = g;
}

// S[f][k] *= gain[k], both halves.  grid (ceil(nbin / 256), min(T, 32768))
__global__ __launch_bounds__(256) void pv_scale_kernel(float* __restrict__ S, long ld, int imo, const float* __restrict__ gain, int nbin, long T) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nbin) return;
    const float g = gain[k];
    for (long f = blockIdx.y; f < T; f += gridDim.y) {
        float* s = S + f * ld + k;
        s[0] *= g; s[imo] *= g;
    }
}

// Kaiser(5.0)-windowed sinc, 10 zero crossings, evaluated where the output sample lies (tdx.h); one thread per output sample
__device__ __forceinline__ double bessel_i0(double x) {      // power series; x <= 5: the 25th term is below 1e-30 of the sum
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k <= 25; ++k) { term *= q / ((double)k * (double)k); sum += term; }
    return sum;
}
__global__ __launch_bounds__(256) void resample_sinc_kernel(const float* __restrict__ x, long n_in, double ratio, long n_out, long n_store,
                                                            float* __restrict__ y) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x, ch = blockIdx.y;
    if (m >= n_store) return;
    float r = 0.f;
    if (m < n_out) {
        const double p = (double)m / ratio;
        const double c = fmin(1.0, ratio), H = 10.0 / c, inv_i0 = 1.0 / bessel_i0(5.0);
        const long j0 = (long)ceil(p - H), j1 = (long)floor(p + H);
        double num = 0.0, den = 0.0;
        for (long j = j0; j <= j1; ++j) {
            const double d = (double)j - p, u = d / H, a = c * d;
            const double sc = a == 0.0 ? 1.0 : sinpi(a) / (M_PI * a);
            const double h = c * sc * bessel_i0(5.0 * sqrt(fmax(0.0, 1.0 - u * u))) * inv_i0;
            den += h;
            if (j >= 0 && j < n_in) num += h * (double)x[ch * n_in + j];
        }
        r = (float)(num / den);
    }
    y[ch * n_store + m] = r;
}

struct Basis { Geo g; tdx::DevBuf dev; const float *Wa = nullptr, *Ws = nullptr, *win2 = nullptr; };

int make_basis(int n_fft, int device, std::unique_ptr<Basis>& out) {
    const Geo g = geo(n_fft, n_fft / 4);
    tdx::Loader ld;       // (no blob: the bases are computed here in double, then staged and uploaded like weights)
    // analysis [2 * NPAIR][n_fft]: row k = hann * cos, row NPAIR + k = -hann * sin; rows of the bins nbin.. are zero
    // synthesis [n_fft][KS]: frame[n] = hann[n] / n_fft * sum_k w_k (re_k cos - im_k sin), w = 1 at DC and Nyquist, else 2
    const std::vector<double> win = tdx::hann_periodic(n_fft);
    std::unique_ptr<Basis> b(new Basis());
    b->g = g;
    tdx::push_stft_basis(ld, g, win.data(), tdx::divided(win, n_fft).data(), b->Wa, b->Ws);
    const size_t oW = ld.room(b->win2, (size_t)n_fft);
    for (int n = 0; n < n_fft; ++n) ld.host[oW + n] = (float)(win[n] * win[n]);
    TRY(ld.finish("tdx_pvoc_prepare", false, device, b->dev));
    out = std::move(b);
    return TDX_OK;
}

struct WsPlan { size_t pad, S, S2, frames, stats, total; };      // offsets in floats
inline WsPlan ws_plan(const Geo& g, long C, long n, long Tout) {
    const size_t T = (size_t)(n / g.hop + 1), R = T - 1 + g.cover, To = (size_t)Tout;
    WsPlan w{};
    size_t o = 0;
    w.pad = o; o += al((size_t)C * R * g.hop);
    w.S = o; o += al((size_t)C * R * g.KS);
    w.S2 = o; o += al((size_t)C * To * g.KS);
    w.frames = o; o += al((size_t)C * std::max(To, T) * g.n_fft);
    w.stats = o; o += al((size_t)6 * g.BP);        // two mean curves in double, the gain
    w.total = o;
    return w;
}

}  // namespace

struct tdx_pvoc {
    int device = 0;
    std::mutex mu;
    std::map<int, std::unique_ptr<Basis>> bases;
    const Basis* find(int n_fft) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = bases.find(n_fft);
        return it == bases.end() ? nullptr : it->second.get();
    }
};

namespace {

int check_geo(const char* fn, tdx_pvoc* h, int n_fft, int hop, const Basis** b) {
    if (const char* e = geo_error(n_fft, hop)) return tdx::fail(TDX_E_INVALID, std::string(fn) + ": " + e);
    *b = h->find(n_fft);
    if (!*b) return tdx::fail(TDX_E_INVALID, std::string(fn) + ": no basis for n_fft " + std::to_string(n_fft) + " (call tdx_pvoc_prepare first)");
    return TDX_OK;
}
int check_plan(const char* fn, const int32_t* idx_host, int T, int Tout) {
    if (Tout < 1 || Tout > (1 << 30)) return tdx::fail(TDX_E_INVALID, std::string(fn) + ": the plan needs 1 .. 2^30 output frames");
    for (int t = 0; t < Tout; ++t)
        if (idx_host[t] < 0 || idx_host[t] >= T)
            return tdx::fail(TDX_E_INVALID, std::string(fn) + ": plan entry " + std::to_string(t) + " is outside the " + std::to_string(T) + " frames");
    return TDX_OK;
}

// pad + analysis GEMM of C channels of n samples into the rows view at ws.S
int analysis(const Basis& b, int hop, const float* x, int C, long n, float* pad, float* S, hipStream_t st) {
    Geo g = b.g; g.hop = hop; g.cover = (g.n_fft + hop - 1) / hop;
    const long T = n / hop + 1, R = T - 1 + g.cover;
    hipLaunchKernelGGL(pv_pad_kernel, dim3((unsigned)R, C), dim3(256), 0, st, x, n, g.n_fft, hop, R, pad);
    LAUNCH_CHECK();
    const int M = (int)(C * R - (g.cover - 1));      // the last row computed ends with the last float of `pad`
    TRY((linear_f32<true>(pad, hop, b.Wa, M, g.NPAIR, g.n_fft, EpiSpec{S, g.KS, g.BP, g.BP}, st, 0, g.NPAIR)));
    return TDX_OK;
}

// synthesis GEMM of C x rows spectrum rows (rows view) + the gather of `length` samples per channel from the first nF frames
int synthesis(const Basis& b, int hop, const float* S2, int C, long rows, int nF, long length, float* frames, float* y, hipStream_t st) {
    const Geo& g = b.g;
    TRY(linear_f32(S2, g.KS, b.Ws, (int)(C * rows), g.n_fft, g.KS, EpiBiasAct<ActNone>{nullptr, frames, g.n_fft}, st));
    if (length > 0) {
        hipLaunchKernelGGL(pv_gather_kernel, dim3((unsigned)((length + 255) / 256), C), dim3(256), 0, st, frames, rows * g.n_fft, nF, g.n_fft, hop, b.win2,
                           length, y);
        LAUNCH_CHECK();
    }
    return TDX_OK;
}

inline int frames_used(int Tout, long length, int n_fft, int hop) {      // librosa.istft with a length
    return (int)std::min<long>(Tout, (length + n_fft + hop - 1) / hop);
}

void relayout(const SpecView& s, const SpecView& d, int nbin, int nstore, long T, int C, hipStream_t st) {
    hipLaunchKernelGGL(pv_relayout_kernel, dim3((nstore + 255) / 256, (unsigned)std::min<long>(T, MAX_GRID_Y), C), dim3(256), 0, st, s, d, nbin, nstore, T);
}

}  // namespace

extern "C" {

int tdx_pvoc_create(int device, tdx_pvoc** out) {
    if (!out) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_create: null argument");
    if (device < 0) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_create: device must be >= 0");
    std::unique_ptr<tdx_pvoc> h(new tdx_pvoc());
    h->device = device;
    std::unique_ptr<Basis> b;
    TRY(make_basis(2048, device, b));
    h->bases[2048] = std::move(b);
    *out = h.release();
    return TDX_OK;
}

int tdx_pvoc_destroy(tdx_pvoc* h) {
    delete h;
    return TDX_OK;
}

int tdx_pvoc_prepare(tdx_pvoc* h, int n_fft) {
    if (!h) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_prepare: null argument");
    if (const char* e = geo_error(n_fft, n_fft / 4)) return tdx::fail(TDX_E_INVALID, std::string("tdx_pvoc_prepare: ") + e);
    if (h->find(n_fft)) return TDX_OK;
    std::unique_ptr<Basis> b;
    TRY(make_basis(n_fft, h->device, b));
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->bases.count(n_fft)) h->bases[n_fft] = std::move(b);
    return TDX_OK;
}

size_t tdx_pvoc_workspace_bytes(const tdx_pvoc* h, int n_fft, int hop, int C, long n, long Tout) {
    if (!h || geo_error(n_fft, hop) || C < 1 || C > MAX_CH || n < 0 || n > MAX_N || Tout < 0 || Tout > INT32_MAX) return 0;
    return ws_plan(geo(n_fft, hop), C, n, Tout).total * sizeof(float);
}

int tdx_pvoc_stretch(tdx_pvoc* h, const float* x_dev, int C, long n, const int32_t* idx_host, const int32_t* idx_dev, const double* alpha_dev,
                     int Tout, long length, float* y_dev, float* tap_spec_dev, float* tap_stretched_dev, void* ws_, size_t ws_bytes, void* stream) {
    const char* fn = "tdx_pvoc_stretch";
    if (!h || !x_dev || !idx_host || !idx_dev || !alpha_dev || !y_dev || !ws_) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_stretch: null argument");
    if (C < 1 || C > MAX_CH) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_stretch: need 1 <= C <= 65535");
    if (n < 1 || n > MAX_N) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_stretch: the clip is empty or longer than 2^36 samples");
    if (length < 1 || length > MAX_N) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_stretch: length must lie in [1, 2^36]");
    const int n_fft = 2048, hop = 512;
    const Basis* b;
    TRY(check_geo(fn, h, n_fft, hop, &b));
    const Geo g = geo(n_fft, hop);
    const long T = n / hop + 1, R = T - 1 + g.cover;
    if ((double)C * (double)std::max<long>(R, Tout) > 2.0e9) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_stretch: more than 2e9 frame rows in one call");
    TRY(check_plan(fn, idx_host, (int)T, Tout));
    const WsPlan wp = ws_plan(g, C, n, Tout);
    if (ws_bytes < wp.total * sizeof(float)) return tdx::fail(TDX_E_WORKSPACE, "tdx_pvoc_stretch: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)ws_;
    float *pad = ws + wp.pad, *S = ws + wp.S, *S2 = ws + wp.S2, *frames = ws + wp.frames;
    TRY(analysis(*b, hop, x_dev, C, n, pad, S, st));
    if (tap_spec_dev) { relayout(rows_view(S, R, g), cplx_view(tap_spec_dev, T, g), g.nbin, g.nbin, T, C, st); LAUNCH_CHECK(); }
    PvArgs pa{rows_view(S, R, g), rows_view(S2, Tout, g), idx_dev, alpha_dev, (int)T, Tout, g.nbin, g.BP, hop, n_fft};
    hipLaunchKernelGGL(pv_kernel, dim3(g.BP / SC_BINS, C), dim3(SC_THREADS), 0, st, pa);
    LAUNCH_CHECK();
    if (tap_stretched_dev) { relayout(rows_view(S2, Tout, g), cplx_view(tap_stretched_dev, Tout, g), g.nbin, g.nbin, Tout, C, st); LAUNCH_CHECK(); }
    return synthesis(*b, hop, S2, C, Tout, frames_used(Tout, length, n_fft, hop), length, frames, y_dev, st);
}

int tdx_pvoc_vocode(tdx_pvoc* h, const float* D_dev, int nbin, int T, int hop, const int32_t* idx_host, const int32_t* idx_dev,
                    const double* alpha_dev, int Tout, float* out_dev, void* stream) {
    const char* fn = "tdx_pvoc_vocode";
    if (!h || !D_dev || !idx_host || !idx_dev || !alpha_dev || !out_dev) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_vocode: null argument");
    if (nbin < 2 || nbin > MAX_NFFT / 2 + 1) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_vocode: need 2 <= bins <= 2049");
    if (T < 1) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_vocode: the spectrum has no frames");
    if (hop < 1 || hop > 2 * (nbin - 1)) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_vocode: hop must lie in [1, n_fft]");
    TRY(check_plan(fn, idx_host, T, Tout));
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    const SpecView in{const_cast<float*>(D_dev), 0, 2L * nbin, 2, 1}, out{out_dev, 0, 2L * nbin, 2, 1};
    PvArgs pa{in, out, idx_dev, alpha_dev, T, Tout, nbin, nbin, hop, 2 * (nbin - 1)};
    hipLaunchKernelGGL(pv_kernel, dim3((nbin + SC_BINS - 1) / SC_BINS, 1), dim3(SC_THREADS), 0, (hipStream_t)stream, pa);
    LAUNCH_CHECK();
    return TDX_OK;
}

int tdx_pvoc_istft(tdx_pvoc* h, const float* D_dev, int T, int n_fft, int hop, long length, float* y_dev, void* ws_, size_t ws_bytes, void* stream) {
    const char* fn = "tdx_pvoc_istft";
    if (!h || !D_dev || !y_dev || !ws_) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_istft: null argument");
    if (T < 1) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_istft: the spectrum has no frames");
    const Basis* b;
    TRY(check_geo(fn, h, n_fft, hop, &b));
    if (length < 0) length = (long)hop * (T - 1);
    if (length > MAX_N) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_istft: length must be <= 2^36");
    const Geo g = geo(n_fft, hop);
    const WsPlan wp = ws_plan(g, 1, 0, T);
    if (ws_bytes < wp.total * sizeof(float)) return tdx::fail(TDX_E_WORKSPACE, "tdx_pvoc_istft: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)ws_;
    float *S2 = ws + wp.S2, *frames = ws + wp.frames;
    relayout(cplx_view(const_cast<float*>(D_dev), T, g), rows_view(S2, T, g), g.nbin, g.BP, T, 1, st);
    LAUNCH_CHECK();
    return synthesis(*b, hop, S2, 1, T, frames_used(T, length, n_fft, hop), length, frames, y_dev, st);
}

int tdx_pvoc_eq_match(tdx_pvoc* h, const float* src_dev, long n_src, const float* tgt_dev, long n_tgt, const float* tgt_stft_dev, int T_tgt,
                      int n_fft, int hop, float* y_dev, float* tap_spec_dev, double* tap_mean_src_dev, double* tap_mean_tgt_dev,
                      float* tap_gain_dev, void* ws_, size_t ws_bytes, void* stream) {
    const char* fn = "tdx_pvoc_eq_match";
    if (!h || !src_dev || !y_dev || !ws_) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_eq_match: null argument");
    if (!tgt_dev == !tgt_stft_dev) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_eq_match: give the target as samples or as a spectrum, one of the two");
    if (n_src < 1 || n_src > MAX_N) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_eq_match: the source is empty or longer than 2^36 samples");
    if (tgt_dev && (n_tgt < 1 || n_tgt > MAX_N)) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_eq_match: the target is empty or longer than 2^36 samples");
    if (tgt_stft_dev && T_tgt < 1) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_eq_match: the target spectrum has no frames");
    const Basis* b;
    TRY(check_geo(fn, h, n_fft, hop, &b));
    const Geo g = geo(n_fft, hop);
    const long nmax = tgt_dev ? std::max(n_src, n_tgt) : n_src;
    if ((double)(nmax / hop + 1 + g.cover) > 2.0e9) return tdx::fail(TDX_E_INVALID, "tdx_pvoc_eq_match: more than 2e9 frames");
    const WsPlan wp = ws_plan(g, 1, nmax, 0);
    if (ws_bytes < wp.total * sizeof(float)) return tdx::fail(TDX_E_WORKSPACE, "tdx_pvoc_eq_match: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)ws_;
    float *pad = ws + wp.pad, *S = ws + wp.S, *frames = ws + wp.frames;
    double *ms = (double*)(ws + wp.stats), *mt = ms + g.BP;
    float* gain = (float*)(mt + g.BP);
    const dim3 mgrid((g.nbin + SC_BINS - 1) / SC_BINS);
    if (tgt_dev) {
        const long Tt = n_tgt / hop + 1;
        TRY(analysis(*b, hop, tgt_dev, 1, n_tgt, pad, S, st));
        hipLaunchKernelGGL(pv_mean_kernel, mgrid, dim3(SC_THREADS), 0, st, rows_view(S, Tt - 1 + g.cover, g), (int)Tt, g.nbin, mt);
    } else {
        hipLaunchKernelGGL(pv_mean_kernel, mgrid, dim3(SC_THREADS), 0, st, cplx_view(const_cast<float*>(tgt_stft_dev), T_tgt, g), T_tgt, g.nbin, mt);
    }
    LAUNCH_CHECK();
    const long T = n_src / hop + 1, R = T - 1 + g.cover;
    TRY(analysis(*b, hop, src_dev, 1, n_src, pad, S, st));
    if (tap_spec_dev) { relayout(rows_view(S, R, g), cplx_view(tap_spec_dev, T, g), g.nbin, g.nbin, T, 1, st); LAUNCH_CHECK(); }
    hipLaunchKernelGGL(pv_mean_kernel, mgrid, dim3(SC_THREADS), 0, st, rows_view(S, R, g), (int)T, g.nbin, ms);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(pv_gain_kernel, dim3((g.nbin + 255) / 256), dim3(256), 0, st, ms, mt, g.nbin, gain, tap_mean_src_dev, tap_mean_tgt_dev, tap_gain_dev);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(pv_scale_kernel, dim3((g.nbin + 255) / 256, (unsigned)std::min<long>(T, MAX_GRID_Y)), dim3(256), 0, st, S, (long)g.KS, g.BP, gain, g.nbin, T);
    LAUNCH_CHECK();
    return synthesis(*b, hop, S, 1, T, (int)T, (long)hop * (T - 1), frames, y_dev, st);
}

int tdx_resample_sinc(const float* x_dev, int C, long n_in, double ratio, float* y_dev, long n_store, void* stream) {
    if (!x_dev || !y_dev) return tdx::fail(TDX_E_INVALID, "tdx_resample_sinc: null argument");
    if (C < 1 || C > MAX_CH) return tdx::fail(TDX_E_INVALID, "tdx_resample_sinc: need 1 <= C <= 65535");
    if (n_in < 1 || n_in > MAX_N) return tdx::fail(TDX_E_INVALID, "tdx_resample_sinc: the clip is empty or longer than 2^36 samples");
    if (!(ratio >= 1.0 / 64 && ratio <= 64.0)) return tdx::fail(TDX_E_INVALID, "tdx_resample_sinc: the ratio must lie in [1/64, 64]");
    if (n_store < 1 || n_store > MAX_N) return tdx::fail(TDX_E_INVALID, "tdx_resample_sinc: n_store must lie in [1, 2^36]");
    const long n_out = tdx_resample_sinc_length(n_in, ratio);
    hipLaunchKernelGGL(resample_sinc_kernel, dim3((unsigned)((n_store + 255) / 256), C), dim3(256), 0, (hipStream_t)stream, x_dev, n_in, ratio, n_out,
                       n_store, y_dev);
    LAUNCH_CHECK();
    return TDX_OK;
}

long tdx_resample_sinc_length(long n_in, double ratio) { return n_in < 1 || !(ratio > 0.0) ? 0 : (long)ceil((double)n_in * ratio); }

}  // extern "C"
