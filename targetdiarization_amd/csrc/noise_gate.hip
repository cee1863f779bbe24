// noise_gate.hip — noisereduce's non-stationary spectral gate on MI355X: the body of the reference's denoise_vocal when the MDX
// model is absent or fast_mode is set (AudioProcessor.py:655 `nr.reduce_noise(y=audio_data, sr=sampling_rate)`; third-party
// algorithm, restated from upstream — DESIGN 8.19).
//
// One call gates every buffer of every clip and channel.  A buffer is one padded chunk of one channel (noise_gate.py
// chunk_plan); the host describes it by a table entry of 8 int64:
//     [0] src_off  packed-input index of buffer sample 0 (may be negative: the padding in front of a clip)
//     [1] v0 [2] v1   buffer samples [v0, v1) exist in the input, the others are zero
//     [3] k0 [4] k1   buffer samples [k0, k1) are kept
//     [5] dst_off  packed-output index of buffer sample k0
//     [6] L        buffer length; F = 1 + L / 256 frames, frame f covers buffer samples [256 f - 512, 256 f + 512)
//     [7] row0     first row of the buffer in its round
// A buffer owns F + 3 rows of 256 floats of the padded signal, so that frame f is the 1024 floats from row row0 + f on and the
// analysis GEMM reads its frames as overlapping rows (pitch 256, K 1024); the 3 rows between two buffers give frames that
// straddle them: they are computed by the two GEMMs and never read.  Buffers go into rounds in order; a round is closed when the
// next buffer would take it past rows_per_launch rows.  Seven launches per round, whatever the number of buffers:
//     ng_pad_kernel      zero-padded signal
//     gemm (PAIRED)      S = frame x (hann * DFT), |S|                      EpiSpecMag
//     ng_scan_kernel     forward and backward first-order smoothing of |S| along time + the sigmoid mask
//     ng_smooth_f_kernel triangular smoothing of the mask along frequency
//     ng_smooth_t_kernel triangular smoothing along time, prop_decrease, S *= mask in place
//     gemm               frames = S x (Hermitian weights * inverse DFT * hann / 4)
//     ng_gather_kernel   every kept sample = (its four frame entries, summed in a fixed order) / 384
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/tdx.h"
#include "dft_basis.hpp"
#include "epilogues.hpp"

using namespace tdx;

namespace {

constexpr int NFFT = 1024, HOP = 256, NBIN = 513;
constexpr int BP = 528;                  // pitch of a bin row (columns 513.. of the spectrum halves are exact zeros)
constexpr int NPAIR = 576;               // bins padded to the paired GEMM's 64-column tiles
constexpr int KS = 2 * BP;               // spectrum row [re | im]: the K of the synthesis GEMM (33 x 32)
constexpr tdx::StftGeo GEO = tdx::stft_geo(NFFT);
static_assert(NBIN == GEO.nbin && BP == GEO.BP && NPAIR == GEO.NPAIR && KS == GEO.KS, "the kernels' constants are the shared STFT geometry");
constexpr int XROWS = 3;                 // rows a buffer owns beyond its frames
constexpr int SEG = 64;                  // frames per scan segment: fixed, so that the summation order depends on the buffer alone
constexpr int SC_BINS = 16, SC_SLOTS = 64, SC_THREADS = SC_BINS * SC_SLOTS;
constexpr int MAXSEG = 512;              // segments per buffer the scan's LDS carries hold
constexpr int MAXF = MAXSEG * SEG;
constexpr int MAX_SMOOTH = 128;
constexpr int MAX_BUFS = 65535;
constexpr int TAB = 8;

struct Buf { long src, v0, v1, k0, k1, dst, L, row0; int F; };
__device__ __forceinline__ Buf load_buf(const long* __restrict__ tab, int j) {
    const long* t = tab + (long)j * TAB;
    Buf b;
    b.src = t[0]; b.v0 = t[1]; b.v1 = t[2]; b.k0 = t[3]; b.k1 = t[4]; b.dst = t[5]; b.L = t[6]; b.row0 = t[7];
    b.F = (int)(b.L / HOP) + 1;
    return b;
}

// grid (max rows of a buffer, buffers of the round)
__global__ __launch_bounds__(256) void ng_pad_kernel(const float* __restrict__ x, const long* __restrict__ tab, int j0, float* __restrict__ pad) {
    const Buf b = load_buf(tab, j0 + blockIdx.y);
    if ((int)blockIdx.x >= b.F + XROWS) return;
    const long i = (long)blockIdx.x * HOP + threadIdx.x - NFFT / 2;
    pad[(b.row0 + blockIdx.x) * HOP + threadIdx.x] = (i >= b.v0 && i < b.v1) ? x[b.src + i] : 0.f;
}

// y[f] = b A[f] + a y[f-1] seeded with y[-1] = A[0], then s[f] = b y[f] + a s[f+1] seeded with s[F] = y[F-1]: scipy's filtfilt
// (padtype=None) of the one-pole filter.  A linear scan is associative, so time is cut into segments of SEG frames:
//   1. every segment is scanned from a zero carry (SEG dependent FMAs; the segments of a buffer run side by side),
//   2. one thread per bin hands the carries on through LDS: c[s+1] = end[s] + a^SEG c[s]  (F / SEG dependent FMAs),
//   3. the fix-up local[f] + a^(f - f0 + 1) c[s] of all frames at once.
// A workgroup owns 16 bins of one buffer over all of its frames: 64 segment slots x 16 bins, slot t takes segments t, t + 64, ...
// Layout [frame][bin]: the 16 lanes of a slot read 64 consecutive bytes.  The local values live in the plane that receives the
// result (Y forward, M backward); the thread that wrote one is the thread that fixes it up.  The mask is computed in the
// backward fix-up, so s is never stored (unless a tap asks).
struct ScanArgs {
    const float* A; float* Y; float* M;
    const long* tab; int j0;
    float b, a; double a_d;
    float thresh, slope;
    float *tap_mag, *tap_smooth, *tap_mask;     // buffer 0 of the call only
};
__global__ __launch_bounds__(SC_THREADS) void ng_scan_kernel(ScanArgs p) {
    __shared__ float endv[MAXSEG][SC_BINS];     // step 1: the local end of a segment; step 2 replaces it by the carry into it
    __shared__ float apow[SEG];                 // a^(k+1)
    __shared__ float seed[SC_BINS];
    const int j = p.j0 + blockIdx.y;
    const Buf bf = load_buf(p.tab, j);
    const int F = bf.F, nseg = (F + SEG - 1) / SEG;
    const int tid = threadIdx.x, bl = tid & (SC_BINS - 1), slot = tid / SC_BINS;
    const int bin = blockIdx.x * SC_BINS + bl;
    const bool act = bin < NBIN;
    const long base = bf.row0 * BP + (act ? bin : 0);
    const float* __restrict__ A = p.A + base;
    float* __restrict__ Y = p.Y + base;
    float* __restrict__ M = p.M + base;
    if (tid < SEG) apow[tid] = (float)pow(p.a_d, (double)(tid + 1));
    const float a = p.a, b = p.b;

    // ---- forward
    if (act)
        for (int s = slot; s < nseg; s += SC_SLOTS) {
            const int f0 = s * SEG, f1 = min(f0 + SEG, F);
            float acc = 0.f;
            for (int f = f0; f < f1; ++f) { acc = fmaf(a, acc, b * A[(long)f * BP]); Y[(long)f * BP] = acc; }
            endv[s][bl] = acc;
        }
    __syncthreads();
    if (act && tid < SC_BINS) {
        float c = A[0];
        for (int s = 0; s < nseg; ++s) { const float e = endv[s][bl]; endv[s][bl] = c; c = fmaf(apow[SEG - 1], c, e); }
    }
    __syncthreads();
    if (act)
        for (int s = slot; s < nseg; s += SC_SLOTS) {
            const int f0 = s * SEG, f1 = min(f0 + SEG, F);
            const float c = endv[s][bl];
            float last = 0.f;
            for (int f = f0; f < f1; ++f) { last = fmaf(apow[f - f0], c, Y[(long)f * BP]); Y[(long)f * BP] = last; }
            if (f1 == F) seed[bl] = last;
        }
    __syncthreads();
    // ---- backward over y (each thread re-reads the y it wrote)
    if (act)
        for (int s = slot; s < nseg; s += SC_SLOTS) {
            const int f0 = s * SEG, f1 = min(f0 + SEG, F);
            float acc = 0.f;
            for (int f = f1 - 1; f >= f0; --f) { acc = fmaf(a, acc, b * Y[(long)f * BP]); M[(long)f * BP] = acc; }
            endv[s][bl] = acc;
        }
    __syncthreads();
    if (act && tid < SC_BINS) {
        float c = seed[bl];
        for (int s = nseg - 1; s >= 0; --s) { const float e = endv[s][bl]; endv[s][bl] = c; c = fmaf(apow[min(SEG, F - s * SEG) - 1], c, e); }
    }
    __syncthreads();
    if (act) {
        const bool tap = j == 0;
        for (int s = slot; s < nseg; s += SC_SLOTS) {
            const int f0 = s * SEG, f1 = min(f0 + SEG, F);
            const float c = endv[s][bl];
            for (int f = f0; f < f1; ++f) {
                const float sv = fmaf(apow[f1 - 1 - f], c, M[(long)f * BP]);
                const float av = A[(long)f * BP];
                // s == 0 (digital silence): upstream divides 0 by 0; the mask is 0 here
                const float m = sv == 0.f ? 0.f : 1.f / (1.f + expf(-(((av - sv) / sv) - p.thresh) * p.slope));
                M[(long)f * BP] = m;
                if (tap) {
                    const long o = (long)f * NBIN + bin;
                    if (p.tap_mag) p.tap_mag[o] = av;
                    if (p.tap_smooth) p.tap_smooth[o] = sv;
                    if (p.tap_mask) p.tap_mask[o] = m;
                }
            }
        }
    }
}

// tap j of the normalised triangle tri(k) / sum: (k + 1 - |j - k|) / (k + 1)^2, j = 0 .. 2k
__device__ __forceinline__ float tri_tap(int j, int k, float inv) { return (float)(k + 1 - abs(j - k)) * inv; }

// along frequency, zero boundary: one workgroup per frame.  grid (max frames of a buffer, buffers of the round)
__global__ __launch_bounds__(256) void ng_smooth_f_kernel(const float* __restrict__ M, float* __restrict__ Mf, const long* __restrict__ tab, int j0, int nf) {
    __shared__ float row[NBIN + 2 * MAX_SMOOTH];
    const Buf b = load_buf(tab, j0 + blockIdx.y);
    if ((int)blockIdx.x >= b.F) return;
    const long r = (b.row0 + blockIdx.x) * BP;
    for (int i = threadIdx.x; i < NBIN + 2 * nf; i += 256) { const int k = i - nf; row[i] = (k >= 0 && k < NBIN) ? M[r + k] : 0.f; }
    __syncthreads();
    const float inv = 1.f / (float)((nf + 1) * (nf + 1));
    for (int k = threadIdx.x; k < NBIN; k += 256) {
        float acc = 0.f;
        for (int j = 0; j <= 2 * nf; ++j) acc = fmaf(tri_tap(j, nf, inv), row[k + j], acc);
        Mf[r + k] = acc;
    }
}

// along time, zero boundary, then m * prop + (1 - prop) and S *= m in place.  grid (3, max frames of a buffer, buffers of the round)
__global__ __launch_bounds__(256) void ng_smooth_t_kernel(const float* __restrict__ Mf, float* __restrict__ S, const long* __restrict__ tab, int j0, int nt,
                                                           float prop, float* __restrict__ tap_msmooth) {
    const int j = j0 + blockIdx.z;
    const Buf b = load_buf(tab, j);
    const int f = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (f >= b.F || k >= NBIN) return;
    const float inv = 1.f / (float)((nt + 1) * (nt + 1));
    const int lo = max(0, nt - f), hi = min(2 * nt, nt + b.F - 1 - f);      // rows f + i - nt inside [0, F)
    const float* col = Mf + b.row0 * BP + k;
    float acc = 0.f;
    for (int i = lo; i <= hi; ++i) acc = fmaf(tri_tap(i, nt, inv), col[(long)(f + i - nt) * BP], acc);
    if (tap_msmooth && j == 0) tap_msmooth[(long)f * NBIN + k] = acc;
    const float m = acc * prop + (1.f - prop);
    float* s = S + (b.row0 + f) * KS + k;
    s[0] *= m; s[BP] *= m;
}

// kept sample i lies in frames q - 1 .. q + 2, q = i / 256, at offsets r + 768, r + 512, r + 256, r.  grid (max kept / 256, buffers)
__global__ __launch_bounds__(256) void ng_gather_kernel(const float* __restrict__ fr, const long* __restrict__ tab, int j0, float* __restrict__ y) {
    const Buf b = load_buf(tab, j0 + blockIdx.y);
    const long i = b.k0 + (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= b.k1) return;
    const long q = i / HOP; const int r = (int)(i - q * HOP);
    const float* p = fr + (b.row0 + q - 1) * NFFT + r;
    const float v = (p[768] + p[NFFT + 512]) + (p[2 * NFFT + 256] + p[3 * NFFT]);
    y[b.dst + (i - b.k0)] = v * (1.0f / 384.0f);
}

struct WsPlan { size_t pad, S, A, Y, M, Mf, total; };      // offsets in floats; the synthesis frames reuse A and Y
inline WsPlan ws_plan(long rows) {
    const size_t R = (size_t)rows;
    WsPlan w{};
    size_t o = 0;
    w.pad = o; o += al(R * HOP);
    w.S = o; o += al(R * KS);
    w.A = o; o += R * BP;
    w.Y = o; o += al(R * BP);
    w.M = o; o += al(R * BP);
    w.Mf = o; o += al(R * BP);
    w.total = o;
    return w;
}
static_assert(2 * BP >= NFFT, "the synthesis frames must fit the A and Y planes");

}  // namespace

struct tdx_ngate {
    int device = 0;
    tdx::DevBuf dev; const float *Wa = nullptr, *Ws = nullptr;
};

extern "C" {

int tdx_ngate_create(int device, tdx_ngate** out) {
    if (!out) return tdx::fail(TDX_E_INVALID, "tdx_ngate_create: null argument");
    if (device < 0) return tdx::fail(TDX_E_INVALID, "tdx_ngate_create: device must be >= 0");
    tdx::Loader ld;       // (no blob: the bases are computed here in double, then staged and uploaded like weights)
    // analysis [2 * 576][1024]: row k = hann * cos, row 576 + k = -hann * sin; rows of the bins 513.. are zero
    // synthesis [1024][2 * 528]: frame[n] = hann[n] / 4 * 1/1024 * sum_k w_k (re_k cos - im_k sin), w = 1 at DC and Nyquist, else 2
    // (the 1/4 and the gather's 1/384 make the overlap-add envelope: four hann^2 at hop 256 sum to 1.5 = 4 * 384 / 1024)
    const std::vector<double> win = tdx::hann_periodic(NFFT);
    std::unique_ptr<tdx_ngate> h(new tdx_ngate());
    h->device = device;
    tdx::push_stft_basis(ld, GEO, win.data(), tdx::divided(win, 4.0).data(), h->Wa, h->Ws);
    TRY(ld.finish("tdx_ngate_create", false, device, h->dev));
    *out = h.release();
    return TDX_OK;
}

int tdx_ngate_destroy(tdx_ngate* h) {
    delete h;
    return TDX_OK;
}

long tdx_ngate_rows(long L) { return L < 1 ? 0 : L / HOP + 1 + XROWS; }

size_t tdx_ngate_workspace_bytes(const tdx_ngate* h, long rows) {
    if (!h || rows < 1 + XROWS || rows > (1L << 24)) return 0;
    return ws_plan(rows).total * sizeof(float);
}

int tdx_ngate_forward(tdx_ngate* h, const float* x_dev, long n_total, const int64_t* table_host, const int64_t* table_dev, int nbuf,
                      long rows_per_launch, double b, int nf, int nt, float thresh, float slope, float prop_decrease, float* y_dev,
                      float* tap_mag_dev, float* tap_smooth_dev, float* tap_mask_dev, float* tap_msmooth_dev, void* ws_, size_t ws_bytes,
                      void* stream) {
    if (!h || !x_dev || !table_host || !table_dev || !y_dev || !ws_) return tdx::fail(TDX_E_INVALID, "tdx_ngate_forward: null argument");
    if (n_total < 1) return tdx::fail(TDX_E_INVALID, "tdx_ngate_forward: n_total must be >= 1");
    if (nbuf < 1 || nbuf > MAX_BUFS) return tdx::fail(TDX_E_INVALID, "tdx_ngate_forward: need 1 <= nbuf <= 65535");
    if (!(b > 0.0 && b <= 1.0)) return tdx::fail(TDX_E_INVALID, "tdx_ngate_forward: the filter coefficient b must lie in (0, 1]");
    if (nf < 0 || nf > MAX_SMOOTH || nt < 0 || nt > MAX_SMOOTH) return tdx::fail(TDX_E_INVALID, "tdx_ngate_forward: need 0 <= nf, nt <= 128");
    if (!(prop_decrease >= 0.f && prop_decrease <= 1.f)) return tdx::fail(TDX_E_INVALID, "tdx_ngate_forward: prop_decrease must lie in [0, 1]");
    if (rows_per_launch < 1 + XROWS || rows_per_launch > (1L << 24)) return tdx::fail(TDX_E_INVALID, "tdx_ngate_forward: rows_per_launch must lie in [4, 2^24]");
    // the table is the only thing the kernels index with: every entry is checked here, and the rounds are planned from it
    struct Round { int j0, j1; long rows; int maxF; long maxKeep; };
    std::vector<Round> rounds;
    long max_rows = 0;
    for (int j = 0; j < nbuf; ++j) {
        const int64_t* t = table_host + (size_t)j * TAB;
        const long src = t[0], v0 = t[1], v1 = t[2], k0 = t[3], k1 = t[4], dst = t[5], L = t[6], row0 = t[7];
        const std::string at = "tdx_ngate_forward: buffer " + std::to_string(j) + ": ";
        if (L < 1 || L / HOP + 1 > MAXF) return tdx::fail(TDX_E_INVALID, at + "length must give 1 .. 32768 frames");
        const long F = L / HOP + 1, rows = F + XROWS;
        if (rows > rows_per_launch) return tdx::fail(TDX_E_INVALID, at + "needs " + std::to_string(rows) + " rows, more than rows_per_launch");
        if (v0 < 0 || v1 < v0 || v1 > L) return tdx::fail(TDX_E_INVALID, at + "valid range outside the buffer");
        if (src < -L || src > n_total || (v1 > v0 && (src + v0 < 0 || src + v1 > n_total))) return tdx::fail(TDX_E_INVALID, at + "valid range outside the input");
        if (k0 < 0 || k1 < k0 || k1 > L) return tdx::fail(TDX_E_INVALID, at + "keep range outside the buffer");
        if (k1 > k0 && (k0 < HOP || k1 > HOP * (L / HOP - 1)))
            return tdx::fail(TDX_E_INVALID, at + "a kept sample lacks one of its four frames (padding must be >= 1024)");
        if (dst < 0 || dst > n_total || k1 - k0 > n_total - dst) return tdx::fail(TDX_E_INVALID, at + "keep range outside the output");
        if (rounds.empty() || rounds.back().rows + rows > rows_per_launch) rounds.push_back(Round{j, j, 0, 0, 0});
        Round& r = rounds.back();
        if (row0 != r.rows) return tdx::fail(TDX_E_INVALID, at + "row0 does not follow the round plan");
        r.j1 = j + 1; r.rows += rows; r.maxF = std::max(r.maxF, (int)F); r.maxKeep = std::max(r.maxKeep, k1 - k0);
        max_rows = std::max(max_rows, r.rows);
    }
    const WsPlan wp = ws_plan(max_rows);
    if (ws_bytes < wp.total * sizeof(float)) return tdx::fail(TDX_E_WORKSPACE, "tdx_ngate_forward: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)ws_;
    float *pad = ws + wp.pad, *S = ws + wp.S, *A = ws + wp.A, *Y = ws + wp.Y, *M = ws + wp.M, *Mf = ws + wp.Mf, *frames = A;
    const long* tab = (const long*)table_dev;
    for (const Round& r : rounds) {
        const int nb = r.j1 - r.j0;
        const int Mrows = (int)(r.rows - XROWS);            // the last row computed ends with the last float of `pad`
        hipLaunchKernelGGL(ng_pad_kernel, dim3(r.maxF + XROWS, nb), dim3(256), 0, st, x_dev, tab, r.j0, pad);
        LAUNCH_CHECK();
        TRY((linear_f32<true>(pad, HOP, h->Wa, Mrows, NPAIR, NFFT, EpiSpecMag{S, A, KS, BP, BP, BP}, st, 0, NPAIR)));
        ScanArgs sa{A, Y, M, tab, r.j0, (float)b, (float)(1.0 - b), 1.0 - b, thresh, slope, tap_mag_dev, tap_smooth_dev, tap_mask_dev};
        hipLaunchKernelGGL(ng_scan_kernel, dim3((NBIN + SC_BINS - 1) / SC_BINS, nb), dim3(SC_THREADS), 0, st, sa);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(ng_smooth_f_kernel, dim3(r.maxF, nb), dim3(256), 0, st, M, Mf, tab, r.j0, nf);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(ng_smooth_t_kernel, dim3((NBIN + 255) / 256, r.maxF, nb), dim3(256), 0, st, Mf, S, tab, r.j0, nt, prop_decrease, tap_msmooth_dev);
        LAUNCH_CHECK();
        TRY(linear_f32(S, KS, h->Ws, Mrows, NFFT, KS, EpiBiasAct<ActNone>{nullptr, frames, NFFT}, st));
        if (r.maxKeep > 0) {
            hipLaunchKernelGGL(ng_gather_kernel, dim3((unsigned)((r.maxKeep + 255) / 256), nb), dim3(256), 0, st, frames, tab, r.j0, y_dev);
            LAUNCH_CHECK();
        }
    }
    return TDX_OK;
}

}  // extern "C"
