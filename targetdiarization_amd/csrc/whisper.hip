// whisper.hip — Whisper on MI355X (include/tdx.h N10): the reference's third local recogniser,
// `AutoModelForSpeechSeq2Seq.from_pretrained(...)` + `generate(task="transcribe", language="chinese", num_beams=1, prompt_ids=...)`
// (ASRProcessor.py:244-251, 489-514).  Hugging Face transformers' WhisperForConditionalGeneration is the upstream;
// tests/whisper_oracle.py restates it and tests/test_whisper_host.py pins the restatement to it.  Everything fp32.
//
//   log-mel   reflect-padded clips as overlapping rows (pitch 160) x [window * DFT basis] on the fp32 MFMA core (re, im pairs ->
//             power), x Slaney mel bank -> log10, transposed store; per-clip max, clamp at max - 8, (x + 4) / 4
//   encoder   conv1 / conv2 as GEMMs over channel-last rows with a zero frame on either side (taps contiguous, conv2 at row pitch
//             2 d), GELU, + positions; L pre-LN layers: LayerNorm rows, q / k / v / out / fc1 / fc2 through linear_f32, attention
//             as one streaming-softmax kernel (no score map is ever stored); final LayerNorm; the cross K / V of every decoder layer
//   decode    one loop (wh_decode_run) behind tdx_whisper_decode, tdx_whisper_decode_xattn and tdx_whisper_decode_ts; the first two
//             are the third with the same prefix in every row, begin = prefix_len and the timestamp rules off.
//             One token per clip per step, B <= 32, state on the device (cur_tok, pos, done, and per row its prefix, its last
//             step and the rules' history: WhState): embed; per layer a skinny Linear
//             launch for q | k | v (k, v land in the cache row `pos`), single-query attention in key chunks of 256 + a combine,
//             out_proj + residual, the same for the cross attention over the precomputed K / V, fc1 + GELU, fc2 + residual; the
//             vocabulary head in 64-column slices (max, argmax, sum exp per row and slice, suppression mask applied, logits never
//             stored; wh_head_kernel<BT, TS>: TS = false keeps one running triple per thread, TS = true the rules' two classes
//             and the no-speech pair; SAMPLE = true, tdx_whisper_decode_ts_sample, also a draw from softmax(logits / T) per row by
//             the Gumbel-max trick) and one combine launch that writes the per-position outputs, the next token, pos + 1
//             and the done flags.  The host enqueues 16 steps at a time and then reads one pinned word (the number of finished clips).
//   times     word timestamps: a capturing call is the same loop plus, per layer with a listed alignment head,
//             one launch that writes the head's softmax row over the encoder positions; tdx_token_align normalises those rows over
//             the tokens, median-filters along the frames, averages the heads and runs the dynamic time warping of a clip in one
//             workgroup along the anti-diagonals (transformers' _extract_token_timestamps).
//
// Skinny Linear (wh_skinny_kernel): a workgroup owns 4 output columns; its 4 waves split K in interleaved 256-float chunks, a
// lane keeps B x 4 accumulators (plain fp32 FMA; every weight element is loaded once for all B rows), the 64 lanes meet in a
// transposing butterfly (126 exchanges for 128 sums), the 4 waves in LDS.  The summation order of an output element is the same
// whatever B is and whichever rows share the launch, so a clip decoded alone gives the bits it gives in a batch.  From 9 rows on
// the Linear runs on MFMA tiles instead (wh_skinny_mfma_kernel + wh_sk_finish_kernel, further down), with the same property.
#include <climits>
#include <cmath>
#include <cstdlib>

#include "dft_basis.hpp"
#include "epilogues.hpp"
#include "whisper_noise.hpp"

using namespace tdx;

namespace {

constexpr int DK = 64;                                   // head width of every Whisper size
constexpr int NFFT = 400, HOP = 160, NBIN = 201;
constexpr int NBINP = 256;                               // bins padded to the paired GEMM's 64-column tiles
constexpr int KFR = 416;                                 // frame length padded to a multiple of 32 (basis columns 400.. are zero)
constexpr int PWP = 224;                                 // pitch of the power rows (columns 201.. are exact zeros)
constexpr int MELP = 128;                                // mel rows of the filter bank image (rows n_mels.. are zero)
constexpr int WH_MAXB = 32, WH_CHUNK = 16;               // clips per decode call; steps enqueued between two host reads
constexpr int WH_SLICE = 64;                             // vocabulary columns per head workgroup
constexpr int WH_KEYS = 256;                             // keys per single-query attention workgroup
constexpr int WH_MAXCTX = 1 << 15;
constexpr int WH_XROW_LDS = 4096;                         // scores of that many encoder positions stay in LDS
constexpr int WH_XROW_NT = 1024;                          // threads of the alignment heads' softmax workgroup
constexpr int WH_MAXHEADS = 64;                           // alignment heads of a capturing decode
constexpr float LN_EPS = 1e-5f;

__device__ __forceinline__ float gelu_erf(float v) { return ActGelu::f(v); }

// ------------------------------------------------------------------------------------------------ log-mel
// the clip cut / zero-padded to P samples, reflect-padded by 200 on either side, then zeros up to the row pitch
__global__ __launch_bounds__(256) void wh_pad_kernel(const float* __restrict__ wav, const int* __restrict__ lens, long N, int P, int pitch,
                                                      float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= pitch) return;
    long n = lens ? (long)lens[b] : N;
    n = n < 0 ? 0 : (n > N ? N : n);
    float v = 0.f;
    if (i < P + NFFT) {
        int j = i - NFFT / 2;
        if (j < 0) j = -j;
        if (j >= P) j = 2 * (P - 1) - j;
        if (j < n) v = wav[(long)b * N + j];
    }
    out[(long)b * pitch + i] = v;
}
struct EpiPow {
    float* pw;
    __device__ EpiNone col(int, int) const { return EpiNone{}; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store2(int, int m, int c, float re, float im, EpiNone, EpiNone) const {
        if (c < PWP) pw[(long)m * PWP + c] = re * re + im * im;
    }
};
// row m = rp * b + f is frame f of clip b when f < T; feat [B][n_mels][T]
struct EpiLogMelT {
    float* feat; int rp, T, n_mels;
    __device__ EpiNone col(int, int) const { return EpiNone{}; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int, int m, int n, float v, EpiNone, EpiNone) const {
        const int b = m / rp, f = m - b * rp;
        if (f < T && n < n_mels) feat[((long)b * n_mels + n) * T + f] = v > 1e-10f ? log10f(v) : -10.0f;      // the floor is exact: log10f(1e-10f) is not
    }
};
// per clip: the maximum of the whole map, then max(x, max - 8) -> (x + 4) / 4
__global__ __launch_bounds__(1024) void wh_clamp_kernel(float* __restrict__ feat, long n) {
    __shared__ float red[16];
    float* x = feat + (long)blockIdx.x * n;
    const int tid = threadIdx.x;
    float mx = -INFINITY;
    for (long i = tid; i < n; i += 1024) mx = fmaxf(mx, x[i]);
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = red[0];
    for (int w = 1; w < 16; ++w) mx = fmaxf(mx, red[w]);
    const float lo = mx - 8.0f;
    for (long i = tid; i < n; i += 1024) x[i] = (fmaxf(x[i], lo) + 4.0f) / 4.0f;
}
// tdx_whisper_logmel_long: `count` samples of the reflect-padded clip from padded index s0 on (padded index q is clip index
// q - 200, mirrored about 0 and N - 1 as often as it takes, like numpy's reflect); zeros past the padded clip.  N >= 2.
__global__ __launch_bounds__(256) void wh_pad_long_kernel(const float* __restrict__ wav, long N, long s0, int count, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const long q = s0 + i;
    float v = 0.f;
    if (q < N + NFFT) {
        const long period = 2 * (N - 1);
        long j = (q - NFFT / 2) % period;
        if (j < 0) j += period;
        if (j >= N) j = period - j;
        v = wav[j];
    }
    out[i] = v;
}
// the maximum of a whole clip's map in two launches: WH_MAXPART partial maxima, then every workgroup joins them and clamps its share
constexpr int WH_MAXPART = 256;
__global__ __launch_bounds__(1024) void wh_max_part_kernel(const float* __restrict__ x, long n, float* __restrict__ part) {
    __shared__ float red[16];
    const int tid = threadIdx.x;
    float mx = -INFINITY;
    for (long i = (long)blockIdx.x * 1024 + tid; i < n; i += (long)gridDim.x * 1024) mx = fmaxf(mx, x[i]);
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
        mx = red[0];
        for (int w = 1; w < 16; ++w) mx = fmaxf(mx, red[w]);
        part[blockIdx.x] = mx;
    }
}
__global__ __launch_bounds__(1024) void wh_clamp_long_kernel(float* __restrict__ x, long n, const float* __restrict__ part) {
    __shared__ float red[16];
    const int tid = threadIdx.x;
    float mx = tid < WH_MAXPART ? part[tid] : -INFINITY;
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = red[0];
    for (int w = 1; w < 16; ++w) mx = fmaxf(mx, red[w]);
    const float lo = mx - 8.0f;
    for (long i = (long)blockIdx.x * 1024 + tid; i < n; i += (long)gridDim.x * 1024) x[i] = (fmaxf(x[i], lo) + 4.0f) / 4.0f;
}

// ------------------------------------------------------------------------------------------------ encoder
// feat [B][n_mels][T] -> channel-last rows [B][T + 2][MP] with a zero frame on either side and zero channels n_mels..MP-1
__global__ void wh_chlast_kernel(const float* __restrict__ feat, int n_mels, int T, int MP, float* __restrict__ xc) {
    const int r = blockIdx.x, b = blockIdx.y, c = threadIdx.x;
    float v = 0.f;
    if (r >= 1 && r <= T && c < n_mels) v = feat[((long)b * n_mels + c) * T + r - 1];
    xc[((long)b * (T + 2) + r) * MP + c] = v;
}
// rows 0 and T + 1 of every clip of c1 [B][T + 2][d]
__global__ void wh_zero_edge_kernel(float* __restrict__ c1, int T, int d) {
    float* p = c1 + ((long)blockIdx.y * (T + 2) + (blockIdx.x ? T + 1 : 0)) * d;
    for (int i = threadIdx.x; i < d; i += blockDim.x) p[i] = 0.f;
}
// conv1: GEMM row m = (T + 2) b + t -> c1 row (T + 2) b + t + 1
struct EpiConv1 {
    const float* b; float* out; int T, d;
    __device__ float col(int, int n) const { return n < d ? b[n] : 0.f; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int, int m, int n, float v, EpiNone, float c) const {
        const int bi = m / (T + 2), t = m - bi * (T + 2);
        if (t < T && n < d) out[((long)bi * (T + 2) + t + 1) * d + n] = gelu_erf(v + c);
    }
};
// conv2: GEMM row m = (S + 1) b + t -> x row S b + t, + the position row t
struct EpiConv2 {
    const float* b; const float* pos; float* out; int S, d;
    __device__ float col(int, int n) const { return n < d ? b[n] : 0.f; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int, int m, int n, float v, EpiNone, float c) const {
        const int bi = m / (S + 1), t = m - bi * (S + 1);
        if (t < S && n < d) out[((long)bi * S + t) * d + n] = gelu_erf(v + c) + pos[(long)t * d + n];
    }
};
// LayerNorm of rows of d floats (d % 4 == 0), one wave per row, two passes (mean, then the centred squares)
__global__ __launch_bounds__(256) void wh_ln_rows_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ be,
                                                          float* __restrict__ y, long M, int d) {
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (m >= M) return;
    const float* xr = x + m * d;
    float s = 0.f;
    for (int k = 4 * lane; k < d; k += 256) { const f32x4 v = ldg4(xr + k); s += (v[0] + v[1]) + (v[2] + v[3]); }
    const float mean = wave_sum(s) / (float)d;
    float q = 0.f;
    for (int k = 4 * lane; k < d; k += 256) {
        const f32x4 v = ldg4(xr + k);
        const float a0 = v[0] - mean, a1 = v[1] - mean, a2 = v[2] - mean, a3 = v[3] - mean;
        q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + LN_EPS);
    for (int k = 4 * lane; k < d; k += 256) {
        const f32x4 v = ldg4(xr + k), gv = ldg4(g + k), bv = ldg4(be + k);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf((v[j] - mean) * rstd, gv[j], bv[j]);
        *reinterpret_cast<f32x4*>(y + m * d + k) = o;
    }
}
// Full softmax attention over S keys, head width 64, q scaled by 1/8 on load.  Workgroup (qt, h, b): 64 queries; thread
// (query t >> 2, part t & 3) owns 16 of the 64 dimensions of its query and of its output; a 64-key tile of K and V sits in LDS
// (every lane of a quad reads the same key row: broadcasts); the four parts of a score meet in two DPP quad exchanges; the
// softmax streams in chunks of 8 keys with a running maximum, so no score leaves the registers.
__global__ __launch_bounds__(256) void wh_enc_attn_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                           float* __restrict__ out, int S, int d) {
    __shared__ __attribute__((aligned(16))) float Ks[64 * DK];
    __shared__ __attribute__((aligned(16))) float Vs[64 * DK];
    const int tid = threadIdx.x, qi = tid >> 2, p = tid & 3;
    const int h = blockIdx.y, b = blockIdx.z;
    const int qg = blockIdx.x * 64 + qi;
    const long base = (long)b * S * d + (long)h * DK;
    float qv[16], acc[16];
    {
        const float* qr = q + base + (long)min(qg, S - 1) * d + 16 * p;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 t = ldg4(qr + 4 * i);
#pragma unroll
            for (int j = 0; j < 4; ++j) { qv[4 * i + j] = t[j] * 0.125f; acc[4 * i + j] = 0.f; }
        }
    }
    float mrun = -INFINITY, lrun = 0.f;
    for (int k0 = 0; k0 < S; k0 += 64) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, r = e >> 4, c = (e & 15) * 4;
            const long off = base + (long)min(k0 + r, S - 1) * d + c;
            *reinterpret_cast<f32x4*>(Ks + r * DK + c) = ldg4(k + off);
            *reinterpret_cast<f32x4*>(Vs + r * DK + c) = ldg4(v + off);
        }
        __syncthreads();
#pragma unroll 1
        for (int j0 = 0; j0 < 64 && k0 + j0 < S; j0 += 8) {
            float s[8];
            float cm = -INFINITY;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const float* kr = Ks + (j0 + jj) * DK + 16 * p;
                float a = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(kr + 4 * i);
#pragma unroll
                    for (int j = 0; j < 4; ++j) a = fmaf(qv[4 * i + j], t[j], a);
                }
                a += h3_dpp(a, 0);
                a += h3_dpp(a, 1);
                s[jj] = (k0 + j0 + jj < S) ? a : -INFINITY;
                cm = fmaxf(cm, s[jj]);
            }
            if (cm > mrun) {
                const float sc = expf(mrun - cm);
                lrun *= sc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] *= sc;
                mrun = cm;
            }
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const float pj = expf(s[jj] - mrun);
                lrun += pj;
                const float* vr = Vs + (j0 + jj) * DK + 16 * p;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(vr + 4 * i);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[4 * i + j] = fmaf(pj, t[j], acc[4 * i + j]);
                }
            }
        }
    }
    if (qg < S) {
        float* o = out + base + (long)qg * d + 16 * p;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f32x4 t;
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = acc[4 * i + j] / lrun;
            *reinterpret_cast<f32x4*>(o + 4 * i) = t;
        }
    }
}

// ------------------------------------------------------------------------------------------------ decode step
__global__ __launch_bounds__(256) void wh_embed_kernel(const float* __restrict__ tok, const float* __restrict__ pe, const int* __restrict__ cur,
                                                        const int* __restrict__ pos, float* __restrict__ x, int d) {
    const int b = blockIdx.x;
    const float* t = tok + (long)cur[b] * d;
    const float* p = pe + (long)pos[b] * d;
    for (int i = threadIdx.x; i < d; i += 256) x[(long)b * d + i] = t[i] + p[i];
}

// one output of a skinny launch: y[row(b)][n] = act((x . W[n]) + bias[n]) + res[b][n]; row(b) = b, or brow * b + pos[b]
// (the cache row of the token being decoded) when brow > 0
struct SkJob { const float* W; const float* bias; const float* res; float* y; long ld; int brow; int gelu; };
struct SkArgs { const float* x; const float* lng; const float* lnb; const int* pos; int B, N, K; SkJob job[3]; };

// LayerNorm statistics of the B rows into LDS (mean, 1 / std): wave w takes the rows w, w + 4, ... and walks them together, so
// that the loads of its (up to 8) rows are in flight at once; per row the sums run over k in ascending order
__device__ __forceinline__ void sk_stats(const SkArgs& a, float* stat, int wave, int lane) {
    constexpr int R = WH_MAXB / 4;
    float s[R], mean[R], q[R];
#pragma unroll
    for (int i = 0; i < R; ++i) { s[i] = 0.f; q[i] = 0.f; }
    for (int k = 4 * lane; k < a.K; k += 256)
#pragma unroll
        for (int i = 0; i < R; ++i)
            if (wave + 4 * i < a.B) { const f32x4 v = ldg4(a.x + (long)(wave + 4 * i) * a.K + k); s[i] += (v[0] + v[1]) + (v[2] + v[3]); }
#pragma unroll
    for (int i = 0; i < R; ++i) mean[i] = wave_sum(s[i]) / (float)a.K;
    for (int k = 4 * lane; k < a.K; k += 256)
#pragma unroll
        for (int i = 0; i < R; ++i)
            if (wave + 4 * i < a.B) {
                const f32x4 v = ldg4(a.x + (long)(wave + 4 * i) * a.K + k);
                const float a0 = v[0] - mean[i], a1 = v[1] - mean[i], a2 = v[2] - mean[i], a3 = v[3] - mean[i];
                q[i] += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
            }
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const float rstd = 1.0f / sqrtf(wave_sum(q[i]) / (float)a.K + LN_EPS);
        if (lane == 0 && wave + 4 * i < a.B) { stat[2 * (wave + 4 * i)] = mean[i]; stat[2 * (wave + 4 * i) + 1] = rstd; }
    }
}
// acc[4 b + c] += sum over this wave's k of LN?(x)[b][k] * W[n0 + c][k]; wave w owns the 256-float chunks w, w + 4, ...
template <int BT>
__device__ __forceinline__ void sk_accumulate(const SkArgs& a, const float* __restrict__ W, int n0, const float* stat, int wave, int lane, float (&acc)[4 * BT]) {
    const float* Wr[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) Wr[c] = W + (long)min(n0 + c, a.N - 1) * a.K;
    const bool ln = a.lng != nullptr;
    for (int k = (wave * 64 + lane) * 4; k < a.K; k += 1024) {
        f32x4 wv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) wv[c] = ldg4(Wr[c] + k);
        f32x4 g{1.f, 1.f, 1.f, 1.f}, be{0.f, 0.f, 0.f, 0.f};
        if (ln) { g = ldg4(a.lng + k); be = ldg4(a.lnb + k); }
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            f32x4 xv = ldg4(a.x + (long)min(b, a.B - 1) * a.K + k);
            if (ln) {
                const float mean = stat[2 * min(b, a.B - 1)], rstd = stat[2 * min(b, a.B - 1) + 1];
#pragma unroll
                for (int j = 0; j < 4; ++j) xv[j] = fmaf((xv[j] - mean) * rstd, g[j], be[j]);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[4 * b + c] = fmaf(xv[j], wv[c][j], acc[4 * b + c]);
        }
    }
}
// Sums NV values per lane over the 64 lanes.  While more than one value is left a step halves them: a lane keeps the half its
// bit M selects and receives the partner's sums for it; the remaining steps are plain exchanges.  A sum is the same tree over
// the lanes (masks 32, 16, ... 1) wherever in the array it sits.  Lanes whose `writer` stays set hold values idx .. idx + N - 1.
template <int N, int M>
__device__ __forceinline__ void sk_butterfly(float* v, int lane, int& idx, bool& writer, int& nleft) {
    if constexpr (M == 0) { nleft = N; }
    else {
        const bool up = (lane & M) != 0;
        if constexpr (N > 1) {
            constexpr int H = N / 2;
#pragma unroll
            for (int i = 0; i < H; ++i) {
                const float send = up ? v[i] : v[i + H], keep = up ? v[i + H] : v[i];
                v[i] = keep + __shfl_xor(send, M, 64);
            }
            if (up) idx += H;
            sk_butterfly<H, M / 2>(v, lane, idx, writer, nleft);
        } else {
            v[0] += __shfl_xor(v[0], M, 64);
            if (up) writer = false;
            sk_butterfly<1, M / 2>(v, lane, idx, writer, nleft);
        }
    }
}
template <int BT>
__device__ __forceinline__ void sk_reduce_to_lds(float (&acc)[4 * BT], int lane, float* out) {
    int idx = 0, nleft = 0;
    bool writer = true;
    sk_butterfly<4 * BT, 32>(acc, lane, idx, writer, nleft);
    if (writer) {
        if constexpr (4 * BT >= 128) { out[idx] = acc[0]; out[idx + 1] = acc[1]; }
        else out[idx] = acc[0];
    }
}

// grid (ceil(N / 4), jobs)
template <int BT>
__global__ __launch_bounds__(256) void wh_skinny_kernel(SkArgs a) {
    __shared__ float stat[2 * WH_MAXB];
    __shared__ float red[4][4 * BT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SkJob& jb = a.job[blockIdx.y];
    const int n0 = blockIdx.x * 4;
    if (a.lng) { sk_stats(a, stat, wave, lane); __syncthreads(); }
    float acc[4 * BT];
#pragma unroll
    for (int i = 0; i < 4 * BT; ++i) acc[i] = 0.f;
    sk_accumulate<BT>(a, jb.W, n0, stat, wave, lane, acc);
    sk_reduce_to_lds<BT>(acc, lane, red[wave]);
    __syncthreads();
    for (int e = tid; e < 4 * BT; e += 256) {
        const int b = e >> 2, n = n0 + (e & 3);
        if (b >= a.B || n >= a.N) continue;
        float v = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
        v += jb.bias ? jb.bias[n] : 0.f;
        if (jb.gelu) v = gelu_erf(v);
        if (jb.res) v += jb.res[(long)b * a.N + n];
        const long row = jb.brow > 0 ? (long)jb.brow * b + a.pos[b] : b;
        jb.y[row * jb.ld + n] = v;
    }
}

// Skinny Linear for 9..32 rows.  At that many rows an fp32-FMA lane would need 128 accumulators and 32 loads of x per weight
// load; here the rows are one operand of v_mfma_f32_32x32x2_f32 (exact fp32 products; operand map of gemm.hpp / sensevoice.hip:
// lane l supplies x[row l&31][k] and W[col l&31][k] for the four k = 8 kc + 4 (l>>5) + j of one 16-byte load), so a wave keeps 16
// accumulators and reads as many bytes of x (from L2) as of W.  Workgroup (column tile of 32, K split s, job): its 4 waves take
// the 8-float k blocks kc = 4 s + w, + 4 KS, ...; the waves meet in LDS and one partial [32][32] goes to the workspace.
// wh_sk_finish_kernel adds the KS partials in order and applies bias / GELU / residual / the cache row.  KS depends on N and K
// only, x is LayerNorm'ed once by wh_ln_rows_kernel: a row's bits do not depend on the other rows of the launch.
constexpr int SKM_PITCH = 33;
__global__ __launch_bounds__(256) void wh_skinny_mfma_kernel(SkArgs a, int KS, float* __restrict__ partial) {
    __shared__ float red[4][32 * SKM_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const int n0 = blockIdx.x * 32, s = blockIdx.y, job = blockIdx.z;
    const float* __restrict__ W = a.job[job].W;
    const float* const xr = a.x + (long)min(l31, a.B - 1) * a.K + 4 * hh;
    const float* const wr = W + (long)min(n0 + l31, a.N - 1) * a.K + 4 * hh;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int nkc = a.K >> 3;
#pragma unroll 4
    for (int kc = 4 * s + wave; kc < nkc; kc += 4 * KS) {
        const f32x4 av = ldg4(xr + 8 * kc), bv = ldg4(wr + 8 * kc);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc, 0, 0, 0);
    }
    // D: col = l31, row = (r&3) + 8*(r>>2) + 4*hh
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][((r & 3) + 8 * (r >> 2) + 4 * hh) * SKM_PITCH + l31] = acc[r];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = tid + 256 * i, row = e >> 5, col = e & 31, o = row * SKM_PITCH + col;
        if (row < a.B && n0 + col < a.N)
            partial[(((long)job * KS + s) * WH_MAXB + row) * a.N + n0 + col] = ((red[0][o] + red[1][o]) + red[2][o]) + red[3][o];
    }
}
// grid (ceil(B N / 256), jobs)
__global__ __launch_bounds__(256) void wh_sk_finish_kernel(SkArgs a, int KS, const float* __restrict__ partial) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)a.B * a.N) return;
    const int b = (int)(e / a.N), n = (int)(e - (long)b * a.N), job = blockIdx.y;
    const SkJob& jb = a.job[job];
    float v = 0.f;
    for (int s = 0; s < KS; ++s) v += partial[(((long)job * KS + s) * WH_MAXB + b) * a.N + n];
    v += jb.bias ? jb.bias[n] : 0.f;
    if (jb.gelu) v = gelu_erf(v);
    if (jb.res) v += jb.res[(long)b * a.N + n];
    const long row = jb.brow > 0 ? (long)jb.brow * b + a.pos[b] : b;
    jb.y[row * jb.ld + n] = v;
}
constexpr int SKM_MAXKS = 8;
inline int skm_splits(int N, int K) {          // enough workgroups to pull on every CU; at least one k block per wave
    const int tiles = (N + 31) / 32;
    return std::max(1, std::min(std::min(SKM_MAXKS, (256 + tiles - 1) / tiles), K / 32));
}

// (max, argmax, sum of exp(v - max)) of a set of logits; the empty set is (-inf, INT_MAX, 0).  Ties: the lowest id, like torch.argmax.
struct WhTop { float m; int i; float s; };
__device__ __forceinline__ void wh_merge(WhTop& a, const WhTop& b) {
    if (b.i == INT_MAX) return;
    if (a.i == INT_MAX) { a = b; return; }
    const float mx = fmaxf(a.m, b.m);
    a.s = a.s * expf(a.m - mx) + b.s * expf(b.m - mx);
    if (b.m > a.m || (b.m == a.m && b.i < a.i)) a.i = b.i;
    a.m = mx;
}
// what the vocabulary head hands to wh_next_kernel
struct WhHeadOut { float* pm; int* pi; float* ps; float* nm; float* nsum; float* nlogit; };
// Sampled decoding (tdx_whisper_decode_ts_sample).  temp [B] (0: the row decodes greedily), stream [B] on the device;
// zm / zi / zv [cls][B][nsl]: per class, row and slice the record of the perturbed maximum.  The sampling instantiations are launched
// only when some row has temp > 0: a call whose temperatures are all 0 runs the greedy kernels.
struct WhSample { const float* temp; const unsigned long long* stream; unsigned long long seed; float* zm; int* zi; float* zv; };
// (max z, its id, the raw logit of that id) over a set of ids; the empty set is (-inf, INT_MAX, 0).  Ties in z: the lowest id.  Only
// comparisons: joining records gives the same result in any order.
struct WhDraw { float z; int i; float v; };
__device__ __forceinline__ void wh_draw_add(WhDraw& a, const WhDraw& b) {
    if (b.i != INT_MAX && (a.i == INT_MAX || b.z > a.z || (b.z == a.z && b.i < a.i))) a = b;
}
__device__ __forceinline__ void wh_top_add(WhTop& top, float v, int n) {
    if (top.i == INT_MAX) top = WhTop{v, n, 1.f};
    else if (v > top.m) { top.s = top.s * expf(top.m - v) + 1.f; top.m = v; top.i = n; }
    else top.s += expf(v - top.m);
}
// Vocabulary head: workgroup s sweeps columns [64 s, 64 s + 64) four at a time through the skinny Linear's loop (W = the token
// embedding, no bias); thread (b, c) keeps the running triples of row b over its columns; one triple per (class, row, slice) goes
// out, pm / pi / ps [cls][B][nsl].  mask[n] bit 0: suppressed at every step, bit 1: suppressed for the rows whose `first` is set.
// bnd [4][WH_MAXB] (the device state's TS_BND rows): text_lo, ts_lo, ts_hi, first.
// TS = false (tdx_whisper_decode, tdx_whisper_decode_xattn: the rules are off): one triple over every id the mask allows, one class.
// TS = true (tdx_whisper_decode_ts): id n < tb is allowed when n >= text_lo and n != tb - 1 (<|notimestamps|>), id n >= tb when
// ts_lo <= n <= ts_hi; class 0 over the allowed ids below tb, class 1 over those from tb up (a slice can hold both).  want_ns: a
// third pair (max, sum exp) over every id of the slice, no mask, and the logit of id ns_id.
// SAMPLE (tdx_whisper_decode_ts_sample, with TS): a row with temp[b] > 0 also keeps, per class, the record (max z, its id, that id's
// raw logit v) of z = v / temp[b] + g over exactly the ids the class's triple admits; g is the noise of whisper_noise.hpp at the
// position pos[b] + 1 of the id being chosen.  All 256 threads compute the slice's noise into LDS ahead of the column loop (16
// Philox calls per sampling row), so none of it sits in the serial epilogue of a group of four columns.  Ties in z: the lowest id.
template <int BT, bool TS, bool SAMPLE>
__global__ __launch_bounds__(256) void wh_head_kernel(SkArgs a, const unsigned char* __restrict__ mask, const int* __restrict__ bnd, int tb, int want_ns,
                                                       int ns_id, WhHeadOut o, int nsl, WhSample sp) {
    static_assert(TS || !SAMPLE, "sampling runs under the timestamp rules");
    constexpr int NC = TS ? 3 : 1;
    __shared__ float stat[2 * WH_MAXB];
    __shared__ float red[4][4 * BT];
    __shared__ float tm[NC][4 * BT], tsum[NC][4 * BT];
    __shared__ int ti[NC][4 * BT];
    __shared__ float gn[SAMPLE ? BT : 1][WH_SLICE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if constexpr (SAMPLE) {
        for (int e = tid; e < BT * (WH_SLICE / 4); e += 256) {
            const int b = e / (WH_SLICE / 4), q = e % (WH_SLICE / 4);
            if (b < a.B && sp.temp[b] > 0.f) {
                const Philox4 r = wh_noise_words(sp.seed, sp.stream[b], a.pos[b] + 1, blockIdx.x * (WH_SLICE / 4) + q);
#pragma unroll
                for (int c = 0; c < 4; ++c) gn[b][4 * q + c] = wh_gumbel(r.w[c]);
            }
        }
        __syncthreads();
    }
    if (a.lng) { sk_stats(a, stat, wave, lane); __syncthreads(); }
    const int rb = min(tid >> 2, a.B - 1);
    const int text_lo = TS ? bnd[rb] : 0, ts_lo = TS ? bnd[WH_MAXB + rb] : 0, ts_hi = TS ? bnd[2 * WH_MAXB + rb] : 0;
    const int deny = bnd[3 * WH_MAXB + rb] ? 3 : 1;
    WhTop top[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) top[k] = WhTop{-INFINITY, INT_MAX, 0.f};
    WhDraw zt[2] = {WhDraw{-INFINITY, INT_MAX, 0.f}, WhDraw{-INFINITY, INT_MAX, 0.f}};
    float temp = 0.f;
    if constexpr (SAMPLE) temp = sp.temp[rb];
    for (int g = 0; g < WH_SLICE / 4; ++g) {
        const int n0 = blockIdx.x * WH_SLICE + 4 * g;
        if (n0 >= a.N) break;                                       // (uniform over the workgroup)
        float acc[4 * BT];
#pragma unroll
        for (int i = 0; i < 4 * BT; ++i) acc[i] = 0.f;
        sk_accumulate<BT>(a, a.job[0].W, n0, stat, wave, lane, acc);
        sk_reduce_to_lds<BT>(acc, lane, red[wave]);
        __syncthreads();
        if (tid < 4 * BT) {
            const int n = n0 + (tid & 3);
            if (n < a.N) {
                const float v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
                if constexpr (TS) {
                    if (want_ns) {
                        wh_top_add(top[2], v, 0);
                        if (n == ns_id && (tid >> 2) < a.B) o.nlogit[tid >> 2] = v;
                    }
                    const bool ok = n < tb ? (n >= text_lo && n != tb - 1) : (n >= ts_lo && n <= ts_hi);
                    if (ok && !(mask[n] & deny)) {
                        wh_top_add(top[n < tb ? 0 : 1], v, n);
                        if constexpr (SAMPLE) {
                            if (temp > 0.f) wh_draw_add(zt[n < tb ? 0 : 1], WhDraw{v / temp + gn[rb][4 * g + (tid & 3)], n, v});
                        }
                    }
                } else {
                    if (!(mask[n] & deny)) wh_top_add(top[0], v, n);
                }
            }
        }
        __syncthreads();
    }
    if (tid < 4 * BT)
#pragma unroll
        for (int k = 0; k < NC; ++k) { tm[k][tid] = top[k].m; ti[k][tid] = top[k].i; tsum[k][tid] = top[k].s; }
    __syncthreads();
    if (tid < BT && tid < a.B) {
        for (int k = 0; k < (TS ? (want_ns ? 3 : 2) : 1); ++k) {
            WhTop t{-INFINITY, INT_MAX, 0.f};
            for (int c = 0; c < 4; ++c) wh_merge(t, WhTop{tm[k][4 * tid + c], ti[k][4 * tid + c], tsum[k][4 * tid + c]});
            if (k < 2) {
                const long q = ((long)k * a.B + tid) * nsl + blockIdx.x;
                o.pm[q] = t.m; o.pi[q] = t.i; o.ps[q] = t.s;
            } else {
                const long q = (long)tid * nsl + blockIdx.x;
                o.nm[q] = t.m; o.nsum[q] = t.s;
            }
        }
    }
    if constexpr (SAMPLE) {
        __syncthreads();                                            // tm / ti / tsum have been read: their first two classes carry the records
        if (tid < 4 * BT)
#pragma unroll
            for (int k = 0; k < 2; ++k) { tm[k][tid] = zt[k].z; ti[k][tid] = zt[k].i; tsum[k][tid] = zt[k].v; }
        __syncthreads();
        if (tid < BT && tid < a.B) {
            for (int k = 0; k < 2; ++k) {
                WhDraw t{-INFINITY, INT_MAX, 0.f};
                for (int c = 0; c < 4; ++c) wh_draw_add(t, WhDraw{tm[k][4 * tid + c], ti[k][4 * tid + c], tsum[k][4 * tid + c]});
                const long q = ((long)k * a.B + tid) * nsl + blockIdx.x;
                sp.zm[q] = t.z; sp.zi[q] = t.i; sp.zv[q] = t.v;
            }
        }
    }
}

// Decode state on the device.  prefix [B][T]: every row's own prefix.  ti [WH_TS_ROWS][WH_MAXB] ints: the host fills the first six
// rows (a row's prefix length, where its history starts, its last step, the last position it may generate, the position of
// <|startoftranscript|> or -1, the first captured position); the kernels own the rest (the history and the allowed intervals of
// Whisper's timestamp rules, transformers' WhisperTimeStampLogitsProcessor).
struct WhState { int* cur; int* pos; int* done; int* ndone; const int* prefix; int* ti; };
enum { TS_PLEN = 0, TS_BEGIN, TS_PEND, TS_GENTO, TS_SOT, TS_FIRSTROW, TS_H1, TS_H2, TS_HN, TS_LAST, TS_BND, WH_TS_ROWS = TS_BND + 4 };
// on = 0: no timestamp rules (tdx_whisper_decode, tdx_whisper_decode_xattn); tb, V and max_init are then not read
struct WhTsRules { int on, tb, eos, V, max_init; };
// the allowed intervals of the step that predicts the id after the history (h1 = its last id, h2 = the one before, hn = its
// length capped at 2, last = its last timestamp id or -1); first: the history is empty and the id is the first generated one.
// Rules off: every text id, no timestamp id.
__device__ __forceinline__ void wh_ts_bounds(int* __restrict__ ti, int b, bool first, WhTsRules r) {
    int text_lo = 0, ts_lo = INT_MAX, ts_hi = -1;
    if (r.on) {
        const int hn = ti[TS_HN * WH_MAXB + b], h1 = ti[TS_H1 * WH_MAXB + b], h2 = ti[TS_H2 * WH_MAXB + b], last = ti[TS_LAST * WH_MAXB + b];
        ts_lo = r.tb; ts_hi = r.V - 1;
        const bool last_ts = hn >= 1 && h1 >= r.tb, pen_ts = hn < 2 || h2 >= r.tb;
        if (last_ts) { if (pen_ts) ts_lo = INT_MAX; else text_lo = r.eos; }
        if (last >= 0) ts_lo = max(ts_lo, (last_ts && !pen_ts) ? last : last + 1);
        if (first) { text_lo = INT_MAX; if (r.max_init >= 0) ts_hi = min(ts_hi, r.tb + r.max_init); }
    }
    int* bnd = ti + TS_BND * WH_MAXB;
    bnd[b] = text_lo; bnd[WH_MAXB + b] = ts_lo; bnd[2 * WH_MAXB + b] = ts_hi; bnd[3 * WH_MAXB + b] = first ? 1 : 0;
}
__device__ __forceinline__ void wh_ts_push(int* __restrict__ ti, int b, int id, int tb) {
    ti[TS_H2 * WH_MAXB + b] = ti[TS_H1 * WH_MAXB + b];
    ti[TS_H1 * WH_MAXB + b] = id;
    ti[TS_HN * WH_MAXB + b] = min(ti[TS_HN * WH_MAXB + b] + 1, 2);
    if (id >= tb) ti[TS_LAST * WH_MAXB + b] = id;
}
__global__ void wh_init_kernel(WhState s, int B, int T, WhTsRules r, int* __restrict__ counts) {
    const int b = threadIdx.x;
    int* ti = s.ti;
    if (b < B) {
        s.cur[b] = s.prefix[(long)b * T]; s.pos[b] = 0; s.done[b] = 0; counts[b] = 0;
        ti[TS_HN * WH_MAXB + b] = 0; ti[TS_H1 * WH_MAXB + b] = -1; ti[TS_H2 * WH_MAXB + b] = -1; ti[TS_LAST * WH_MAXB + b] = -1;
        wh_ts_bounds(ti, b, ti[TS_BEGIN * WH_MAXB + b] == 1, r);
    }
    if (b == 0) *s.ndone = 0;
}
// the slices of a row -> one triple; 32 lanes per clip
__device__ __forceinline__ WhTop wh_join_slices(const float* __restrict__ pm, const int* __restrict__ pi, const float* __restrict__ ps, long row, int nsl, int l) {
    WhTop t{-INFINITY, INT_MAX, 0.f};
    for (int j = l; j < nsl; j += 32) wh_merge(t, WhTop{pm[row * nsl + j], pi ? pi[row * nsl + j] : 0, ps[row * nsl + j]});
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) {
        WhTop u{__shfl_xor(t.m, o, 64), __shfl_xor(t.i, o, 64), __shfl_xor(t.s, o, 64)};
        // both partners must end with the same triple: merge (lower lane's, upper lane's) in that order on both
        WhTop lo = (l & o) ? u : t, hi = (l & o) ? t : u;
        wh_merge(lo, hi);
        t = lo;
    }
    return t;
}
// the slices' records of a row's two classes (rows r0, r1 of zm / zi / zv) -> one each; 32 lanes per clip.  A lane has the loads of
// WH_JOIN slices of both classes in flight at once: one slice per trip made the join a chain of load latencies (26 trips at 811
// slices, 26 us per step at the large-v3 vocabulary).
constexpr int WH_JOIN = 8;
__device__ __forceinline__ void wh_join_draws(const WhSample& sp, long r0, long r1, int nsl, int l, WhDraw& t0, WhDraw& t1) {
    for (int j0 = l; j0 < nsl; j0 += 32 * WH_JOIN) {
        WhDraw a[WH_JOIN], b[WH_JOIN];
#pragma unroll
        for (int u = 0; u < WH_JOIN; ++u) {
            const int j = j0 + 32 * u;
            a[u] = b[u] = WhDraw{-INFINITY, INT_MAX, 0.f};
            if (j < nsl) {
                a[u] = WhDraw{sp.zm[r0 * nsl + j], sp.zi[r0 * nsl + j], sp.zv[r0 * nsl + j]};
                b[u] = WhDraw{sp.zm[r1 * nsl + j], sp.zi[r1 * nsl + j], sp.zv[r1 * nsl + j]};
            }
        }
#pragma unroll
        for (int u = 0; u < WH_JOIN; ++u) { wh_draw_add(t0, a[u]); wh_draw_add(t1, b[u]); }
    }
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) {
        wh_draw_add(t0, WhDraw{__shfl_xor(t0.z, o, 64), __shfl_xor(t0.i, o, 64), __shfl_xor(t0.v, o, 64)});
        wh_draw_add(t1, WhDraw{__shfl_xor(t1.z, o, 64), __shfl_xor(t1.i, o, 64), __shfl_xor(t1.v, o, 64)});
    }
}
// The step after the head, block = 32 B threads: joins the slices of class 0 and, under the rules, of class 1, and applies the mass
// rule (every id below tb is denied when the log-sum-exp of the allowed timestamp logits exceeds the largest allowed text logit;
// with class 1 empty the merge leaves class 0's triple as it is); writes the step's outputs (argmax, its log-softmax), the
// no-speech probability at the step that fed sot_pos, the next token (of the row's own prefix while it lasts, then the generated
// one), pos + 1, the history and the allowed intervals of the next step, the done flag and the count of finished clips.  A row
// is done after eos or after its own last step (pend).
// SAMPLE: a row with temp[b] > 0 draws its id.  The mass rule is decided on the raw triples as above (upstream applies the rules to the
// untempered log-softmax before the draw); if the timestamps win, the id is class 1's perturbed winner, otherwise the larger z of
// the two classes' winners (equal z: the lower id).  The score is the chosen id's untempered log-probability over the allowed
// set, v - (t.m + logf(t.s)).  A row with temp[b] = 0 takes the greedy branch, bit for bit.
template <bool SAMPLE>
__global__ __launch_bounds__(1024) void wh_next_kernel(WhHeadOut o, int nsl, WhState s, int B, int T, WhTsRules r, int* __restrict__ ids,
                                                        float* __restrict__ score, int* __restrict__ counts, float* __restrict__ nospeech, WhSample sp) {
    __shared__ int fin[WH_MAXB];
    const int b = threadIdx.x >> 5, l = threadIdx.x & 31;
    int* ti = s.ti;
    // the row's state first: these loads are in flight while the slices are joined, not in the serial tail of lane 0
    const int p = s.pos[b], plen = ti[TS_PLEN * WH_MAXB + b], begin = ti[TS_BEGIN * WH_MAXB + b], gen_to = ti[TS_GENTO * WH_MAXB + b],
              pend = ti[TS_PEND * WH_MAXB + b], sot = ti[TS_SOT * WH_MAXB + b], fed = s.prefix[(long)b * T + min(p + 1, T - 1)];
    int d = s.done[b];
    const WhTop text = wh_join_slices(o.pm, o.pi, o.ps, b, nsl, l);
    WhTop ts{-INFINITY, INT_MAX, 0.f}, ns{-INFINITY, INT_MAX, 0.f};
    if (r.on) ts = wh_join_slices(o.pm, o.pi, o.ps, (long)B + b, nsl, l);
    if (nospeech) ns = wh_join_slices(o.nm, nullptr, o.nsum, b, nsl, l);
    WhDraw ztext{-INFINITY, INT_MAX, 0.f}, zts{-INFINITY, INT_MAX, 0.f};
    float temp = 0.f;
    if constexpr (SAMPLE) {
        temp = sp.temp[b];
        if (temp > 0.f) wh_join_draws(sp, b, (long)B + b, nsl, l, ztext, zts);
    }
    if (l == 0) {
        if (!d) {
            WhTop t = text;
            const bool ts_wins = ts.i != INT_MAX && (text.i == INT_MAX || ts.m + logf(ts.s) > text.m);
            if (ts_wins) t = ts;
            else wh_merge(t, ts);
            int am = t.i == INT_MAX ? r.eos : t.i;
            float sc = -logf(t.s);
            if constexpr (SAMPLE) {
                if (temp > 0.f) {
                    WhDraw pick = zts;
                    if (!ts_wins) wh_draw_add(pick, ztext);
                    if (pick.i != INT_MAX) { am = pick.i; sc = pick.v - (t.m + logf(t.s)); }
                }
            }
            ids[(long)b * T + p] = am;
            score[(long)b * T + p] = sc;
            if (nospeech && p == sot) nospeech[b] = expf(o.nlogit[b] - ns.m) / ns.s;
            int nxt;
            if (p + 1 < plen) nxt = fed;
            else {
                nxt = am;
                if (p < gen_to) { counts[b] += 1; if (nxt == r.eos) d = 1; }
            }
            if (p + 1 >= pend) d = 1;
            if (r.on && p + 1 >= begin) wh_ts_push(ti, b, nxt, r.tb);
            wh_ts_bounds(ti, b, p + 2 == begin, r);
            s.cur[b] = nxt;
            if (d) s.done[b] = 1;
            else s.pos[b] = min(p + 1, T - 1);
        }
        fin[b] = d;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int i = 0; i < B; ++i) n += fin[i];
        *s.ndone = n;
    }
}

// Single-query attention, one workgroup per (key chunk of 256, head, clip): scores of the chunk's keys (q scaled by 1/8),
// their maximum, exponentials and sum, then the 64 outputs as 4 groups of 64 keys x 64 lanes (a V row is one
// coalesced 256-byte read).  The chunk's (max, sum, unnormalised output) goes to the workspace; wh_attn_comb_kernel joins the
// chunks.  The number of keys is pos[b] + 1 (self attention over the cache) or nfix (cross attention).
__global__ __launch_bounds__(256) void wh_attn_part_kernel(const float* __restrict__ q, const float* __restrict__ Kc, const float* __restrict__ Vc,
                                                            long clip_stride, int d, const int* __restrict__ pos, int nfix, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float qs[DK];
    __shared__ float sc[WH_KEYS];
    __shared__ float red[4];
    __shared__ float ored[4][DK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z, nch = gridDim.x, H = gridDim.y;
    const int n = pos ? pos[b] + 1 : nfix;
    float* po = part + (((long)b * H + h) * nch + c) * (DK + 2);
    const int j0 = c * WH_KEYS;
    if (j0 >= n) {                                                  // (uniform over the workgroup)
        if (tid < DK) po[2 + tid] = 0.f;
        if (tid == 0) { po[0] = -INFINITY; po[1] = 0.f; }
        return;
    }
    if (tid < DK) qs[tid] = q[(long)b * d + h * DK + tid] * 0.125f;
    __syncthreads();
    const float* Kb = Kc + (long)b * clip_stride + h * DK;
    const float* Vb = Vc + (long)b * clip_stride + h * DK;
    // scores: 16 lanes per key (a K row is one coalesced 256-byte read, 4 keys per wave instruction), 16 keys per pass
    {
        const int sub = tid & 15, kg = tid >> 4;
        const f32x4 u = *reinterpret_cast<const f32x4*>(qs + 4 * sub);
#pragma unroll 8
        for (int ps = 0; ps < WH_KEYS / 16; ++ps) {
            const int jk = j0 + 16 * ps + kg;
            const f32x4 t = ldg4(Kb + (long)min(jk, n - 1) * d + 4 * sub);
            const float dot = h3_row16_sum(fmaf(u[3], t[3], fmaf(u[2], t[2], fmaf(u[1], t[1], u[0] * t[0]))));
            if (sub == 0) sc[16 * ps + kg] = jk < n ? dot : -INFINITY;
        }
    }
    __syncthreads();
    const int j = j0 + tid;
    const float s = sc[tid];
    float mx = wave_max(s);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float pj = j < n ? expf(s - mx) : 0.f;
    const float ls = wave_sum(pj);
    __syncthreads();                                                // red and sc have been read by all
    sc[tid] = pj;
    if (lane == 0) red[wave] = ls;
    __syncthreads();
    float a = 0.f;
    const int jend = min(64, n - j0 - 64 * wave);
#pragma unroll 8
    for (int jj = 0; jj < jend; ++jj) a = fmaf(sc[64 * wave + jj], Vb[(long)(j0 + 64 * wave + jj) * d + lane], a);
    ored[wave][lane] = a;
    __syncthreads();
    if (tid < DK) po[2 + tid] = ((ored[0][tid] + ored[1][tid]) + ored[2][tid]) + ored[3][tid];
    if (tid == 0) { po[0] = mx; po[1] = ((red[0] + red[1]) + red[2]) + red[3]; }
}
// grid (H, B), 64 threads
__global__ __launch_bounds__(64) void wh_attn_comb_kernel(const float* __restrict__ part, int nch, float* __restrict__ out, int d) {
    const int h = blockIdx.x, b = blockIdx.y, H = gridDim.x, i = threadIdx.x;
    const float* p = part + ((long)b * H + h) * nch * (DK + 2);
    float mx = -INFINITY;
    for (int c = 0; c < nch; ++c) mx = fmaxf(mx, p[c * (DK + 2)]);
    float l = 0.f, o = 0.f;
    for (int c = 0; c < nch; ++c) {
        const float w = expf(p[c * (DK + 2)] - mx);
        l = fmaf(p[c * (DK + 2) + 1], w, l);
        o = fmaf(p[c * (DK + 2) + 2 + i], w, o);
    }
    out[(long)b * d + h * DK + i] = o / l;
}

// Cross-attention probabilities of the alignment heads (tdx_whisper_decode_xattn), launched after a listed layer's cross q
// projection: workgroup (listed head, clip) recomputes the head's S scores from q and the layer's cross K (16 lanes per key, as
// above), then a full softmax over S: raw scores, the maximum, exponentials and their sum, the quotient; the intermediate values live
// in LDS up to 4096 positions and in the output row itself beyond.  1024 threads and four key rounds in flight: one workgroup per (head, clip) is a chain of dependent loads, and with 256
// threads and one round at a time it cost 55 us a launch.  The row is pos[b] - first_rows[b] (the device state's TS_FIRSTROW row); a finished clip, a head of another layer or a row outside the buffer: nothing is
// written.  The attention kernels above are not touched, so the decode's own results keep their bits.
__global__ __launch_bounds__(WH_XROW_NT) void wh_xattn_row_kernel(const float* __restrict__ q, const float* __restrict__ Kc, long clip_stride, int S, int d,
                                                            int layer, const int* __restrict__ heads, const int* __restrict__ pos,
                                                            const int* __restrict__ done, const int* __restrict__ first_rows, int max_rows,
                                                            float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float qs[DK];
    __shared__ float red[WH_XROW_NT / 64];
    __shared__ float slds[WH_XROW_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hi = blockIdx.x, b = blockIdx.y, nh = gridDim.x;
    if (heads[2 * hi] != layer || done[b]) return;                  // (uniform over the workgroup, like the two returns below)
    const int row = pos[b] - first_rows[b];
    if (row < 0 || row >= max_rows) return;
    const int h = heads[2 * hi + 1];
    float* o = out + (((size_t)b * nh + hi) * max_rows + row) * (size_t)S;
    float* sc = S <= WH_XROW_LDS ? slds : o;                        // scores and exponentials: LDS when they fit, else the row itself
    if (tid < DK) qs[tid] = q[(long)b * d + h * DK + tid] * 0.125f;
    __syncthreads();
    const float* Kb = Kc + (long)b * clip_stride + h * DK;
    const int sub = tid & 15, kg = tid >> 4;
    const f32x4 u = *reinterpret_cast<const f32x4*>(qs + 4 * sub);
    float mx = -INFINITY;
    constexpr int KPR = WH_XROW_NT / 16;                            // keys per round
    for (int j0 = 0; j0 < S; j0 += 4 * KPR) {
        f32x4 t[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) t[r] = ldg4(Kb + (long)min(j0 + r * KPR + kg, S - 1) * d + 4 * sub);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int jk = j0 + r * KPR + kg;
            const float dot = h3_row16_sum(fmaf(u[3], t[r][3], fmaf(u[2], t[r][2], fmaf(u[1], t[r][1], u[0] * t[r][0]))));
            if (sub == 0 && jk < S) { sc[jk] = dot; mx = fmaxf(mx, dot); }
        }
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();                                                // the scores are visible to the workgroup
    mx = red[0];
#pragma unroll
    for (int w = 1; w < WH_XROW_NT / 64; ++w) mx = fmaxf(mx, red[w]);
    float ls = 0.f;
    for (int j = tid; j < S; j += WH_XROW_NT) { const float e = expf(sc[j] - mx); sc[j] = e; ls += e; }
    ls = wave_sum(ls);
    __syncthreads();                                                // red has been read by all
    if (lane == 0) red[wave] = ls;
    __syncthreads();
    float l = red[0];
#pragma unroll
    for (int w = 1; w < WH_XROW_NT / 64; ++w) l += red[w];
    for (int j = tid; j < S; j += WH_XROW_NT) o[j] = sc[j] / l;            // a thread's own exponentials
}

// ------------------------------------------------------------------------------------------------ token alignment
// tdx_token_align (transformers' _extract_token_timestamps on the device).  W [B][nh][max_rows][S]; clip b uses rows < n, frames < m.
constexpr int AL_MAXROWS = 2048, AL_MAXW = 31, AL_NT = 512;
__device__ __forceinline__ int al_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// mean and population standard deviation over the token axis of every (clip, head, frame): two passes (mean, then the centred
// squares), the sums in fp64 (full rate here) so that the mean is the rounded exact one.  grid (ceil(S / 256), nh, B)
__global__ __launch_bounds__(256) void al_stats_kernel(const float* __restrict__ W, int max_rows, int S, const int* __restrict__ nrows,
                                                        const int* __restrict__ nframes, float* __restrict__ mean, float* __restrict__ sd) {
    const int j = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y, b = blockIdx.z, nh = gridDim.y;
    const int n = al_clamp(nrows[b], 0, max_rows), m = al_clamp(nframes[b], 1, S);
    if (n < 2 || j >= m) return;
    const float* w = W + ((size_t)b * nh + h) * max_rows * (size_t)S + j;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += (double)w[(size_t)i * S];
    const float mu = (float)(s / n);
    double q = 0.0;
    for (int i = 0; i < n; ++i) { const float c = w[(size_t)i * S] - mu; q += (double)c * (double)c; }
    mean[((size_t)b * nh + h) * S + j] = mu;
    sd[((size_t)b * nh + h) * S + j] = sqrtf((float)(q / n));
}
// z = (W - mean) / std (0 where std is 0), the median of `width` along the frames with reflect padding (none when m <= width / 2,
// as upstream), the mean over the heads.  Thread (frame j, row i = blockIdx.y, clip).  CW: the width at compile time (the window
// stays in registers) or 0 for any odd width up to AL_MAXW.
template <int CW>
__global__ __launch_bounds__(256) void al_filter_kernel(const float* __restrict__ W, int nh, int max_rows, int S, const int* __restrict__ nrows,
                                                         const int* __restrict__ nframes, int width, const float* __restrict__ mean,
                                                         const float* __restrict__ sd, float* __restrict__ M) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y, b = blockIdx.z;
    const int n = al_clamp(nrows[b], 0, max_rows), m = al_clamp(nframes[b], 1, S);
    if (n < 2 || i >= n || j >= m) return;
    const int w = CW ? CW : width, pad = w / 2;
    const bool plain = m <= pad || w == 1;
    float acc = 0.f;
    for (int h = 0; h < nh; ++h) {
        const float* wr = W + (((size_t)b * nh + h) * max_rows + i) * (size_t)S;
        const float* mu = mean + ((size_t)b * nh + h) * S;
        const float* sg = sd + ((size_t)b * nh + h) * S;
        if (plain) { acc += sg[j] > 0.f ? (wr[j] - mu[j]) / sg[j] : 0.f; continue; }
        float v[CW ? CW : AL_MAXW];
        for (int t = 0; t < w; ++t) {
            int jj = j + t - pad;
            if (jj < 0) jj = -jj;
            if (jj >= m) jj = 2 * (m - 1) - jj;
            v[t] = sg[jj] > 0.f ? (wr[jj] - mu[jj]) / sg[jj] : 0.f;
        }
        for (int a = 0; a <= pad; ++a)                              // selection up to the middle element
            for (int c = a + 1; c < w; ++c)
                if (v[c] < v[a]) { const float t = v[a]; v[a] = v[c]; v[c] = t; }
        acc += v[pad];
    }
    M[((size_t)b * max_rows + i) * (size_t)S + j] = acc / (float)nh;
}
// Dynamic time warping on -M, one workgroup per clip, as transformers' _dynamic_time_warping: cost[i][j] = -M[i-1][j-1] +
// min(cost[i-1][j-1], cost[i-1][j], cost[i][j-1]) in fp32, strict comparisons, a tie goes left.  The workgroup walks the
// anti-diagonals k = i + j; thread t owns the rows t + 1, t + 513, ... (R of them); the last two diagonals live in LDS indexed by
// i (index 0 and index k are the borders: inf, and 0 at the origin), three buffers in rotation, so one barrier per diagonal
// separates the writes of diagonal k from the reads of k + 1 and from the writes of k + 1 into the buffer k - 2 was read from.
// The value of M a thread needs next is loaded a diagonal ahead.  The trace goes out as bytes; thread 0 walks it back from the
// last cell: the frame of row i is the column at which the path leaves the row going back (upstream's time_indices[jumps]).
template <int R>
__global__ __launch_bounds__(AL_NT) void al_dtw_kernel(const float* __restrict__ M, int max_rows, int S, const int* __restrict__ nrows,
                                                        const int* __restrict__ nframes, unsigned char* __restrict__ trace, int* __restrict__ frames) {
    __shared__ float dg[3][R * AL_NT + 1];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int n = al_clamp(nrows[b], 0, min(max_rows, R * AL_NT)), m = al_clamp(nframes[b], 1, S);
    if (n == 0) return;                                             // (uniform)
    if (n == 1) { if (tid == 0) frames[(size_t)b * max_rows] = 0; return; }
    const float* Mb = M + (size_t)b * max_rows * (size_t)S;
    unsigned char* tb = trace + (size_t)b * max_rows * (size_t)S;
    if (tid == 0) { dg[0][0] = 0.f; dg[1][0] = INFINITY; dg[1][1] = INFINITY; }
    float nxt[R];
#pragma unroll
    for (int r = 0; r < R; ++r) nxt[r] = (tid + r * AL_NT == 0) ? Mb[0] : 0.f;      // diagonal 2 is the cell (1, 1)
    __syncthreads();
    for (int k = 2; k <= n + m; ++k) {
        float* cur = dg[k % 3];
        const float* p1 = dg[(k + 2) % 3];
        const float* p2 = dg[(k + 1) % 3];
        const int ilo = max(1, k - m), ihi = min(n, k - 1);
        const int nlo = max(1, k + 1 - m), nhi = min(n, k);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = tid + 1 + r * AL_NT;
            const float mv = nxt[r];
            if (i >= nlo && i <= nhi) nxt[r] = Mb[(size_t)(i - 1) * S + (k - i)];       // the cell (i, k + 1 - i)
            if (i >= ilo && i <= ihi) {
                const float c0 = p2[i - 1], c1 = p1[i - 1], c2 = p1[i];
                float c; unsigned char t;
                if (c0 < c1 && c0 < c2) { c = c0; t = 0; }
                else if (c1 < c0 && c1 < c2) { c = c1; t = 1; }
                else { c = c2; t = 2; }
                cur[i] = -mv + c;
                tb[(size_t)(i - 1) * S + (k - i - 1)] = t;
            }
        }
        if (tid == 0) { cur[0] = INFINITY; if (k <= n) cur[k] = INFINITY; }
        __syncthreads();
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        int i = n, j = m;
        while (i > 0) {
            const int t = j > 0 ? tb[(size_t)(i - 1) * S + (j - 1)] : 1;
            if (t != 2) frames[(size_t)b * max_rows + i - 1] = max(j - 1, 0);
            if (t == 0) { --i; --j; } else if (t == 1) --i; else --j;
        }
    }
}
struct AlignWs { size_t mean, sd, M, trace, total; };
AlignWs align_ws(size_t B, size_t nh, size_t max_rows, size_t S) {
    AlignWs w; size_t o = 0;
    w.mean = o; o += al(B * nh * S); w.sd = o; o += al(B * nh * S);
    w.M = o; o += al(B * max_rows * S);
    w.trace = o; o += al((B * max_rows * S + 3) / 4);
    w.total = o;
    return w;
}

struct AttnW { const float *ln_g = nullptr, *ln_b = nullptr, *Wq = nullptr, *bq = nullptr, *Wk = nullptr, *Wv = nullptr, *bv = nullptr, *Wo = nullptr, *bo = nullptr; };
struct EncLayer { AttnW sa; const float *ln2_g = nullptr, *ln2_b = nullptr, *W1 = nullptr, *b1 = nullptr, *W2 = nullptr, *b2 = nullptr; };
struct DecLayer { AttnW sa, ca; const float *ln3_g = nullptr, *ln3_b = nullptr, *W1 = nullptr, *b1 = nullptr, *W2 = nullptr, *b2 = nullptr; };

// the stage_* functions bind the fields of a layer that already sits in the handle's vector (Loader::bind)
void push_linear(Loader& ld, const float*& dst, const std::string& name, int N, int K) {       // rows padded to the GEMM's 128-column tiles
    ld.push(dst, ld.get(name, {(uint32_t)N, (uint32_t)K}), (size_t)N * K, (size_t)up(N, 128) * K);
}
void stage_attn(Loader& ld, const std::string& pre, const std::string& ln, int d, AttnW& w) {
    ld.push(w.ln_g, ld.get(ln + ".weight", d), d); ld.push(w.ln_b, ld.get(ln + ".bias", d), d);
    push_linear(ld, w.Wq, pre + ".q_proj.weight", d, d); ld.push(w.bq, ld.get(pre + ".q_proj.bias", d), d);
    push_linear(ld, w.Wk, pre + ".k_proj.weight", d, d);
    push_linear(ld, w.Wv, pre + ".v_proj.weight", d, d); ld.push(w.bv, ld.get(pre + ".v_proj.bias", d), d);
    push_linear(ld, w.Wo, pre + ".out_proj.weight", d, d); ld.push(w.bo, ld.get(pre + ".out_proj.bias", d), d);
}
template <class Layer>      // EncLayer (final norm ln2_*) or DecLayer (ln3_*)
void stage_ffn(Loader& ld, const std::string& pre, int d, int ffn, const float*& ln_g, const float*& ln_b, Layer& w) {
    ld.push(ln_g, ld.get(pre + "final_layer_norm.weight", d), d); ld.push(ln_b, ld.get(pre + "final_layer_norm.bias", d), d);
    push_linear(ld, w.W1, pre + "fc1.weight", ffn, d); ld.push(w.b1, ld.get(pre + "fc1.bias", ffn), ffn);
    push_linear(ld, w.W2, pre + "fc2.weight", d, ffn); ld.push(w.b2, ld.get(pre + "fc2.bias", d), d);
}

double hz_to_mel(double f) { return f < 1000.0 ? 3.0 * f / 200.0 : 15.0 + std::log(f / 1000.0) * (27.0 / std::log(6.4)); }
double mel_to_hz(double m) { return m < 15.0 ? 200.0 * m / 3.0 : 1000.0 * std::exp(std::log(6.4) / 27.0 * (m - 15.0)); }

template <int BT>
int launch_skinny_t(const SkArgs& a, int njobs, hipStream_t st) {
    hipLaunchKernelGGL(wh_skinny_kernel<BT>, dim3((a.N + 3) / 4, njobs), dim3(256), 0, st, a);
    LAUNCH_CHECK();
    return TDX_OK;
}
// B <= 8: the fp32-FMA kernel, LayerNorm inside.  B > 8: LayerNorm rows into `xn` once, the MFMA kernel, the finish kernel.
int launch_skinny(SkArgs a, int njobs, float* xn, float* partial, hipStream_t st) {
    if (a.B <= 1) return launch_skinny_t<1>(a, njobs, st);
    if (a.B <= 2) return launch_skinny_t<2>(a, njobs, st);
    if (a.B <= 4) return launch_skinny_t<4>(a, njobs, st);
    if (a.B <= 8) return launch_skinny_t<8>(a, njobs, st);
    if (a.lng) {
        hipLaunchKernelGGL(wh_ln_rows_kernel, dim3((a.B + 3) / 4), dim3(256), 0, st, a.x, a.lng, a.lnb, xn, (long)a.B, a.K);
        LAUNCH_CHECK();
        a.x = xn; a.lng = nullptr; a.lnb = nullptr;
    }
    const int KS = skm_splits(a.N, a.K);
    hipLaunchKernelGGL(wh_skinny_mfma_kernel, dim3((a.N + 31) / 32, KS, njobs), dim3(256), 0, st, a, KS, partial);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(wh_sk_finish_kernel, dim3((unsigned)(((long)a.B * a.N + 255) / 256), njobs), dim3(256), 0, st, a, KS, (const float*)partial);
    LAUNCH_CHECK();
    return TDX_OK;
}
template <int BT, bool TS, bool SAMPLE>
int launch_head_t(const SkArgs& a, const unsigned char* mask, const int* bnd, int tb, int want_ns, int ns_id, const WhHeadOut& o, int nsl,
                  const WhSample& sp, hipStream_t st) {
    hipLaunchKernelGGL((wh_head_kernel<BT, TS, SAMPLE>), dim3(nsl), dim3(256), 0, st, a, mask, bnd, tb, want_ns, ns_id, o, nsl, sp);
    LAUNCH_CHECK();
    return TDX_OK;
}
// TS: the timestamp rules are on (two classes of triples, the no-speech pair when want_ns); SAMPLE: the rows' draws as well
template <bool TS, bool SAMPLE = false>
int launch_head(const SkArgs& a, const unsigned char* mask, const int* bnd, int tb, int want_ns, int ns_id, const WhHeadOut& o, int nsl, hipStream_t st,
                const WhSample& sp = WhSample{}) {
    if (a.B <= 1) return launch_head_t<1, TS, SAMPLE>(a, mask, bnd, tb, want_ns, ns_id, o, nsl, sp, st);
    if (a.B <= 2) return launch_head_t<2, TS, SAMPLE>(a, mask, bnd, tb, want_ns, ns_id, o, nsl, sp, st);
    if (a.B <= 4) return launch_head_t<4, TS, SAMPLE>(a, mask, bnd, tb, want_ns, ns_id, o, nsl, sp, st);
    if (a.B <= 8) return launch_head_t<8, TS, SAMPLE>(a, mask, bnd, tb, want_ns, ns_id, o, nsl, sp, st);
    if (a.B <= 16) return launch_head_t<16, TS, SAMPLE>(a, mask, bnd, tb, want_ns, ns_id, o, nsl, sp, st);
    return launch_head_t<32, TS, SAMPLE>(a, mask, bnd, tb, want_ns, ns_id, o, nsl, sp, st);
}
SkJob sk_job(const float* W, const float* bias, const float* res, float* y, long ld, int brow = 0, int gelu = 0) {
    return SkJob{W, bias, res, y, ld, brow, gelu};
}

}  // namespace

struct tdx_whisper {
    int device = 0;
    tdx_whisper_config c{};
    int MP = 0;                       // mel channels of the conv1 rows (multiple of 32)
    tdx::DevBuf dev;
    int* pinned = nullptr;            // the host word the decode loop reads
    const float *dft = nullptr, *melw = nullptr, *c1w = nullptr, *c1b = nullptr, *c2w = nullptr, *c2b = nullptr, *epos = nullptr,
        *eln_g = nullptr, *eln_b = nullptr, *tok = nullptr, *dpos = nullptr, *dln_g = nullptr, *dln_b = nullptr;
    std::vector<EncLayer> enc;
    std::vector<DecLayer> dec;
    ~tdx_whisper() { if (pinned) (void)hipHostFree(pinned); }
};

namespace {

// workspace layouts (floats)
struct LogmelWs { size_t pw, total; };
LogmelWs logmel_ws(const tdx_whisper* h, int B) {
    const size_t rp = 2 * (size_t)h->c.n_audio_ctx + 3;
    LogmelWs w;
    w.pw = al(B * rp * HOP); w.total = w.pw + al(B * rp * PWP);
    return w;
}
struct EncWs { size_t xc, c1, x, xn, q, k, v, ao, hb, total; };
EncWs enc_ws(const tdx_whisper* h, int B) {
    const size_t S = h->c.n_audio_ctx, T = 2 * S, d = h->c.d_model, M = B * S;
    EncWs w; size_t o = 0;
    w.xc = o; o += al(B * (T + 2) * h->MP);
    w.c1 = o; o += al(B * (T + 2) * d);
    w.x = o; o += al(M * d); w.xn = o; o += al(M * d); w.q = o; o += al(M * d); w.k = o; o += al(M * d); w.v = o; o += al(M * d); w.ao = o; o += al(M * d);
    w.hb = o; o += al(M * (size_t)h->c.enc_ffn);
    w.total = o;
    return w;
}
// pm, pi, ps: the head's triples [2][B][nsl] (two classes); nm, nsum, nlogit: the no-speech pairs; ti: the rows' state; prefix [B][T]
struct DecWs { size_t x, xn, skp, q, ao, hb, part, state, mask, heads, ti, pm, pi, ps, nm, nsum, nlogit, prefix, cache, total; int nsl, nch_self, nch_cross; };
DecWs dec_ws(const tdx_whisper* h, int B) {
    const size_t d = h->c.d_model, T = h->c.n_text_ctx, H = h->c.dec_heads;
    DecWs w; size_t o = 0;
    w.nsl = (h->c.vocab + WH_SLICE - 1) / WH_SLICE;
    w.nch_self = (h->c.n_text_ctx + WH_KEYS - 1) / WH_KEYS;
    w.nch_cross = (h->c.n_audio_ctx + WH_KEYS - 1) / WH_KEYS;
    w.x = o; o += al(B * d); w.xn = o; o += al(B * d);
    w.skp = o; o += B > 8 ? al((size_t)3 * SKM_MAXKS * WH_MAXB * std::max<size_t>(d, h->c.dec_ffn)) : 0;
    w.q = o; o += al(B * d); w.ao = o; o += al(B * d); w.hb = o; o += al(B * (size_t)h->c.dec_ffn);
    w.part = o; o += al(B * H * (size_t)std::max(w.nch_self, w.nch_cross) * (DK + 2));
    w.state = o; o += al(4 * WH_MAXB);
    w.mask = o; o += al(((size_t)h->c.vocab + 3) / 4);
    w.heads = o; o += al(2 * WH_MAXHEADS);
    w.ti = o; o += al((size_t)WH_TS_ROWS * WH_MAXB);
    w.pm = o; o += al((size_t)2 * B * w.nsl); w.pi = o; o += al((size_t)2 * B * w.nsl); w.ps = o; o += al((size_t)2 * B * w.nsl);
    w.nm = o; o += al((size_t)B * w.nsl); w.nsum = o; o += al((size_t)B * w.nsl); w.nlogit = o; o += al(WH_MAXB);
    w.prefix = o; o += al((size_t)B * T);
    w.cache = o; o += al((size_t)h->c.dec_layers * 2 * B * T * d);
    w.total = o;
    return w;
}
// what tdx_whisper_decode_ts_sample keeps behind the common workspace (floats from its end): the rows' temperatures and streams and
// the head's records zm, zi, zv [2][B][nsl]
struct SampleWs { size_t temp, stream, zm, zi, zv, total; };
SampleWs sample_ws(const tdx_whisper* h, int B) {
    const size_t nsl = (h->c.vocab + WH_SLICE - 1) / WH_SLICE;
    SampleWs w; size_t o = 0;
    w.temp = o; o += al(WH_MAXB); w.stream = o; o += al(2 * WH_MAXB);
    w.zm = o; o += al(2 * B * nsl); w.zi = o; o += al(2 * B * nsl); w.zv = o; o += al(2 * B * nsl);
    w.total = o;
    return w;
}

}  // namespace

extern "C" {

int tdx_whisper_create(const tdx_whisper_config* cfg, const void* blob, size_t blob_bytes, int device, tdx_whisper** out) {
    if (!cfg || !blob || !out) return tdx::fail(TDX_E_INVALID, "tdx_whisper_create: bad argument");
    const tdx_whisper_config c = *cfg;
    if (c.d_model < DK || c.enc_heads < 1 || c.dec_heads < 1 || c.d_model != DK * c.enc_heads || c.d_model != DK * c.dec_heads)
        return tdx::fail(TDX_E_INVALID, "tdx_whisper_create: d_model / heads must be 64 in the encoder and the decoder");
    if (!c.gelu) return tdx::fail(TDX_E_INVALID, "tdx_whisper_create: activation_function must be \"gelu\" (exact erf)");
    if (c.n_mels != 80 && c.n_mels != 128) return tdx::fail(TDX_E_INVALID, "tdx_whisper_create: n_mels must be 80 or 128");
    if (c.n_audio_ctx < 1 || c.n_audio_ctx > WH_MAXCTX) return tdx::fail(TDX_E_INVALID, "tdx_whisper_create: n_audio_ctx must be in [1, 32768]");
    if (c.n_text_ctx < 1 || c.n_text_ctx > WH_MAXCTX) return tdx::fail(TDX_E_INVALID, "tdx_whisper_create: n_text_ctx must be in [1, 32768]");
    if (c.vocab < 2) return tdx::fail(TDX_E_INVALID, "tdx_whisper_create: vocab must be at least 2");
    if (c.enc_layers < 1 || c.dec_layers < 1) return tdx::fail(TDX_E_INVALID, "tdx_whisper_create: enc_layers and dec_layers must be at least 1");
    if (c.enc_ffn < 64 || c.enc_ffn % 64 || c.dec_ffn < 64 || c.dec_ffn % 64)
        return tdx::fail(TDX_E_INVALID, "tdx_whisper_create: enc_ffn and dec_ffn must be positive multiples of 64");
    tdx::Loader ld;
    if (!ld.parse(blob, blob_bytes)) return tdx::fail(TDX_E_BLOB, "tdx_whisper_create: malformed TDXW blob");
    const int d = c.d_model, MP = up(c.n_mels, 32), dP = up(d, 128);
    std::unique_ptr<tdx_whisper> h(new tdx_whisper());
    h->device = device; h->c = c; h->MP = MP;
    h->enc.resize(c.enc_layers); h->dec.resize(c.dec_layers);

    // window x DFT basis, rows c (re) and NBINP + c (im); the Slaney mel bank [MELP][PWP]
    const size_t dft = ld.room(h->dft, (size_t)2 * NBINP * KFR), mel = ld.room(h->melw, (size_t)MELP * PWP);
    tdx::fill_dft_analysis(ld.host.data() + dft, NFFT, NBIN, NBINP, KFR, tdx::hann_periodic(NFFT).data());
    {
        const int nm = c.n_mels;
        std::vector<double> ff(nm + 2);
        const double m0 = hz_to_mel(0.0), m1 = hz_to_mel(8000.0);
        for (int i = 0; i < nm + 2; ++i) ff[i] = mel_to_hz(m0 + (m1 - m0) * i / (nm + 1));
        for (int j = 0; j < nm; ++j)
            for (int b = 0; b < NBIN; ++b) {
                const double f = 8000.0 * b / (NBIN - 1);
                const double down = (f - ff[j]) / (ff[j + 1] - ff[j]), upw = (ff[j + 2] - f) / (ff[j + 2] - ff[j + 1]);
                const double v = std::max(0.0, std::min(down, upw)) * (2.0 / (ff[j + 2] - ff[j]));
                ld.host[mel + (size_t)j * PWP + b] = (float)v;
            }
    }
    // conv weights [d][cin][3] -> [dP][3][cin padded]
    const size_t c1w = ld.room(h->c1w, (size_t)dP * 3 * MP), c2w = ld.room(h->c2w, (size_t)dP * 3 * d);
    if (const float* w = ld.get("model.encoder.conv1.weight", {(uint32_t)d, (uint32_t)c.n_mels, 3u}))
        for (int n = 0; n < d; ++n) for (int ci = 0; ci < c.n_mels; ++ci) for (int t = 0; t < 3; ++t)
            ld.host[c1w + ((size_t)n * 3 + t) * MP + ci] = w[((size_t)n * c.n_mels + ci) * 3 + t];
    if (const float* w = ld.get("model.encoder.conv2.weight", {(uint32_t)d, (uint32_t)d, 3u}))
        for (int n = 0; n < d; ++n) for (int ci = 0; ci < d; ++ci) for (int t = 0; t < 3; ++t)
            ld.host[c2w + ((size_t)n * 3 + t) * d + ci] = w[((size_t)n * d + ci) * 3 + t];
    ld.push(h->c1b, ld.get("model.encoder.conv1.bias", d), d); ld.push(h->c2b, ld.get("model.encoder.conv2.bias", d), d);
    ld.push(h->epos, ld.get("model.encoder.embed_positions.weight", {(uint32_t)c.n_audio_ctx, (uint32_t)d}), (size_t)c.n_audio_ctx * d);
    for (int l = 0; l < c.enc_layers; ++l) {
        const std::string p = "model.encoder.layers." + std::to_string(l) + ".";
        EncLayer& w = h->enc[l];
        stage_attn(ld, p + "self_attn", p + "self_attn_layer_norm", d, w.sa);
        stage_ffn(ld, p, d, c.enc_ffn, w.ln2_g, w.ln2_b, w);
    }
    ld.push(h->eln_g, ld.get("model.encoder.layer_norm.weight", d), d); ld.push(h->eln_b, ld.get("model.encoder.layer_norm.bias", d), d);
    const float* tokp = ld.get("model.decoder.embed_tokens.weight", {(uint32_t)c.vocab, (uint32_t)d});
    ld.push(h->tok, tokp, (size_t)c.vocab * d);
    ld.push(h->dpos, ld.get("model.decoder.embed_positions.weight", {(uint32_t)c.n_text_ctx, (uint32_t)d}), (size_t)c.n_text_ctx * d);
    for (int l = 0; l < c.dec_layers; ++l) {
        const std::string p = "model.decoder.layers." + std::to_string(l) + ".";
        DecLayer& w = h->dec[l];
        stage_attn(ld, p + "self_attn", p + "self_attn_layer_norm", d, w.sa);
        stage_attn(ld, p + "encoder_attn", p + "encoder_attn_layer_norm", d, w.ca);
        stage_ffn(ld, p, d, c.dec_ffn, w.ln3_g, w.ln3_b, w);
    }
    ld.push(h->dln_g, ld.get("model.decoder.layer_norm.weight", d), d); ld.push(h->dln_b, ld.get("model.decoder.layer_norm.bias", d), d);
    if (const float* po = ld.get_optional("proj_out.weight", (size_t)c.vocab * d))
        if (tokp && memcmp(po, tokp, (size_t)c.vocab * d * sizeof(float)) != 0)
            return tdx::fail(TDX_E_BLOB, "tdx_whisper_create: proj_out.weight differs from model.decoder.embed_tokens.weight (the head is tied)");
    TRY(ld.finish("tdx_whisper_create", true, device, h->dev));
    {
        tdx::DeviceGuard guard(device);
        if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
        const hipError_t rc = hipHostMalloc((void**)&h->pinned, 64, hipHostMallocDefault);
        if (rc != hipSuccess) { h->pinned = nullptr; return tdx::fail_hip(rc, __FILE__, __LINE__); }
    }
    *out = h.release();
    return TDX_OK;
}

int tdx_whisper_destroy(tdx_whisper* h) {
    delete h;
    return TDX_OK;
}

size_t tdx_whisper_workspace_bytes(const tdx_whisper* h, int B) {
    if (!h || B < 1 || B > WH_MAXB) return 0;
    return std::max(std::max(logmel_ws(h, B).total, enc_ws(h, B).total), dec_ws(h, B).total) * sizeof(float);
}

size_t tdx_whisper_decode_sample_workspace_bytes(const tdx_whisper* h, int B) {
    if (!h || B < 1 || B > WH_MAXB) return 0;
    return tdx_whisper_workspace_bytes(h, B) + sample_ws(h, B).total * sizeof(float);
}

double tdx_whisper_flops(const tdx_whisper* h, int B, int steps) {
    if (!h || B < 1 || steps < 0) return 0.0;
    const double d = h->c.d_model, S = h->c.n_audio_ctx, M = B * S;
    const double enc = 2.0 * B * 2.0 * S * 3.0 * h->c.n_mels * d + 2.0 * M * 3.0 * d * d
                     + h->c.enc_layers * (2.0 * M * (4.0 * d * d + 2.0 * d * h->c.enc_ffn) + 4.0 * B * S * S * d)
                     + h->c.dec_layers * 2.0 * M * 2.0 * d * d;
    const double step = h->c.dec_layers * (2.0 * B * (8.0 * d * d + 2.0 * d * h->c.dec_ffn) + 4.0 * B * S * d) + 2.0 * B * d * (double)h->c.vocab;
    return enc + steps * step;
}

int tdx_whisper_logmel(tdx_whisper* h, const float* wav_dev, const int* lens_dev, int B, long N, float* feat_dev, void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !wav_dev || !feat_dev || !ws_ || B < 1 || B > WH_MAXB || N < 1) return tdx::fail(TDX_E_INVALID, "tdx_whisper_logmel: bad argument (1 <= B <= 32, N >= 1)");
    if (ws_bytes < tdx_whisper_workspace_bytes(h, B)) return tdx::fail(TDX_E_WORKSPACE, "tdx_whisper_logmel: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    const int T = 2 * h->c.n_audio_ctx, rp = T + 3, pitch = rp * HOP, P = T * HOP;
    const LogmelWs w = logmel_ws(h, B);
    float* pad = (float*)ws_; float* pw = (float*)ws_ + w.pw;
    hipLaunchKernelGGL(wh_pad_kernel, dim3((pitch + 255) / 256, B), dim3(256), 0, st, wav_dev, lens_dev, N, P, pitch, pad);
    LAUNCH_CHECK();
    // the last row computed is B rp - 3: it ends 64 floats before the end of `pad`; the last frame kept is B rp - 4
    const int M = B * rp - 2;
    TRY((linear_f32<true>(pad, HOP, h->dft, M, NBINP, KFR, EpiPow{pw}, st, 0, NBINP)));
    TRY(linear_f32(pw, PWP, h->melw, M, MELP, PWP, EpiLogMelT{feat_dev, rp, T, h->c.n_mels}, st));
    hipLaunchKernelGGL(wh_clamp_kernel, dim3(B), dim3(1024), 0, st, feat_dev, (long)h->c.n_mels * T);
    LAUNCH_CHECK();
    return TDX_OK;
}

int tdx_whisper_encode(tdx_whisper* h, const float* feat_dev, int B, float* enc_dev, float* enc_state_dev, void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !feat_dev || !ws_ || (!enc_dev && !enc_state_dev) || B < 1 || B > WH_MAXB) return tdx::fail(TDX_E_INVALID, "tdx_whisper_encode: bad argument (1 <= B <= 32)");
    if (ws_bytes < tdx_whisper_workspace_bytes(h, B)) return tdx::fail(TDX_E_WORKSPACE, "tdx_whisper_encode: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    const tdx_whisper_config& c = h->c;
    const int S = c.n_audio_ctx, T = 2 * S, d = c.d_model, dP = up(d, 128), MP = h->MP, H = c.enc_heads, ffn = c.enc_ffn;
    const long M = (long)B * S;
    const EncWs w = enc_ws(h, B);
    float* f = (float*)ws_;
    float *xc = f + w.xc, *c1 = f + w.c1, *x = f + w.x, *xn = f + w.xn, *q = f + w.q, *k = f + w.k, *v = f + w.v, *ao = f + w.ao, *hb = f + w.hb;
    hipLaunchKernelGGL(wh_chlast_kernel, dim3(T + 2, B), dim3(MP), 0, st, feat_dev, c.n_mels, T, MP, xc);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(wh_zero_edge_kernel, dim3(2, B), dim3(256), 0, st, c1, T, d);
    LAUNCH_CHECK();
    // overlapping rows: the last row computed is the last one kept, nothing is read past a buffer's end
    TRY(linear_f32(xc, MP, h->c1w, B * (T + 2) - 2, dP, 3 * MP, EpiConv1{h->c1b, c1, T, d}, st));
    TRY(linear_f32(c1, 2L * d, h->c2w, B * (S + 1) - 1, dP, 3 * d, EpiConv2{h->c2b, h->epos, x, S, d}, st));
    const dim3 lng((unsigned)((M + 3) / 4));
    for (int l = 0; l < c.enc_layers; ++l) {
        const EncLayer& L = h->enc[l];
        hipLaunchKernelGGL(wh_ln_rows_kernel, lng, dim3(256), 0, st, x, L.sa.ln_g, L.sa.ln_b, xn, M, d);
        LAUNCH_CHECK();
        TRY(linear_f32(xn, d, L.sa.Wq, (int)M, dP, d, EpiBiasActN<>{L.sa.bq, q, d, d}, st));
        TRY(linear_f32(xn, d, L.sa.Wk, (int)M, dP, d, EpiBiasActN<>{nullptr, k, d, d}, st));
        TRY(linear_f32(xn, d, L.sa.Wv, (int)M, dP, d, EpiBiasActN<>{L.sa.bv, v, d, d}, st));
        hipLaunchKernelGGL(wh_enc_attn_kernel, dim3((S + 63) / 64, H, B), dim3(256), 0, st, q, k, v, ao, S, d);
        LAUNCH_CHECK();
        TRY(linear_f32(ao, d, L.sa.Wo, (int)M, dP, d, EpiBiasResN<>{L.sa.bo, x, x, d, d}, st));
        hipLaunchKernelGGL(wh_ln_rows_kernel, lng, dim3(256), 0, st, x, L.ln2_g, L.ln2_b, xn, M, d);
        LAUNCH_CHECK();
        TRY(linear_f32(xn, d, L.W1, (int)M, up(ffn, 128), d, EpiBiasActN<ActGelu>{L.b1, hb, ffn, ffn}, st));
        TRY(linear_f32(hb, ffn, L.W2, (int)M, dP, ffn, EpiBiasResN<>{L.b2, x, x, d, d}, st));
    }
    float* e = enc_dev ? enc_dev : xn;
    hipLaunchKernelGGL(wh_ln_rows_kernel, lng, dim3(256), 0, st, x, h->eln_g, h->eln_b, e, M, d);
    LAUNCH_CHECK();
    if (enc_state_dev)
        for (int l = 0; l < c.dec_layers; ++l) {
            const AttnW& A = h->dec[l].ca;
            float* Kc = enc_state_dev + (size_t)(2 * l) * M * d;
            float* Vc = enc_state_dev + (size_t)(2 * l + 1) * M * d;
            TRY(linear_f32(e, d, A.Wk, (int)M, dP, d, EpiBiasActN<>{nullptr, Kc, d, d}, st));
            TRY(linear_f32(e, d, A.Wv, (int)M, dP, d, EpiBiasActN<>{A.bv, Vc, d, d}, st));
        }
    return TDX_OK;
}

// the capture of the alignment heads: (layer, head) pairs and the rows of the buffer; first_row: tdx_whisper_decode_xattn's, for
// every clip (the clips of tdx_whisper_decode_ts have one each)
struct WhCapture { const int* heads_host; int nh, first_row, max_rows; float* xattn_dev; };

// the argument checks the decode entry points share, each with its own message
static int wh_check_capture(const std::string& fn, const WhCapture& cap) {
    if (cap.nh < 1 || cap.nh > WH_MAXHEADS) return tdx::fail(TDX_E_INVALID, fn + ": nh must be in [1, 64]");
    if (cap.max_rows < 1) return tdx::fail(TDX_E_INVALID, fn + ": max_rows must be at least 1");
    if (cap.first_row < 0) return tdx::fail(TDX_E_INVALID, fn + ": first_row must not be negative");
    if (!cap.heads_host || !cap.xattn_dev) return tdx::fail(TDX_E_INVALID, fn + ": heads_host and xattn_dev must not be NULL");
    return TDX_OK;
}
static int wh_listed_layers(const std::string& fn, const WhCapture& cap, int Ld, int H, std::vector<char>& listed) {
    for (int i = 0; i < cap.nh; ++i) {
        const int l = cap.heads_host[2 * i], hd = cap.heads_host[2 * i + 1];
        if (l < 0 || l >= Ld || hd < 0 || hd >= H)
            return tdx::fail(TDX_E_INVALID, fn + ": alignment head (" + std::to_string(l) + ", " + std::to_string(hd) + ") outside the decoder's layers / heads");
        listed[l] = 1;
    }
    return TDX_OK;
}
// mask[id] bit 0: suppressed at every step, bit 1: at the first generated step
static int wh_static_mask(const std::string& fn, int V, const int* suppress_host, int n_suppress, const int* begin_suppress_host, int n_begin,
                          std::vector<unsigned char>& mask) {
    mask.assign(((size_t)V + 3) / 4 * 4, 0);
    for (int i = 0; i < n_suppress; ++i) {
        if (suppress_host[i] < 0 || suppress_host[i] >= V) return tdx::fail(TDX_E_INVALID, fn + ": suppressed id outside the vocabulary");
        mask[suppress_host[i]] |= 1;
    }
    for (int i = 0; i < n_begin; ++i) {
        if (begin_suppress_host[i] < 0 || begin_suppress_host[i] >= V) return tdx::fail(TDX_E_INVALID, fn + ": begin-suppressed id outside the vocabulary");
        mask[begin_suppress_host[i]] |= 2;
    }
    return TDX_OK;
}

static SkArgs wh_sk_args(const WhState& s, int B, const float* xin, const float* g, const float* be, int N, int K) {
    SkArgs a{};
    a.x = xin; a.lng = g; a.lnb = be; a.pos = s.pos; a.B = B; a.N = N; a.K = K;
    return a;
}
// One decode step up to the vocabulary head, shared by the three decode entry points: the embedding of every row's current token
// and the decoder layers.
struct WhStepCtx {
    tdx_whisper* h; const DecWs* w; float* f; WhState s; int B; const float* enc_state_dev; const WhCapture* cap; const char* listed;
    const int* heads_dev; hipStream_t st;
};
static int wh_decoder_step(const WhStepCtx& c) {
    tdx_whisper* h = c.h;
    const DecWs& w = *c.w;
    const WhState& s = c.s;
    const WhCapture* cap = c.cap;
    hipStream_t st = c.st;
    const int B = c.B, T = h->c.n_text_ctx, d = h->c.d_model, H = h->c.dec_heads, S = h->c.n_audio_ctx, ffn = h->c.dec_ffn, Ld = h->c.dec_layers;
    float* f = c.f;
    float *x = f + w.x, *xn = f + w.xn, *skp = f + w.skp, *q = f + w.q, *ao = f + w.ao, *hb = f + w.hb, *part = f + w.part, *cache = f + w.cache;
    const float* enc_state_dev = c.enc_state_dev;
    const size_t lay = (size_t)B * T * d;                       // one layer's K (or V) cache
    const size_t clay = (size_t)B * S * d;                      // one layer's cross K (or V)
    auto sk = [&](const float* xin, const float* g, const float* be, int N, int K) { return wh_sk_args(s, B, xin, g, be, N, K); };
    hipLaunchKernelGGL(wh_embed_kernel, dim3(B), dim3(256), 0, st, h->tok, h->dpos, s.cur, s.pos, x, d);
    LAUNCH_CHECK();
    for (int l = 0; l < Ld; ++l) {
        const DecLayer& L = h->dec[l];
        float* Kc = cache + (size_t)(2 * l) * lay;
        float* Vc = cache + (size_t)(2 * l + 1) * lay;
        SkArgs a = sk(x, L.sa.ln_g, L.sa.ln_b, d, d);
        a.job[0] = sk_job(L.sa.Wq, L.sa.bq, nullptr, q, d);
        a.job[1] = sk_job(L.sa.Wk, nullptr, nullptr, Kc, d, T);
        a.job[2] = sk_job(L.sa.Wv, L.sa.bv, nullptr, Vc, d, T);
        TRY(launch_skinny(a, 3, xn, skp, st));
        hipLaunchKernelGGL(wh_attn_part_kernel, dim3(w.nch_self, H, B), dim3(256), 0, st, q, Kc, Vc, (long)T * d, d, s.pos, 0, part);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(wh_attn_comb_kernel, dim3(H, B), dim3(64), 0, st, part, w.nch_self, ao, d);
        LAUNCH_CHECK();
        a = sk(ao, nullptr, nullptr, d, d);
        a.job[0] = sk_job(L.sa.Wo, L.sa.bo, x, x, d);
        TRY(launch_skinny(a, 1, xn, skp, st));
        a = sk(x, L.ca.ln_g, L.ca.ln_b, d, d);
        a.job[0] = sk_job(L.ca.Wq, L.ca.bq, nullptr, q, d);
        TRY(launch_skinny(a, 1, xn, skp, st));
        if (cap && c.listed[l]) {
            hipLaunchKernelGGL(wh_xattn_row_kernel, dim3(cap->nh, B), dim3(WH_XROW_NT), 0, st, q, enc_state_dev + (size_t)(2 * l) * clay, (long)S * d, S, d, l,
                               c.heads_dev, (const int*)s.pos, (const int*)s.done, (const int*)(s.ti + TS_FIRSTROW * WH_MAXB), cap->max_rows, cap->xattn_dev);
            LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(wh_attn_part_kernel, dim3(w.nch_cross, H, B), dim3(256), 0, st, q, enc_state_dev + (size_t)(2 * l) * clay,
                           enc_state_dev + (size_t)(2 * l + 1) * clay, (long)S * d, d, (const int*)nullptr, S, part);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(wh_attn_comb_kernel, dim3(H, B), dim3(64), 0, st, part, w.nch_cross, ao, d);
        LAUNCH_CHECK();
        a = sk(ao, nullptr, nullptr, d, d);
        a.job[0] = sk_job(L.ca.Wo, L.ca.bo, x, x, d);
        TRY(launch_skinny(a, 1, xn, skp, st));
        a = sk(x, L.ln3_g, L.ln3_b, ffn, d);
        a.job[0] = sk_job(L.W1, L.b1, nullptr, hb, ffn, 0, 1);
        TRY(launch_skinny(a, 1, xn, skp, st));
        a = sk(hb, nullptr, nullptr, d, ffn);
        a.job[0] = sk_job(L.W2, L.b2, x, x, d);
        TRY(launch_skinny(a, 1, xn, skp, st));
    }
    return TDX_OK;
}

// The host image of the rows' state (rows TS_PLEN .. TS_FIRSTROW of `ti`) and every row's prefix at pitch T.
struct WhRows {
    std::vector<int> st, prefix;
    int T, p_end = 0;
    WhRows(int B, int T_) : st((size_t)(TS_FIRSTROW + 1) * WH_MAXB, 0), prefix((size_t)B * T_, 0), T(T_) {}
    // steps p = 0 .. pend - 1 read the token at position p and write cache row p (< T); the tokens at positions plen .. gen_to are
    // generated by the steps plen - 1 .. gen_to - 1.  With nothing to generate the prefix is still scored whole.
    void set(int b, int plen, int begin, int max_new, int sot, int first_row) {
        const int gen_to = plen - 1 + std::min(max_new, T - plen), pend = std::max(plen, gen_to);
        st[TS_PLEN * WH_MAXB + b] = plen; st[TS_BEGIN * WH_MAXB + b] = begin; st[TS_PEND * WH_MAXB + b] = pend; st[TS_GENTO * WH_MAXB + b] = gen_to;
        st[TS_SOT * WH_MAXB + b] = sot; st[TS_FIRSTROW * WH_MAXB + b] = first_row;
        p_end = std::max(p_end, pend);
    }
};

// The decode loop of the three entry points, which have checked their own arguments and filled `rows`: the static mask, the
// workspace check, the uploads, the init launch, then 16 steps at a time (decoder layers, head, next) and one pinned read.
// rules.on selects the head's instantiation; nospeech_dev (rules on only) asks for the no-speech pair.  draws (rules on only):
// tdx_whisper_decode_ts_sample's temperatures, streams and seed; the head and the step then run their sampling instantiations
// and the workspace carries sample_ws behind the common one.
struct WhDraws { std::vector<float> temp; std::vector<unsigned long long> stream; unsigned long long seed; };
static int wh_decode_run(const std::string& fn, tdx_whisper* h, const float* enc_state_dev, int B, const WhRows& rows, const WhTsRules& rules,
                         const int* suppress_host, int n_suppress, const int* begin_suppress_host, int n_begin, int no_speech_id, float* nospeech_dev,
                         const WhCapture* cap, const std::vector<char>& listed, int* step_ids_dev, float* step_scores_dev, int* counts_dev, void* ws_,
                         size_t ws_bytes, void* stream, const WhDraws* draws = nullptr) {
    const int V = h->c.vocab, T = h->c.n_text_ctx, d = h->c.d_model;
    std::vector<unsigned char> mask;
    TRY(wh_static_mask(fn, V, suppress_host, n_suppress, begin_suppress_host, n_begin, mask));
    if (ws_bytes < (draws ? tdx_whisper_decode_sample_workspace_bytes(h, B) : tdx_whisper_workspace_bytes(h, B)))
        return tdx::fail(TDX_E_WORKSPACE, fn + ": workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    const DecWs w = dec_ws(h, B);
    float* f = (float*)ws_;
    float* x = f + w.x;
    const WhHeadOut ho{f + w.pm, (int*)(f + w.pi), f + w.ps, f + w.nm, f + w.nsum, f + w.nlogit};
    int* sti = (int*)(f + w.state);
    int* ti = (int*)(f + w.ti);
    int* prefix_dev = (int*)(f + w.prefix);
    unsigned char* mask_dev = (unsigned char*)(f + w.mask);
    int* heads_dev = (int*)(f + w.heads);
    const WhState s{sti, sti + WH_MAXB, sti + 2 * WH_MAXB, sti + 3 * WH_MAXB, prefix_dev, ti};
    hipError_t rc = hipMemcpyAsync(prefix_dev, rows.prefix.data(), sizeof(int) * rows.prefix.size(), hipMemcpyHostToDevice, st);
    if (rc == hipSuccess) rc = hipMemcpyAsync(ti, rows.st.data(), sizeof(int) * rows.st.size(), hipMemcpyHostToDevice, st);
    if (rc == hipSuccess) rc = hipMemcpyAsync(mask_dev, mask.data(), mask.size(), hipMemcpyHostToDevice, st);
    if (rc == hipSuccess && cap) rc = hipMemcpyAsync(heads_dev, cap->heads_host, sizeof(int) * 2 * cap->nh, hipMemcpyHostToDevice, st);
    WhSample sp{};
    bool sampling = false;                                      // no row with temp > 0: the greedy kernels, nothing uploaded
    for (int b = 0; draws && b < B; ++b) sampling |= draws->temp[b] > 0.f;
    if (sampling) {
        const SampleWs sw = sample_ws(h, B);
        float* g = (float*)((char*)ws_ + tdx_whisper_workspace_bytes(h, B));
        sp = WhSample{g + sw.temp, (const unsigned long long*)(g + sw.stream), draws->seed, g + sw.zm, (int*)(g + sw.zi), g + sw.zv};
        if (rc == hipSuccess) rc = hipMemcpyAsync(g + sw.temp, draws->temp.data(), sizeof(float) * B, hipMemcpyHostToDevice, st);
        if (rc == hipSuccess) rc = hipMemcpyAsync(g + sw.stream, draws->stream.data(), sizeof(unsigned long long) * B, hipMemcpyHostToDevice, st);
    }
    if (rc != hipSuccess) return tdx::fail_hip(rc, __FILE__, __LINE__);
    hipLaunchKernelGGL(wh_init_kernel, dim3(1), dim3(64), 0, st, s, B, T, rules, counts_dev);
    LAUNCH_CHECK();
    const WhStepCtx ctx{h, &w, f, s, B, enc_state_dev, cap, listed.data(), (const int*)heads_dev, st};
    const int* bnd = ti + TS_BND * WH_MAXB;
    int status = TDX_OK;
    auto step = [&]() -> int {
        TRY(wh_decoder_step(ctx));
        SkArgs a = wh_sk_args(s, B, x, h->dln_g, h->dln_b, V, d);
        a.job[0] = sk_job(h->tok, nullptr, nullptr, nullptr, 0);
        if (sampling) {
            TRY((launch_head<true, true>(a, mask_dev, bnd, rules.tb, nospeech_dev != nullptr, no_speech_id, ho, w.nsl, st, sp)));
            hipLaunchKernelGGL(wh_next_kernel<true>, dim3(1), dim3(32 * B), 0, st, ho, w.nsl, s, B, T, rules, step_ids_dev, step_scores_dev, counts_dev,
                               nospeech_dev, sp);
        } else {
            TRY(rules.on ? launch_head<true>(a, mask_dev, bnd, rules.tb, nospeech_dev != nullptr, no_speech_id, ho, w.nsl, st)
                         : launch_head<false>(a, mask_dev, bnd, 0, 0, 0, ho, w.nsl, st));
            hipLaunchKernelGGL(wh_next_kernel<false>, dim3(1), dim3(32 * B), 0, st, ho, w.nsl, s, B, T, rules, step_ids_dev, step_scores_dev, counts_dev,
                               nospeech_dev, sp);
        }
        LAUNCH_CHECK();
        return TDX_OK;
    };
    for (int p = 0; p < rows.p_end && status == TDX_OK;) {
        const int n = std::min(WH_CHUNK, rows.p_end - p);
        for (int i = 0; i < n && status == TDX_OK; ++i) status = step();
        p += n;
        // one host read per chunk: the number of finished clips (also what keeps the host copies alive until they have been read)
        rc = hipMemcpyAsync(h->pinned, s.ndone, sizeof(int), hipMemcpyDeviceToHost, st);
        if (rc == hipSuccess) rc = hipStreamSynchronize(st);
        if (rc != hipSuccess) return tdx::fail_hip(rc, __FILE__, __LINE__);
        if (*h->pinned >= B) break;
    }
    return status;
}

// tdx_whisper_decode and tdx_whisper_decode_xattn: one prefix for every row, begin = prefix_len, no rules, no no-speech pair
static int wh_decode_plain(const std::string& fn, const WhCapture* cap, tdx_whisper* h, const float* enc_state_dev, int B, const int* prefix_host,
                           int prefix_len, const int* suppress_host, int n_suppress, const int* begin_suppress_host, int n_begin, int eos, int max_new,
                           int* step_ids_dev, float* step_scores_dev, int* counts_dev, void* ws_, size_t ws_bytes, void* stream) {
    if (cap) TRY(wh_check_capture(fn, *cap));
    if (!h || !enc_state_dev || !prefix_host || !step_ids_dev || !step_scores_dev || !counts_dev || !ws_ || B < 1 || B > WH_MAXB || prefix_len < 1 ||
        n_suppress < 0 || n_begin < 0 || (n_suppress > 0 && !suppress_host) || (n_begin > 0 && !begin_suppress_host) || max_new < 0)
        return tdx::fail(TDX_E_INVALID, fn + ": bad argument (1 <= B <= 32, prefix_len >= 1, max_new >= 0)");
    const tdx_whisper_config& c = h->c;
    const int V = c.vocab, T = c.n_text_ctx;
    if (prefix_len > T) return tdx::fail(TDX_E_INVALID, fn + ": the prefix is longer than n_text_ctx");
    std::vector<char> listed(c.dec_layers, 0);
    if (cap) TRY(wh_listed_layers(fn, *cap, c.dec_layers, c.dec_heads, listed));
    if (eos < 0 || eos >= V) return tdx::fail(TDX_E_INVALID, fn + ": eos outside the vocabulary");
    for (int i = 0; i < prefix_len; ++i)
        if (prefix_host[i] < 0 || prefix_host[i] >= V) return tdx::fail(TDX_E_INVALID, fn + ": prefix id outside the vocabulary");
    WhRows rows(B, T);
    for (int b = 0; b < B; ++b) {
        std::copy(prefix_host, prefix_host + prefix_len, rows.prefix.begin() + (size_t)b * T);
        rows.set(b, prefix_len, prefix_len, max_new, -1, cap ? cap->first_row : 0);
    }
    return wh_decode_run(fn, h, enc_state_dev, B, rows, WhTsRules{0, 0, eos, V, -1}, suppress_host, n_suppress, begin_suppress_host, n_begin, 0, nullptr, cap,
                         listed, step_ids_dev, step_scores_dev, counts_dev, ws_, ws_bytes, stream);
}

int tdx_whisper_decode(tdx_whisper* h, const float* enc_state_dev, int B, const int* prefix_host, int prefix_len, const int* suppress_host, int n_suppress,
                       const int* begin_suppress_host, int n_begin, int eos, int max_new, int* step_ids_dev, float* step_scores_dev, int* counts_dev,
                       void* ws_, size_t ws_bytes, void* stream) {
    return wh_decode_plain("tdx_whisper_decode", nullptr, h, enc_state_dev, B, prefix_host, prefix_len, suppress_host, n_suppress, begin_suppress_host,
                           n_begin, eos, max_new, step_ids_dev, step_scores_dev, counts_dev, ws_, ws_bytes, stream);
}

int tdx_whisper_decode_xattn(tdx_whisper* h, const float* enc_state_dev, int B, const int* prefix_host, int prefix_len, const int* suppress_host,
                             int n_suppress, const int* begin_suppress_host, int n_begin, int eos, int max_new, const int* heads_host, int nh,
                             int first_row, int max_rows, float* xattn_dev, int* step_ids_dev, float* step_scores_dev, int* counts_dev, void* ws_,
                             size_t ws_bytes, void* stream) {
    const WhCapture cap{heads_host, nh, first_row, max_rows, xattn_dev};
    return wh_decode_plain("tdx_whisper_decode_xattn", &cap, h, enc_state_dev, B, prefix_host, prefix_len, suppress_host, n_suppress,
                           begin_suppress_host, n_begin, eos, max_new, step_ids_dev, step_scores_dev, counts_dev, ws_, ws_bytes, stream);
}

// tdx_whisper_decode_ts and, with draws, tdx_whisper_decode_ts_sample
static int wh_decode_ts(const std::string& fn, const WhDraws* draws, tdx_whisper* h, const float* enc_state_dev, int B, const int* prefix_host, int max_prefix,
                        const int* prefix_len_host, const int* begin_host, const int* suppress_host, int n_suppress, const int* begin_suppress_host,
                        int n_begin, int eos, int no_timestamps_id, int max_initial_timestamp_index, const int* max_new_host, int no_speech_id,
                        const int* sot_pos_host, float* nospeech_dev, const int* heads_host, int nh, const int* first_row_host, int max_rows,
                        float* xattn_dev, int* step_ids_dev, float* step_scores_dev, int* counts_dev, void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !enc_state_dev || !prefix_host || !prefix_len_host || !max_new_host || !step_ids_dev || !step_scores_dev || !counts_dev || !ws_ || B < 1 ||
        B > WH_MAXB || max_prefix < 1 || n_suppress < 0 || n_begin < 0 || (n_suppress > 0 && !suppress_host) || (n_begin > 0 && !begin_suppress_host))
        return tdx::fail(TDX_E_INVALID, fn + ": bad argument (1 <= B <= 32, max_prefix >= 1)");
    const tdx_whisper_config& c = h->c;
    const int V = c.vocab, T = c.n_text_ctx;
    const int tb = no_timestamps_id + 1;
    if (no_timestamps_id < 0 || tb >= V) return tdx::fail(TDX_E_INVALID, fn + ": the first timestamp id (no_timestamps_id + 1) is outside the vocabulary");
    if (eos < 0 || eos >= V) return tdx::fail(TDX_E_INVALID, fn + ": eos outside the vocabulary");
    if (eos >= tb) return tdx::fail(TDX_E_INVALID, fn + ": eos must be below the first timestamp id");
    if (nospeech_dev && !sot_pos_host) return tdx::fail(TDX_E_INVALID, fn + ": sot_pos_host must not be NULL when nospeech_dev is given");
    if (nospeech_dev && (no_speech_id < 0 || no_speech_id >= V)) return tdx::fail(TDX_E_INVALID, fn + ": no_speech_id outside the vocabulary");
    const WhCapture capv{heads_host, nh, 0, max_rows, xattn_dev};
    const WhCapture* cap = heads_host ? &capv : nullptr;
    std::vector<char> listed(c.dec_layers, 0);
    if (cap) {
        TRY(wh_check_capture(fn, *cap));
        TRY(wh_listed_layers(fn, *cap, c.dec_layers, c.dec_heads, listed));
    }
    WhRows rows(B, T);
    for (int b = 0; b < B; ++b) {
        const int pl = prefix_len_host[b];
        const std::string row = "row " + std::to_string(b);
        if (pl < 1 || pl > max_prefix) return tdx::fail(TDX_E_INVALID, fn + ": prefix_len of " + row + " outside [1, max_prefix]");
        if (pl >= T) return tdx::fail(TDX_E_INVALID, fn + ": the prefix of " + row + " leaves no room in n_text_ctx");
        if (max_new_host[b] < 0) return tdx::fail(TDX_E_INVALID, fn + ": max_new of " + row + " is negative");
        const int bg = begin_host ? begin_host[b] : pl;
        if (bg < 1 || bg > pl) return tdx::fail(TDX_E_INVALID, fn + ": begin of " + row + " outside [1, prefix_len]");
        if (nospeech_dev && (sot_pos_host[b] < 0 || sot_pos_host[b] >= pl)) return tdx::fail(TDX_E_INVALID, fn + ": sot_pos of " + row + " outside its prefix");
        const int fr = first_row_host ? first_row_host[b] : pl;
        if (cap && fr < 0) return tdx::fail(TDX_E_INVALID, fn + ": first_row of " + row + " is negative");
        for (int i = 0; i < pl; ++i) {
            const int id = prefix_host[(size_t)b * max_prefix + i];
            if (id < 0 || id >= V) return tdx::fail(TDX_E_INVALID, fn + ": prefix id outside the vocabulary");
            rows.prefix[(size_t)b * T + i] = id;
        }
        rows.set(b, pl, bg, max_new_host[b], nospeech_dev ? sot_pos_host[b] : -1, fr);
    }
    // (an index past the last timestamp id allows every timestamp: clamped, so that tb + index cannot overflow)
    const WhTsRules rules{1, tb, eos, V, std::min(max_initial_timestamp_index, V - 1 - tb)};
    return wh_decode_run(fn, h, enc_state_dev, B, rows, rules, suppress_host, n_suppress, begin_suppress_host, n_begin, no_speech_id, nospeech_dev, cap, listed,
                         step_ids_dev, step_scores_dev, counts_dev, ws_, ws_bytes, stream, draws);
}

int tdx_whisper_decode_ts(tdx_whisper* h, const float* enc_state_dev, int B, const int* prefix_host, int max_prefix, const int* prefix_len_host,
                          const int* begin_host, const int* suppress_host, int n_suppress, const int* begin_suppress_host, int n_begin, int eos,
                          int no_timestamps_id, int max_initial_timestamp_index, const int* max_new_host, int no_speech_id, const int* sot_pos_host,
                          float* nospeech_dev, const int* heads_host, int nh, const int* first_row_host, int max_rows, float* xattn_dev,
                          int* step_ids_dev, float* step_scores_dev, int* counts_dev, void* ws_, size_t ws_bytes, void* stream) {
    return wh_decode_ts("tdx_whisper_decode_ts", nullptr, h, enc_state_dev, B, prefix_host, max_prefix, prefix_len_host, begin_host, suppress_host, n_suppress,
                        begin_suppress_host, n_begin, eos, no_timestamps_id, max_initial_timestamp_index, max_new_host, no_speech_id, sot_pos_host,
                        nospeech_dev, heads_host, nh, first_row_host, max_rows, xattn_dev, step_ids_dev, step_scores_dev, counts_dev, ws_, ws_bytes, stream);
}

int tdx_whisper_decode_ts_sample(tdx_whisper* h, const float* enc_state_dev, int B, const int* prefix_host, int max_prefix, const int* prefix_len_host,
                                 const int* begin_host, const int* suppress_host, int n_suppress, const int* begin_suppress_host, int n_begin, int eos,
                                 int no_timestamps_id, int max_initial_timestamp_index, const int* max_new_host, int no_speech_id,
                                 const int* sot_pos_host, float* nospeech_dev, const int* heads_host, int nh, const int* first_row_host, int max_rows,
                                 float* xattn_dev, int* step_ids_dev, float* step_scores_dev, int* counts_dev, const float* temperature_host,
                                 const unsigned long long* stream_host, unsigned long long seed, void* ws_, size_t ws_bytes, void* stream) {
    const std::string fn = "tdx_whisper_decode_ts_sample";
    if (B < 1 || B > WH_MAXB) return tdx::fail(TDX_E_INVALID, fn + ": bad argument (1 <= B <= 32, max_prefix >= 1)");
    if (!temperature_host) return tdx::fail(TDX_E_INVALID, fn + ": temperature_host must not be NULL");
    if (!stream_host) return tdx::fail(TDX_E_INVALID, fn + ": stream_host must not be NULL");
    WhDraws draws{std::vector<float>(temperature_host, temperature_host + B), std::vector<unsigned long long>(stream_host, stream_host + B), seed};
    for (int b = 0; b < B; ++b)
        if (!(draws.temp[b] >= 0.f) || std::isinf(draws.temp[b]))
            return tdx::fail(TDX_E_INVALID, fn + ": temperature of row " + std::to_string(b) + " must be finite and not negative");
    return wh_decode_ts(fn, &draws, h, enc_state_dev, B, prefix_host, max_prefix, prefix_len_host, begin_host, suppress_host, n_suppress, begin_suppress_host,
                        n_begin, eos, no_timestamps_id, max_initial_timestamp_index, max_new_host, no_speech_id, sot_pos_host, nospeech_dev, heads_host, nh,
                        first_row_host, max_rows, xattn_dev, step_ids_dev, step_scores_dev, counts_dev, ws_, ws_bytes, stream);
}

constexpr int WH_LONG_FBLK = 4096;
constexpr long WH_LONG_MAXN = 1L << 30;

size_t tdx_whisper_logmel_long_workspace_bytes(const tdx_whisper* h, long N) {
    if (!h || N < 1 || N > WH_LONG_MAXN) return 0;
    const size_t nb = (size_t)std::max<long>(1, std::min<long>(WH_LONG_FBLK, N / HOP));
    return (al((nb + 3) * HOP) + al(nb * PWP) + al(WH_MAXPART)) * sizeof(float);
}

int tdx_whisper_logmel_long(tdx_whisper* h, const float* wav_dev, long N, float* feat_dev, void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !wav_dev || !ws_) return tdx::fail(TDX_E_INVALID, "tdx_whisper_logmel_long: NULL argument");
    if (N < 1 || N > WH_LONG_MAXN) return tdx::fail(TDX_E_INVALID, "tdx_whisper_logmel_long: N must be in [1, 2^30]");
    const long F = N / HOP;
    if (F == 0) return TDX_OK;                                   // shorter than one hop: no frame, nothing to write
    if (!feat_dev) return tdx::fail(TDX_E_INVALID, "tdx_whisper_logmel_long: feat_dev must not be NULL");
    if (ws_bytes < tdx_whisper_logmel_long_workspace_bytes(h, N)) return tdx::fail(TDX_E_WORKSPACE, "tdx_whisper_logmel_long: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    const size_t nbmax = (size_t)std::min<long>(WH_LONG_FBLK, F);
    float* pad = (float*)ws_;
    float* pw = pad + al((nbmax + 3) * HOP);
    float* part = pw + al(nbmax * PWP);
    for (long f0 = 0; f0 < F; f0 += WH_LONG_FBLK) {
        const int nb = (int)std::min<long>(WH_LONG_FBLK, F - f0);
        // row r of the block is frame f0 + r: KFR floats from pad + HOP r; the last row ends at HOP nb + 256, 224 floats before count
        const int count = (nb + 3) * HOP;
        hipLaunchKernelGGL(wh_pad_long_kernel, dim3((count + 255) / 256), dim3(256), 0, st, wav_dev, N, f0 * HOP, count, pad);
        LAUNCH_CHECK();
        TRY((linear_f32<true>(pad, HOP, h->dft, nb, NBINP, KFR, EpiPow{pw}, st, 0, NBINP)));
        // EpiLogMelT with one "clip" whose map starts at frame f0 of the row pitch F
        TRY(linear_f32(pw, PWP, h->melw, nb, MELP, PWP, EpiLogMelT{feat_dev + f0, INT_MAX, (int)F, h->c.n_mels}, st));
    }
    const long n = (long)h->c.n_mels * F;
    hipLaunchKernelGGL(wh_max_part_kernel, dim3(WH_MAXPART), dim3(1024), 0, st, (const float*)feat_dev, n, part);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(wh_clamp_long_kernel, dim3(WH_MAXPART), dim3(1024), 0, st, feat_dev, n, (const float*)part);
    LAUNCH_CHECK();
    return TDX_OK;
}

size_t tdx_token_align_workspace_bytes(int B, int nh, int max_rows, int n_audio_ctx) {
    if (B < 1 || B > 65535 || nh < 1 || nh > WH_MAXHEADS || max_rows < 1 || max_rows > AL_MAXROWS || n_audio_ctx < 1 || n_audio_ctx > WH_MAXCTX) return 0;
    return align_ws(B, nh, max_rows, n_audio_ctx).total * sizeof(float);
}

int tdx_token_align(const float* xattn_dev, int B, int nh, int max_rows, int n_audio_ctx, const int* nrows_dev, const int* nframes_dev, int median_width,
                    int* frames_dev, float* matrix_dev, void* ws_, size_t ws_bytes, void* stream) {
    if (nh < 1 || nh > WH_MAXHEADS) return tdx::fail(TDX_E_INVALID, "tdx_token_align: nh must be in [1, 64]");
    if (max_rows < 1 || max_rows > AL_MAXROWS) return tdx::fail(TDX_E_INVALID, "tdx_token_align: max_rows must be in [1, 2048]");
    if (median_width < 1 || median_width > AL_MAXW || median_width % 2 == 0)
        return tdx::fail(TDX_E_INVALID, "tdx_token_align: median_width must be odd and in [1, 31]");
    if (B < 1 || B > 65535 || n_audio_ctx < 1 || n_audio_ctx > WH_MAXCTX)
        return tdx::fail(TDX_E_INVALID, "tdx_token_align: bad argument (1 <= B <= 65535, 1 <= n_audio_ctx <= 32768)");
    if (!xattn_dev || !nrows_dev || !nframes_dev || !frames_dev || !ws_) return tdx::fail(TDX_E_INVALID, "tdx_token_align: NULL argument");
    if (ws_bytes < tdx_token_align_workspace_bytes(B, nh, max_rows, n_audio_ctx)) return tdx::fail(TDX_E_WORKSPACE, "tdx_token_align: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int S = n_audio_ctx;
    const AlignWs w = align_ws(B, nh, max_rows, S);
    float* f = (float*)ws_;
    float *mean = f + w.mean, *sd = f + w.sd, *M = matrix_dev ? matrix_dev : f + w.M;
    unsigned char* trace = (unsigned char*)(f + w.trace);
    const unsigned nb = (unsigned)((S + 255) / 256);
    hipLaunchKernelGGL(al_stats_kernel, dim3(nb, nh, B), dim3(256), 0, st, xattn_dev, max_rows, S, nrows_dev, nframes_dev, mean, sd);
    LAUNCH_CHECK();
    if (median_width == 7)
        hipLaunchKernelGGL(al_filter_kernel<7>, dim3(nb, max_rows, B), dim3(256), 0, st, xattn_dev, nh, max_rows, S, nrows_dev, nframes_dev, 7, (const float*)mean,
                           (const float*)sd, M);
    else
        hipLaunchKernelGGL(al_filter_kernel<0>, dim3(nb, max_rows, B), dim3(256), 0, st, xattn_dev, nh, max_rows, S, nrows_dev, nframes_dev, median_width,
                           (const float*)mean, (const float*)sd, M);
    LAUNCH_CHECK();
    if (max_rows <= AL_NT)
        hipLaunchKernelGGL(al_dtw_kernel<1>, dim3(B), dim3(AL_NT), 0, st, (const float*)M, max_rows, S, nrows_dev, nframes_dev, trace, frames_dev);
    else if (max_rows <= 2 * AL_NT)
        hipLaunchKernelGGL(al_dtw_kernel<2>, dim3(B), dim3(AL_NT), 0, st, (const float*)M, max_rows, S, nrows_dev, nframes_dev, trace, frames_dev);
    else
        hipLaunchKernelGGL(al_dtw_kernel<4>, dim3(B), dim3(AL_NT), 0, st, (const float*)M, max_rows, S, nrows_dev, nframes_dev, trace, frames_dev);
    LAUNCH_CHECK();
    return TDX_OK;
}

}  // extern "C"
