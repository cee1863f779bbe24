// silero_vad.hip — silero-VAD v5, 16 kHz branch (a 256-point STFT magnitude at hop 128 over a 640-sample window, four
// Conv1d(k=3) + ReLU, one LSTMCell(128,128) carried from 32 ms chunk to chunk, a 128 -> 1 sigmoid head) on MI355X.  The model
// behind `get_speech_timestamps` in TargetDiarizationStream.should_wait_for_next_chunk (TargetDiarizationStream.py:128-131) and
// AudioProcessor.separate_speaker(low_gpu_ram=True) (AudioProcessor.py:903-905); third-party, parity unpinned
// [upstream-recall] — tests/silero_vad_oracle.py restates the network, DESIGN §8.13 governs.  The state machine that turns
// probabilities into timestamps stays on the host (targetdiarization_amd/silero.py): a sequential scan over one float per chunk.
// wav [total_chunks*512] (clips packed, each zero-padded to whole chunks) + chunk_starts [nclips+1] -> prob [total_chunks];
// taps: the encoder output [total_chunks,128] and the LSTM h [total_chunks,128].
//
// The model is ~1.4 MFLOP per chunk; per clip it is a strictly sequential chain of one LSTM step per chunk.
// 9 launches per forward, whatever nclips and total_chunks (N = total_chunks); everything fp32, activations channel-last:
//   window_kernel    per chunk the 640-sample window: 64 samples of context (zeros at a clip's first chunk), the chunk, 64
//                    samples of right reflect pad (the chunk's own tail mirrored, never the next chunk); also zeroes the
//                    per-chunk padding frames of the two convolution inputs below
//   GEMM (paired)    STFT: frames f = 0..3 of a chunk are window[128f .. 128f+256), i.e. rows of pitch 128 over the windows
//                    (lda = 128, 5 rows per chunk, the fifth is not stored) x basis [256 -> (re_k, im_k) pairs]; the
//                    epilogue has re_k and im_k in one thread and stores sqrt(re^2 + im^2) into X0
//   GEMM x 4         the convolutions over channel-last rows.  X0 / X1 hold 6 frames per chunk [0, f0, f1, f2, f3, 0], so
//                    taps t-1, t, t+1 of a frame are 3C contiguous floats: conv 0 (129 -> 128, stride 1) is lda = C over X0,
//                    conv 1 (128 -> 64, stride 2) is lda = 2C over X1; rows that straddle two chunks are computed and not
//                    stored.  conv 2 (64 -> 64, stride 2, one output frame) reads [f0 | f1] with taps 1, 2 only and conv 3
//                    (64 -> 128, one frame in, one out) the middle tap only: the taps dropped multiply the zero frames.
//                    bias + ReLU in the epilogues
//   GEMM             the LSTM input projection [N,128] x [128,512] + (b_ih + b_hh), columns permuted to unit*4 + gate
//   silero_rec_kernel the recurrence: ONE launch, one workgroup per clip walking chunk_starts[c] .. chunk_starts[c+1]
//   head_kernel      p = sigmoid(w . relu(h) + b), one wave per chunk
// No reduction uses atomics; a row of a GEMM depends on its own A row alone and the recurrence on its clip alone, so a clip's
// result does not depend on its neighbours in the batch.
//
// The recurrence follows pyannet.hip's lstm_rec_kernel with one direction, one clip per workgroup and per-clip
// lengths: 512 threads, thread (u, q) = (tid / 4, tid % 4) keeps rows i, f, g, o of unit u, columns 32q..32q+31 of W_hh in 128
// registers for the whole launch — here as (i, f) and (g, o) row PAIRS, so that a step's 128 FMAs against the broadcast h are
// 64 packed ones (v_pk_fma_f32).  h goes through LDS, double-buffered (quarter pitch 36 floats), one barrier per step; two DPP
// quad exchanges give every lane of a quad the four gate sums; lane q then evaluates gate q's nonlinearity alone and four quad
// broadcasts hand every lane the four activations (the update is most of a step's vector instructions: DESIGN §8.13, Measured);
// the projected input of step s + 2 is loaded at step s.  The cell update uses expf / tanhf, no fast-math.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tdx.h"
#include "epilogues.hpp"
#include "weight_pack.hpp"

using namespace tdx;

namespace {

constexpr int CHUNK = 512, CTX = 64, WIN = CTX + CHUNK + CTX;              // 640
constexpr int NFFT = 256, HOP = 128, NBIN = 129, NBINP = 192;              // bins padded to the paired GEMM's 64-column tiles
constexpr int WROWS = WIN / HOP;                                           // 5 rows of pitch 128 per window, 4 of them frames
constexpr int NFR = 4, PER = 6;                                            // frames per chunk; rows per chunk of X0 / X1
constexpr int P0 = 160;                                                    // X0 row pitch: 129 channels + zeros (3 * 160 = 15 * 32)
constexpr int C1 = 128, C2 = 64, C3 = 64, C4 = 128;
constexpr int HID = 128, GATES = 4 * HID;
constexpr int NCLIPS_MAX = 1024, CHUNKS_MAX = 1 << 20;
constexpr int REC_THREADS = 512, H_PITCH = 4 * 36;

typedef float f32x2 __attribute__((ext_vector_type(2)));

// (a) windows + the zero frames.  One block per chunk i of the packed batch; the chunk is the first of its clip when
// chunk_starts holds i (binary search: ascending, every clip has >= 1 chunk).
__global__ __launch_bounds__(256) void window_kernel(const float* __restrict__ wav, const int* __restrict__ starts, int nclips,
                                                      float* __restrict__ win, float* __restrict__ x0, float* __restrict__ x1) {
    const int i = blockIdx.x, tid = threadIdx.x;
    int a = 0, b = nclips;                      // the last c with starts[c] <= i
    while (b - a > 1) { const int mid = (a + b) >> 1; if (starts[mid] <= i) a = mid; else b = mid; }
    const bool first = i == 0 || starts[a] == i;
    const float* x = wav + (size_t)i * CHUNK;
    float* w = win + (size_t)i * WIN;
    for (int p = tid; p < WIN; p += 256) {
        float v;
        if (p < CTX) v = first ? 0.f : x[p - CTX];
        else if (p < CTX + CHUNK) v = x[p - CTX];
        else v = x[2 * (CTX + CHUNK) - 2 - p - CTX];          // window position 574 - (p - 576)
        w[p] = v;
    }
    float* z0 = x0 + (size_t)i * PER * P0;
    for (int p = tid; p < 2 * P0; p += 256) z0[p < P0 ? p : (PER - 1) * P0 + p - P0] = 0.f;
    float* z1 = x1 + (size_t)i * PER * C1;
    z1[tid < C1 ? tid : (PER - 1) * C1 + tid - C1] = 0.f;
}

// STFT magnitude from the (re_k, im_k) column pair; window row m = 5 i + f -> X0 row 6 i + 1 + f, all P0 columns (the basis
// rows past bin 128 are zero, so the padding columns are stored as exact zeros)
struct EpiMag {
    float* x0;
    __device__ EpiNone col(int, int) const { return EpiNone{}; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store2(int, int m, int c, float re, float im, EpiNone, EpiNone) const {
        const int i = m / WROWS, f = m - i * WROWS;
        if (f < NFR && c < P0) x0[((long)i * PER + 1 + f) * P0 + c] = sqrtf(re * re + im * im);
    }
};

// a convolution's rows: GEMM row m = per * i + t is output frame t of chunk i when t < keep; stored with bias + ReLU at
// out[i * cs + t * fs + off + n], n < nreal
struct EpiFrames {
    const float* b; float* out; int per, keep, cs, fs, off, nreal;
    __device__ float col(int, int n) const { return b[n]; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int, int m, int n, float v, EpiNone, float c) const {
        const int i = m / per, t = m - i * per;
        if (t < keep && n < nreal) out[(long)i * cs + t * fs + off + n] = fmaxf(v + c, 0.f);
    }
};

// lane L of the caller's quad to all four lanes (DPP quad_perm [L,L,L,L])
template <int L>
__device__ __forceinline__ float quad_bcast(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), L * 0x55, 0xF, 0xF, true));
}

// (b) the recurrence (file comment).  xp [N][512]: column u*4 + gate (i, f, g, o); whh [512][128]: row u*4 + gate;
// y [N][128].  Workgroup c walks chunks [starts[c], starts[c+1]) clamped to [0, total].
__global__ __launch_bounds__(REC_THREADS) void silero_rec_kernel(const float* __restrict__ xp, const float* __restrict__ whh,
                                                                  const int* __restrict__ starts, int total, float* __restrict__ y) {
    __shared__ __attribute__((aligned(16))) float hs[2][H_PITCH];
    const int tid = threadIdx.x, u = tid >> 2, q = tid & 3;
    const int s0 = max(starts[blockIdx.x], 0), n = min(starts[blockIdx.x + 1], total) - s0;
    if (n <= 0) return;
    f32x2 wif[32], wgo[32];
    {
        const float* wp = whh + (size_t)(u * 4) * HID + q * 32;
#pragma unroll
        for (int k = 0; k < 32; k += 4) {
            const f32x4 vi = ldg4(wp + k), vf = ldg4(wp + HID + k), vg = ldg4(wp + 2 * HID + k), vo = ldg4(wp + 3 * HID + k);
#pragma unroll
            for (int j = 0; j < 4; ++j) { wif[k + j] = f32x2{vi[j], vf[j]}; wgo[k + j] = f32x2{vg[j], vo[j]}; }
        }
    }
    if (tid < H_PITCH) hs[0][tid] = 0.f;
    const float* xcol = xp + (size_t)s0 * GATES + tid;
    float c = 0.f, xa = xcol[0], xb = n > 1 ? xcol[GATES] : 0.f;
    const int hw = (u >> 5) * 36 + (u & 31);
    float* yo = y + (size_t)s0 * HID + u;
    __syncthreads();
    for (int s = 0; s < n; ++s) {
        const int cur = s & 1;
        const float xc = xa;
        xa = xb;
        if (s + 2 < n) xb = xcol[(size_t)(s + 2) * GATES];
        f32x2 aif = {q == 0 ? xc : 0.f, q == 1 ? xc : 0.f}, ago = {q == 2 ? xc : 0.f, q == 3 ? xc : 0.f};
        f32x2 bif = {0.f, 0.f}, bgo = {0.f, 0.f};
        const f32x4* hp = reinterpret_cast<const f32x4*>(&hs[cur][q * 36]);
#pragma unroll
        for (int k4 = 0; k4 < 8; ++k4) {
            const f32x4 hv = hp[k4];
            const f32x2 h0 = {hv[0], hv[0]}, h1 = {hv[1], hv[1]}, h2 = {hv[2], hv[2]}, h3 = {hv[3], hv[3]};
            aif = __builtin_elementwise_fma(wif[k4 * 4], h0, aif);     ago = __builtin_elementwise_fma(wgo[k4 * 4], h0, ago);
            bif = __builtin_elementwise_fma(wif[k4 * 4 + 1], h1, bif); bgo = __builtin_elementwise_fma(wgo[k4 * 4 + 1], h1, bgo);
            aif = __builtin_elementwise_fma(wif[k4 * 4 + 2], h2, aif); ago = __builtin_elementwise_fma(wgo[k4 * 4 + 2], h2, ago);
            bif = __builtin_elementwise_fma(wif[k4 * 4 + 3], h3, bif); bgo = __builtin_elementwise_fma(wgo[k4 * 4 + 3], h3, bgo);
        }
        aif += bif; ago += bgo;
        float a0 = aif[0], a1 = aif[1], a2 = ago[0], a3 = ago[1];
        a0 += h3_dpp(a0, 0); a1 += h3_dpp(a1, 0); a2 += h3_dpp(a2, 0); a3 += h3_dpp(a3, 0);
        a0 += h3_dpp(a0, 1); a1 += h3_dpp(a1, 1); a2 += h3_dpp(a2, 1); a3 += h3_dpp(a3, 1);
        // lane q of the quad evaluates gate q's nonlinearity alone (a wave runs one sigmoid and one tanhf instead of three and
        // one); four quad broadcasts hand every lane the four activations
        const float aq = q == 0 ? a0 : q == 1 ? a1 : q == 2 ? a2 : a3;
        const float act = q == 2 ? tanhf(aq) : sigmoid_full(aq);
        const float cn = fmaf(quad_bcast<1>(act), c, quad_bcast<0>(act) * quad_bcast<2>(act));
        const float h = quad_bcast<3>(act) * tanhf(cn);
        c = cn;
        if (q == 0) {
            hs[cur ^ 1][hw] = h;
            yo[(size_t)s * HID] = h;
        }
        __syncthreads();
    }
}

// (c) the head: p[t] = sigmoid(b + sum_k w[k] relu(h[t][k])), one wave per chunk, lane l takes k = l and l + 64
__global__ __launch_bounds__(256) void head_kernel(const float* __restrict__ h, const float* __restrict__ w, const float* __restrict__ bias,
                                                    float* __restrict__ prob, int rows) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= rows) return;                                                  // wave-uniform
    const float* r = h + (size_t)t * HID;
    const float v = wave_sum(fmaf(w[lane + 64], fmaxf(r[lane + 64], 0.f), w[lane] * fmaxf(r[lane], 0.f)));
    if (lane == 0) prob[t] = sigmoid_full(v + bias[0]);
}

using Conv = tdx::GemmW;

}  // namespace

struct tdx_silero {
    int device = 0;
    tdx::DevBuf dev;
    size_t basis;
    Conv conv[4], proj;
    size_t whh, head_w, head_b;
};

extern "C" {

int tdx_silero_create(const void* blob, size_t blob_bytes, int device, tdx_silero** out) {
    if (!blob || !out) return tdx::fail(TDX_E_INVALID, "tdx_silero_create: null argument");
    tdx::Loader ld;
    if (!ld.parse(blob, blob_bytes)) return tdx::fail(TDX_E_BLOB, "tdx_silero_create: malformed TDXW blob");
    std::unique_ptr<tdx_silero> h(new tdx_silero());
    {   // basis [258][256]: rows 0..128 real, 129..257 imaginary -> [2 * 192][256], re_k at row k, im_k at row 192 + k
        const float* b = ld.get("stft.forward_basis_buffer", {(uint32_t)(2 * NBIN), 1u, (uint32_t)NFFT});
        h->basis = ld.room((size_t)2 * NBINP * NFFT);
        if (b) {
            memcpy(ld.host.data() + h->basis, b, (size_t)NBIN * NFFT * sizeof(float));
            memcpy(ld.host.data() + h->basis + (size_t)NBINP * NFFT, b + (size_t)NBIN * NFFT, (size_t)NBIN * NFFT * sizeof(float));
        }
    }
    // Conv1d weight [Cout][Cin][3] -> GEMM B [Npad][Kp], column (k - k0) * pitch + c for taps k0 .. k0 + nk - 1 (channel-last
    // input rows of `pitch` floats); rows Cout.., columns past Cin of a tap zero
    auto conv = [&](int i, int cout, int cin, int pitch, int k0, int nk) -> Conv {
        const std::string p = "encoder." + std::to_string(i) + ".reparam_conv.";
        const float* w = ld.get(p + "weight", {(uint32_t)cout, (uint32_t)cin, 3u});
        const float* b = ld.get(p + "bias", {(uint32_t)cout});
        return tdx::push_conv_gemm(ld, w, nullptr, b, cout, cin, 3, GEMM_BN, pitch, nk * pitch, k0, nk);
    };
    h->conv[0] = conv(0, C1, NBIN, P0, 0, 3);
    h->conv[1] = conv(1, C2, C1, C1, 0, 3);
    h->conv[2] = conv(2, C3, C2, C2, 1, 2);
    h->conv[3] = conv(3, C4, C3, C3, 1, 1);
    {   // LSTMCell: W_ih rows permuted to u*4 + gate, bias b_ih + b_hh likewise; W_hh in the same row order
        const float* wih = ld.get("decoder.rnn.weight_ih", {(uint32_t)GATES, (uint32_t)HID});
        const float* whh = ld.get("decoder.rnn.weight_hh", {(uint32_t)GATES, (uint32_t)HID});
        const float* bih = ld.get("decoder.rnn.bias_ih", {(uint32_t)GATES});
        const float* bhh = ld.get("decoder.rnn.bias_hh", {(uint32_t)GATES});
        Conv& pj = h->proj;
        pj.N = GATES; pj.Npad = GATES; pj.Kp = HID;
        pj.w = ld.room((size_t)GATES * HID); pj.b = ld.room(GATES);
        h->whh = ld.room((size_t)GATES * HID);
        tdx::push_lstm_gates(ld, wih, whh, bih, bhh, HID, HID, pj, h->whh, 0);
    }
    h->head_w = ld.push(ld.get("decoder.decoder.2.weight", {1u, (uint32_t)HID, 1u}), HID);
    h->head_b = ld.push(ld.get("decoder.decoder.2.bias", {1u}), 1);
    h->device = device;
    TRY(ld.finish("tdx_silero_create", true, device, h->dev));
    *out = h.release();
    return TDX_OK;
}

int tdx_silero_destroy(tdx_silero* h) {
    delete h;
    return TDX_OK;
}

namespace {
struct WsPlan { size_t win, x0, x1, x2, x3, feat, xp, hh, total; };
inline WsPlan ws_plan(int total_chunks) {
    const size_t N = (size_t)total_chunks;
    WsPlan w{};
    w.win = al(N * WIN); w.x0 = al(N * PER * P0); w.x1 = al(N * PER * C1); w.x2 = al(N * 2 * C2); w.x3 = al(N * C3);
    w.feat = al(N * C4); w.xp = al(N * GATES); w.hh = al(N * HID);
    w.total = w.win + w.x0 + w.x1 + w.x2 + w.x3 + w.feat + w.xp + w.hh;
    return w;
}
inline bool in_limits(int nclips, int total_chunks) {
    return nclips >= 1 && nclips <= NCLIPS_MAX && total_chunks >= nclips && total_chunks <= CHUNKS_MAX;
}
}  // namespace

size_t tdx_silero_workspace_bytes(const tdx_silero* h, int nclips, int total_chunks) {
    if (!h || !in_limits(nclips, total_chunks)) return 0;
    return ws_plan(total_chunks).total * sizeof(float);
}

double tdx_silero_flops(const tdx_silero* h, int total_chunks) {
    if (!h || total_chunks < 1) return 0.0;
    double per = 2.0 * NFR * (2 * NBIN) * NFFT;
    per += 2.0 * 3 * (4.0 * C1 * NBIN + 2.0 * C2 * C1 + 1.0 * C3 * C2 + 1.0 * C4 * C3);
    per += 2.0 * 2 * GATES * HID + 2.0 * HID;
    return per * total_chunks;
}

int tdx_silero_forward(tdx_silero* h, const float* wav, const int* starts, int nclips, int total_chunks, float* prob, float* tap_feat,
                       float* tap_h, void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !wav || !starts || !prob || !ws_) return tdx::fail(TDX_E_INVALID, "tdx_silero_forward: bad argument");
    if (!in_limits(nclips, total_chunks))
        return tdx::fail(TDX_E_INVALID, "tdx_silero_forward: need 1 <= nclips <= 1024, every clip >= 1 chunk, total_chunks <= 2^20");
    const WsPlan wp = ws_plan(total_chunks);
    if (ws_bytes < wp.total * sizeof(float)) return tdx::fail(TDX_E_WORKSPACE, "tdx_silero_forward: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    const int N = total_chunks;
    float* win = (float*)ws_;
    float* x0 = win + wp.win; float* x1 = x0 + wp.x0; float* x2 = x1 + wp.x1; float* x3 = x2 + wp.x2;
    float* feat = tap_feat ? tap_feat : x3 + wp.x3;
    float* xp = x3 + wp.x3 + wp.feat;
    float* hh = tap_h ? tap_h : xp + wp.xp;
    const float* dev = h->dev;

    hipLaunchKernelGGL(window_kernel, dim3((unsigned)N), dim3(256), 0, st, wav, starts, nclips, win, x0, x1);
    LAUNCH_CHECK();
    // the last stored row of each overlapping-row GEMM is the last one computed: nothing is read past a buffer's end
    TRY((linear_f32<true>(win, HOP, dev + h->basis, WROWS * N - 1, NBINP, NFFT, EpiMag{x0}, st, 0, NBINP)));
    {
        const Conv& l = h->conv[0];
        TRY(linear_f32(x0, P0, dev + l.w, PER * N - 2, l.Npad, l.Kp, EpiFrames{dev + l.b, x1, PER, NFR, PER * C1, C1, C1, l.N}, st, up(l.N, 32)));
    }
    {
        const Conv& l = h->conv[1];
        TRY(linear_f32(x1, 2 * C1, dev + l.w, 3 * N - 1, l.Npad, l.Kp, EpiFrames{dev + l.b, x2, 3, 2, 2 * C2, C2, 0, l.N}, st, up(l.N, 32)));
    }
    {
        const Conv& l = h->conv[2];
        TRY(linear_f32(x2, 2 * C2, dev + l.w, N, l.Npad, l.Kp, EpiBiasActN<ActRelu>{dev + l.b, x3, C3, l.N}, st, up(l.N, 32)));
    }
    {
        const Conv& l = h->conv[3];
        TRY(linear_f32(x3, C3, dev + l.w, N, l.Npad, l.Kp, EpiBiasAct<ActRelu>{dev + l.b, feat, C4}, st));
    }
    TRY(linear_f32(feat, C4, dev + h->proj.w, N, GATES, HID, EpiBiasAct<>{dev + h->proj.b, xp, GATES}, st));
    hipLaunchKernelGGL(silero_rec_kernel, dim3((unsigned)nclips), dim3(REC_THREADS), 0, st, (const float*)xp, dev + h->whh, starts, N, hh);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(head_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, (const float*)hh, dev + h->head_w, dev + h->head_b, prob, N);
    LAUNCH_CHECK();
    return TDX_OK;
}

}  // extern "C"
