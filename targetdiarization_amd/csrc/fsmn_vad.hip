// fsmn_vad.hip — FSMN-VAD (funasr fsmn_vad_streaming: WavFrontend LFR 5/1 + CMVN, two input linears, four FSMN blocks with a
// causal 20-tap depthwise memory, two output linears, softmax over 248) on MI355X.  Replaces `self.vad.generate(...)` in
// ASRProcessor.vad_detection (ASRProcessor.py:742-817); third-party, parity unpinned [upstream-recall] —
// tests/fsmn_vad_oracle.py restates the network.  The segmenter (E2EVadModel's window detector) stays on the host
// (targetdiarization_amd/vad.py): it is a sequential scan over one bit per frame.
// feat [rows,80] (tdx_fbank mode 1; the frames of all clips packed back to back) + starts [nclips+1] -> p0 [rows] (posterior
// of class 0, the only silence class) and, when asked, the whole posterior [rows,248].
//
// The model is ~0.85 MFLOP per frame: its cost is launches and bytes.  16 launches per forward, whatever nclips:
//   lfr_cmvn_kernel                 A0[rows][416] = ((frames t-2..t+2, clamped to the row's clip) + shift) * scale, zero pad;
//                                   also writes the row -> clip-start table the memory kernel reads
//   GEMM  in_linear2 . in_linear1   [250 x 400] folded on the host in fp64 (no activation between them), + bias, ReLU
//   4 x { GEMM linear (250 -> 128, no bias) ; memory_kernel ; GEMM affine (128 -> 250) + bias, ReLU }
//   GEMM  out_linear2 . out_linear1 [248 x 250] folded likewise, + bias
//   softmax_kernel                  one wave per row
// Dense layers: fp32 MFMA core (gemm.hpp), dimensions zero-padded to its tiles (400 -> 416, 250 -> 256, 248 -> 256); the padded
// weight rows and bias entries are zero, so the padded output columns are written as exact zeros and the next GEMM's padded K
// columns never see uninitialised memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tdx.h"
#include "epilogues.hpp"
#include "weight_pack.hpp"

using namespace tdx;

namespace {

constexpr int NMEL = 80, LFR_M = 5, DIN = 400, DINP = 416, H1 = 140, DL = 250, DLP = 256, DP = 128, TAPS = 20, NLAYER = 4;
constexpr int NCLS = 248, NCLSP = 256;
constexpr int MAX_ROWS = 1 << 22;
constexpr int LFR_ROWS = 16;          // rows per block of lfr_cmvn_kernel
constexpr int MEM_ROWS = 8;           // consecutive rows per thread of memory_kernel

// (a) LFR 5/1 + CMVN.  Row t of clip [s, e): columns j*80 + q = (feat[clamp(t-2+j, s, e-1)][q] + shift) * scale, j = 0..4;
// columns 400..415 are the GEMM's K padding (zero).  The first LFR_ROWS threads find their row's clip by binary search
// (starts is ascending, starts[0] = 0, starts[nclips] = rows; empty clips are legal) and publish its start in cstart[].
__global__ __launch_bounds__(256) void lfr_cmvn_kernel(const float* __restrict__ feat, const int* __restrict__ starts, int nclips,
                                                        const float* __restrict__ shift, const float* __restrict__ scale,
                                                        float* __restrict__ a0, int* __restrict__ cstart, int rows) {
    __shared__ int s_lo[LFR_ROWS], s_hi[LFR_ROWS];
    const int r0 = blockIdx.x * LFR_ROWS, tid = threadIdx.x;
    if (tid < LFR_ROWS) {
        const int t = r0 + tid;
        int lo = 0, hi = 0;
        if (t < rows) {
            int a = 0, b = nclips;              // the last c with starts[c] <= t
            while (b - a > 1) { const int mid = (a + b) >> 1; if (starts[mid] <= t) a = mid; else b = mid; }
            lo = starts[a]; hi = starts[a + 1];
            cstart[t] = lo;
        }
        s_lo[tid] = lo; s_hi[tid] = hi;
    }
    __syncthreads();
    constexpr int Q = DINP / 4;               // float4 per output row
    for (int i = tid; i < LFR_ROWS * Q; i += 256) {
        const int lr = i / Q, k = (i - lr * Q) * 4, t = r0 + lr;
        if (t >= rows) break;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (k < DIN) {
            const int j = k / NMEL, q = k - j * NMEL;
            const int src = min(max(t - (LFR_M - 1) / 2 + j, s_lo[lr]), s_hi[lr] - 1);
            const f32x4 x = ldg4(feat + (long)src * NMEL + q), sh = ldg4(shift + k), sc = ldg4(scale + k);
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = (x[c] + sh[c]) * sc[c];
        }
        *reinterpret_cast<f32x4*>(a0 + (long)t * DINP + k) = v;
    }
}

// (b) FSMN memory: m[t][c] = p[t][c] + sum_{j=0..19} w[j][c] * p[t-19+j][c], rows before the clip's first frame read as zero.
// A thread owns 4 channels and MEM_ROWS consecutive rows: the 27 source rows are loaded once and the taps stay in registers.
__global__ __launch_bounds__(256) void memory_kernel(const float* __restrict__ p, const float* __restrict__ w,      // w [20][128]
                                                      const int* __restrict__ cstart, float* __restrict__ m, int rows) {
    const int c = (threadIdx.x & 31) * 4;
    const int t0 = (blockIdx.x * 8 + (threadIdx.x >> 5)) * MEM_ROWS;
    if (t0 >= rows) return;
    f32x4 wt[TAPS];
#pragma unroll
    for (int j = 0; j < TAPS; ++j) wt[j] = ldg4(w + j * DP + c);
    int cs[MEM_ROWS];
    f32x4 acc[MEM_ROWS];
#pragma unroll
    for (int r = 0; r < MEM_ROWS; ++r) {
        cs[r] = cstart[min(t0 + r, rows - 1)];
        acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int d = 0; d < MEM_ROWS + TAPS - 1; ++d) {
        const int src = t0 - (TAPS - 1) + d;                    // <= t0 + MEM_ROWS - 1
        const f32x4 v = ldg4(p + (long)min(max(src, 0), rows - 1) * DP + c);
#pragma unroll
        for (int r = 0; r < MEM_ROWS; ++r) {
            const int j = d - r;                                // tap of output row t0 + r that reads src
            if (j < 0 || j >= TAPS) continue;
            const f32x4 u = sel4(src >= cs[r], v);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[r][q] = fmaf(wt[j][q], u[q], acc[r][q]);
            if (j == TAPS - 1) acc[r] += v;                     // the identity path: src == t0 + r
        }
    }
#pragma unroll
    for (int r = 0; r < MEM_ROWS; ++r)
        if (t0 + r < rows) *reinterpret_cast<f32x4*>(m + (long)(t0 + r) * DP + c) = acc[r];
}

// (c) softmax over the 248 classes of a row, one wave per row: p0[t] = posterior of class 0; post[t][0..247] when post != NULL
__global__ __launch_bounds__(256) void softmax_kernel(const float* __restrict__ logits, float* __restrict__ p0, float* __restrict__ post, int rows) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= rows) return;                                                  // wave-uniform: a surplus wave of the last block
    const bool on = lane * 4 < NCLS;
    const f32x4 x = ldg4(logits + (long)t * NCLSP + (on ? lane * 4 : 0));
    float mx = on ? fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])) : -INFINITY;
    mx = wave_max(mx);
    f32x4 e;
#pragma unroll
    for (int q = 0; q < 4; ++q) e[q] = on ? expf(x[q] - mx) : 0.f;
    const float inv = 1.0f / wave_sum((e[0] + e[1]) + (e[2] + e[3]));
    if (lane == 0) p0[t] = e[0] * inv;
    if (post && on) *reinterpret_cast<f32x4*>(post + (long)t * NCLS + lane * 4) = e * inv;
}

struct Lin : tdx::GemmW { bool bias = true; };

// v + b (optionally ReLU); every column of the padded width is stored (see the file comment)
int dense(const float* A, const float* dev, const Lin& l, int M, float* out, bool relu, hipStream_t st) {
    const float* b = l.bias ? dev + l.b : nullptr;
    if (relu) return linear_f32(A, l.Kp, dev + l.w, M, l.Npad, l.Kp, EpiBiasAct<ActRelu>{b, out, l.Npad}, st);
    return linear_f32(A, l.Kp, dev + l.w, M, l.Npad, l.Kp, EpiBiasAct<>{b, out, l.Npad}, st);
}

}  // namespace

struct tdx_fsmnvad {
    int device = 0;
    tdx::DevBuf dev;
    size_t shift, scale;
    Lin in, lin[NLAYER], aff[NLAYER], out;
    size_t mem[NLAYER];
};

extern "C" {

int tdx_fsmnvad_create(const void* blob, size_t blob_bytes, int device, tdx_fsmnvad** out) {
    if (!blob || !out) return tdx::fail(TDX_E_INVALID, "tdx_fsmnvad_create: null argument");
    tdx::Loader ld;
    if (!ld.parse(blob, blob_bytes)) return tdx::fail(TDX_E_BLOB, "tdx_fsmnvad_create: malformed TDXW blob");
    // `b` . `a` : two linears with no activation between them, as one matrix; the product is taken in fp64
    auto folded = [&](const std::string& a, const std::string& b, int Nin, int Nmid, int Nout, int Np, int Kp) -> Lin {
        const float *Wa = ld.get(a + "weight", {(uint32_t)Nmid, (uint32_t)Nin}), *ba = ld.get(a + "bias", {(uint32_t)Nmid});
        const float *Wb = ld.get(b + "weight", {(uint32_t)Nout, (uint32_t)Nmid}), *bb = ld.get(b + "bias", {(uint32_t)Nout});
        std::vector<double> W((size_t)Nout * Nin, 0.0), bias(Nout, 0.0);
        if (ld.ok()) for (int n = 0; n < Nout; ++n) {
            double acc = bb[n];
            for (int j = 0; j < Nmid; ++j) {
                const double wb = Wb[(size_t)n * Nmid + j];
                acc += wb * (double)ba[j];
                const float* ra = Wa + (size_t)j * Nin;
                double* rw = W.data() + (size_t)n * Nin;
                for (int k = 0; k < Nin; ++k) rw[k] += wb * (double)ra[k];
            }
            bias[n] = acc;
        }
        return Lin{tdx::push_linear(ld, W.data(), bias.data(), Nout, Nin, Np, Kp)};
    };
    auto plain = [&](const std::string& p, bool with_bias, int N, int K, int Np, int Kp) -> Lin {
        const float* Wp = ld.get(p + "weight", {(uint32_t)N, (uint32_t)K});
        const float* bp = with_bias ? ld.get(p + "bias", {(uint32_t)N}) : nullptr;
        return Lin{tdx::push_linear(ld, Wp, bp, N, K, Np, Kp), with_bias};
    };
    std::unique_ptr<tdx_fsmnvad> h(new tdx_fsmnvad());
    h->shift = ld.push(ld.get("cmvn.shift", {(uint32_t)DIN}), DIN, DINP);
    h->scale = ld.push(ld.get("cmvn.scale", {(uint32_t)DIN}), DIN, DINP);
    h->in = folded("encoder.in_linear1.linear.", "encoder.in_linear2.linear.", DIN, H1, DL, DLP, DINP);
    for (int i = 0; i < NLAYER; ++i) {
        const std::string p = "encoder.fsmn." + std::to_string(i) + ".";
        h->lin[i] = plain(p + "linear.linear.", false, DP, DL, DP, DLP);
        h->mem[i] = ld.push_tapmajor(ld.get(p + "fsmn_block.conv_left.weight", {(uint32_t)DP, 1u, (uint32_t)TAPS, 1u}), DP, TAPS);      // [128,1,20,1] -> [20][128]
        h->aff[i] = plain(p + "affine.linear.", true, DL, DP, DLP, DP);
    }
    h->out = folded("encoder.out_linear1.linear.", "encoder.out_linear2.linear.", DL, H1, NCLS, NCLSP, DLP);
    h->device = device;
    TRY(ld.finish("tdx_fsmnvad_create", true, device, h->dev));
    *out = h.release();
    return TDX_OK;
}

int tdx_fsmnvad_destroy(tdx_fsmnvad* h) {
    delete h;
    return TDX_OK;
}

namespace {
struct WsPlan { size_t a0, x, p, cstart, total; };
inline WsPlan ws_plan(int rows) {
    WsPlan w{};
    const size_t M = (size_t)rows;
    w.a0 = al(M * DINP + 64); w.x = al(M * DLP + 64); w.p = al(M * DP + 64); w.cstart = al(M + 64);
    w.total = w.a0 + 2 * w.x + 2 * w.p + w.cstart;
    return w;
}
}  // namespace

size_t tdx_fsmnvad_workspace_bytes(const tdx_fsmnvad* h, int rows) {
    if (!h || rows < 1 || rows > MAX_ROWS) return 0;
    return ws_plan(rows).total * sizeof(float);
}

double tdx_fsmnvad_flops(const tdx_fsmnvad* h, int rows) {
    if (!h || rows < 1) return 0.0;
    // the network as published (unfolded): the folded pairs do less work, the figure stays comparable with the reference
    double per = 2.0 * (DIN * H1 + H1 * DL + DL * H1 + H1 * NCLS);
    per += NLAYER * (2.0 * DL * DP + 2.0 * TAPS * DP + 2.0 * DP * DL);
    return per * rows;
}

int tdx_fsmnvad_forward(tdx_fsmnvad* h, const float* feat, const int32_t* starts, int nclips, int rows, float* p0, float* post,
                        void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !feat || !starts || !p0 || !ws_ || nclips < 1) return tdx::fail(TDX_E_INVALID, "tdx_fsmnvad_forward: bad argument");
    if (rows < 1 || rows > MAX_ROWS) return tdx::fail(TDX_E_INVALID, "tdx_fsmnvad_forward: rows must be in [1, 2^22]");
    const WsPlan wp = ws_plan(rows);
    if (ws_bytes < wp.total * sizeof(float)) return tdx::fail(TDX_E_WORKSPACE, "tdx_fsmnvad_forward: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)ws_;
    float* a0 = ws;
    float* x[2] = {a0 + wp.a0, a0 + wp.a0 + wp.x};
    float* p = x[1] + wp.x;
    float* m = p + wp.p;
    int* cstart = (int*)(m + wp.p);
    const float* dev = h->dev;

    hipLaunchKernelGGL(lfr_cmvn_kernel, dim3((unsigned)((rows + LFR_ROWS - 1) / LFR_ROWS)), dim3(256), 0, st, feat, (const int*)starts, nclips,
                       dev + h->shift, dev + h->scale, a0, cstart, rows);
    LAUNCH_CHECK();
    TRY(dense(a0, dev, h->in, rows, x[0], true, st));
    int cur = 0;
    for (int i = 0; i < NLAYER; ++i, cur ^= 1) {
        TRY(dense(x[cur], dev, h->lin[i], rows, p, false, st));
        hipLaunchKernelGGL(memory_kernel, dim3((unsigned)((rows + 8 * MEM_ROWS - 1) / (8 * MEM_ROWS))), dim3(256), 0, st, p, dev + h->mem[i], cstart, m, rows);
        LAUNCH_CHECK();
        TRY(dense(m, dev, h->aff[i], rows, x[cur ^ 1], true, st));
    }
    TRY(dense(x[cur], dev, h->out, rows, x[cur ^ 1], false, st));
    hipLaunchKernelGGL(softmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x[cur ^ 1], p0, post, rows);
    LAUNCH_CHECK();
    return TDX_OK;
}

}  // extern "C"
