// pf_timestamps.hip — Paraformer's upsampling timestamp predictor on MI355X (funasr CifPredictorV3's second head, as the
// "paraformer-large-vad-punc" bundle of ASRProcessor.py:424 carries it; third-party, parity unpinned, tests/pf_timestamps_oracle.py).
//   enc [B,T,512] --ConvTranspose1d(512,512,3,stride 3)--> [B,3T,512] --BLSTM(512)--> [B,3T,1024] --Linear(1024,1)-->
//   a = relu(smooth * sigmoid(.) - noise) --a *= counts / sum(a)--> us_alphas --integrate-and-fire scan--> us_peaks      (U = 3T)
// The transposed convolution (kernel = stride: no overlap) is ONE GEMM [B*T,512] x [512,1536] whose row (b,t) holds the three
// output frames 3t, 3t+1, 3t+2; the input projection of both LSTM directions is ONE GEMM [B*U,512] x [512,4096] with
// b_ih + b_hh folded in; both run on the x3 core through linear_h3.
//
// The recurrence (pfts_lstm_rec_kernel) is the part nothing else here could serve: with hidden 512 one direction's W_hh is
// 4 MB of fp32, which no workgroup holds (pyannet.hip keeps its 128-wide W_hh in registers).  This kernel has NO wait between
// workgroups: one workgroup owns (a tile of PFTS_CT clips, one direction) for the whole sequence, keeps h in LDS and c in
// registers, and re-reads W_hh every step.  W_hh is stored transposed, [k][unit*4 + gate]: thread u reads the four gate weights
// of its unit as one 16-byte load, a wave reads 1 KB contiguous, and the tile's clips share every load.  The workgroup's 1024
// threads are two halves of the k range (512 units x 2), summed through LDS in a fixed order: every clip's result is
// independent of its tile mates.  Blocks alternate directions (dir = block & 1): blocks b and b + 8 tend to share an XCD, so
// an XCD's 4 MB L2 mostly sees ONE direction's 4 MB matrix.  The step time is set by what one CU can pull from L2
// (DESIGN §8.16), not by the FMAs: up to the tile size more clips cost nothing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/tdx.h"
#include "pf_timestamps.hpp"

using namespace tdx;

// the head's 12 tensors, in the order in which a missing one is reported
static const char* const PFTS_TENSORS[12] = {
    "predictor.upsample_cnn.weight", "predictor.upsample_cnn.bias",
    "predictor.blstm.weight_ih_l0", "predictor.blstm.weight_hh_l0", "predictor.blstm.bias_ih_l0", "predictor.blstm.bias_hh_l0",
    "predictor.blstm.weight_ih_l0_reverse", "predictor.blstm.weight_hh_l0_reverse", "predictor.blstm.bias_ih_l0_reverse",
    "predictor.blstm.bias_hh_l0_reverse", "predictor.cif_output2.weight", "predictor.cif_output2.bias"};

namespace {

constexpr int D = 512, HID = 512, GATES = 4 * HID, XP = 2 * GATES, YW = 2 * HID, UPS = 3;
constexpr int PFTS_CT = 4, PFTS_THREADS = 2 * HID, PFTS_KH = HID / 2;
constexpr float PFTS_THRESHOLD = 1.0f - 1e-4f;

// xp [B*U][4096]: column dir*2048 + u*4 + gate (i, f, g, o), biases included; whhT [2][512 (k)][2048 (u*4 + gate)];
// y [B*U][1024] = [h_fwd | h_bwd].  grid = 2 * ceil(B / PFTS_CT) blocks: dir = block & 1, clip tile = block >> 1.
__global__ __launch_bounds__(PFTS_THREADS) void pfts_lstm_rec_kernel(const float* __restrict__ xp, const float* __restrict__ whhT,
                                                                      float* __restrict__ y, int B, int U) {
    __shared__ __attribute__((aligned(16))) float hs[2][PFTS_CT][HID];           // h of the tile, double buffered over the steps
    __shared__ __attribute__((aligned(16))) f32x4 part[PFTS_CT][HID];            // gate sums of the upper k half
    const int tid = threadIdx.x, u = tid & (HID - 1), kh = tid >> 9;
    const int dir = blockIdx.x & 1, b0 = (blockIdx.x >> 1) * PFTS_CT, nb = min(PFTS_CT, B - b0);
    for (int i = tid; i < 2 * PFTS_CT * HID; i += PFTS_THREADS) (&hs[0][0][0])[i] = 0.f;      // rows >= nb stay zero
    const float* wp = whhT + ((size_t)dir * HID + (size_t)kh * PFTS_KH) * GATES + u * 4;
    const float* xcol = xp + (size_t)b0 * U * XP + dir * GATES + u * 4;
    float c[PFTS_CT];
#pragma unroll
    for (int b = 0; b < PFTS_CT; ++b) c[b] = 0.f;
    __syncthreads();
    for (int s = 0; s < U; ++s) {
        const int t = dir ? U - 1 - s : s, cur = s & 1;
        f32x4 acc[PFTS_CT];
#pragma unroll
        for (int b = 0; b < PFTS_CT; ++b) {        // the lower half starts from the projected input (requested ahead of the k loop)
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            acc[b] = (kh == 0 && b < nb) ? ldg4(xcol + ((size_t)b * U + t) * XP) : zero;
        }
        const float* hb = &hs[cur][0][kh * PFTS_KH];
#pragma unroll 2
        for (int k = 0; k < PFTS_KH; k += 4) {
            const f32x4 w0 = ldg4(wp + (size_t)k * GATES), w1 = ldg4(wp + (size_t)(k + 1) * GATES);
            const f32x4 w2 = ldg4(wp + (size_t)(k + 2) * GATES), w3 = ldg4(wp + (size_t)(k + 3) * GATES);
#pragma unroll
            for (int b = 0; b < PFTS_CT; ++b) {
                const f32x4 hv = *reinterpret_cast<const f32x4*>(hb + b * HID + k);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float a = acc[b][g];
                    a = fmaf(w0[g], hv[0], a); a = fmaf(w1[g], hv[1], a); a = fmaf(w2[g], hv[2], a); a = fmaf(w3[g], hv[3], a);
                    acc[b][g] = a;
                }
            }
        }
        if (kh == 1) {
#pragma unroll
            for (int b = 0; b < PFTS_CT; ++b) part[b][u] = acc[b];
        }
        __syncthreads();
        if (kh == 0) {
#pragma unroll
            for (int b = 0; b < PFTS_CT; ++b) {
                if (b < nb) {
                    const f32x4 a = acc[b] + part[b][u];
                    const float cn = fmaf(sigmoid_full(a[1]), c[b], sigmoid_full(a[0]) * tanhf(a[2]));
                    const float h = sigmoid_full(a[3]) * tanhf(cn);
                    c[b] = cn;
                    hs[cur ^ 1][b][u] = h;
                    y[((size_t)(b0 + b) * U + t) * YW + dir * HID + u] = h;
                }
            }
        }
        __syncthreads();
    }
}

// raw[m] = relu(smooth * sigmoid(y[m,:] . w + b0) - noise): one wave per row of 1024
__global__ __launch_bounds__(256) void pfts_alpha_kernel(const float* __restrict__ y, const float* __restrict__ w, const float* __restrict__ b0,
                                                          float* __restrict__ raw, long M, float smooth, float noise) {
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int lane = threadIdx.x & 63;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < YW / 256; ++i) {
        const f32x4 a = ldg4(y + m * YW + i * 256 + lane * 4), q = ldg4(w + i * 256 + lane * 4);
        v = fmaf(a[0], q[0], v); v = fmaf(a[1], q[1], v); v = fmaf(a[2], q[2], v); v = fmaf(a[3], q[3], v);
    }
    v = wave_sum(v) + b0[0];
    if (lane == 0) raw[m] = fmaxf(smooth * sigmoid_full(v) - noise, 0.f);
}

// per clip: alphas = raw * (counts / sum raw) (a clip whose sum is 0 is left unscaled: the formula would give NaN), then funasr's
// cif_wo_hidden: ONE thread walks the clip in the reference's fp32 operation order (no prefix-sum reformulation: the firing
// decisions must be those of the sequential loop) — integ += a; peak = integ; if (integ >= thr) integ -= thr.
__global__ __launch_bounds__(256) void pfts_norm_scan_kernel(const float* __restrict__ raw, const int* __restrict__ counts, float* __restrict__ alphas,
                                                              float* __restrict__ peaks, int U) {
    __shared__ float ws4[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* r = raw + (size_t)b * U;
    float* a = alphas + (size_t)b * U;
    float s = 0.f;
    for (int i = tid; i < U; i += 256) s += r[i];
    s = wave_sum(s);
    if ((tid & 63) == 0) ws4[tid >> 6] = s;
    __syncthreads();
    const float sum = (ws4[0] + ws4[1]) + (ws4[2] + ws4[3]);
    const float scale = (float)counts[b] / sum;
    for (int i = tid; i < U; i += 256) a[i] = sum > 0.f ? r[i] * scale : r[i];
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        float integ = 0.f;
        float* p = peaks + (size_t)b * U;
        for (int i = 0; i < U; ++i) {
            integ += a[i];
            p[i] = integ;
            if (integ >= PFTS_THRESHOLD) integ -= PFTS_THRESHOLD;
        }
    }
}

}  // namespace

bool pfts_stage(Loader& ld, PfTsHead& w) {
    int have = 0;
    for (const char* n : PFTS_TENSORS) have += ld.blob.find(n) ? 1 : 0;
    if (!have) return false;
    const uint32_t d = D, g = GATES, hd = HID;
    // ConvTranspose1d weight [in][out][3] -> GEMM weight [j*512 + out][in]; the bias three times
    const float* cw = ld.get(PFTS_TENSORS[0], {d, d, (uint32_t)UPS});
    const float* cb = ld.get(PFTS_TENSORS[1], {d});
    const size_t Wup = ld.room(w.Wup, (size_t)UPS * D * D);
    const size_t bup = ld.room(w.bup, (size_t)UPS * D);
    if (cw) for (int ci = 0; ci < D; ++ci) for (int co = 0; co < D; ++co) for (int j = 0; j < UPS; ++j)
        ld.host[Wup + ((size_t)j * D + co) * D + ci] = cw[((size_t)ci * D + co) * UPS + j];
    if (cb) for (int j = 0; j < UPS; ++j) for (int co = 0; co < D; ++co) ld.host[bup + (size_t)j * D + co] = cb[co];
    // both directions' W_ih as one [4096][512] matrix with rows dir*2048 + u*4 + gate, bias b_ih + b_hh; W_hh transposed
    GemmW ih; ih.N = XP; ih.Npad = XP; ih.Kp = D;
    ih.w = ld.room(w.Wih, (size_t)XP * D);
    ih.b = ld.room(w.bih, XP);
    const size_t whhT = ld.room(w.whhT, (size_t)2 * HID * GATES);
    for (int dir = 0; dir < 2; ++dir) {
        const float* wih = ld.get(PFTS_TENSORS[2 + 4 * dir], {g, d});
        const float* whh = ld.get(PFTS_TENSORS[3 + 4 * dir], {g, hd});
        const float* bi = ld.get(PFTS_TENSORS[4 + 4 * dir], {g});
        const float* bh = ld.get(PFTS_TENSORS[5 + 4 * dir], {g});
        push_lstm_gates(ld, wih, whh, bi, bh, HID, D, ih, whhT, dir * GATES, true);
    }
    ld.push(w.w2, ld.get(PFTS_TENSORS[10], {1u, (uint32_t)YW}), YW);
    ld.push(w.b2, ld.get(PFTS_TENSORS[11], {1u}), 1);
    return true;
}

void pfts_queue_planes(PfTsHead& w, std::vector<PlaneJob>& jobs) {
    w.present = true;
    jobs.push_back({w.Wup, UPS * D, D, &w.hup.p, &w.hup.s});
    jobs.push_back({w.Wih, XP, D, &w.hih.p, &w.hih.s});
}

// raw alphas | planes of the current GEMM's A operand (<= B*U rows of 512) + row scales | upsampled [B*U][512] | xp [B*U][4096] | y [B*U][1024]
size_t pfts_work_floats(size_t B, size_t T) {
    const size_t MU = B * T * UPS;
    return al(MU) + al(MU * D) + al(MU) + al(MU * D) + al(MU * XP) + al(MU * YW);
}

int pfts_forward(const PfTsHead& w, const float* enc, int B, int T, const int* counts, float* us_alphas, float* us_peaks, float* tap,
                 float* ws, hipStream_t st) {
    const long M = (long)B * T, MU = M * UPS;
    const int U = T * UPS;
    float* raw = ws;
    unsigned char* hp = (unsigned char*)(raw + al(MU));
    float* hs = (float*)hp + al(MU * D);
    float* up = hs + al(MU);
    float* xp = up + al(MU * D);
    float* y = tap ? tap : xp + al(MU * XP);
    if (launch_h3_split_rows(enc, D, hp, hs, M, D, st) != hipSuccess) return fail_hip(hipGetLastError(), __FILE__, __LINE__);
    TRY(linear_h3(hp, hs, (int)M, w.hup, UPS * D, D, EpiBiasAct<>{w.bup, up, UPS * D}, st));       // row (b,t) = frames 3t..3t+2 of [B][U][512]
    if (launch_h3_split_rows(up, D, hp, hs, MU, D, st) != hipSuccess) return fail_hip(hipGetLastError(), __FILE__, __LINE__);
    TRY(linear_h3(hp, hs, (int)MU, w.hih, XP, D, EpiBiasAct<>{w.bih, xp, XP}, st));
    hipLaunchKernelGGL(pfts_lstm_rec_kernel, dim3(2 * ((B + PFTS_CT - 1) / PFTS_CT)), dim3(PFTS_THREADS), 0, st, (const float*)xp, w.whhT, y, B, U);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(pfts_alpha_kernel, dim3((unsigned)((MU + 3) / 4)), dim3(256), 0, st, (const float*)y, w.w2, w.b2, raw, MU, w.smooth, w.noise);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(pfts_norm_scan_kernel, dim3(B), dim3(256), 0, st, (const float*)raw, counts, us_alphas, us_peaks, U);
    LAUNCH_CHECK();
    return TDX_OK;
}
