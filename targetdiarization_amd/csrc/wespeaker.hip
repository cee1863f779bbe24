// wespeaker.hip — WeSpeaker ResNet34 (wespeaker `ResNet34`, m_channels 32, feat_dim 80, embed_dim 256, TSTP, one embedding
// layer; pyannote.audio `WeSpeakerResNet34`) with pyannote's masked statistics pooling, on MI355X.  The embedding model of
// pyannote speaker-diarization-3.1, i.e. the cross-chunk identity inside `self.od_pipeline` (TargetDiarization.py:84);
// third-party, parity unpinned [upstream-recall] — tests/wespeaker_oracle.py restates the architecture, DESIGN §8.14 governs.
// feat [B,F,80] (tdx_fbank mode 2) + weights [B,S,Fw] -> embedding [B,S,256].
//
// Layout: channel-last fp32 everywhere; rows = (b, h = mel, w = time).  Every BatchNorm follows a bias-free convolution and
// is folded into it at load time; ReLU and the residual are epilogues.
//  * stem_kernel: 1 -> 32, reads feat[b, w, h] transposed.
//  * conv3x3_narrow_kernel<C>, C = 32 / 64: the 13 stride-1 3x3 convolutions with Cin = Cout = C (all of layer1, layer2 but
//    layer2.0.conv1).  A block owns a spatial tile, stages it with its halo in LDS once and multiplies against the taps'
//    weights from LDS with the block's N equal to C.  TDX_WESPK_NARROW=1 / 0 (read at create) picks it or the shared core; the default is the measured faster one.
//  * every other convolution (stride 2, 1x1 shortcuts, N = 128 / 256): implicit GEMM on the fp32-MFMA core (gemm.hpp CONV).
//  * wespk_pool_kernel: the trunk runs ONCE per chunk; its [B,10,T',256] output is pooled under each of the S masks.
//  * seg1_kernel: Linear 5120 -> 256.
// No atomics, no memset, no allocation, one stream: every reduction has a fixed order that depends on its own (b, s) alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/tdx.h"
#include "epilogues.hpp"
#include "weight_pack.hpp"

using namespace tdx;

namespace {

constexpr int EMB = 256, MEL = 80, C0 = 32, NSTAGE = 4, POOLC = 256, POOLH = 10, STATS = 2 * POOLC * POOLH;
const int kBlocks[NSTAGE] = {3, 4, 6, 3};
constexpr int MAX_B = 64, MAX_S = 8;
constexpr bool kNarrowDefault = true;

// conv1: conv3x3(1->32, pad 1) + BN + ReLU on x[b, h=mel, w=time] = feat[b, w, h] -> rows (b, h, w) x 32
__global__ __launch_bounds__(256) void stem_kernel(const float* __restrict__ feat, const float* __restrict__ w9,   // [9][32]
                                                    const float* __restrict__ bias, float* __restrict__ out, int F, long rows) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;     // (row, channel quad): 8 quads per row
    if (i >= rows * 8) return;
    const long m = i >> 3;
    const int c = (int)(i & 7) * 4;
    const int w = (int)(m % F), h = (int)((m / F) % MEL);
    const long b = m / ((long)F * MEL);
    float4 acc = *reinterpret_cast<const float4*>(bias + c);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int ih = h + t / 3 - 1, iw = w + t % 3 - 1;
        if (ih >= 0 && ih < MEL && iw >= 0 && iw < F) {
            const float x = feat[(b * F + iw) * MEL + ih];
            const float4 k = *reinterpret_cast<const float4*>(w9 + t * C0 + c);
            acc.x = fmaf(k.x, x, acc.x); acc.y = fmaf(k.y, x, acc.y); acc.z = fmaf(k.z, x, acc.z); acc.w = fmaf(k.w, x, acc.w);
        }
    }
    acc.x = fmaxf(acc.x, 0.f); acc.y = fmaxf(acc.y, 0.f); acc.z = fmaxf(acc.z, 0.f); acc.w = fmaxf(acc.w, 0.f);
    *reinterpret_cast<float4*>(out + m * C0 + c) = acc;
}

// ---------------------------------------------------------------- the narrow 3x3 convolution
// out[b,h,w,:] = relu(bias + sum_taps W[tap] x[b,h+dy,w+dx,:] (+ res[b,h,w,:])), stride 1, pad 1, Cin = Cout = C, NHWC fp32.
//   block  : 4 waves; a tile of TH = 4*MT rows x 32 columns of output pixels, and WT such tiles side by side, one after the
//            other.  Wave v owns rows v*MT .. v*MT+MT-1 of the tile: MT MFMA row tiles of 32 pixels, C/32 column tiles.
//   LDS    : xs  (TH+2) x 34 pixels x (C+4) floats — the input tile with its halo, read from global ONCE per block;
//            wsm taps-of-a-group x C x (C+4) floats — [tap][cout][cin]; all 9 taps at C = 32 (staged once per block), the 3
//            taps of one kernel row at C = 64 (staged per group and tile).  Both are register staged: the loads of the next
//            tile / group are in flight while this one is multiplied.  The pitch C+4 makes the 16-byte fragment reads
//            (lane = pixel or cout, 4 consecutive cin) conflict free, as gemm.hpp's pitch 36 does.
//            C = 32: 29 376 + 41 472 = 70 848 B (two blocks per CU); C = 64: 92 480 + 52 224 = 144 704 B (one).
//   MFMA   : v_mfma_f32_32x32x2_f32, operand map of gemm.hpp: lane l supplies A[pixel l&31][k] and B[k][cout l&31] for the
//            four k = 8 kc + 4 (l>>5) + j of one 16-byte LDS read — the same permutation on both operands.
//   store  : the accumulators (lane = cout) go through the wave's own rows of xs, so that a lane ends with 4 consecutive
//            channels of a pixel: bias, residual and ReLU on float4, 16-byte channel-last stores.
template <int C> struct NarrowCfg {
    static constexpr int MT = C == 32 ? 1 : 2, TH = 4 * MT, TW = 32, P = C + 4;
    static constexpr int NG = C == 32 ? 1 : 3, GT = 9 / NG;                // tap groups, taps per group
    static constexpr int XS = (TH + 2) * (TW + 2) * P, WS = GT * C * P;    // floats
    static constexpr size_t LDS_BYTES = (size_t)(XS + WS) * sizeof(float);
};

template <int C>
__global__ __launch_bounds__(256) void conv3x3_narrow_kernel(const float* __restrict__ x, const float* __restrict__ wt,      // [9][C][C]
                                                              const float* __restrict__ bias, const float* __restrict__ res,
                                                              float* __restrict__ out, int H, int W, int WT) {
    using K = NarrowCfg<C>;
    constexpr int MT = K::MT, TH = K::TH, TW = K::TW, P = K::P, NT = C / 32, NG = K::NG, GT = K::GT, C4 = C / 4;
    __shared__ __attribute__((aligned(16))) float lds[K::XS + K::WS];
    float* xs = lds;
    float* wsm = lds + K::XS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const int b = blockIdx.z, h0 = blockIdx.y * TH;
    const long img = (long)b * H * W;

    // Register-staged prefetch, as in gemm.hpp: the next tile's pixels and the next group's weights are loaded from global
    // while this tile / group is multiplied, and written to LDS behind the barrier that ends its readers.
    constexpr int XN4 = (TH + 2) * (TW + 2) * C4, XR = (XN4 + 255) / 256, WN4 = GT * C * C4, WR = WN4 / 256;
    static_assert(WN4 % 256 == 0, "a weight group is a whole number of 16-byte loads per thread");
    f32x4 xr[XR], wr[WR];
    auto load_x = [&](int w0) {
#pragma unroll
        for (int j = 0; j < XR; ++j) {
            const int i = tid + 256 * j;
            const int p = i / C4, c = (i - p * C4) * 4;
            const int ph = p / (TW + 2), pw = p - ph * (TW + 2);
            const int gh = h0 + ph - 1, gw = w0 + pw - 1;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (i < XN4 && gh >= 0 && gh < H && gw >= 0 && gw < W) v = ldg4(x + (img + (long)gh * W + gw) * C + c);
            xr[j] = v;
        }
    };
    auto store_x = [&]() {
#pragma unroll
        for (int j = 0; j < XR; ++j) {
            const int i = tid + 256 * j;
            const int p = i / C4, c = (i - p * C4) * 4;
            if (i < XN4) *reinterpret_cast<f32x4*>(xs + p * P + c) = xr[j];
        }
    };
    auto load_w = [&](int g) {
#pragma unroll
        for (int j = 0; j < WR; ++j) {
            const int i = tid + 256 * j;
            const int row = i / C4, c = (i - row * C4) * 4;       // row = (tap in group, cout)
            wr[j] = ldg4(wt + ((long)g * GT * C + row) * C + c);
        }
    };
    auto store_w = [&]() {
#pragma unroll
        for (int j = 0; j < WR; ++j) {
            const int i = tid + 256 * j;
            const int row = i / C4, c = (i - row * C4) * 4;
            *reinterpret_cast<f32x4*>(wsm + row * P + c) = wr[j];
        }
    };
    const int tiles_w = (W + TW - 1) / TW;
    const int ntiles = min(WT, tiles_w - (int)blockIdx.x * WT);       // >= 1: the grid is ceil(tiles_w / WT) wide
    load_x(blockIdx.x * WT * TW);
    load_w(0);
    for (int wtile = 0; wtile < ntiles; ++wtile) {
        const int w0 = (blockIdx.x * WT + wtile) * TW;
        const bool last_tile = wtile + 1 == ntiles;
        __syncthreads();                                      // the previous tile's readers of xs are done
        store_x();
        if (!last_tile) load_x(w0 + TW);
        f32x16 acc[MT][NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

#pragma unroll 1
        for (int g = 0; g < NG; ++g) {
            if (NG > 1 || wtile == 0) {
                if (NG > 1) __syncthreads();                  // the previous group's readers of wsm are done
                store_w();
                if (NG > 1 && !(last_tile && g == NG - 1)) load_w(g + 1 == NG ? 0 : g + 1);
            }
            __syncthreads();
#pragma unroll 1
            for (int t = 0; t < GT; ++t) {
                const int tap = g * GT + t, ty = tap / 3, tx = tap - ty * 3;
                const float* bp = wsm + (t * C + l31) * P + 4 * hh;
                const float* ap = xs + ((wave * MT + ty) * (TW + 2) + l31 + tx) * P + 4 * hh;
#pragma unroll
                for (int kc = 0; kc < C / 8; ++kc) {
                    f32x4 av[MT], bv[NT];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) av[mt] = *reinterpret_cast<const f32x4*>(ap + mt * (TW + 2) * P + 8 * kc);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const f32x4*>(bp + nt * 32 * P + 8 * kc);
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                            for (int q = 0; q < 4; ++q)
                                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt][q], bv[nt][q], acc[mt][nt], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                      // every wave has read its last input pixel: xs becomes the output stage
        // D: col = l31, row = (r&3) + 8*(r>>2) + 4*hh.  Wave `wave` writes MT x 32 pixel rows of pitch P at its own offset.
        float* os = xs + wave * MT * 32 * P;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    os[(mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh) * P + nt * 32 + l31] = acc[mt][nt][r];
        __syncthreads();
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int gh = h0 + wave * MT + mt;
            for (int i = lane; i < 32 * C4; i += 64) {
                const int px = i / C4, c = (i - px * C4) * 4;
                const int gw = w0 + px;
                if (gh >= H || gw >= W) continue;
                const long o = (img + (long)gh * W + gw) * C + c;
                f32x4 v = *reinterpret_cast<const f32x4*>(os + (mt * 32 + px) * P + c);
                const f32x4 bb = ldg4(bias + c);
                if (res) {
                    const f32x4 rr = ldg4(res + o);
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = fmaxf((v[j] + bb[j]) + rr[j], 0.f);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j] + bb[j], 0.f);
                }
                *reinterpret_cast<f32x4*>(out + o) = v;
            }
        }
    }
}

// ---------------------------------------------------------------- masked statistics pooling
// x rows (b, h, t) x 256 channels; feature (c, h) -> index c*10 + h.  One workgroup per (h, s, b), one thread per channel.
// w'[t] = w[b, s, (t*Fw)/Tp] (nearest); no weights: all ones.  Two passes in fp32 in the order of t.
__global__ __launch_bounds__(POOLC) void wespk_pool_kernel(const float* __restrict__ x, const float* __restrict__ wts, float* __restrict__ stats,
                                                            int Tp, int S, int Fw) {
    const int h = blockIdx.x, s = blockIdx.y, b = blockIdx.z, c = threadIdx.x;
    const float* p = x + ((long)(b * POOLH + h) * Tp) * POOLC + c;
    const float* wp = wts ? wts + ((long)b * S + s) * Fw : nullptr;
    float v1 = 0.f, v2 = 0.f, sx = 0.f;
    for (int t = 0; t < Tp; ++t) {
        const float w = wp ? wp[(int)(((long)t * Fw) / Tp)] : 1.f;
        v1 += w; v2 = fmaf(w, w, v2);
        sx = fmaf(w, p[(long)t * POOLC], sx);
    }
    float* o = stats + ((long)b * S + s) * STATS + c * POOLH + h;
    if (v1 == 0.f) {                                          // upstream's 0/0: the whole row is NaN
        const float qnan = __int_as_float(0x7fc00000);
        o[0] = qnan; o[POOLC * POOLH] = qnan;
        return;
    }
    const float mean = sx / v1;
    float q = 0.f;
    for (int t = 0; t < Tp; ++t) {
        const float w = wp ? wp[(int)(((long)t * Fw) / Tp)] : 1.f;
        const float d = p[(long)t * POOLC] - mean;
        q = fmaf(w * d, d, q);
    }
    o[0] = mean;
    o[POOLC * POOLH] = sqrtf(q / (v1 - v2 / v1 + 1e-8f));
}

// seg_1: emb[r][n] = bias[n] + stats[r] . W[n]      (K = 5120)
__global__ __launch_bounds__(256) void seg1_kernel(const float* __restrict__ stats, const float* __restrict__ W,
                                                    const float* __restrict__ bias, float* __restrict__ emb) {
    __shared__ float red[4];
    const int n = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const float* s = stats + (long)r * STATS;
    const float* w = W + (long)n * STATS;
    float acc = 0.f;
    for (int k = tid * 4; k < STATS; k += 1024) {
        const float4 a = *reinterpret_cast<const float4*>(s + k);
        const float4 c = *reinterpret_cast<const float4*>(w + k);
        acc = fmaf(a.x, c.x, acc); acc = fmaf(a.y, c.y, acc); acc = fmaf(a.z, c.z, acc); acc = fmaf(a.w, c.w, acc);
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) emb[(long)r * EMB + n] = (red[0] + red[1]) + (red[2] + red[3]) + bias[n];
}

struct ConvW : tdx::GemmW { size_t wn = 0; };      // w: [Npad][taps][cinp = cin] (shared core); wn: [9][N][cin] (narrow) or 0
struct BlockW { ConvW c1, c2, sc; bool has_sc; int cin, cout, stride; };

// a convolution as an implicit GEMM on the shared fp32 core (a third copy of the launcher of eres2net.hip / campplus.hip: those
// two differ in their stride arguments, and hoisting one would change what the other compiles to)
template <class Epi>
int conv_gemm(const float* A, const float* dev, const ConvW& cw, int B, int Hin, int Win, int Hout, int Wout, int stride, Epi e, hipStream_t st) {
    const long M = (long)B * Hout * Wout;
    GemmArgs g = make_args((int)M, cw.Npad, make_seg(A, cw.cinp, dev + cw.w, (long)cw.taps * cw.cinp, cw.cinp));
    g.n_valid = up(cw.N, 32);
    g.cv_Hin = Hin; g.cv_Win = Win; g.cv_Hout = Hout; g.cv_Wout = Wout; g.cv_stride = stride; g.cv_ntaps = cw.taps; g.cv_cin = cw.cinp;
    if (launch_gemm<false, false, false, false, Epi, 0, true>(g, 1, e, st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
    return TDX_OK;
}

template <int C>
int conv_narrow(const float* x, const float* dev, const ConvW& cw, const float* res, float* out, int B, int H, int W, hipStream_t st) {
    using K = NarrowCfg<C>;
    // tiles per block: 4 at C = 32 (the weights are staged once per block); 1 at C = 64 (they are restaged per tile anyway,
    // and more, smaller blocks fill the CUs evenly)
    const int tiles_w = (W + K::TW - 1) / K::TW, WT = C == 32 ? std::min(tiles_w, 4) : 1;
    const dim3 grid((unsigned)((tiles_w + WT - 1) / WT), (unsigned)((H + K::TH - 1) / K::TH), (unsigned)B);
    hipLaunchKernelGGL(conv3x3_narrow_kernel<C>, grid, dim3(256), 0, st, x, dev + cw.wn, dev + cw.b, res, out, H, W, WT);
    LAUNCH_CHECK();
    return TDX_OK;
}

}  // namespace

struct tdx_wespk {
    int device = 0;
    bool narrow = kNarrowDefault;
    tdx::DevBuf dev;
    size_t stem_w, stem_b, seg_w, seg_b;
    std::vector<BlockW> blocks;
};

extern "C" {

int tdx_wespk_create(const void* blob, size_t blob_bytes, int device, tdx_wespk** out) {
    if (!blob || !out) return tdx::fail(TDX_E_INVALID, "tdx_wespk_create: null argument");
    tdx::Loader ld;
    if (!ld.parse(blob, blob_bytes)) return tdx::fail(TDX_E_BLOB, "tdx_wespk_create: malformed TDXW blob");
    using tdx::BN;
    auto bn = [&](const std::string& p, int N) -> BN {      // eval BatchNorm `p` -> y = x*s + sh
        const float *g = ld.get(p + "weight", {(uint32_t)N}), *be = ld.get(p + "bias", {(uint32_t)N});
        const float *mu = ld.get(p + "running_mean", {(uint32_t)N}), *var = ld.get(p + "running_var", {(uint32_t)N});
        return tdx::bn_fold(g, be, mu, var, N);
    };
    // bias-free conv [N,cin,k,k] + eval BatchNorm -> [Npad][taps][cin] + bias[Npad]; with `narrow` also [taps][N][cin]
    auto fold = [&](const std::string& wname, const std::string& bnp, int N, int cin, int k, bool narrow) -> ConvW {
        const float* W = ld.get(wname, {(uint32_t)N, (uint32_t)cin, (uint32_t)k, (uint32_t)k});
        const BN b = bn(bnp, N);
        ConvW cw{tdx::push_conv_gemm(ld, W, b.s.data(), b.sh.data(), N, cin, k * k, up(N, 128), cin)};
        if (narrow) cw.wn = ld.room((size_t)cw.taps * N * cin);
        if (narrow && W) for (int n = 0; n < N; ++n)
            for (int t = 0; t < cw.taps; ++t)
                memcpy(&ld.host[cw.wn + ((size_t)t * N + n) * cin], &ld.host[cw.w + ((size_t)n * cw.taps + t) * cin], cin * sizeof(float));
        return cw;
    };
    std::unique_ptr<tdx_wespk> h(new tdx_wespk());
    {   // TDX_WESPK_NARROW (read here, so that one process can hold both): 1 = the 13 narrow convolutions on conv3x3_narrow_kernel,
        // 0 = on the shared core; unset = kNarrowDefault, the faster of the two as measured
        const char* e = getenv("TDX_WESPK_NARROW");
        h->narrow = (e && e[1] == 0 && (e[0] == '0' || e[0] == '1')) ? e[0] == '1' : kNarrowDefault;
    }
    {   // resnet.conv1 [32,1,3,3] + bn1 -> w9[9][32], bias[32]
        const float* W = ld.get("resnet.conv1.weight", {(uint32_t)C0, 1, 3, 3});
        tdx::push_stem9(ld, W, bn("resnet.bn1.", C0), C0, h->stem_w, h->stem_b);
    }
    int cin = C0;
    for (int L = 0; L < NSTAGE; ++L) {
        const int cout = C0 << L;
        for (int i = 0; i < kBlocks[L]; ++i) {
            const std::string p = "resnet.layer" + std::to_string(L + 1) + "." + std::to_string(i) + ".";
            BlockW bw{};
            bw.cin = cin; bw.cout = cout; bw.stride = (i == 0 && L > 0) ? 2 : 1;
            bw.has_sc = bw.stride != 1 || cin != cout;
            const bool nar = cout <= 64;
            bw.c1 = fold(p + "conv1.weight", p + "bn1.", cout, cin, 3, nar && bw.stride == 1 && cin == cout);
            bw.c2 = fold(p + "conv2.weight", p + "bn2.", cout, cout, 3, nar);
            if (bw.has_sc) bw.sc = fold(p + "shortcut.0.weight", p + "shortcut.1.", cout, cin, 1, false);
            h->blocks.push_back(bw);
            cin = cout;
        }
    }
    h->seg_w = ld.push(ld.get("resnet.seg_1.weight", {(uint32_t)EMB, (uint32_t)STATS}), (size_t)EMB * STATS);
    h->seg_b = ld.push(ld.get("resnet.seg_1.bias", {(uint32_t)EMB}), EMB);
    h->device = device;
    TRY(ld.finish("tdx_wespk_create", true, device, h->dev));
    *out = h.release();
    return TDX_OK;
}

int tdx_wespk_destroy(tdx_wespk* h) {
    delete h;
    return TDX_OK;
}

namespace {
struct WsPlan { size_t full, half, stats, total; };
inline bool dims_ok(int B, int F, int S, int Fw) {
    return B >= 1 && B <= MAX_B && F >= 1 && S >= 1 && S <= MAX_S && Fw >= 1 && (long)B * MEL * F <= 0x7fffffffL / C0;
}
inline WsPlan ws_plan(int B, int F, int S) {
    WsPlan w{};
    const int H2 = MEL / 2, W2 = (F - 1) / 2 + 1;
    w.full = al((size_t)B * MEL * F * C0 + 64);             // the largest activation: stem / layer1
    w.half = al((size_t)B * H2 * W2 * 2 * C0 + 64);         // the largest shortcut: layer2.0
    w.stats = al((size_t)B * S * STATS);
    w.total = 3 * w.full + w.half + w.stats;
    return w;
}
}  // namespace

size_t tdx_wespk_workspace_bytes(const tdx_wespk* h, int B, int F, int S) {
    if (!h || !dims_ok(B, F, S, 1)) return 0;
    return ws_plan(B, F, S).total * sizeof(float);
}

int tdx_wespk_forward(tdx_wespk* h, const float* feat, int B, int F, const float* weights, int S, int Fw, float* emb, void* ws_, size_t ws_bytes,
                      void* stream) {
    if (!h || !feat || !emb || !ws_) return tdx::fail(TDX_E_INVALID, "tdx_wespk_forward: null argument");
    if (!dims_ok(B, F, S, Fw))
        return tdx::fail(TDX_E_INVALID, "tdx_wespk_forward: need 1 <= B <= 64, F >= 1, 1 <= S <= 8, Fw >= 1 and B*F*2560 < 2^31");
    if (!weights && S != 1) return tdx::fail(TDX_E_INVALID, "tdx_wespk_forward: no weights means S = 1");
    const WsPlan wp = ws_plan(B, F, S);
    if (ws_bytes < wp.total * sizeof(float)) return tdx::fail(TDX_E_WORKSPACE, "tdx_wespk_forward: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)ws_;
    float* P[3] = {ws, ws + wp.full, ws + 2 * wp.full};
    float* scb = ws + 3 * wp.full;
    float* stats = scb + wp.half;
    const float* dev = h->dev;

    const long rows0 = (long)B * MEL * F;
    hipLaunchKernelGGL(stem_kernel, dim3((unsigned)((rows0 * 8 + 255) / 256)), dim3(256), 0, st, feat, dev + h->stem_w, dev + h->stem_b, P[0], F, rows0);
    LAUNCH_CHECK();
    int xi = 0, H = MEL, W = F;
    for (const BlockW& b : h->blocks) {
        const float* x = P[xi];
        float *t = P[(xi + 1) % 3], *y = P[(xi + 2) % 3];
        const int Ho = (H - 1) / b.stride + 1, Wo = (W - 1) / b.stride + 1;
        // conv1 (stride) + bn1 + relu -> t
        if (h->narrow && b.c1.wn) {
            if (b.cout == 32) TRY(conv_narrow<32>(x, dev, b.c1, nullptr, t, B, H, W, st));
            else TRY(conv_narrow<64>(x, dev, b.c1, nullptr, t, B, H, W, st));
        } else {
            TRY(conv_gemm(x, dev, b.c1, B, H, W, Ho, Wo, b.stride, EpiBiasActN<ActRelu>{dev + b.c1.b, t, b.cout, b.cout}, st));
        }
        const float* r = x;
        if (b.has_sc) {
            TRY(conv_gemm(x, dev, b.sc, B, H, W, Ho, Wo, b.stride, EpiBiasActN<>{dev + b.sc.b, scb, b.cout, b.cout}, st));
            r = scb;
        }
        // relu(bn2(conv2(t)) + shortcut) -> y
        if (h->narrow && b.c2.wn) {
            if (b.cout == 32) TRY(conv_narrow<32>(t, dev, b.c2, r, y, B, Ho, Wo, st));
            else TRY(conv_narrow<64>(t, dev, b.c2, r, y, B, Ho, Wo, st));
        } else {
            TRY(conv_gemm(t, dev, b.c2, B, Ho, Wo, Ho, Wo, 1, EpiBiasResN<ActRelu>{dev + b.c2.b, r, y, b.cout, b.cout}, st));
        }
        xi = (xi + 2) % 3; H = Ho; W = Wo;
    }
    // H = 10, W = T': masked statistics under each of the S masks, then seg_1
    hipLaunchKernelGGL(wespk_pool_kernel, dim3(POOLH, S, B), dim3(POOLC), 0, st, P[xi], weights, stats, W, S, Fw);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(seg1_kernel, dim3(EMB, B * S), dim3(256), 0, st, stats, dev + h->seg_w, dev + h->seg_b, emb);
    LAUNCH_CHECK();
    return TDX_OK;
}

}  // extern "C"
