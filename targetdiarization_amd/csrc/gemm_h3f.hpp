// gemm_h3f.hpp — the split-f16 x3 GEMM (gemm_h3.hpp) with the A operand read as FP32 NHWC pixel rows and split while it is
// staged: the 1x1 convolutions of ERes2NetV2's stages 1-2 (eres2net.hip) without the h3_split_rows_static pass and without
// the planes round trip through HBM.
//
//   C[m][n] = epilogue( sa * sb[n] * sum_k A'[m][k] * B'[n][k] ),   A' = split(x[pix(m)][k] * a_mul)
//
// Same math as h3_split_rows_static followed by gemm_h3_kernel<..., A_CONV> with one tap and sa_mul = 0: xs = x * a_mul,
// hi = f16(xs), lo = f16(xs - hi); the same per-stage LDS image and swizzle, v_mfma_f32_32x32x16_f16, the three products in
// the same order, k ascending, the same per-element epilogue expression: bit-identical results.  Only the A path differs:
//   * waves 4-7 fetch the weight planes (B) by LDS-DMA into a ring of four 16 KB stages, as the wide kernel does (k-tile t+4
//     issued in stage t);
//   * waves 0-3 own 64 tile rows each.  The fp32 values of a k-tile (64 B per row) also come by LDS-DMA, into a RAW ring of
//     three 16 KB slots: k-tile u is requested in stage u-5, and in stage u-2 every lane reads back the 16 B it fetched itself
//     (no barrier: a wave only touches its own 4 KB of a raw slot), splits the four values (5 VALU each) and writes hi and lo
//     (2 x ds_write_b64) into the A image of k-tile u, a ring of two 16 KB images; the fragments are read in stage u-1.
//     Three k-tiles of fp32 are in flight per wave at any time and none of them occupies a register: with the look-ahead in
//     VGPRs (2 stages x 16 registers per staging lane, next to 128 accumulators and 64 fragment registers) the kernel spilled
//     156 registers.  The waves of a SIMD are w and w+4, so the split of an A wave runs under the MFMAs of a B wave.
//   * row m = (b, h, w) of [B, Hout, Wout] reads pixel (b, h*stride, w*stride) of [B, Hin, Win] (the 1x1 case of the cv_*
//     geometry): a stride-2 convolution needs no compacting pass either.
// LDS: B ring 64 KB | A images 32 KB | raw ring 48 KB = 144 KB, one block per CU.
// One static scale for all rows (ReLU20-bounded activations: |x| * a_mul < 65504 is the caller's promise), *sa = 1 / a_mul.
// a_mul is a power of two: the compiler folds x * a_mul into the f16 conversions (v_fma_mix*), one rounding instead of two,
// which gives the bits of the split pass only because the product is exact.
// Epilogues: the store() functors with an empty row() value, with or without aux() (EpiBiasActN, EpiBiasRes, plain stores).
// Shapes: K % 16 == 0, K >= 16 (the rings are deeper than the shortest loop: every prologue / tail step is guarded), any M, N.
#pragma once
#include "gemm_h3.hpp"

namespace tdx {

constexpr int H3F_B = 0;                              // B ring: 4 x 16 KB
constexpr int H3F_AI = 4 * H3_OPER;                   // A images: 2 x 16 KB
constexpr int H3F_RAW = H3F_AI + 2 * H3_OPER;         // raw fp32 ring: 3 x 16 KB
constexpr int H3F_NRAW = 3;
constexpr int H3F_LDS = H3F_RAW + H3F_NRAW * H3_OPER; // 144 KB

// the raw ring is read back through inline asm: the compiler's waitcnt pass would put `s_waitcnt vmcnt(0)` in front of a plain
// LDS load from a region that an outstanding LDS-DMA writes (here it really is the same region: the wait for the right k-tile is
// the counted vmcnt in front of these reads).  As with h3_tr_read the values pass through a fence (lgkmcnt(0) tied to the
// registers) before anything uses them.
template <int OFF>
__device__ __forceinline__ void h3f_raw_read(f32x4& v, unsigned a) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(a), "n"(OFF) : "memory");
}
__device__ __forceinline__ void h3f_raw_fence(f32x4 (&v)[4]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]) :: "memory");
}

// block -> tile: XCD x = blockIdx.x & 7 walks a contiguous range of tiles, the N tiles of one M tile as neighbours in time
// (the second reader of the A rows finds them in the XCD's L2)
template <class Epi>
__global__ __launch_bounds__(H3_THREADS, 2) void gemm_h3f_kernel(H3Args g, float a_mul, Epi epi) {
    using RowT = decltype(epi.row(0, 0));
    static_assert(std::is_empty<RowT>::value, "fp32-A form: functors without a row() value");
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int wm = wave >> 2, wn = wave & 3;

    int bm, bn;
    {
        const int x = blockIdx.x & 7, i = blockIdx.x >> 3;
        const int tile = x * g.mp + i;                   // g.mp = tiles per XCD
        if (tile >= g.tiles_m * g.tiles_n) return;
        bm = tile / g.tiles_n; bn = tile - bm * g.tiles_n;
    }
    constexpr int z = 0;
    const int m0 = bm * H3_BM, n0 = bn * H3_BN;

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const bool stB = wave >= 4;
    // fragment addresses relative to the B stage of a k-tile (h3_stage's `nxt`); a0 is re-aimed per k-tile at its A image
    H3Frag f;
    const int a0row = (wm * 128 + l31) * H3_ROWB;
    {
        const int fl = (l31 >> 2) & 3;
        f.a0 = H3F_AI + a0row;
        f.apl[0] = ((2 * h) ^ fl) << 4; f.apl[1] = ((2 * h + 1) ^ fl) << 4;
#pragma unroll
        for (int tm = 0; tm < 4; ++tm) f.at[tm] = 0;
        f.b0 = (wn * 32 + l31) * H3_ROWB;
        f.bpl[0] = f.apl[0]; f.bpl[1] = f.apl[1];
    }
    // k-tile u: B stage at lds + (u & 3) * 16 KB, A image at lds + H3F_AI + (u & 1) * 16 KB
    auto bstage = [&](int u) -> unsigned char* { return lds + H3F_B + (u & 3) * H3_OPER; };
    auto frag_of = [&](int u) { H3Frag fu = f; fu.a0 = H3F_AI + ((u & 1) - (u & 3)) * H3_OPER + a0row; return fu; };
    const bool full_n = n0 + 128 < g.N;
    const bool wave_on = m0 + wm * 128 < g.M;       // (wave-uniform) this wave's 128 rows exist

    const H3Seg& sg = g.seg[0];
    const int nkt = sg.K / H3_BK;
    f16x8 ah[4], al[4], bh[2], bl[2];
    auto first_frags = [&]() {                      // k-tile 0
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            bh[tn] = h3_frag<false>(h3_addr_b<false>(lds, f, tn, 0));
            bl[tn] = h3_frag<false>(h3_addr_b<false>(lds, f, tn, 1));
        }
#pragma unroll
        for (int tm = 0; tm < 4; ++tm) {
            ah[tm] = h3_frag<false>(h3_addr_a<false>(lds, f, tm, 0));
            al[tm] = h3_frag<false>(h3_addr_a<false>(lds, f, tm, 1));
        }
    };
    const unsigned char* const nogp[4] = {lds, lds, lds, lds};          // (h3_stage without ISSUE never reads them)
    // at most n (0, 1, 2) k-tiles of this wave's LDS-DMA, four pieces each, stay in flight
    auto wait_keep = [&](int n) { if (n >= 2) H3_WAIT_VM(8); else if (n == 1) H3_WAIT_VM(4); else H3_WAIT_VM(0); };

    if (stB) {
        // ---- waves 4-7: the weight rows by LDS-DMA, the ring discipline of gemm_h3_kernel
        const int sdst = (wave & 3) * 4096;
        const unsigned char* gp[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = (wave & 3) * 64 + (lane >> 2) + 16 * j;
            const int n = min(n0 + r, g.N - 1);
            gp[j] = sg.B + (long)n * sg.ldb + (((lane & 3) ^ ((r >> 2) & 3)) << 4);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (p < nkt) {
#pragma unroll
                for (int j = 0; j < 4; ++j) h3_glds16(gp[j] + p * H3_ROWB, bstage(p) + sdst + j * 1024);
            }
        if (nkt >= 4) H3_WAIT_VM(12); else wait_keep(nkt - 1);
        H3_BARRIER();
        first_frags();
        auto run = [&](auto fulln) {
            constexpr bool FN = decltype(fulln)::value;
            int t = 0;
            for (; t + 4 < nkt; ++t) {
                H3_WAIT_VM(8);
                H3_BARRIER();
                if (wave_on)
                    h3_stage<false, false, FN, true, true, 1>(acc, ah, al, bh, bl, bstage(t + 1), frag_of(t + 1), gp, (long)(t + 4) * H3_ROWB,
                                                              bstage(t + 4) + sdst);
                else
                    h3_stage_dma_only<true>(gp, (long)(t + 4) * H3_ROWB, bstage(t + 4) + sdst);
            }
            for (; t + 1 < nkt; ++t) {
                wait_keep(nkt - 2 - t);            // k-tile t+1 has landed; t+2 .. nkt-1 may stay in flight
                H3_BARRIER();
                if (wave_on) h3_stage<false, false, FN, true, false, 1>(acc, ah, al, bh, bl, bstage(t + 1), frag_of(t + 1), nogp, 0, lds);
            }
            if (wave_on) h3_stage<false, false, FN, false, false, 1>(acc, ah, al, bh, bl, lds, f, nogp, 0, lds);
        };
        if (full_n) run(std::true_type{}); else run(std::false_type{});
    } else {
        // ---- waves 0-3: fp32 rows -> raw ring (LDS-DMA) -> split -> A image.  Piece j of a wave: tile rows wave*64 + 16j .. +15, lane ->
        // row +(lane>>2), floats 4q .. 4q+3 of the k-tile with q = lane & 3: chunk q>>1, half q&1 of its hi and lo slots
        const unsigned char* ar[4];
        {
            const int hw = g.cv_Hout * g.cv_Wout;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = wave * 64 + 16 * j + (lane >> 2);
                const int m = min(m0 + r, g.M - 1);
                const int b_ = m / hw, r_ = m - b_ * hw;
                const int h_ = r_ / g.cv_Wout, w_ = r_ - h_ * g.cv_Wout;
                const long pix = (long)b_ * g.cv_Hin * g.cv_Win + (long)(h_ * g.cv_stride) * g.cv_Win + w_ * g.cv_stride;
                ar[j] = sg.A + pix * sg.lda + (lane & 3) * 16;
            }
        }
        const int q = lane & 3, r0 = wave * 64 + (lane >> 2);
        // hi slot of piece 0 (piece j: + j KiB — (r >> 2) & 3 does not depend on j); the lo slot is its neighbour (^ 16)
        const int ad0 = r0 * H3_ROWB + (((2 * (q >> 1)) ^ ((r0 >> 2) & 3)) << 4) + (q & 1) * 8;
        const int rawoff = H3F_RAW + wave * 4096;                       // this wave's 4 KB of a raw slot
        const unsigned rawrd = h3_lds_addr(lds) + rawoff + lane * 16;   // the 16 B this lane fetched (the DMA's destination is lane-linear)
        auto dma = [&](int u, int slot) {
#pragma unroll
            for (int j = 0; j < 4; ++j) h3_glds16(ar[j] + (long)u * (H3_BK * 4), lds + rawoff + slot * H3_OPER + j * 1024);
        };
        // k-tile u (its DMA and those of u+1, u+2 are the ones in flight): raw slot -> split -> image, then k-tile u+3 into the slot
        auto advance = [&](int u, int slot) {
            wait_keep(min(u + 2, nkt - 1) - u);
            f32x4 v[4];
            const unsigned ra = rawrd + slot * H3_OPER;
            h3f_raw_read<0>(v[0], ra); h3f_raw_read<1024>(v[1], ra); h3f_raw_read<2048>(v[2], ra); h3f_raw_read<3072>(v[3], ra);
            h3f_raw_fence(v);
            if (u + 3 < nkt) dma(u + 3, slot);                         // (this lane's reads of the slot have returned)
            unsigned char* img = lds + H3F_AI + (u & 1) * H3_OPER + ad0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f16x4 hi, lo;
#pragma unroll
                for (int i = 0; i < 4; ++i) {                           // the arithmetic of h3_store_chunk
                    const float xs = v[j][i] * a_mul;
                    const _Float16 t = (_Float16)xs;
                    hi[i] = t;
                    lo[i] = (_Float16)(xs - (float)t);
                }
                *reinterpret_cast<f16x4*>(img + j * 1024) = hi;
                *reinterpret_cast<f16x4*>((img + j * 1024) + ((ad0 & 16) ? -16 : 16)) = lo;
            }
        };
        // prologue: k-tiles 0 .. 2 requested, 0 and 1 into their images (3 and 4 requested behind them)
#pragma unroll
        for (int p = 0; p < H3F_NRAW; ++p)
            if (p < nkt) dma(p, p);
        advance(0, 0);
        if (1 < nkt) advance(1, 1);
        H3_BARRIER();
        first_frags();
        // stage t, after its barrier: k-tile t+1 is readable and every wave has left the image of k-tile t (= that of k-tile t+2)
        auto run = [&](auto fulln) {
            constexpr bool FN = decltype(fulln)::value;
            int slot = 2;
            for (int t = 0; t + 1 < nkt; ++t) {
                H3_BARRIER();
                if (t + 2 < nkt) advance(t + 2, slot);
                slot = slot == H3F_NRAW - 1 ? 0 : slot + 1;
                if (wave_on) h3_stage<false, false, FN, true, false, 0>(acc, ah, al, bh, bl, bstage(t + 1), frag_of(t + 1), nogp, 0, lds);
            }
            if (wave_on) h3_stage<false, false, FN, false, false, 0>(acc, ah, al, bh, bl, lds, f, nogp, 0, lds);
        };
        if (full_n) run(std::true_type{}); else run(std::false_type{});
    }

    // ---- epilogue: the non-PAIRED store() paths of gemm_h3_kernel (same expressions, same order), one row scale for all rows
    const float sr = sg.sa[0];
    const float* sb = sg.sb;
    const int sbm = sg.sb_mul;
    const int lrow0 = wm * 128 + 4 * h, lcol0 = wn * 32 + l31;
    auto epilogue = [&](auto tag) {
        constexpr bool CHECK = decltype(tag)::value;
        int lrow = lrow0, lcol = lcol0;
        asm volatile("" : "+v"(lrow), "+v"(lcol));
        auto rowm = [&](int lr) { return CHECK ? min(m0 + lr, g.M - 1) : m0 + lr; };
        int nn[2];
        decltype(epi.col(0, 0)) cc[2];
        float sc[2];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            nn[tn] = n0 + tn * 128 + lcol;
            const int nc = min(nn[tn], g.N - 1);
            cc[tn] = epi.col(z, nc);
            sc[tn] = sb[(long)nc * sbm];
        }
        touch(cc[0]); touch(cc[1]); touch(sc[0]); touch(sc[1]);
        if constexpr (epi_has_aux<Epi>::value) {
            // 16 half row blocks (tn, tm, half): the aux operands run H3_AUX_AHEAD blocks ahead of the stores
            constexpr int AH = H3_AUX_AHEAD;
            decltype(epi.aux(0, 0, 0, RowT{})) ax[AH + 1][8];
            auto fetch = [&](int i, int set) {
                const int tn = i >> 3, tm = (i >> 1) & 3, half = i & 1;
                int lb = lrow + tm * 32;
                asm volatile("" : "+v"(lb));
#pragma unroll
                for (int r8 = 0; r8 < 8; ++r8) {
                    const int r = half * 8 + r8;
                    const int lr = lb + (r & 3) + 8 * (r >> 2);
                    ax[set][r8] = epi.aux(z, rowm(lr), min(nn[tn], g.N - 1), RowT{});
                }
            };
#pragma unroll
            for (int i = 0; i < AH; ++i) fetch(i, i % (AH + 1));
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                __builtin_amdgcn_sched_barrier(0);
                if (i + AH < 16) fetch(i + AH, (i + AH) % (AH + 1));
                const int tn = i >> 3, tm = (i >> 1) & 3, half = i & 1;
                int lb = lrow + tm * 32;
                asm volatile("" : "+v"(lb));
#pragma unroll
                for (int r8 = 0; r8 < 8; ++r8) touch(ax[i % (AH + 1)][r8]);
                if (nn[tn] < g.N) {
#pragma unroll
                    for (int r8 = 0; r8 < 8; ++r8) {
                        const int r = half * 8 + r8;
                        const int lr = lb + (r & 3) + 8 * (r >> 2);
                        if (!CHECK || m0 + lr < g.M)
                            epi.store(z, m0 + lr, nn[tn], acc[tm][tn][r] * (sr * sc[tn]), RowT{}, cc[tn], ax[i % (AH + 1)][r8]);
                    }
                }
            }
        } else {
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                if (nn[tn] >= g.N) continue;
#pragma unroll
                for (int tm = 0; tm < 4; ++tm) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int lr = lrow + tm * 32 + (r & 3) + 8 * (r >> 2);
                        if (!CHECK || m0 + lr < g.M) epi.store(z, m0 + lr, nn[tn], acc[tm][tn][r] * (sr * sc[tn]), RowT{}, cc[tn]);
                    }
                }
            }
        }
    };
    if (m0 + 256 <= g.M) epilogue(std::false_type{}); else epilogue(std::true_type{});
}

// A = fp32 NHWC pixel rows (g.seg[0].A, lda = pixel pitch in BYTES, >= 4 * K, 16-byte aligned), g.seg[0].sa = the device float 1 / a_mul,
// sa_mul = 0; B = weight planes [N][K] + row scales; the 1x1 geometry in g.cv_Hin / cv_Win / cv_Hout / cv_Wout / cv_stride, M = B*Hout*Wout
template <class Epi>
inline hipError_t launch_gemm_h3f(H3Args g, float a_mul, Epi epi, hipStream_t st) {
    static const hipError_t attr_rc = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_h3f_kernel<Epi>), hipFuncAttributeMaxDynamicSharedMemorySize, H3F_LDS);
    (void)attr_rc;
    const H3Seg& sg = g.seg[0];
    if (g.nseg != 1 || g.M < 1 || g.N < 1 || sg.K < 16 || sg.K % 16 || sg.sa_mul != 0 || !sg.A || !sg.B || !sg.sa || !sg.sb) return hipErrorInvalidValue;
    if (sg.lda < 4L * sg.K || sg.lda % 16 || sg.ldb < 4L * sg.K || sg.ldb % 16 || !(a_mul > 0.f)) return hipErrorInvalidValue;
    if (g.cv_Hin < 1 || g.cv_Win < 1 || g.cv_Hout < 1 || g.cv_Wout < 1 || g.cv_stride < 1 || g.M % (g.cv_Hout * g.cv_Wout)) return hipErrorInvalidValue;
    if ((long)(g.cv_Hout - 1) * g.cv_stride >= g.cv_Hin || (long)(g.cv_Wout - 1) * g.cv_stride >= g.cv_Win) return hipErrorInvalidValue;      // every pixel read exists
    g.tiles_m = (g.M + H3_BM - 1) / H3_BM;
    g.tiles_n = (g.N + H3_BN - 1) / H3_BN;
    g.batches = 1;
    g.mp = (g.tiles_m * g.tiles_n + 7) / 8;
    hipLaunchKernelGGL((gemm_h3f_kernel<Epi>), dim3(8 * g.mp), dim3(H3_THREADS), H3F_LDS, st, g, a_mul, epi);
    return hipGetLastError();
}

}  // namespace tdx
