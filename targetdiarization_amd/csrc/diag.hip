// diag.hip — libtdx_diag.so: test hooks and timing diagnostics of the GEMM cores (declared in include/tdx_test.h).
// NOT part of the product library: libtdx.so exports only what include/tdx.h declares.  Used by tests/test_gpu_h3.py
// (numerics of the split-f16 x3 core in all operand modes), tests/test_gpu_h3_forms.py (every operand form and tile map of that core,
// the split producers), tests/test_h3_tile_map.py (its block -> tile map on the host, no device), tests/test_gpu_gemm_f32.py (the fp32
// MFMA core in every operand mode and on both tile maps), tests/test_gpu_epilogues.py (the shared epilogue family), tests/test_gpu_attention_gate.py (the gated attention
// launch exactly as the model issues it), tests/test_dft_basis_host.py (the host-built DFT bases, no device), tests/test_loaders.py
// (the Loader's pointer binding, no device) and by tools/ (timing variants, operand fill rates).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <initializer_list>
#include <string>

#include "../../include/tdx.h"
#include "../../include/tdx_test.h"
#include "dft_basis.hpp"
#include "epilogues.hpp"
#include "fft.hpp"
#include "gemm_h3f.hpp"
#include "mf2_attention.hpp"
#include "weight_pack.hpp"
#include "whisper_noise.hpp"

using namespace tdx;

namespace {
template <class Act>
int linear_epi(const float* a, const float* w, const float* bias, const float* res, float* out, int M, int Npad, int nreal, int K, hipStream_t st) {
    if (res && nreal < Npad) return linear_f32(a, K, w, M, Npad, K, EpiBiasResN<Act>{bias, res, out, Npad, nreal}, st);
    if (res) return linear_f32(a, K, w, M, Npad, K, EpiBiasRes<Act>{bias, res, out, Npad}, st);
    if (nreal < Npad) return linear_f32(a, K, w, M, Npad, K, EpiBiasActN<Act>{bias, out, Npad, nreal}, st);
    return linear_f32(a, K, w, M, Npad, K, EpiBiasAct<Act>{bias, out, Npad}, st);
}

// test-local plain stores of the fp32 core's operand-mode hooks (tdx_gemm_f32 / tdx_gemm_f32_conv): out[z][m][n] = v for n < nreal.
// (EpiStoreZ also stores the zero accumulators of the column tiles the kernel skipped, which would hide a wrongly skipped tile.)
struct EpiPlainN {
    float* out; long ld, strideZ; int nreal;
    __device__ EpiNone col(int, int) const { return EpiNone{}; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store(int z, int m, int n, float v, EpiNone, EpiNone) const {
        if (n < nreal) out[(long)z * strideZ + (long)m * ld + n] = v;
    }
};
struct EpiPlainPair {      // PAIRED: v0 -> column c, v1 -> column pair_off + c, for c < nreal
    float* out; long ld, strideZ; int nreal, pair_off;
    __device__ EpiNone col(int, int) const { return EpiNone{}; }
    __device__ EpiNone row(int, int) const { return EpiNone{}; }
    __device__ void store2(int z, int m, int c, float v0, float v1, EpiNone, EpiNone) const {
        if (c < nreal) {
            float* o = out + (long)z * strideZ + (long)m * ld;
            o[c] = v0; o[pair_off + c] = v1;
        }
    }
};

void plan_out(const GemmArgs& g, int* plan) {
    if (plan) { plan[0] = g.map_mode; plan[1] = g.mp; plan[2] = g.gw; plan[3] = g.tiles_m; plan[4] = g.tiles_n; }
}
template <bool PAIRED, bool CONV>
void plan_of(GemmArgs g, int batches, int* plan) {       // what launch_gemm is about to compute for g
    plan_gemm<PAIRED, CONV>(g, batches);
    plan_out(g, plan);
}

const char* seg_error(const tdx_gemm_seg& s, bool a_kmajor, bool b_kmajor, int batches) {
    if (!s.A || !s.B) return "null operand";
    if (s.K < 32 || s.K % 32) return "need K >= 32, K % 32 == 0";
    if (s.lda < 1 || s.ldb < 1 || s.lda % 4 || s.ldb % 4) return "need lda % 4 == 0, ldb % 4 == 0";
    if (s.strideA < 0 || s.strideB < 0 || s.strideA2 < 0 || s.strideB2 < 0 || s.strideA % 4 || s.strideB % 4 || s.strideA2 % 4 || s.strideB2 % 4)
        return "need batch strides >= 0 and % 4 == 0 (16-byte loads)";
    if (s.zdiv < 1 || s.kchunk < 0) return "need zdiv >= 1, kchunk >= 0";
    // K-major operands read row min(k, kvalid - 1): kvalid = ktotal - z2 * kchunk must stay >= 1 for the largest z2 of the launch
    if ((a_kmajor || b_kmajor) && (long)s.ktotal - (long)(std::min(s.zdiv, batches) - 1) * s.kchunk < 1)
        return "need ktotal - z2 * kchunk >= 1 for every z2 of a K-major operand";
    return nullptr;
}
GemmSeg seg_of(const tdx_gemm_seg& s) {
    GemmSeg r = make_seg(s.A, s.lda, s.B, s.ldb, s.K, s.strideA, s.strideB, s.ktotal);
    r.zdiv = s.zdiv; r.strideA2 = s.strideA2; r.strideB2 = s.strideB2; r.kchunk = s.kchunk; r.ktotal = s.ktotal;
    return r;
}
template <bool A_KMAJOR, bool B_KMAJOR, bool PAIRED, bool CONV, class Epi>
int run_gemm_f32(const GemmArgs& g, int batches, Epi e, int* plan, hipStream_t st) {
    plan_of<PAIRED, CONV>(g, batches, plan);
    const hipError_t r = launch_gemm<A_KMAJOR, B_KMAJOR, PAIRED, false, Epi, 0, CONV>(g, batches, e, st);
    return r == hipSuccess ? TDX_OK : tdx::fail_hip(r, __FILE__, __LINE__);
}

// ---- the x3 core's operand-form hook (tdx_h3_gemm_ex)
H3Seg h3_seg_of(const tdx_h3_seg& s) {
    H3Seg r{};
    r.A = (const unsigned char*)s.A; r.B = (const unsigned char*)s.B; r.sa = s.sa; r.sb = s.sb; r.lda = s.lda; r.ldb = s.ldb;
    r.strideA = s.strideA; r.strideB = s.strideB; r.strideA2 = s.strideA2; r.strideB2 = s.strideB2;
    r.strideSA = s.strideSA; r.strideSB = s.strideSB; r.strideSA2 = s.strideSA2; r.strideSB2 = s.strideSB2;
    r.sa_mul = s.sa_mul; r.sb_mul = s.sb_mul; r.K = s.K; r.zdiv = s.zdiv; r.kchunk = s.kchunk; r.ktotal = s.ktotal;
    r.segk = s.segk; r.strideSeg = s.strideSeg; r.a_shift = s.a_shift; r.a_period = s.a_period; r.a_zero = (const unsigned char*)s.a_zero;
    return r;
}
// form: bit 0 K-major B, bit 1 PAIRED, bit 2 TWOSEG, bit 3 A_CONV.  The optional fields are accepted where the product sets them and nowhere
// else: kchunk / ktotal on <F,T,F,F>, segk on <F,F,F,F>, a_shift / a_period on the first segment of <F,F,F,T> (the only place where the
// kernel also shifts the row scale)
const char* h3_seg_error(const tdx_h3_seg& s, int form, bool first, int batches) {
    const bool twoseg = form & 4, shift_ok = first && form == 4;
    if (!s.A || !s.B || !s.sa || !s.sb) return "null operand or scale";
    if (s.K < 16 || s.K % 16) return "need K >= 16, K % 16 == 0";
    if (twoseg && s.K < 64) return "TWOSEG needs K >= 64 in both segments";
    if (s.lda < 64 || s.ldb < 64 || s.lda % 16 || s.ldb % 16) return "need lda, ldb >= 64 bytes and % 16 == 0 (16-byte loads)";
    for (long v : {s.strideA, s.strideB, s.strideA2, s.strideB2})
        if (v < 0 || v % 16) return "need operand strides >= 0 and % 16 == 0 (16-byte loads)";
    for (long v : {s.strideSA, s.strideSB, s.strideSA2, s.strideSB2, s.strideSeg})
        if (v < 0) return "need scale strides >= 0";
    if (s.zdiv < 1) return "need zdiv >= 1";
    if ((s.sa_mul != 0 && s.sa_mul != 1) || (s.sb_mul != 0 && s.sb_mul != 1)) return "need sa_mul, sb_mul in {0, 1}";
    if (s.kchunk < 0 || s.ktotal < 0) return "need kchunk >= 0, ktotal >= 0";
    if (s.kchunk) {
        if (form != 1) return "kchunk: the one segment of <F,T,F,F> only";
        if (s.kchunk % 16 || s.ktotal % 16) return "need kchunk % 16 == 0, ktotal % 16 == 0";
        // batch z2 covers min(K, ktotal - z2 * kchunk) k rows: at least one k-tile for the largest z2 of the launch
        if ((long)s.ktotal - (long)(std::min(s.zdiv, batches) - 1) * s.kchunk < 16) return "kchunk / ktotal leave a z2 of the launch without a k-tile";
    }
    if (s.segk) {
        if (form != 0) return "segk: the one segment of <F,F,F,F> only";
        if (s.segk < 64 || s.segk % 64 || s.K % s.segk || s.K / s.segk > 8) return "need segk % 64 == 0, K % segk == 0, K / segk <= 8";
    }
    if (s.a_shift || s.a_period) {
        if (!shift_ok) return "a_shift / a_period: the first segment of a row-major TWOSEG launch only";
        if (s.a_shift != -1 || s.a_period < 1) return "need a_shift == -1 with a_period >= 1 (row -1 would be read otherwise)";
        if (!s.a_zero) return "a_period without a_zero";
    }
    return nullptr;
}
void h3_plan_out(const H3Args& g, int* plan) {
    if (plan) { plan[0] = g.map_mode; plan[1] = g.mp; plan[2] = g.gw; plan[3] = g.mc; plan[4] = g.tiles_m; plan[5] = g.tiles_n; }
}
template <bool B_TR, bool PAIRED, bool TWOSEG, bool A_CONV, class Epi>
int run_gemm_h3(const H3Args& g, int batches, Epi e, int* plan, hipStream_t st) {
    H3Args p = g;                       // what launch_gemm_h3x is about to compute for g
    plan_gemm_h3<PAIRED, Epi>(p, batches);
    h3_plan_out(p, plan);
    const hipError_t r = launch_gemm_h3x<false, B_TR, PAIRED, TWOSEG, Epi, 0, A_CONV>(g, batches, e, st);
    return r == hipSuccess ? TDX_OK : tdx::fail_hip(r, __FILE__, __LINE__);
}
}  // namespace

extern "C" {

const char* tdx_diag_last_error(void) { return tdx::last_error().c_str(); }

// timing-only diagnostic: see gemm.hpp VARIANT
int tdx_linear_variant(const float* a, const float* w, int M, int N, int K, float* c, int variant, void* stream) {
    GemmArgs g = make_args(M, N, make_seg(a, K, w, K, K));
    EpiStoreZ e{c, (long)N, 0};
    hipError_t r;
    if (variant == 1) r = launch_gemm<false, false, false, false, EpiStoreZ, 1>(g, 1, e, (hipStream_t)stream);
    else if (variant == 2) r = launch_gemm<false, false, false, false, EpiStoreZ, 2>(g, 1, e, (hipStream_t)stream);
    else if (variant == 3) r = launch_gemm<false, false, false, false, EpiStoreZ, 3>(g, 1, e, (hipStream_t)stream);
    else if (variant == 4) r = launch_gemm<false, false, false, false, EpiStoreZ, 4>(g, 1, e, (hipStream_t)stream);
    else if (variant == 6) r = launch_gemm_x6<false>(g, e, (hipStream_t)stream);
    else r = launch_gemm<false, false, false, false, EpiStoreZ, 0>(g, 1, e, (hipStream_t)stream);
    return r == hipSuccess ? TDX_OK : tdx::fail_hip(r, __FILE__, __LINE__);
}

// the shared epilogue family (epilogues.hpp) on the fp32 core: tests/test_gpu_epilogues.py.  out [M][Npad] =
// act((a [M][K] x w [Npad][K]^T + bias) + res); bias and res may be null, res may be out; columns >= nreal are left alone.
// act: 0 none, 1 relu, 2 relu20, 3 silu, 4 leaky(0.01)
int tdx_linear_epi(const float* a, const float* w, const float* bias, const float* res, float* out, int M, int Npad, int nreal, int K, int act, void* stream) {
    if (!a || !w || !out || M < 1 || Npad < 128 || Npad % 128 || nreal < 1 || nreal > Npad || K < 32 || K % 32 || act < 0 || act > 4)
        return tdx::fail(TDX_E_INVALID, "tdx_linear_epi: need Npad%128==0, 1<=nreal<=Npad, K%32==0, act in 0..4");
    hipStream_t st = (hipStream_t)stream;
    switch (act) {
    case 1: return linear_epi<ActRelu>(a, w, bias, res, out, M, Npad, nreal, K, st);
    case 2: return linear_epi<ActRelu20>(a, w, bias, res, out, M, Npad, nreal, K, st);
    case 3: return linear_epi<ActSilu>(a, w, bias, res, out, M, Npad, nreal, K, st);
    case 4: return linear_epi<ActLeaky<1, 100>>(a, w, bias, res, out, M, Npad, nreal, K, st);
    default: return linear_epi<ActNone>(a, w, bias, res, out, M, Npad, nreal, K, st);
    }
}

// ---- the fp32 core in every operand mode the product issues: tests/test_gpu_gemm_f32.py ------------------------------------------
// Both hooks build a GemmArgs from their arguments and call launch_gemm itself with a plain store (EpiPlainN / EpiPlainPair above).
// They refuse whatever the kernel cannot run safely; the buffers' extents are the caller's business (see include/tdx_test.h).

int tdx_gemm_f32(int a_kmajor, int b_kmajor, int paired, const tdx_gemm_seg* seg0, const tdx_gemm_seg* seg1_or_null, int M, int N, int n_valid,
                 int pair_off, int batches, float* out, long ldo, long strideO, int nreal, int* plan_or_null, void* stream) {
    const auto bad = [](const char* m) { return tdx::fail(TDX_E_INVALID, std::string("tdx_gemm_f32: ") + m); };
    if (!seg0 || !out) return bad("null argument");
    if (paired && a_kmajor) return bad("PAIRED with a K-major A is no product configuration");
    if (M < 1 || batches < 1) return bad("need M >= 1, batches >= 1");
    if (a_kmajor && M % 128) return bad("need M % 128 == 0 with a K-major A (that path has no row guard)");
    if (paired ? (N < 64 || N % 64) : (N < 128 || N % 128)) return bad("need N % 128 == 0 (PAIRED: N % 64 == 0)");
    if (paired ? (nreal < 1 || nreal > N || pair_off < 0 || pair_off % 4) : (nreal < 1 || nreal > n_valid || n_valid > N))
        return bad("need 1 <= nreal <= n_valid <= N (PAIRED: 1 <= nreal <= N, pair_off >= 0, pair_off % 4 == 0)");
    if (ldo < 1 || strideO < 0) return bad("need ldo >= 1, strideO >= 0");
    for (const tdx_gemm_seg* s : {seg0, seg1_or_null})
        if (s)
            if (const char* m = seg_error(*s, a_kmajor != 0, b_kmajor != 0, batches)) return bad(m);
    GemmArgs g = make_args(M, N, seg_of(*seg0));
    if (seg1_or_null) { g.seg[1] = seg_of(*seg1_or_null); g.nseg = 2; }
    if (!paired) g.n_valid = n_valid;
    g.pair_off = paired ? pair_off : 0;
    hipStream_t st = (hipStream_t)stream;
    if (paired) {
        const EpiPlainPair e{out, ldo, strideO, nreal, pair_off};
        return b_kmajor ? run_gemm_f32<false, true, true, false>(g, batches, e, plan_or_null, st)
                        : run_gemm_f32<false, false, true, false>(g, batches, e, plan_or_null, st);
    }
    const EpiPlainN e{out, ldo, strideO, nreal};
    if (a_kmajor && b_kmajor) return run_gemm_f32<true, true, false, false>(g, batches, e, plan_or_null, st);
    if (a_kmajor) return run_gemm_f32<true, false, false, false>(g, batches, e, plan_or_null, st);
    if (b_kmajor) return run_gemm_f32<false, true, false, false>(g, batches, e, plan_or_null, st);
    return run_gemm_f32<false, false, false, false>(g, batches, e, plan_or_null, st);
}

// CONV set the way conv_gemm (eres2net.hip, wespeaker.hip) and head_conv (campplus.hip) set it
int tdx_gemm_f32_conv(const float* a, long lda, const float* w, int B, int Hin, int Win, int Hout, int Wout, int stride, int stride_w, int ntaps,
                      int cin, int N, int n_valid, float* out, long ldo, int nreal, int* plan_or_null, void* stream) {
    const auto bad = [](const char* m) { return tdx::fail(TDX_E_INVALID, std::string("tdx_gemm_f32_conv: ") + m); };
    if (!a || !w || !out) return bad("null argument");
    if (ntaps != 1 && ntaps != 9) return bad("need ntaps 1 or 9");
    if (cin < 32 || cin % 32) return bad("need cin >= 32, cin % 32 == 0");
    if (lda < cin || lda % 4) return bad("need lda >= cin, lda % 4 == 0");
    if (N < 128 || N % 128) return bad("need N % 128 == 0");
    if (nreal < 1 || nreal > n_valid || n_valid > N) return bad("need 1 <= nreal <= n_valid <= N");
    if (B < 1 || Hin < 1 || Win < 1 || Hout < 1 || Wout < 1 || stride < 1 || stride_w < 0) return bad("need positive extents, stride >= 1, stride_w >= 0");
    if ((long)B * Hout * Wout > 0x7fffffffL || (long)B * Hin * Win > 0x7fffffffL) return bad("rows beyond int");
    if (ldo < 1) return bad("need ldo >= 1");
    GemmArgs g = make_args(B * Hout * Wout, N, make_seg(a, lda, w, (long)ntaps * cin, cin));
    g.n_valid = n_valid;
    g.cv_Hin = Hin; g.cv_Win = Win; g.cv_Hout = Hout; g.cv_Wout = Wout; g.cv_stride = stride; g.cv_stride_w = stride_w; g.cv_ntaps = ntaps; g.cv_cin = cin;
    return run_gemm_f32<false, false, false, true>(g, 1, EpiPlainN{out, ldo, 0, nreal}, plan_or_null, (hipStream_t)stream);
}

// ---- the host-built DFT bases (dft_basis.hpp): tests/test_dft_basis_host.py.  Host buffers, no device call.  The fillers write
// their entries and nothing else: `out` is the caller's zeroed image, [rows][ld] for the analysis and [N][ld] for the synthesis.
int tdx_diag_dft_analysis(int N, int nbin, long im_row0, long ld, long rows, int hann, float* out) {
    if (!out || N < 1 || nbin < 1 || nbin > N / 2 + 1 || im_row0 < nbin || im_row0 + nbin > rows || ld < N)
        return tdx::fail(TDX_E_INVALID, "tdx_diag_dft_analysis: need 1 <= nbin <= N / 2 + 1, nbin <= im_row0, im_row0 + nbin <= rows, ld >= N");
    fill_dft_analysis(out, N, nbin, (size_t)im_row0, (size_t)ld, hann ? hann_periodic(N).data() : nullptr);
    return TDX_OK;
}
// gain_kind: 0 = 1 / N (MDX), 1 = hann / 4 (the spectral gate), 2 = hann / N (the phase vocoder, Apollo)
int tdx_diag_dft_synthesis(int N, int nbin, long im_off, long ld, int gain_kind, float* out) {
    if (!out || N < 1 || nbin < 1 || nbin > N / 2 + 1 || im_off < nbin || im_off + nbin > ld || gain_kind < 0 || gain_kind > 2)
        return tdx::fail(TDX_E_INVALID, "tdx_diag_dft_synthesis: need 1 <= nbin <= N / 2 + 1, nbin <= im_off, im_off + nbin <= ld, gain_kind in 0..2");
    const std::vector<double> gain = gain_kind == 0 ? std::vector<double>(N, 1.0 / N) : divided(hann_periodic(N), gain_kind == 1 ? 4.0 : (double)N);
    fill_dft_synthesis(out, N, nbin, (size_t)im_off, (size_t)ld, gain.data());
    return TDX_OK;
}

// ---- the Loader's pointer binding (tdx_common.hpp Loader::bind / resolve): tests/test_loaders.py.  Host buffers, no device call: every
// binding form into a struct of pointer fields and a pre-sized vector of them, the strict checks, resolve() against a host copy of the
// image, every tensor copied out through its bound pointer (the layout is in include/tdx_test.h).
namespace {
struct BindLayer { const float *tap = nullptr, *rows = nullptr; };
struct BindProbe { const float *plain = nullptr, *padded = nullptr, *twice = nullptr, *W = nullptr, *b = nullptr; std::vector<BindLayer> layers; };
}  // namespace
int tdx_diag_loader_bind(const void* blob, size_t blob_bytes, int n, int npad, int L, int C, int k, int N, int K, int Npad, int Kp, float* out,
                         size_t out_floats, int* nonnull) {
    const char* fn = "tdx_diag_loader_bind";
    if (!blob || !out || !nonnull || n < 1 || npad < n || L < 0 || C < 1 || k < 1 || N < 1 || K < 1 || Npad < N || Kp < K)
        return fail(TDX_E_INVALID, std::string(fn) + ": bad argument");
    const size_t sizes[5] = {(size_t)n, (size_t)npad, (size_t)n, (size_t)Npad * Kp, (size_t)Npad}, tap = (size_t)k * C, rows = (size_t)N * Kp;
    if (out_floats != sizes[0] + sizes[1] + sizes[2] + sizes[3] + sizes[4] + L * (tap + rows)) return fail(TDX_E_INVALID, std::string(fn) + ": out_floats does not match");
    Loader ld;
    if (!ld.parse(blob, blob_bytes)) return fail(TDX_E_BLOB, std::string(fn) + ": malformed TDXW blob");
    BindProbe p;
    p.layers.resize(L);           // final size before anything binds into it
    ld.push(p.plain, ld.get("plain", n), n);
    ld.push(p.padded, ld.get("padded", n), n, npad);
    const float* src = ld.get("twice", n);
    const size_t o = ld.room(n);
    ld.bind(p.twice, o);
    if (src) for (int i = 0; i < n; ++i) ld.host[o + i] = 2.0f * src[i];
    bind(ld, p.W, p.b, push_linear(ld, ld.get("lin.weight", {(uint32_t)N, (uint32_t)K}), ld.get("lin.bias", N), N, K, Npad, Kp));
    for (int l = 0; l < L; ++l) {
        const std::string q = "layers." + std::to_string(l) + ".";
        ld.push_tapmajor(p.layers[l].tap, ld.get(q + "tap", (size_t)C * k), C, k);
        ld.push_rows_padded(p.layers[l].rows, ld.get(q + "rows", {(uint32_t)N, (uint32_t)K}), N, K, Kp);
    }
    const int rc = ld.check(fn, true);
    const std::vector<float> image = ld.host;
    if (rc == 0) ld.resolve(image.data());
    const float* field[5] = {p.plain, p.padded, p.twice, p.W, p.b};
    *nonnull = 0;
    for (const float* f : field) *nonnull += f != nullptr;
    for (const BindLayer& w : p.layers) *nonnull += (w.tap != nullptr) + (w.rows != nullptr);
    if (rc != 0) return rc;
    for (int i = 0; i < 5; ++i) { std::copy(field[i], field[i] + sizes[i], out); out += sizes[i]; }
    for (const BindLayer& w : p.layers) { out = std::copy(w.tap, w.tap + tap, out); out = std::copy(w.rows, w.rows + rows, out); }
    return TDX_OK;
}

// diagnostics for the split-f16 x3 core: tests/test_gpu_h3.py, tools/h3_test.py
int tdx_h3_split_rows(const float* x, long ld, void* planes, float* scale, long R, int K, void* stream) {
    if (K % 8 || K > 2048) return tdx::fail(TDX_E_INVALID, "tdx_h3_split_rows: need K%8==0, K<=2048");
    hipError_t r = tdx::launch_h3_split_rows(x, ld, planes, scale, R, K, (hipStream_t)stream);
    return r == hipSuccess ? TDX_OK : tdx::fail_hip(r, __FILE__, __LINE__);
}
int tdx_h3_split_kmajor(const float* x, long ld, void* planes, long K, int N, float s, void* stream) {
    if (N % 128) return tdx::fail(TDX_E_INVALID, "tdx_h3_split_kmajor: need N%128==0");
    const long n = K * (N / 8);
    hipLaunchKernelGGL(tdx::h3_split_kmajor_kernel<0>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ld,
                       (unsigned char*)planes, K, N, s, (const unsigned*)nullptr, (float*)nullptr, 0, 0);
    hipError_t r = hipGetLastError();
    return r == hipSuccess ? TDX_OK : tdx::fail_hip(r, __FILE__, __LINE__);
}
// mode bit 0: A in K-major planes [K][M] (sa = one scale), bit 1: B in K-major planes [K][N] (sb = one scale)
int tdx_h3_gemm_x(int mode, const void* pa, const float* sa, const void* pb, const float* sb, float* c, int M, int N, int K, void* stream) {
    if (K % 16) return tdx::fail(TDX_E_INVALID, "tdx_h3_gemm_x: need K%16==0");
    tdx::H3Args g{};
    const bool atr = mode & 1, btr = mode & 2;
    g.seg[0] = tdx::h3_seg(pa, sa, atr ? 4L * M : 4L * K, pb, sb, btr ? 4L * N : 4L * K, K);
    if (atr) g.seg[0].sa_mul = 0;
    if (btr) g.seg[0].sb_mul = 0;
    g.nseg = 1; g.M = M; g.N = N;
    EpiBiasAct<> e{nullptr, c, N};
    hipError_t r;
    if (atr && btr) r = tdx::launch_gemm_h3x<true, true, false, false>(g, 1, e, (hipStream_t)stream);
    else if (atr) r = tdx::launch_gemm_h3x<true, false, false, false>(g, 1, e, (hipStream_t)stream);
    else if (btr) r = tdx::launch_gemm_h3x<false, true, false, false>(g, 1, e, (hipStream_t)stream);
    else r = tdx::launch_gemm_h3x<false, false, false, false>(g, 1, e, (hipStream_t)stream);
    return r == hipSuccess ? TDX_OK : tdx::fail_hip(r, __FILE__, __LINE__);
}
int tdx_h3_gemm_variant(const void* pa, const float* sa, const void* pb, const float* sb, const float* bias, float* c, int M, int N, int K, int variant, void* stream) {
    tdx::H3Args g{};
    g.seg[0] = tdx::h3_seg(pa, sa, 4L * K, pb, sb, 4L * K, K);
    g.nseg = 1; g.M = M; g.N = N;
    EpiBiasAct<> e{bias, c, N};
    hipError_t r;
    if (variant == 1) r = tdx::launch_gemm_h3<false, EpiBiasAct<>, 1>(g, 1, e, (hipStream_t)stream);
    else if (variant == 2) r = tdx::launch_gemm_h3<false, EpiBiasAct<>, 2>(g, 1, e, (hipStream_t)stream);
    else if (variant == 3) r = tdx::launch_gemm_h3<false, EpiBiasAct<>, 3>(g, 1, e, (hipStream_t)stream);
    else if (variant == 4) r = tdx::launch_gemm_h3<false, EpiBiasAct<>, 4>(g, 1, e, (hipStream_t)stream);
    else if (variant == 9) r = tdx::launch_gemm_h3<false, EpiBiasAct<>, 9>(g, 1, e, (hipStream_t)stream);
    else if (variant == 5) r = tdx::launch_gemm_h3<false, EpiBiasAct<>, 5>(g, 1, e, (hipStream_t)stream);
    else if (variant == 6) r = tdx::launch_gemm_h3<false, EpiBiasAct<>, 6>(g, 1, e, (hipStream_t)stream);
    else r = tdx::launch_gemm_h3<false, EpiBiasAct<>, 0>(g, 1, e, (hipStream_t)stream);
    return r == hipSuccess ? TDX_OK : tdx::fail_hip(r, __FILE__, __LINE__);
}
int tdx_h3_gemm(const void* pa, const float* sa, const void* pb, const float* sb, const float* bias, float* c, int M, int N, int K, void* stream) {
    if (K % 16) return tdx::fail(TDX_E_INVALID, "tdx_h3_gemm: need K%16==0");
    tdx::H3Args g{};
    g.seg[0] = tdx::h3_seg(pa, sa, 4L * K, pb, sb, 4L * K, K);
    g.nseg = 1; g.M = M; g.N = N;
    hipError_t r = tdx::launch_gemm_h3<false>(g, 1, EpiBiasAct<>{bias, c, N}, (hipStream_t)stream);
    return r == hipSuccess ? TDX_OK : tdx::fail_hip(r, __FILE__, __LINE__);
}

// ---- the x3 core in every operand form the product issues, with a plain store: tests/test_gpu_h3_forms.py -----------------------------
// tdx_h3_gemm_ex builds an H3Args from its arguments and calls launch_gemm_h3x itself (EpiPlainN / EpiPlainPair above).  It refuses
// whatever the kernel cannot run safely; the buffers' extents are the caller's business (see include/tdx_test.h).
int tdx_h3_gemm_ex(int b_kmajor, int paired, int twoseg, int a_conv, const tdx_h3_seg* seg0, const tdx_h3_seg* seg1_or_null, int M, int N,
                   int pair_off, int batches, int Hin, int Win, int Hout, int Wout, int stride, int ntaps, int cin, int taps_total,
                   const void* zero_row, float* out, long ldo, long strideO, int nreal, int* plan_or_null, void* stream) {
    const auto bad = [](const char* m) { return tdx::fail(TDX_E_INVALID, std::string("tdx_h3_gemm_ex: ") + m); };
    if (!seg0 || !out) return bad("null argument");
    const int form = (b_kmajor ? 1 : 0) | (paired ? 2 : 0) | (twoseg ? 4 : 0) | (a_conv ? 8 : 0);
    if (form != 0 && form != 1 && form != 2 && form != 4 && form != 7 && form != 8)
        return bad("no product instance: <F,F,F,F>, <F,T,F,F>, <F,F,T,F>, <F,F,F,T>, <F,T,T,T> and A_CONV on <F,F,F,F> only");
    if ((twoseg != 0) != (seg1_or_null != nullptr)) return bad("TWOSEG needs seg1, one segment needs seg1 == NULL");
    if (M < 1 || batches < 1) return bad("need M >= 1, batches >= 1");
    if (N < 1 || ((b_kmajor || paired) && N % 128)) return bad("need N >= 1; N % 128 == 0 with a K-major B or PAIRED");
    if (nreal < 1 || nreal > N || pair_off < 0 || (!paired && pair_off)) return bad("need 1 <= nreal <= N, pair_off >= 0 (PAIRED only)");
    if (paired && b_kmajor && pair_off % 128) return bad("need pair_off % 128 == 0 with a K-major B");
    if (ldo < 1 || strideO < 0) return bad("need ldo >= 1, strideO >= 0");
    if (const char* m = h3_seg_error(*seg0, form, true, batches)) return bad(m);
    if (seg1_or_null)
        if (const char* m = h3_seg_error(*seg1_or_null, form, false, batches)) return bad(m);
    if (b_kmajor)
        for (const tdx_h3_seg* s : {seg0, seg1_or_null})
            if (s && s->ldb < 4L * (pair_off + N)) return bad("need ldb >= 4 * (pair_off + N) bytes with a K-major B");
    H3Args g{};
    g.seg[0] = h3_seg_of(*seg0);
    if (seg1_or_null) g.seg[1] = h3_seg_of(*seg1_or_null);
    g.nseg = seg1_or_null ? 2 : 1; g.M = M; g.N = N; g.pair_off = pair_off;
    if (a_conv) {
        const int nt = taps_total ? taps_total : ntaps;
        if (!zero_row) return bad("A_CONV without zero_row");
        if (nt != 1 && nt != 9) return bad("need 1 or 9 taps in all");
        if (ntaps < 1 || taps_total < 0 || (taps_total && taps_total % ntaps)) return bad("need ntaps >= 1, taps_total % ntaps == 0");
        if (batches != (taps_total ? taps_total / ntaps : 1)) return bad("need batches == taps_total / ntaps (1 without taps_total)");
        if (cin < 64 || cin % 16) return bad("need cin >= 64, cin % 16 == 0");
        if (seg0->K != ntaps * cin) return bad("need K == ntaps * cin");
        if (seg0->lda < 4L * cin) return bad("need lda >= 4 * cin bytes");
        if (Hin < 1 || Win < 1 || Hout < 1 || Wout < 1 || stride < 1) return bad("need positive extents, stride >= 1");
        if ((long)Hout * Wout > 0x7fffffffL || M % (Hout * Wout)) return bad("need M == B * Hout * Wout");
        if ((long)(M / (Hout * Wout)) * Hin * Win > 0x7fffffffL) return bad("rows beyond int");
        g.cv_Hin = Hin; g.cv_Win = Win; g.cv_Hout = Hout; g.cv_Wout = Wout; g.cv_stride = stride; g.cv_ntaps = ntaps; g.cv_cin = cin;
        g.cv_taps_total = taps_total; g.zero_row = (const unsigned char*)zero_row;
    }
    hipStream_t st = (hipStream_t)stream;
    if (paired) {
        const EpiPlainPair e{out, ldo, strideO, nreal, pair_off};
        return b_kmajor ? run_gemm_h3<true, true, true, false>(g, batches, e, plan_or_null, st)
                        : run_gemm_h3<false, true, false, false>(g, batches, e, plan_or_null, st);
    }
    const EpiPlainN e{out, ldo, strideO, nreal};
    if (a_conv) return run_gemm_h3<false, false, false, true>(g, batches, e, plan_or_null, st);
    if (twoseg) return run_gemm_h3<false, false, true, false>(g, batches, e, plan_or_null, st);
    if (b_kmajor) return run_gemm_h3<true, false, false, false>(g, batches, e, plan_or_null, st);
    return run_gemm_h3<false, false, false, false>(g, batches, e, plan_or_null, st);
}

// the x3 core with an fp32 A operand split while it is staged (gemm_h3f.hpp), with a plain store: tests/test_gpu_h3_f32a.py.  The same product
// as tdx_h3_split_rows_static(a, s = a_mul) + tdx_h3_gemm_ex(A_CONV, one tap, sa = inv_dev, sa_mul = 0) on the same data, bit for bit.
int tdx_h3_gemm_f32a(const float* a, long lda, float a_mul, const float* inv_dev, const void* pb, const float* sb, int M, int N, int K,
                     int Hin, int Win, int Hout, int Wout, int stride, float* out, long ldo, int nreal, void* stream) {
    const auto bad = [](const char* m) { return tdx::fail(TDX_E_INVALID, std::string("tdx_h3_gemm_f32a: ") + m); };
    if (!a || !inv_dev || !pb || !sb || !out) return bad("null argument");
    if (M < 1 || N < 1 || K < 16 || K % 16) return bad("need M >= 1, N >= 1, K >= 16, K % 16 == 0");
    if (lda < K || lda % 4) return bad("need lda >= K floats, lda % 4 == 0 (16-byte loads)");
    if (!(a_mul > 0.f) || !(a_mul < 3e38f)) return bad("need 0 < a_mul < inf");
    if (nreal < 1 || nreal > N || ldo < 1) return bad("need 1 <= nreal <= N, ldo >= 1");
    if (Hin < 1 || Win < 1 || Hout < 1 || Wout < 1 || stride < 1) return bad("need positive extents, stride >= 1");
    if ((long)Hout * Wout > 0x7fffffffL || M % (Hout * Wout)) return bad("need M == B * Hout * Wout");
    if ((long)(Hout - 1) * stride >= Hin || (long)(Wout - 1) * stride >= Win) return bad("an output pixel reads outside the image");
    if ((long)(M / (Hout * Wout)) * Hin * Win > 0x7fffffffL) return bad("rows beyond int");
    H3Args g{};
    g.seg[0] = h3_seg(a, inv_dev, 4L * lda, pb, sb, 4L * K, K);
    g.seg[0].sa_mul = 0;
    g.nseg = 1; g.M = M; g.N = N;
    g.cv_Hin = Hin; g.cv_Win = Win; g.cv_Hout = Hout; g.cv_Wout = Wout; g.cv_stride = stride; g.cv_ntaps = 1; g.cv_cin = K;
    const hipError_t r = launch_gemm_h3f(g, a_mul, EpiPlainN{out, ldo, 0, nreal}, (hipStream_t)stream);
    return r == hipSuccess ? TDX_OK : tdx::fail_hip(r, __FILE__, __LINE__);
}

// the plan and the block -> tile map of the x3 core on the host (gemm_h3.hpp plan_gemm_h3 / h3_tile_of_block): tests/test_h3_tile_map.py.
// No device call.
int tdx_h3_plan(int M, int N, int ktot, int batches, int paired, int* plan, int* grid) {
    if (!plan || !grid || M < 1 || N < 1 || ktot < 16 || batches < 1 || (paired && N % 128)) return tdx::fail(TDX_E_INVALID, "tdx_h3_plan: bad argument");
    H3Args g{};
    g.nseg = 1; g.seg[0].K = ktot; g.M = M; g.N = N;
    const dim3 gr = paired ? plan_gemm_h3<true, EpiPlainPair>(g, batches) : plan_gemm_h3<false, EpiPlainN>(g, batches);
    h3_plan_out(g, plan);
    grid[0] = (int)gr.x; grid[1] = (int)gr.y;
    return TDX_OK;
}
// returns 1 if block (bx, by) computes tile (*bm, *bn) of batch *z, 0 if it returns at once, < 0 on a bad argument
int tdx_h3_tile_of_block(const int* plan, int batches, int bx, int by, int* z, int* bm, int* bn) {
    if (!plan || !z || !bm || !bn || bx < 0 || by < 0 || batches < 1 || plan[2] < 1 || plan[4] < 1 || plan[5] < 1 || plan[3] < 0 ||
        (plan[0] == 0 && plan[1] < 1)) {
        tdx::fail(TDX_E_INVALID, "tdx_h3_tile_of_block: bad argument");
        return -1;
    }
    H3Args g{};
    g.map_mode = plan[0]; g.mp = plan[1]; g.gw = plan[2]; g.mc = plan[3]; g.tiles_m = plan[4]; g.tiles_n = plan[5]; g.batches = batches;
    *z = *bm = *bn = -1;
    return h3_tile_of_block(g, (unsigned)bx, (unsigned)by, *z, *bm, *bn) ? 1 : 0;
}

// the split producers that no other hook reaches
int tdx_h3_split_rows_static(const float* x, long ld, void* planes, long R, int K, float s, void* stream) {
    if (!x || !planes || R < 1 || K < 8 || K % 8 || ld < K || ld % 4 || !(s > 0.f) || !(s < 3e38f))
        return tdx::fail(TDX_E_INVALID, "tdx_h3_split_rows_static: need R >= 1, K % 8 == 0, ld >= K, ld % 4 == 0, 0 < s < inf");
    hipError_t r = tdx::launch_h3_split_rows_static(x, ld, planes, R, K, s, (hipStream_t)stream);
    return r == hipSuccess ? TDX_OK : tdx::fail_hip(r, __FILE__, __LINE__);
}
int tdx_h3_split_rows_long(const float* x, long ld, void* planes, float* scale, long R, int K, void* stream) {
    if (!x || !planes || !scale || R < 1 || K < 16 || K % 16 || ld < K || ld % 4)
        return tdx::fail(TDX_E_INVALID, "tdx_h3_split_rows_long: need R >= 1, K % 16 == 0, ld >= K, ld % 4 == 0");
    hipError_t r = tdx::launch_h3_split_rows_long(x, ld, planes, scale, R, K, (hipStream_t)stream);
    return r == hipSuccess ? TDX_OK : tdx::fail_hip(r, __FILE__, __LINE__);
}
int tdx_h3_split_kmajor_ex(const float* x, long ld, void* planes, long K, int N, float s, int absmax, unsigned* mx, float* inv, int S, int Sp,
                           void* stream) {
    const auto bad = [](const char* m) { return tdx::fail(TDX_E_INVALID, std::string("tdx_h3_split_kmajor_ex: ") + m); };
    if (!x || !planes || K < 1 || N < 128 || N % 128 || ld < N || ld % 4) return bad("need K >= 1, N % 128 == 0, ld >= N, ld % 4 == 0");
    if ((mx != nullptr) != (inv != nullptr)) return bad("mx and inv come together");
    if (!mx && (!(s > 0.f) || !(s < 3e38f))) return bad("need 0 < s < inf without mx");
    if (absmax && (!mx || ld != N)) return bad("absmax needs mx and a dense source (ld == N)");
    if (Sp < 0 || (Sp > 0 && (S < 1 || S > Sp || K % Sp))) return bad("need 1 <= S <= Sp, K % Sp == 0 with group padding");
    if (Sp == 0 && S != 0) return bad("S without Sp");
    hipStream_t st = (hipStream_t)stream;
    if (absmax) {       // as attn_make_planes (mf2_attention.hpp) does: max |x| over the source rows into mx[0], zeroed first
        const long rows = Sp > 0 ? (K / Sp) * S : K;
        if (hipMemsetAsync(mx, 0, sizeof(unsigned), st) != hipSuccess) return tdx::fail_hip(hipGetLastError(), __FILE__, __LINE__);
        hipLaunchKernelGGL(tdx::h3_absmax_kernel<0>, dim3(1024), dim3(256), 0, st, x, rows * ld, mx);
        const hipError_t ra = hipGetLastError();
        if (ra != hipSuccess) return tdx::fail_hip(ra, __FILE__, __LINE__);
    }
    const long n = K * (N / 8);
    hipLaunchKernelGGL(tdx::h3_split_kmajor_kernel<0>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, ld, (unsigned char*)planes, K, N,
                       mx ? 1.0f : s, (const unsigned*)mx, inv, S, Sp);
    hipError_t r = hipGetLastError();
    return r == hipSuccess ? TDX_OK : tdx::fail_hip(r, __FILE__, __LINE__);
}

// the gated attention launch on the model's own path: tests/test_gpu_attention_gate.py.  Packs the inputs and prepares the operand
// planes as tdx_cal_attention does, then calls attention_core_h3 the way tdx_mf2_forward does — oP / os / oss set (the planes-out gate
// EpiAttnGatePlOut), u itself as the gate's fp32 u operand — with the kernel choice (h3a) and the segment order (swap) as arguments
// instead of the process-wide TDX_H3A / TDX_H3A_SWAP.  kvu_out gets Kvu [B][128][2E] (the reduced split-K launch).
size_t tdx_attn_gate_planes_workspace_bytes(int B, int S, int E) {
    if (B < 1 || S < 1 || E < 128 || E % 128) return 0;
    int sp, kc; size_t a, b, c, d, e, tot;
    attn_plan(B, S, E, sp, kc, a, b, c, d, e, tot);
    return tot * sizeof(float);
}
int tdx_attn_gate_planes(const float* quad_q, const float* lin_q, const float* quad_k, const float* lin_k, const float* v, const float* u,
                         const float* freqs, int B, int S, int E, int h3a, int swap, void* oP, float* os, float* oss, float* kvu_out,
                         void* ws_, size_t ws_bytes, void* stream) {
    if (!quad_q || !lin_q || !quad_k || !lin_k || !v || !u || !freqs || !oP || !os || !oss || !kvu_out || !ws_)
        return tdx::fail(TDX_E_INVALID, "tdx_attn_gate_planes: null argument");
    if (B < 1 || S < 1 || E < 128 || E % 128) return tdx::fail(TDX_E_INVALID, "tdx_attn_gate_planes: need E % 128 == 0");
    int splits, kchunk; size_t oq, ovu, oA, oslab, okvu, tot;
    attn_plan(B, S, E, splits, kchunk, oq, ovu, oA, oslab, okvu, tot);
    if (ws_bytes < tot * sizeof(float)) return tdx::fail(TDX_E_WORKSPACE, "tdx_attn_gate_planes: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)ws_;
    TRY(attn_pack_inputs(quad_q, lin_q, quad_k, lin_k, v, u, freqs, B, S, E, ws, oq, ovu, st));
    AttnPlanes P;
    TRY(attn_prepare_planes(ws, oq, ovu, okvu, B, S, E, P, st));
    TRY(attention_core_h3(P.qkP, P.qks, P.vuP, nullptr, P.stt, B, S, E, splits, kchunk, ws + oA, P.AbufP, P.Asc, ws + oslab, ws + okvu, P.KvuP, P.kvus,
                          nullptr, nullptr, nullptr, st, h3a != 0, swap != 0, (unsigned char*)oP, os, oss, nullptr, nullptr, nullptr, u));
    const hipError_t r = hipMemcpyAsync(kvu_out, ws + okvu, (size_t)B * QK * 2 * E * sizeof(float), hipMemcpyDeviceToDevice, st);
    return r == hipSuccess ? TDX_OK : tdx::fail_hip(r, __FILE__, __LINE__);
}

}  // extern "C"

// ---- diagnostic: per-CU operand fill rate, LDS-DMA vs register staging (tools/fill_bench.py) -------------
namespace {
template <int MODE>      // 0: global_load_lds_dwordx4 ; 1: global_load_dwordx4 + ds_write_b128
__global__ __launch_bounds__(512, 2) void fill_bench_kernel(const unsigned char* __restrict__ src, long bytes_per_block, int iters, float* sink) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned char* base = src + (long)blockIdx.x * bytes_per_block;
    const long span = bytes_per_block / 32768;        // 32 KB tiles in this block's slab
    float acc = 0.f;
    for (int it = 0; it < iters; ++it) {
        const unsigned char* tile = base + (long)(it % span) * 32768;
        unsigned char* dst = lds + (it & 3) * 32768;
        if (MODE == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(tile + (wave * 4 + j) * 1024 + lane * 16),
                                                 (__attribute__((address_space(3))) void*)(dst + (wave * 4 + j) * 1024), 16, 0, 0);
            if ((it & 1) == 1) { asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); __builtin_amdgcn_s_barrier(); }
        } else {
            tdx::f32x4 r[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = *reinterpret_cast<const tdx::f32x4*>(tile + (wave * 4 + j) * 1024 + lane * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) *reinterpret_cast<tdx::f32x4*>(dst + (wave * 4 + j) * 1024 + lane * 16) = r[j];
            if ((it & 1) == 1) __builtin_amdgcn_s_barrier();
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    acc += reinterpret_cast<const float*>(lds)[threadIdx.x];
    if (acc == 123.456f) sink[0] = acc;
}
// GEMM-shaped fill: every block streams k-tiles of an A slab and a B slab (256 rows each, `stride` bytes per row) shared with
// the other blocks of its XCD, either as the row-major planes deliver them (MODE 1: a wave instruction covers 16 rows x 64 B)
// or as contiguous 16 KB tiles of the same slabs (MODE 0: 1 KB per wave instruction).
template <int MODE>
__global__ __launch_bounds__(512, 2) void fill_bench2_kernel(const unsigned char* __restrict__ src, int stride, int iters, float* sink) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
    const long slab = 256L * stride;
    const unsigned char* a = src + (long)(xcd * 4 + ((local >> 3) & 3)) * slab;
    const unsigned char* b = src + 32 * slab + (long)((local >> 2) & 1) * slab;
    const unsigned char* base = wave < 4 ? a : b;
    const int kts = stride / 64;
    float acc = 0.f;
    for (int it = 0; it < iters; ++it) {
        const int kt = it % kts;
        unsigned char* dst = lds + (it & 3) * 32768;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int slot = (wave & 3) * 4 + j;
            const unsigned char* g = MODE == 0 ? base + (long)kt * 16384 + slot * 1024 + lane * 16
                                               : base + (long)(slot * 16 + (lane >> 2)) * stride + kt * 64 + (lane & 3) * 16;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                             (__attribute__((address_space(3))) void*)(dst + (wave * 4 + j) * 1024), 16, 0, 0);
        }
        if ((it & 1) == 1) { asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); __builtin_amdgcn_s_barrier(); }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    acc += reinterpret_cast<const float*>(lds)[threadIdx.x];
    if (acc == 123.456f) sink[0] = acc;
}
}  // namespace
// column-strip streaming (the K^T[V|U] operand pattern): block = (row range, strip); per k row it fetches `seg` contiguous bytes
// of a `pitch`-byte row; 32 KB per iteration.  pitch == seg: a contiguous stream.
namespace {
__global__ __launch_bounds__(512, 2) void fill_bench3_kernel(const unsigned char* __restrict__ src, long pitch, int seg, long rows_per_block, int strips, int iters, float* sink) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int strip = blockIdx.x % strips;
    const long row0 = (long)(blockIdx.x / strips) * rows_per_block;
    const int per_row = seg / 1024;                  // 1 KB instructions per row
    const int rows_per_it = 32 / per_row;
    float acc = 0.f;
    for (int it = 0; it < iters; ++it) {
        unsigned char* dst = lds + (it & 3) * 32768;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = wave * 4 + j;              // instruction 0..31 of this iteration
            const long r = row0 + ((long)it * rows_per_it + i / per_row) % rows_per_block;
            const unsigned char* g = src + r * pitch + (long)strip * seg + (i % per_row) * 1024 + lane * 16;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                             (__attribute__((address_space(3))) void*)(dst + i * 1024), 16, 0, 0);
        }
        if ((it & 1) == 1) { asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); __builtin_amdgcn_s_barrier(); }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    acc += reinterpret_cast<const float*>(lds)[threadIdx.x];
    if (acc == 123.456f) sink[0] = acc;
}
}  // namespace
extern "C" int tdx_fill_bench3(const void* src, long pitch, int seg, long rows_per_block, int strips, int blocks, int iters, float* sink, void* stream) {
    static bool set = false;
    if (!set) { hipFuncSetAttribute(reinterpret_cast<const void*>(&fill_bench3_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 131072); set = true; }
    hipLaunchKernelGGL(fill_bench3_kernel, dim3(blocks), dim3(512), 131072, (hipStream_t)stream, (const unsigned char*)src, pitch, seg, rows_per_block, strips, iters, sink);
    return hipGetLastError() == hipSuccess ? TDX_OK : TDX_E_HIP;
}
extern "C" int tdx_fill_bench2(int mode, const void* src, int stride, int blocks, int iters, float* sink, void* stream) {
    static bool set = false;
    if (!set) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&fill_bench2_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
        hipFuncSetAttribute(reinterpret_cast<const void*>(&fill_bench2_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
        set = true;
    }
    if (mode == 0) hipLaunchKernelGGL(fill_bench2_kernel<0>, dim3(blocks), dim3(512), 131072, (hipStream_t)stream, (const unsigned char*)src, stride, iters, sink);
    else hipLaunchKernelGGL(fill_bench2_kernel<1>, dim3(blocks), dim3(512), 131072, (hipStream_t)stream, (const unsigned char*)src, stride, iters, sink);
    return hipGetLastError() == hipSuccess ? TDX_OK : TDX_E_HIP;
}
extern "C" int tdx_fill_bench(int mode, const void* src, long bytes_per_block, int blocks, int iters, float* sink, void* stream) {
    static bool set = false;
    if (!set) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&fill_bench_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
        hipFuncSetAttribute(reinterpret_cast<const void*>(&fill_bench_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
        set = true;
    }
    if (mode == 0) hipLaunchKernelGGL(fill_bench_kernel<0>, dim3(blocks), dim3(512), 131072, (hipStream_t)stream, (const unsigned char*)src, bytes_per_block, iters, sink);
    else hipLaunchKernelGGL(fill_bench_kernel<1>, dim3(blocks), dim3(512), 131072, (hipStream_t)stream, (const unsigned char*)src, bytes_per_block, iters, sink);
    return hipGetLastError() == hipSuccess ? TDX_OK : TDX_E_HIP;
}

// the FFT of fft.hpp under a small tile (include/tdx_test.h): tests/test_gpu_fft.py
static bool fft_tile_ok(int tile_log2) { return tile_log2 >= tdx::fft::MIN_TILE_LOG2 && tile_log2 <= tdx::fft::MAX_TILE_LOG2; }
extern "C" size_t tdx_test_fft_workspace_bytes(long n, int batch, int tile_log2) {
    if (tdx::fft::size_error(n, batch) || !fft_tile_ok(tile_log2)) return 0;
    return std::max<size_t>(tdx::fft::c2c_ws_floats(n, batch, tile_log2), 64) * sizeof(float);
}
extern "C" int tdx_test_fft_passes(int m, int tile_log2) { return m < 0 || m > 27 || !fft_tile_ok(tile_log2) ? 0 : tdx::fft::passes_of(m, tile_log2); }
extern "C" int tdx_test_fft_c2c(const float* x_dev, long n, int batch, int inverse, float* y_dev, void* ws, size_t ws_bytes, void* stream, int tile_log2) {
    if (!x_dev || !y_dev || !ws || x_dev == y_dev) return tdx::fail(TDX_E_INVALID, "tdx_test_fft_c2c: need x_dev, y_dev, ws, x_dev != y_dev");
    if (const char* e = tdx::fft::size_error(n, batch)) return tdx::fail(TDX_E_INVALID, std::string("tdx_test_fft_c2c: ") + e);
    if (!fft_tile_ok(tile_log2)) return tdx::fail(TDX_E_INVALID, "tdx_test_fft_c2c: need 4 <= tile_log2 <= 12");
    if (ws_bytes < tdx_test_fft_workspace_bytes(n, batch, tile_log2)) return tdx::fail(TDX_E_INVALID, "tdx_test_fft_c2c: workspace too small");
    return tdx::fft::c2c(x_dev, n, batch, inverse != 0, y_dev, (float*)ws, tile_log2, (hipStream_t)stream);
}

// the noise of Whisper's sampled decoding as the vocabulary head computes it (whisper_noise.hpp): tests/test_gpu_whisper_fallback.py
namespace {
__global__ __launch_bounds__(256) void whisper_noise_kernel(unsigned long long seed, unsigned long long row_stream, int p, int n0, int count,
                                                             float* __restrict__ g, unsigned* __restrict__ word) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int n = n0 + i;
    const unsigned w = tdx::wh_noise_words(seed, row_stream, p, n >> 2).w[n & 3];
    word[i] = w;
    g[i] = tdx::wh_gumbel(w);
}
}  // namespace
extern "C" int tdx_test_whisper_noise(unsigned long long seed, unsigned long long row_stream, int p, int n0, int count, float* g_dev, unsigned* word_dev,
                                      void* stream) {
    if (!g_dev || !word_dev || n0 < 0 || p < 0 || count < 1 || n0 > INT_MAX - count)
        return tdx::fail(TDX_E_INVALID, "tdx_test_whisper_noise: need g_dev, word_dev, n0 >= 0, p >= 0, count >= 1");
    hipLaunchKernelGGL(whisper_noise_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed, row_stream, p, n0, count, g_dev, word_dev);
    return hipGetLastError() == hipSuccess ? TDX_OK : TDX_E_HIP;
}
