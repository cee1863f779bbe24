/* tdx_test.h — exports of libtdx_diag.so: test hooks and timing diagnostics of the GEMM cores.
 *
 * NOT part of the product boundary (include/tdx.h / libtdx.so).  libtdx_diag.so is a separate library built
 * from csrc/diag.hip over the same kernel headers; tests/test_gpu_h3.py checks the numerics of the split-f16 x3
 * core through it, tests/test_gpu_gemm_f32.py the operand modes and tile maps of the fp32 MFMA core,
 * tests/test_gpu_epilogues.py the shared epilogues, tests/test_gpu_attention_gate.py the gated attention launch,
 * and tools/ time its variants.  Same conventions as tdx.h (device pointers, void* stream, 0 = ok). */
#ifndef TDX_TEST_H
#define TDX_TEST_H

#ifdef __cplusplus
extern "C" {
#endif

const char* tdx_diag_last_error(void);

/* fp32 rows x[R][ld] -> split-f16 planes [R][K/8][2][8] + one power-of-two scale per row (gemm_h3.hpp) */
int tdx_h3_split_rows(const float* x_dev, long ld, void* planes_dev, float* scale_dev, long R, int K, void* stream);
/* fp32 x[K][ld] -> K-major planes [K][N/32][2][32] with the static scale s */
int tdx_h3_split_kmajor(const float* x_dev, long ld, void* planes_dev, long K, int N, float s, void* stream);
/* C[M,N] = A B^T on the x3 core; mode bit 0: A in K-major planes (sa = one scale), bit 1: B in K-major planes */
int tdx_h3_gemm_x(int mode, const void* pa, const float* sa, const void* pb, const float* sb, float* c_dev,
                  int M, int N, int K, void* stream);
/* row-major planes, bias epilogue */
int tdx_h3_gemm(const void* pa, const float* sa, const void* pb, const float* sb, const float* bias_dev, float* c_dev,
                int M, int N, int K, void* stream);
/* timing variants of the x3 main loop (gemm_h3.hpp VARIANT: 0 product, 1 no loads, 2 no fragment reads, 3 neither,
 * 4 no barrier, 5 ping-pong, 6 v_mfma_f32_16x16x32_f16 instead of 32x32x16 (same flops), 9 loads never waited for); only 0 and 5
 * produce correct results.  (The narrow two-blocks-per-CU kernel and the pair-stage 16x16x32 kernel of round 2 — variants 10 / 16 /
 * 20 — lost inside the model and were removed in round 3; their measurements are in DESIGN.md §4.1e.) */
int tdx_h3_gemm_variant(const void* pa, const float* sa, const void* pb, const float* sb, const float* bias_dev,
                        float* c_dev, int M, int N, int K, int variant, void* stream);
/* timing variants of the fp32-MFMA core (gemm.hpp VARIANT) and the x6 core (variant 6) */
int tdx_linear_variant(const float* a_dev, const float* w_dev, int M, int N, int K, float* c_dev, int variant, void* stream);
/* the shared epilogue family (csrc/epilogues.hpp) on the fp32-MFMA core: out[M][Npad] = act((a[M][K] w[Npad][K]^T + bias) + res),
 * columns >= nreal left untouched.  bias_or_null, res_or_null may be NULL; res may be out.  Picks EpiBiasAct / EpiBiasActN /
 * EpiBiasRes(N) from the arguments.  act: 0 none, 1 relu, 2 relu20, 3 silu, 4 leaky_relu(0.01).  Npad % 128 == 0, K % 32 == 0. */
int tdx_linear_epi(const float* a_dev, const float* w_dev, const float* bias_or_null, const float* res_or_null, float* out_dev,
                   int M, int Npad, int nreal, int K, int act, void* stream);

/* the fp32-MFMA core (csrc/gemm.hpp gemm_f32_kernel / launch_gemm) in every operand mode the product issues, with a plain store:
 *   out[z*strideO + m*ldo + n] = sum over segments, sum over k of A_seg[z][m][k] * B_seg[z][k][n]      for n < nreal.
 * One K segment as GemmSeg has it: A row-major [M][lda] (K contiguous) or, with a_kmajor, [K][lda] (M contiguous); B row-major
 * [N][ldb] (a weight) or, with b_kmajor, [K][ldb].  Batch z = z1 * zdiv + z2 reads A + z1*strideA + z2*strideA2 (B likewise); rows
 * k >= ktotal - z2*kchunk of a K-major operand count as zero (row-major operands ignore kchunk / ktotal). */
typedef struct tdx_gemm_seg {
    const float* A;
    const float* B;
    long lda, ldb, strideA, strideB, strideA2, strideB2;
    int K, zdiv, kchunk, ktotal;
} tdx_gemm_seg;
/* a_kmajor / b_kmajor / paired pick the template instance: <F,F>, <T,F>, <F,T>, <T,T>, and PAIRED on <F,F> and <F,T>.  PAIRED: N pair
 * columns; column c pairs B column c with B column pair_off + c and stores them to out columns c and pair_off + c (c < nreal; n_valid
 * unused).  Otherwise columns >= n_valid are skipped by the kernel, and nreal <= n_valid <= N.  plan_or_null (host, 5 ints) receives
 * what launch_gemm planned for this launch: map_mode, mp, gw, tiles_m, tiles_n.
 * Refused (TDX_E_INVALID): K % 32, N % 128 (PAIRED: N % 64), lda % 4, ldb % 4, strides % 4, M < 1, M % 128 with a_kmajor (no row
 * guard on that path), zdiv < 1, ktotal - z2*kchunk < 1 for a z2 of the launch with a K-major operand (the clamped row would be -1),
 * a null pointer.  The caller owns the extents: a row-major B needs N (PAIRED: pair_off + N) rows, a K-major B 128-column reads from
 * every valid row (32 floats of slack behind the last row when ldb < 128), a K-major A needs M % 128 == 0 columns. */
int tdx_gemm_f32(int a_kmajor, int b_kmajor, int paired, const tdx_gemm_seg* seg0, const tdx_gemm_seg* seg1_or_null, int M, int N,
                 int n_valid, int pair_off, int batches, float* out_dev, long ldo, long strideO, int nreal, int* plan_or_null,
                 void* stream);
/* CONV = true, the implicit GEMM of the 3x3 (ntaps 9, zero padding 1) and 1x1 (ntaps 1) NHWC convolutions, set up as conv_gemm
 * (eres2net.hip, wespeaker.hip) and head_conv (campplus.hip) do: a [B*Hin*Win][lda], w [N][ntaps*cin] (tap-major), out row
 * m = (b, ho, wo) reads input row (b, ho*stride + dy, wo*(stride_w ? stride_w : stride) + dx).  out[m*ldo + n] for n < nreal.
 * Refused: ntaps outside {1, 9}, cin % 32, lda % 4, lda < cin, N % 128, nreal > n_valid, n_valid > N, a null pointer. */
int tdx_gemm_f32_conv(const float* a_dev, long lda, const float* w_dev, int B, int Hin, int Win, int Hout, int Wout, int stride,
                      int stride_w, int ntaps, int cin, int N, int n_valid, float* out_dev, long ldo, int nreal, int* plan_or_null,
                      void* stream);

/* the gated attention launch of a FLASH layer exactly as tdx_mf2_forward issues it (csrc/mf2_attention.hpp attention_core_h3 with the
 * planes-out gate): o = (att_u*v) * sigmoid(att_v*u) as row-major split-f16 planes oP [B*S][4E bytes] with one scale os and one sum of
 * squares oss per (128-channel segment, token): [E/128][B*S] floats each.  Inputs as tdx_cal_attention (four fp32 heads [B][S][128],
 * v, u [B][S][E], rotary freqs [16]); u is also the gate's fp32 u operand.  h3a: 1 = the half-height kernel (gemm_h3a.hpp), 0 = the
 * wide one (what TDX_H3A selects in the model); swap: the order of the two K segments on the half-height kernel (TDX_H3A_SWAP).
 * kvu_out [B][128][2E] gets the reduced lin_k^T [v|u].  E % 128 == 0. */
size_t tdx_attn_gate_planes_workspace_bytes(int B, int S, int E);
int tdx_attn_gate_planes(const float* quad_q, const float* lin_q, const float* quad_k, const float* lin_k, const float* v,
                         const float* u, const float* freqs, int B, int S, int E, int h3a, int swap, void* oP_dev, float* os_dev,
                         float* oss_dev, float* kvu_out_dev, void* workspace, size_t workspace_bytes, void* stream);

/* the host-built "window x DFT" GEMM operands (csrc/dft_basis.hpp fill_dft_analysis / fill_dft_synthesis) into a HOST buffer the caller
 * has zeroed; no device is touched: tests/test_dft_basis_host.py.  Analysis: out [rows][ld], re X_k in row k, im X_k in row im_row0 + k
 * (k < nbin), columns n < N, periodic Hann window if `hann`, else none.  Synthesis (c2r of the bins k < nbin): out [N][ld], re weights in
 * column k, im weights in column im_off + k; gain_kind 0: 1 / N, 1: hann[n] / 4, 2: hann[n] / N.  Refused: nbin > N / 2 + 1, im blocks that
 * overlap the re blocks or leave the buffer, ld < N (analysis). */
int tdx_diag_dft_analysis(int N, int nbin, long im_row0, long ld, long rows, int hann, float* out_host);
int tdx_diag_dft_synthesis(int N, int nbin, long im_off, long ld, int gain_kind, float* out_host);

/* the weight loader's pointer binding (csrc/tdx_common.hpp Loader::bind / resolve), on the host alone: tests/test_loaders.py.  Reads from
 * a TDXW blob the tensors plain [n], padded [n], twice [n], lin.weight [N][K], lin.bias [N] and, for l < L, layers.l.tap [C][k] and
 * layers.l.rows [N][K]; stages them through the binding forms (push, push with padding to npad, room + bind of 2 x twice, push_linear to
 * [Npad][Kp] with its two binds, push_tapmajor, push_rows_padded to Kp), runs the strict checks, resolves against a host copy of the image
 * and copies every staged tensor out through its bound pointer: plain [n] | padded [npad] | twice [n] | W [Npad][Kp] | b [Npad] | per layer
 * tap [k][C], rows [N][Kp] (out_floats must be exactly that).  *nonnull = the bound fields that are not null on return: 5 + 2 L on
 * success, 0 when a check fails (TDX_E_BLOB with the tensor's name in tdx_last_error). */
int tdx_diag_loader_bind(const void* blob, size_t blob_bytes, int n, int npad, int L, int C, int k, int N, int K, int Npad, int Kp,
                         float* out_host, size_t out_floats, int* nonnull);

/* per-CU operand fill rates (tools/fill_bench*.py) */
int tdx_fill_bench(int mode, const void* src_dev, long bytes_per_block, int blocks, int iters, float* sink_dev, void* stream);
int tdx_fill_bench2(int mode, const void* src_dev, int stride, int blocks, int iters, float* sink_dev, void* stream);
int tdx_fill_bench3(const void* src_dev, long pitch, int seg, long rows_per_block, int strips, int blocks, int iters,
                    float* sink_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TDX_TEST_H */
