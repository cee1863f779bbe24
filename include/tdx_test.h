/* tdx_test.h — exports of libtdx_diag.so: test hooks and timing diagnostics of the GEMM cores.
 *
 * NOT part of the product boundary (include/tdx.h / libtdx.so).  libtdx_diag.so is a separate library built
 * from csrc/diag.hip over the same kernel headers; tests/test_gpu_h3.py checks the numerics of the split-f16 x3
 * core through it, tests/test_gpu_h3_forms.py and tests/test_h3_tile_map.py its operand forms, producers and tile map,
 * tests/test_gpu_gemm_f32.py the operand modes and tile maps of the fp32 MFMA core,
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

/* the split-f16 x3 core (csrc/gemm_h3.hpp gemm_h3_kernel / launch_gemm_h3x) in every operand form the product issues, with a plain
 * store: tests/test_gpu_h3_forms.py.
 *   out[z*strideO + m*ldo + n] = sum over segments of sa[m] * sb[n] * sum over k of A'[z][m][k] * B'[z][n][k]      for n < nreal.
 * One K segment, field for field the H3Seg of gemm_h3.hpp (strides of the planes in BYTES, of the scales in floats): A row-major planes
 * (pitch lda); B row-major planes [N][..] (a weight) or, with b_kmajor, K-major planes [k][N/32][2][32] (ldb = pitch of a k row).  Batch
 * z = z1 * zdiv + z2 reads A + z1*strideA + z2*strideA2, sa + z1*strideSA + z2*strideSA2 (B, sb likewise).  kchunk > 0: batch z2 covers
 * min(K, ktotal - z2*kchunk) k.  segk > 0: one row scale per K segment of segk values, segment j's at sa + j*strideSeg.  a_shift /
 * a_period / a_zero: the token shift (operand row m - 1; a_zero, >= 4*K zero bytes, for m % a_period == 0). */
typedef struct tdx_h3_seg {
    const void* A;
    const void* B;
    const float* sa;
    const float* sb;
    long lda, ldb;
    long strideA, strideB, strideA2, strideB2;
    long strideSA, strideSB, strideSA2, strideSB2;
    int sa_mul, sb_mul;
    int K;
    int zdiv;
    int kchunk, ktotal;
    int segk;
    long strideSeg;
    int a_shift, a_period;
    const void* a_zero;
} tdx_h3_seg;
/* b_kmajor / paired / twoseg / a_conv pick the template instance <A_TR = false, B_TR, PAIRED, TWOSEG, ., 0, A_CONV>: <F,F,F,F>, <F,T,F,F>,
 * <F,F,T,F>, <F,F,F,T>, <F,T,T,T> and <F,F,F,F> with A_CONV; anything else is refused (K-major A stays with tdx_h3_gemm_x).  PAIRED: N pair
 * columns; column c pairs B column c with B column pair_off + c and stores them to out columns c and pair_off + c (c < nreal).  A_CONV
 * (implicit GEMM over NHWC pixel rows, M = B*Hout*Wout): K = ntaps*cin, tap (dy, dx) reads pixel (b, h*stride + dy, w*stride + dx) or
 * zero_row (>= 4*cin zero bytes) outside the image; taps_total > 0 splits the taps over `batches` = taps_total / ntaps slabs (the
 * caller sets strideB = 4*ntaps*cin).  The other forms ignore the A_CONV arguments.  plan_or_null (host, 6 ints) receives what
 * launch_gemm_h3x planned: map_mode, mp, gw, mc, tiles_m, tiles_n.
 * Refused (TDX_E_INVALID): a null pointer, M < 1, batches < 1, K % 16, K < 64 in a TWOSEG segment, N % 128 with a K-major B or PAIRED,
 * lda / ldb / operand strides % 16, a K-major ldb < 4*(pair_off + N), zdiv < 1, sa_mul / sb_mul outside {0, 1}, kchunk anywhere but
 * <F,T,F,F>, segk anywhere but <F,F,F,F> (where the product sets them), kchunk % 16, ktotal % 16, a z2 of the launch left without a k-tile, segk % 64, K % segk, K / segk > 8,
 * a_shift / a_period anywhere but the first segment of <F,F,F,T>, a_shift != -1, a_period without a_zero, and for A_CONV: cin < 64,
 * cin % 16, K != ntaps*cin, no zero_row, taps in all not 1 or 9, batches != taps_total / ntaps, M % (Hout*Wout).  The caller owns the
 * extents: every row the kernel can address after its clamps (rows < M, B rows < N or < pair_off + N, k rows < ktotal) must exist. */
int tdx_h3_gemm_ex(int b_kmajor, int paired, int twoseg, int a_conv, const tdx_h3_seg* seg0, const tdx_h3_seg* seg1_or_null, int M, int N,
                   int pair_off, int batches, int Hin, int Win, int Hout, int Wout, int stride, int ntaps, int cin, int taps_total,
                   const void* zero_row, float* out_dev, long ldo, long strideO, int nreal, int* plan_or_null, void* stream);
/* the fp32-A operand form of the x3 core (csrc/gemm_h3f.hpp): A = fp32 NHWC pixel rows a_dev [B*Hin*Win][lda floats] split WHILE STAGED with
 * the static scale a_mul, a power of two (xs = x * a_mul, hi = f16(xs), lo = f16(xs - hi); |x| * a_mul < 65504 is the caller's), *inv_dev = 1 / a_mul, B =
 * row-major weight planes [N][K] + row scales.  Output row m = (b, h, w) of [B, Hout, Wout] reads pixel (b, h*stride, w*stride):
 *   out[m*ldo + n] = inv * sb[n] * sum over k of A'[pix(m)][k] * B'[n][k]      for n < nreal,
 * bit-identical to tdx_h3_split_rows_static + tdx_h3_gemm_ex(a_conv = 1, ntaps = 1, sa_mul = 0) on the same data.  Refused: a null pointer,
 * K % 16, lda < K, lda % 4, M % (Hout*Wout), an output pixel that reads outside the image. */
int tdx_h3_gemm_f32a(const float* a_dev, long lda, float a_mul, const float* inv_dev, const void* pb, const float* sb, int M, int N, int K,
                     int Hin, int Win, int Hout, int Wout, int stride, float* out_dev, long ldo, int nreal, void* stream);
/* the plan of launch_gemm_h3x (plan_gemm_h3) and its block -> tile map (h3_tile_of_block) on the HOST, no device touched:
 * tests/test_h3_tile_map.py.  tdx_h3_plan: plan[6] as above and grid[2] = (gridDim.x, gridDim.y) for one launch of M x N (PAIRED: N pair
 * columns) over ktot = the sum of the segments' K.  tdx_h3_tile_of_block: 1 and (*z, *bm, *bn) if block (bx, by) of that launch
 * computes a tile, 0 if it returns at once, -1 on a bad argument. */
int tdx_h3_plan(int M, int N, int ktot, int batches, int paired, int* plan, int* grid);
int tdx_h3_tile_of_block(const int* plan, int batches, int bx, int by, int* z, int* bm, int* bn);
/* the split producers no other hook reaches.  static: row-major planes [R][Kp/8][2][8] (Kp = K rounded up to 16, tail zero) with the
 * caller's scale s.  long: rows of any length (K % 16 == 0; the product uses it beyond 2048), one power-of-two scale per row.
 * kmajor_ex: tdx_h3_split_kmajor with the exact scale (mx_dev / inv_dev given: the exponent-aligned scale of the float whose bits are
 * mx_dev[0], its inverse to inv_dev[0]; absmax != 0 first computes mx_dev[0] = max |x| over the source rows, which needs ld == N) and
 * with group padding (Sp > 0: k rows are [K/Sp][Sp], row (b, t) reads source row b*S + t, zero for t >= S). */
int tdx_h3_split_rows_static(const float* x_dev, long ld, void* planes_dev, long R, int K, float s, void* stream);
int tdx_h3_split_rows_long(const float* x_dev, long ld, void* planes_dev, float* scale_dev, long R, int K, void* stream);
int tdx_h3_split_kmajor_ex(const float* x_dev, long ld, void* planes_dev, long K, int N, float s, int absmax, unsigned* mx_dev,
                           float* inv_dev, int S, int Sp, void* stream);

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

/* the noise of Whisper's sampled decoding (csrc/whisper_noise.hpp) for the ids n0 .. n0 + count - 1 at context position
 * p of the row stream `row_stream` under `seed`: word_dev [count] the raw Philox4x32-10 words, g_dev [count] the Gumbel values the
 * vocabulary head adds.  tests/test_gpu_whisper_fallback.py.  Refused: a null pointer, n0 < 0, p < 0, count < 1. */
int tdx_test_whisper_noise(unsigned long long seed, unsigned long long row_stream, int p, int n0, int count, float* g_dev, unsigned* word_dev,
                           void* stream);

/* tdx_fft_c2c (csrc/fft.hpp) with a tile of 2^tile_log2 points, 4 <= tile_log2 <= 12, in place of TDX_FFT_TILE: the same kernels and
 * the same planner, so that the multi-pass plans occur at small sizes (tests/test_gpu_fft.py).  tdx_test_fft_passes: the passes of a
 * power-of-two transform of 2^m points under that tile (host only), 0 for arguments outside 0 <= m <= 27. */
size_t tdx_test_fft_workspace_bytes(long n, int batch, int tile_log2);
int tdx_test_fft_passes(int m, int tile_log2);
int tdx_test_fft_c2c(const float* x_dev, long n, int batch, int inverse, float* y_dev, void* ws, size_t ws_bytes, void* stream, int tile_log2);

/* per-CU operand fill rates (tools/fill_bench*.py) */
int tdx_fill_bench(int mode, const void* src_dev, long bytes_per_block, int blocks, int iters, float* sink_dev, void* stream);
int tdx_fill_bench2(int mode, const void* src_dev, int stride, int blocks, int iters, float* sink_dev, void* stream);
int tdx_fill_bench3(const void* src_dev, long pitch, int seg, long rows_per_block, int strips, int blocks, int iters,
                    float* sink_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TDX_TEST_H */
