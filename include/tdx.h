/* tdx.h — C-ABI of the MI355X-native TargetDiarization hot path (libtdx.so).
 *
 * The reference (ishine/TargetDiarization) is pure Python and has no FFI; its "plugin
 * boundary" for this path is four Python call sites.  Each entry point below replaces one
 * of them (reference file:line cited per function).  The Python host in
 * targetdiarization_amd/ binds these with ctypes (see INTEGRATION.md for the stub a
 * reference maintainer would add).
 *
 * Conventions
 *  - plain C types only; every pointer named *_dev is a DEVICE pointer owned by the caller
 *    (PyTorch-ROCm allocates; `tensor.data_ptr()`), every stream is a hipStream_t passed
 *    as void*.  The library owns only the opaque model handle (weights + tables).
 *  - every function returns 0 on success, non-zero TDX_E_* otherwise; no C++ exception
 *    crosses the boundary; tdx_last_error() returns a thread-local message.
 *  - all launches are asynchronous on the given stream; no hipMalloc/hipFree/sync inside
 *    a forward call (graph-capture safe).
 *  - threading: a handle is immutable after create (weights + tables); every *_forward /
 *    predict / decode call may be issued concurrently from several host threads on ONE handle
 *    provided each concurrent call has its OWN workspace and its OWN stream.  The only
 *    per-call state the library keeps is tdx_mf2's fork/join context (one side stream + three
 *    events PER CALLER STREAM, created on the first eager forward on that stream under an
 *    internal mutex; a forward on a stream that is being captured and has no context yet runs
 *    unforked: same results).  Two calls that share a workspace or a stream must be ordered
 *    by the caller (the Python host serialises per model object: _lib.HandleGuard).
 *    tdx_mf2_profile_* and tdx_mf2_enable_taps are single-caller diagnostics (profile slots
 *    are claimed under the same mutex; do not toggle them while forwards are in flight).
 */
#ifndef TDX_H
#define TDX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDX_OK 0
#define TDX_E_INVALID 1   /* bad argument / shape */
#define TDX_E_BLOB 2      /* weight blob malformed or tensor missing */
#define TDX_E_HIP 3       /* HIP runtime error */
#define TDX_E_WORKSPACE 4 /* workspace too small */

/* library version string, e.g. "tdx 0.1.0 gfx950" */
const char* tdx_version(void);
/* thread-local description of the last non-zero status returned on this thread */
const char* tdx_last_error(void);

/* ------------------------------------------------------------------------------------
 * H1  MossFormer2 separator — replaces `self.separater(audio_data_tensor)`
 *     AudioProcessor.py:943  (model: look2hear/models/mossformer2.py:563-589)
 *     loader replaces BaseModel.from_pretrain  base_model.py:52-64
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_mf2 tdx_mf2;

typedef struct tdx_mf2_config {
    int32_t num_blocks;   /* 24  (mossformer2.py:535) */
    int32_t channels;     /* 512 (in_channels == out_channels, :533-534); must be 512 */
    int32_t kernel_size;  /* 16  (:536), stride = kernel_size/2 */
    int32_t num_spks;     /* 2   (:538); must be 2 */
    int32_t group_size;   /* 256 (mossformer_block.py:434) */
    int32_t reserved[3];
} tdx_mf2_config;

/* weights_blob: host memory in the TDXW container (targetdiarization_amd/weights.py:pack_blob)
 * holding the reference's state_dict tensors under their reference names. */
int tdx_mf2_create(const tdx_mf2_config* cfg, const void* weights_blob, size_t blob_bytes,
                   int device, tdx_mf2** out);
int tdx_mf2_destroy(tdx_mf2* h);
/* bytes of device workspace tdx_mf2_forward needs for a [B,T] batch (0 on bad shape) */
size_t tdx_mf2_workspace_bytes(const tdx_mf2* h, int B, int T);
/* wav_dev [B,T] f32 -> out_dev [B,2,T] f32.  All B windows must have the same T (the
 * reference never pads a batch: mossformer_block.py:485 passes no mask). */
int tdx_mf2_forward(tdx_mf2* h, const float* wav_dev, int B, int T, float* out_dev,
                    void* workspace_dev, size_t workspace_bytes, void* stream);
/* algorithmic FLOPs (2*MAC) of one forward at [B,T] — SURVEY.md §8(d) accounting */
double tdx_mf2_flops(const tdx_mf2* h, int B, int T);

/* keep copies of the layer-0 intermediates and the mask for tdx_mf2_tap (costs workspace) */
int tdx_mf2_enable_taps(tdx_mf2* h, int on);

/* Live timing of the dominant kernel (the to_hidden+to_qk GEMM, one launch per block per
 * forward): after enable, each forward records a HIP event pair around that launch on the
 * forward's stream until max_records pairs are used; collect (after the caller synchronised
 * the stream) returns the summed elapsed ms and the number of launches, and re-arms. */
int tdx_mf2_profile_enable(tdx_mf2* h, int max_records);
int tdx_mf2_profile_collect(tdx_mf2* h, double* total_ms, int* launches);

/* test/diagnostic tap: copy a named intermediate of the LAST forward on (h, workspace)
 * into dst_dev (f32).  names: "enc","z","after_flash0","after_fsmn0","after_stack","mask".
 * Layouts are token-major ([B,S,C]; "mask" is [2,B,S,C]).  Returns element count via *n.
 * "headroom": [num_blocks][2] = the largest |f16| written under each layer's static plane scale for (v|u, lin_k) — the scales
 * are bounds derived from the weights (2^15 after scaling); 2^15 / value is the headroom the bound left (needs taps). */
int tdx_mf2_tap(tdx_mf2* h, const char* name, int B, int T, void* workspace_dev,
                float* dst_dev, size_t dst_elems, size_t* n, void* stream);

/* ------------------------------------------------------------------------------------
 * Stand-alone ops exported for parity tests of individual reference functions
 * ---------------------------------------------------------------------------------- */
/* FLASH_ShareA_FFConvM.cal_attention (mossformer_block.py:222-294), non-causal, no mask.
 * q/k inputs [B,S,128] are the four OffsetScale heads BEFORE rotary; v,u [B,S,E], E%64==0.
 * freqs_dev: 16 rotary frequencies.  att_v/att_u out [B,S,E]. */
int tdx_cal_attention(const float* quad_q_dev, const float* lin_q_dev, const float* quad_k_dev,
                      const float* lin_k_dev, const float* v_dev, const float* u_dev,
                      const float* freqs_dev, int B, int S, int E, float* att_v_dev,
                      float* att_u_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
size_t tdx_cal_attention_workspace_bytes(int B, int S, int E);

/* DilatedDenseNet.forward (fsmn.py:103-111) on token-major p[B,S,256] -> out[B,S,256].
 * w1[256,39], w2[256,2,39], in_g/in_b[2,256] (InstanceNorm affine), prelu[2,256]. */
int tdx_dilated_dense_net(const float* p_dev, int B, int S, const float* w1_dev,
                          const float* w2_dev, const float* in_g_dev, const float* in_b_dev,
                          const float* prelu_dev, float* out_dev, void* workspace_dev,
                          size_t workspace_bytes, void* stream);
size_t tdx_dilated_dense_net_workspace_bytes(int B, int S);

/* C[M,N] = A[M,K] * W[N,K]^T (+bias[N]); fp32 MFMA; N%128==0, K%32==0.  Test hook for the
 * GEMM core every nn.Linear / 1x1 Conv1d on the path goes through. */
int tdx_linear(const float* a_dev, const float* w_dev, const float* bias_dev, int M, int N, int K,
               float* c_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * a2  Kaldi fbank front-end ("mel frontend") — replaces torchaudio.compliance.kaldi.fbank as
 *     called inside modelscope's ERes2NetV2 pipeline (reached from TargetASR.py:161) and
 *     funasr's WavFrontend (reached from ASRProcessor.py:424).  [third-party algorithm]
 *     mode 0 = speaker front-end: povey window, input in [-1,1], per-utterance mean removed
 *     mode 1 = ASR front-end: hamming window, input x32768 (LFR/CMVN: tdx_lfr_cmvn)
 *     mode 2 = WeSpeaker front-end: mode 1's window and scale, mode 0's mean removal
 *     wav_dev [B,N] -> feat_dev [B,F,80], F = tdx_fbank_frames(N) = 1 + (N-400)/160.
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_fbank tdx_fbank;
int tdx_fbank_create(int mode, int device, tdx_fbank** out);
int tdx_fbank_destroy(tdx_fbank* h);
int tdx_fbank_frames(int N);
size_t tdx_fbank_workspace_bytes(int B, int N);
int tdx_fbank_forward(tdx_fbank* h, const float* wav_dev, int B, int N, float* feat_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream);
/* funasr WavFrontend.apply_lfr(m=7,n=6) + apply_cmvn: feat [B,F,80] -> out [B,ceil(F/6),560],
 * out = (stacked + shift[560]) * scale[560] */
int tdx_lfr_cmvn(const float* feat_dev, int B, int F, const float* shift_dev, const float* scale_dev,
                 float* out_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * a1  MDX block STFT / iSTFT — replaces ConvTDFNet.stft / .istft  AudioProcessor.py:82-120
 *     (torch.stft(n_fft, hop, hann periodic, center=True) on chunks of hop*(dim_t-1) samples,
 *     packed (L-re, L-im, R-re, R-im) x dim_f x dim_t; inverse zero-pads bins >= dim_f).
 *     x_dev [R, chunk] <-> spec_dev [R, 2, dim_f, dim_t], R = n_blocks * 2 channels.
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_stft tdx_stft;
int tdx_stft_create(int n_fft, int hop, int dim_f, int dim_t, int device, tdx_stft** out);
int tdx_stft_destroy(tdx_stft* h);
int tdx_stft_chunk_size(const tdx_stft* h);
size_t tdx_stft_workspace_bytes(const tdx_stft* h, int R);
int tdx_stft_forward(tdx_stft* h, const float* x_dev, int R, float* spec_dev, void* workspace_dev,
                     size_t workspace_bytes, void* stream);
int tdx_stft_inverse(tdx_stft* h, const float* spec_dev, int R, float* y_dev, void* workspace_dev,
                     size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * N3  MDX-Net denoiser body — replaces `self.mdx_model.run(None, {"input": mix_spec})[0]`  AudioProcessor.py:630
 *     (an onnxruntime session over UVR-MDX-NET-*.onnx, AudioProcessor.py:224-241: third-party; the network is KUIELab's
 *     ConvTDFNet / TFC-TDF v2: first 1x1 conv, n = num_blocks/2 encoder levels of [l x (3x3 conv + BN + ReLU) + TDF bottleneck
 *     Linear pair over frequency] with 2x2 stride-2 down convs, bottleneck block, n decoder levels with 2x2 transposed convs and
 *     multiplicative skips, final 1x1 conv).  blob: TDXW container with the PyTorch module names of that class (first_conv.*,
 *     encoding_blocks.{i}.tfc.H.{j}.*, encoding_blocks.{i}.tdf.*, ds.{i}.*, bottleneck_block.*, us.{i}.*, decoding_blocks.{i}.*,
 *     final_conv.*), BatchNorm2d in eval mode.  spec_dev [B,4,dim_f,dim_t] (tdx_stft_forward output) -> out_dev, same shape.
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_mdx tdx_mdx;
typedef struct tdx_mdx_config {
    int32_t num_blocks;   /* L = 11 (AudioProcessor.py:241) */
    int32_t l;            /* convolutions per TFC block (3) */
    int32_t g;            /* channel growth per level (32; multiple of 32) */
    int32_t k;            /* TFC kernel size; must be 3 */
    int32_t bn;           /* TDF bottleneck factor (8) */
    int32_t dim_f;        /* 3072 */
    int32_t dim_t;        /* frames per block: 256 (the reference passes dim_t = 8 meaning 2^8) */
    int32_t reserved;
} tdx_mdx_config;
int tdx_mdx_create(const tdx_mdx_config* cfg, const void* weights_blob, size_t blob_bytes, int device, tdx_mdx** out);
int tdx_mdx_destroy(tdx_mdx* h);
size_t tdx_mdx_workspace_bytes(const tdx_mdx* h, int B);
double tdx_mdx_flops(const tdx_mdx* h, int B);
int tdx_mdx_forward(tdx_mdx* h, const float* spec_dev, int B, float* out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * N3  CT-Transformer punctuation restorer — replaces the neural forward of `self.punc.inference(input=text)`
 *     ASRProcessor.punctuation_restore  ASRProcessor.py:880-897  (funasr CTTransformer.punc_forward: third-party):
 *     Embedding(vocab, 256) -> SANM encoder (num_blocks layers, d 256, 8 heads, FFN 1024, FSMN k = 11) -> Linear(256, npunc).
 *     blob: TDXW container with funasr's names (embed.weight, encoder.encoders0.0.*, encoder.encoders.{i}.*, encoder.after_norm.*,
 *     decoder.*).  ids_dev int32 [B,T] (T <= 1024) -> logits_dev [B,T,npunc].  lens_dev: null (every row has T tokens) or int32 [B]:
 *     row b holds lens[b] <= T tokens, the rest is padding — masked in the attention and zero in the FSMN memory, like funasr's
 *     padding mask, so that the valid positions equal the unbatched result (rows of many texts in one launch sequence); logits of
 *     padding positions are unspecified.  The mini-sentence windows, the sentence cache and the text assembly are host logic
 *     (targetdiarization_amd/punctuation.py).
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_punc tdx_punc;
int tdx_punc_create(int num_blocks, int vocab, int npunc, const void* weights_blob, size_t blob_bytes, int device, tdx_punc** out);
int tdx_punc_destroy(tdx_punc* h);
size_t tdx_punc_workspace_bytes(const tdx_punc* h, int B, int T);
int tdx_punc_forward(tdx_punc* h, const int* ids_dev, const int* lens_dev, int B, int T, float* logits_dev, void* workspace_dev, size_t workspace_bytes,
                     void* stream);

/* ------------------------------------------------------------------------------------
 * a12 Paraformer-large SANM encoder — replaces the encoder forward inside
 *     `self.asr['paraformer'].generate(input=wav, hotword=...)`  ASRProcessor.py:424
 *     (funasr SANMEncoder: third-party; 1+49 pre-LN layers, d=512, 4 heads, FSMN memory k=11).
 *     blob: TDXW container with funasr's names (encoder.encoders0.0.*, encoder.encoders.{i}.*,
 *     encoder.after_norm.*).  feats_dev [B,T,560] (tdx_lfr_cmvn output) -> out_dev [B,T,512].
 *     lens_host: NULL, or B lengths that must all equal T (callers bucket segments by length,
 *     as for the separator; no padding mask is implemented).
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_pfenc tdx_pfenc;
int tdx_pfenc_create(int num_blocks, const void* weights_blob, size_t blob_bytes, int device, tdx_pfenc** out);
int tdx_pfenc_destroy(tdx_pfenc* h);
size_t tdx_pfenc_workspace_bytes(const tdx_pfenc* h, int B, int T);
double tdx_pfenc_flops(const tdx_pfenc* h, int B, int T);
int tdx_pfenc_forward(tdx_pfenc* h, const float* feats_dev, const int* lens_host, int B, int T,
                      float* out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * N2  Paraformer CIF predictor + non-autoregressive SANM decoder — replaces the rest of
 *     `self.asr['paraformer'].generate(input=wav, hotword=...)` after the encoder  ASRProcessor.py:424
 *     (funasr CifPredictorV2 + ParaformerSANMDecoder: third-party; 16 layers FFN -> FSMN memory -> cross attention,
 *     one FFN-only layer, LayerNorm, vocabulary projection).  blob: TDXW container with funasr's names
 *     (predictor.cif_conv1d / cif_output, decoder.decoders.{i}.*, decoder.decoders3.0.*, decoder.after_norm,
 *     decoder.output_layer).  Two calls because the number of tokens is data dependent:
 *       predict: enc_dev [B,T,512] -> alphas_dev [B,T+1] (tail frame appended), emb_dev [B,T+1,512] (the fired frames
 *                first, zero beyond), counts_dev int32 [B] = floor(sum alphas), peaks_dev int32 [B,T+1] (frame of fire k, -1)
 *       decode : the first L rows of every utterance of emb_dev (L = max count, read back by the host), masked by
 *                counts_dev, with enc_dev as attention memory -> ids_dev int32 [B,L] (argmax), score_dev [B,L] (log-softmax
 *                at the argmax) or NULL.
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_pfdec tdx_pfdec;
int tdx_pfdec_create(int num_blocks, int vocab, const void* weights_blob, size_t blob_bytes, int device, tdx_pfdec** out);
int tdx_pfdec_destroy(tdx_pfdec* h);
size_t tdx_pfdec_predict_workspace_bytes(const tdx_pfdec* h, int B, int T);
int tdx_pfdec_predict(tdx_pfdec* h, const float* enc_dev, int B, int T, float* alphas_dev, float* emb_dev, int* counts_dev,
                      int* peaks_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
size_t tdx_pfdec_decode_workspace_bytes(const tdx_pfdec* h, int B, int L, int T);
int tdx_pfdec_decode(tdx_pfdec* h, const float* emb_dev, int emb_rows, const int* counts_dev, const float* enc_dev, int B, int L,
                     int T, int* ids_dev, float* score_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * N2t Paraformer's upsampling timestamp predictor — the second head of funasr's CifPredictorV3 (BiCifParaformer, the
 *     "paraformer-large-vad-punc" bundle behind ASRProcessor.py:424; third-party), on the tdx_pfdec handle.  OPTIONAL AS A SET:
 *     a blob with none of the head's 12 tensors (predictor.upsample_cnn.{weight,bias}, predictor.blstm.{weight_ih,weight_hh,
 *     bias_ih,bias_hh}_l0 and the same four with _reverse, predictor.cif_output2.{weight,bias}) creates the decoder as before
 *     (has_timestamps = 0); with some but not all of them tdx_pfdec_create fails with TDX_E_BLOB naming the first missing one.
 *       timestamps: enc_dev [B,T,512] (the encoder output itself), counts_dev int32 [B] (tdx_pfdec_predict), U = 3T ->
 *                   ConvTranspose1d(512,512,3,stride 3) -> BLSTM(512) -> a = relu(smooth_factor2 * sigmoid(Linear(1024,1)) -
 *                   noise_threshold2) (0.25 / 0.01; tdx_pfdec_set_alpha2) -> us_alphas_dev [B,U] = a * counts / sum(a) (a clip
 *                   whose sum is 0 stays unscaled) -> us_peaks_dev [B,U]: funasr's cif_wo_hidden with threshold 1 - 1e-4, the
 *                   running integral at every frame, walked sequentially in fp32.  tap_blstm_dev: NULL or [B,U,1024], the BLSTM
 *                   output.  On return the first B*U floats of the workspace hold the alphas before the re-normalisation.
 *                   On a handle without the head: TDX_E_INVALID.  The workspace is 6146 floats per upsampled frame (24 KB:
 *                   the projected LSTM input of both directions dominates).
 *       set_cif_residual: the main predictor branch is relu(conv(x) + bias + x) in CifPredictorV2 and relu(conv(x) + bias) in
 *                   V3 [upstream-recall]; create sets 1 without the head (as before) and 0 with it, this call overrides.
 * ---------------------------------------------------------------------------------- */
int tdx_pfdec_has_timestamps(const tdx_pfdec* h);
int tdx_pfdec_set_cif_residual(tdx_pfdec* h, int on);
int tdx_pfdec_set_alpha2(tdx_pfdec* h, float smooth_factor2, float noise_threshold2);
size_t tdx_pfdec_timestamps_workspace_bytes(const tdx_pfdec* h, int B, int T);
int tdx_pfdec_timestamps(tdx_pfdec* h, const float* enc_dev, int B, int T, const int* counts_dev, float* us_alphas_dev,
                         float* us_peaks_dev, float* tap_blstm_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * a10 ERes2NetV2-w24s4ep4 speaker embedding — replaces
 *     `self.embedding[embedding_model](wav_file, output_emb=True)['embs']`  TargetASR.py:161
 *     (modelscope / 3D-Speaker ERes2NetV2: third-party).  blob: TDXW container with the
 *     3D-Speaker module names (conv1, bn1, layer{1..4}.{i}.*, layer3_ds, fuse34, seg_1).
 *     feat_dev [B,F,80] = tdx_fbank mode-0 output (mean-normalised fbank) -> emb_dev [B,192].
 *     All B utterances share F (bucket by length); F >= 9.
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_eres2net tdx_eres2net;
int tdx_eres2net_create(const void* weights_blob, size_t blob_bytes, int device, tdx_eres2net** out);
int tdx_eres2net_destroy(tdx_eres2net* h);
size_t tdx_eres2net_workspace_bytes(const tdx_eres2net* h, int B, int F);
double tdx_eres2net_flops(const tdx_eres2net* h, int B, int F);
int tdx_eres2net_forward(tdx_eres2net* h, const float* feat_dev, int B, int F, float* emb_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * a11  cosine scoring — replaces TargetASR.cosine_similarity  TargetASR.py:144-152
 *      emb_dev [N,D] f32, ref_dev [D] f32 -> scores_dev [N] f32 (1.0 if either vector is
 *      all-zero, else cos clipped to [0,1]).
 * ---------------------------------------------------------------------------------- */
int tdx_cosine_scores(const float* emb_dev, const float* ref_dev, int N, int D, float* scores_dev,
                      void* stream);

/* ------------------------------------------------------------------------------------
 * N3   integrated loudness (ITU-R BS.1770-4) — replaces AudioProcessor.meter_loudness
 *      AudioProcessor.py:1123-1127 (pyloudnorm.Meter(rate).integrated_loudness, third-party) on
 *      device-resident clips: wav_dev [B,N] f32 mono -> lufs_dev [B] f64 (-inf for silence).
 *      N must cover one 400 ms gating block (the reference raises ValueError otherwise).
 * ---------------------------------------------------------------------------------- */
size_t tdx_loudness_workspace_bytes(int B, long N, int rate);
int tdx_loudness(const float* wav_dev, int B, long N, int rate, double* lufs_dev, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * N3   rational polyphase resampler — replaces AudioProcessor.audio_resample  AudioProcessor.py:549-569
 *      (librosa.resample, third-party; parity unpinned: the filter is the caller's — the Python host designs a
 *      Kaiser-windowed sinc like scipy.signal.resample_poly).  x_dev [C][n_in] -> y_dev [C][n_out],
 *      n_out = ceil(n_in*up/down); h_dev: 2*half+1 taps with DC gain `up`; the filter delay is removed.
 * ---------------------------------------------------------------------------------- */
int tdx_resample_poly(const float* x_dev, long n_in, int C, int up, int down, const float* h_dev, int half,
                      float* y_dev, long n_out, void* stream);

/* ------------------------------------------------------------------------------------
 * N3   Apollo band-split RoFormer restorer — replaces `self.restorer(audio_data_tensor)` in
 *      AudioProcessor.restore_audio  AudioProcessor.py:959-980 (look2hear/models/apollo.py with
 *      sr=44100, win=20, feature_dim=256, layer=num_layers; num_layers >= 1, the reference ships 6).
 *      blob: TDXW container with the reference's state-dict names (BN.*, net.{l}.*, output.*, the rotary
 *      buffers cos_freq / sin_freq included); names AND shapes are checked both ways (strict load),
 *      any mismatch is TDX_E_BLOB before device work.
 *      x_dev: nclips clips at 44.1 kHz, concatenated (clip c at sample offset lens[0] + ... + lens[c-1]);
 *      y_dev: same layout.  lens_host: nclips lengths, each >= 442 (the reflect pad of the STFT needs it).
 *      items_host: NULL (one item per clip: the whole clip, nitems = nclips) or nitems x 5 int32
 *      {clip, frame_lo, frame_hi, sample_lo, sample_hi}: the item runs the net on frames [frame_lo, frame_hi)
 *      of the clip (T = 1 + n / 441 frames, frame t centred on sample 441 t) and writes y over samples
 *      [sample_lo, sample_hi) only.  The net is local in time (receptive field +-54 frames): a frame within 54
 *      of a window edge that is not a clip edge is inexact, and an item whose samples read such a frame is
 *      TDX_E_INVALID.  1 <= nitems <= 64; frames of the call = sum over items of (frame_hi - frame_lo).
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_apollo tdx_apollo;
int tdx_apollo_create(int num_layers, const void* weights_blob, size_t blob_bytes, int device, tdx_apollo** out);
int tdx_apollo_destroy(tdx_apollo* h);
size_t tdx_apollo_workspace_bytes(const tdx_apollo* h, int frames);
double tdx_apollo_flops(const tdx_apollo* h, int frames);
int tdx_apollo_forward(tdx_apollo* h, const float* x_dev, const int64_t* lens_host, int nclips, const int32_t* items_host, int nitems,
                       float* y_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * N4   CAM++ speaker-embedding extractor (3D-Speaker speakerlab/models/campplus: FCM head + D-TDNN with
 *      context-aware masking, 192-d) — the embedding model of modelscope's
 *      speech_campplus_speaker-diarization_common pipeline (TargetDiarization.py:73) and
 *      `self.embedding['campp']` (TargetASR.py:109).
 *      blob: TDXW container with 3D-Speaker's state-dict names (head.*, xvector.*; num_batches_tracked
 *      dropped); strict both ways: a missing and an unexpected tensor are TDX_E_BLOB with the name in
 *      tdx_last_error().  BatchNorm is eval-mode (eps 1e-5) and folded where a convolution precedes it.
 *      feat_dev [B,F,80] = tdx_fbank mode-0 output (mean-normalised fbank) -> emb_dev [B,192].
 *      All B utterances share F; F >= 9 (workspace_bytes returns 0 below that).
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_campp tdx_campp;
int tdx_campp_create(const void* weights_blob, size_t blob_bytes, int device, tdx_campp** out);
int tdx_campp_destroy(tdx_campp* h);
size_t tdx_campp_workspace_bytes(const tdx_campp* h, int B, int F);
double tdx_campp_flops(const tdx_campp* h, int B, int F);
int tdx_campp_forward(tdx_campp* h, const float* feat_dev, int B, int F, float* emb_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * N5   FSMN-VAD frame posteriors — replaces `self.vad.generate(input=audio_data, cache={})` in
 *      ASRProcessor.vad_detection  ASRProcessor.py:742-817 (funasr fsmn_vad_streaming, third-party; parity
 *      unpinned [upstream-recall]: WavFrontend LFR 5/1 + CMVN, in_linear1/2, four FSMN blocks with a causal
 *      20-tap depthwise memory, out_linear1/2, softmax over 248).  The segmenter that turns posteriors into
 *      [start_ms, end_ms] ranges runs on the host (targetdiarization_amd/vad.py).
 *      blob: TDXW container with funasr's state-dict names under "encoder." plus "cmvn.shift"[400] and
 *      "cmvn.scale"[400] (the <AddShift> / <Rescale> vectors of am.mvn); strict both ways: a missing and an
 *      unexpected tensor are TDX_E_BLOB with the name in tdx_last_error(), before any device work.
 *      feat_dev [rows,80] = tdx_fbank mode-1 frames of nclips clips packed back to back; starts_dev int32
 *      [nclips+1] on the DEVICE, ascending, starts[0] = 0, starts[nclips] = rows: clip c owns rows
 *      [starts[c], starts[c+1]) (an empty clip is legal, a clip of one frame too).  LFR edge replication and the
 *      zero history of the FSMN memory are per clip: no value crosses a clip boundary.
 *      p0_dev [rows]: posterior of class 0 (the only silence class); post_dev: NULL or [rows,248].
 *      1 <= rows <= 2^22 (workspace_bytes returns 0 outside).  16 launches per call whatever nclips.
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_fsmnvad tdx_fsmnvad;
int tdx_fsmnvad_create(const void* weights_blob, size_t blob_bytes, int device, tdx_fsmnvad** out);
int tdx_fsmnvad_destroy(tdx_fsmnvad* h);
size_t tdx_fsmnvad_workspace_bytes(const tdx_fsmnvad* h, int rows);
double tdx_fsmnvad_flops(const tdx_fsmnvad* h, int rows);
int tdx_fsmnvad_forward(tdx_fsmnvad* h, const float* feat_dev, const int32_t* starts_dev, int nclips, int rows,
                        float* p0_dev, float* post_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * N6   PyanNet speaker segmentation — the network inside `self.od_pipeline` (pyannote speaker-diarization-3.1,
 *      TargetDiarization.py:84,132,143; pyannote segmentation-3.0, third-party; parity unpinned [upstream-recall]):
 *      InstanceNorm1d(1) on the waveform, SincNet (80 sinc filters of 251 taps at stride 10, two k5 convolutions, each
 *      stage abs/-, MaxPool3, InstanceNorm1d, leaky_relu), a 4-layer bidirectional LSTM of 128 units, linears 256->128->128
 *      with leaky_relu, a 7-class classifier and log-softmax.  The classes are the powerset of at most 2 of 3 local
 *      speakers: {}, {0}, {1}, {2}, {0,1}, {0,2}, {1,2}.  Chunking, clustering and track building run on the host
 *      (targetdiarization_amd/overlap.py).
 *      blob: TDXW container with pyannote's state-dict names (sincnet.*, lstm.*, linear.*, classifier.*; without the
 *      derived filterbank.n_ / window_ buffers); strict both ways like the other models.
 *      wav_dev [B,T]: 16 kHz chunks, 1261 <= T <= 160000 and 1 <= B <= 1024 (frames / workspace_bytes return 0 outside);
 *      logp_dev [B,F,7] with F = tdx_pyannet_frames(T) (one frame per 270 samples, receptive field 991);
 *      tap_sincnet [B,F,60] and tap_lstm [B,F,256] are NULL or receive the SincNet and the LSTM output.
 *      A chunk's result does not depend on the other chunks of the batch.  22 launches per call whatever B and T;
 *      the recurrence is one launch per LSTM layer.
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_pyannet tdx_pyannet;
int tdx_pyannet_create(const void* weights_blob, size_t blob_bytes, int device, tdx_pyannet** out);
int tdx_pyannet_destroy(tdx_pyannet* h);
int tdx_pyannet_frames(int T);
int tdx_pyannet_chunk_tile(void);      /* chunks one workgroup of the recurrence kernel walks (a launch has ceil(B / tile) x 2 workgroups) */
size_t tdx_pyannet_workspace_bytes(const tdx_pyannet* h, int B, int T);
double tdx_pyannet_flops(const tdx_pyannet* h, int B, int T);
int tdx_pyannet_forward(tdx_pyannet* h, const float* wav_dev, int B, int T, float* logp_dev, float* tap_sincnet,
                        float* tap_lstm, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * N7   silero-VAD per-chunk speech probabilities — the network inside `get_speech_timestamps(audio, self.vad_model)`
 *      (TargetDiarizationStream.py:128-131, AudioProcessor.py:903-905; silero-vad v5, 16 kHz branch, third-party; parity
 *      unpinned [upstream-recall]).  Per 512-sample chunk: a 640-sample window (64 samples of context, zeros at a clip's
 *      first chunk; the chunk; 64 samples of right reflect pad of the chunk's own tail), 4 frames of 256 at hop 128 against
 *      the stored STFT basis -> magnitudes [129,4], four Conv1d(k=3, pad=1) + ReLU with strides 1, 2, 2, 1
 *      ([129,4] -> [128,4] -> [64,2] -> [64,1] -> [128,1], zero padding per chunk), LSTMCell(128,128) with (h, c) zero at
 *      the clip's first chunk and carried chunk to chunk, p = sigmoid(w . relu(h) + b).  The state machine that turns
 *      probabilities into timestamps runs on the host (targetdiarization_amd/silero.py).
 *      blob: TDXW container with the 16 kHz branch's state-dict names without the `_model.` prefix
 *      (stft.forward_basis_buffer, encoder.{0..3}.reparam_conv.*, decoder.rnn.*, decoder.decoder.2.*); strict both ways
 *      like the other models.
 *      wav_dev [total_chunks*512]: the clips packed back to back, each already zero-padded to whole chunks;
 *      chunk_starts_dev int32 [nclips+1] on the DEVICE, strictly ascending, starts[0] = 0, starts[nclips] = total_chunks:
 *      clip c owns chunks [starts[c], starts[c+1]).  prob_dev [total_chunks]; tap_feat / tap_h: NULL or [total_chunks,128],
 *      the encoder output and the LSTM h.  1 <= nclips <= 1024, every clip >= 1 chunk, total_chunks <= 2^20
 *      (workspace_bytes returns 0 outside, forward TDX_E_INVALID).  A clip's result does not depend on the other clips of
 *      the batch.  9 launches per call whatever nclips and total_chunks; the recurrence is one launch, one workgroup per clip.
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_silero tdx_silero;
int tdx_silero_create(const void* weights_blob, size_t blob_bytes, int device, tdx_silero** out);
int tdx_silero_destroy(tdx_silero* h);
size_t tdx_silero_workspace_bytes(const tdx_silero* h, int nclips, int total_chunks);
double tdx_silero_flops(const tdx_silero* h, int total_chunks);
int tdx_silero_forward(tdx_silero* h, const float* wav_dev, const int* chunk_starts_dev, int nclips, int total_chunks,
                       float* prob_dev, float* tap_feat, float* tap_h, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * N8   WeSpeaker ResNet34 with masked statistics pooling — the embedding inside `self.od_pipeline` (pyannote
 *      speaker-diarization-3.1's `pyannote/wespeaker-voxceleb-resnet34-LM`, TargetDiarization.py:84; wespeaker ResNet34 with
 *      m_channels 32, feat_dim 80, embed_dim 256, TSTP, one embedding layer; third-party, parity unpinned [upstream-recall]):
 *      conv3x3(1->32) + BN + ReLU, BasicBlock stages of 3/4/6/3 blocks at 32/64/128/256 channels (the first block of stages
 *      2-4 with stride 2 and a conv1x1 + BN shortcut), pyannote's StatsPool over time under a per-frame weight, Linear
 *      5120 -> 256.  Eval BatchNorm (eps 1e-5) is folded into the convolution in front of it.
 *      blob: TDXW container with upstream's state-dict names (resnet.conv1.weight, resnet.bn1.*, resnet.layerL.i.*,
 *      resnet.seg_1.*; num_batches_tracked dropped); strict both ways like the other models, before any device work.
 *      feat_dev [B,F,80] = tdx_fbank mode-2 output.  weights_dev [B,S,Fw]: S per-frame masks of every chunk on any frame
 *      grid (resampled to the trunk's T' = ceil(F/8) frames by nearest neighbour, w'[i] = w[(i*Fw)/T']), or NULL with S = 1
 *      for all ones (plain TSTP, unbiased std).  The trunk runs once per chunk and is pooled under each mask:
 *        v1 = sum w', v2 = sum w'^2, mean = sum w' x / v1, std = sqrt(sum w' (x-mean)^2 / (v1 - v2/v1 + 1e-8))
 *      emb_dev [B,S,256]; a row whose resampled weights sum to zero is NaN throughout, as upstream's 0/0 is.
 *      1 <= B <= 64, F >= 1, B*F*2560 < 2^31, 1 <= S <= 8, Fw >= 1 (workspace_bytes returns 0 outside, forward
 *      TDX_E_INVALID).  A (b, s) result does not depend on the other chunks or masks of the call.  All launches go on the
 *      caller's stream: no atomics, no memset, no allocation.  TDX_WESPK_NARROW in the environment of tdx_wespk_create
 *      picks the kernel of the 13 stride-1 3x3 convolutions of the 32- and 64-channel stages (a property of the handle):
 *      1 = conv3x3_narrow_kernel, 0 = the shared GEMM core; unset = the faster of the two as measured.
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_wespk tdx_wespk;
int tdx_wespk_create(const void* weights_blob, size_t blob_bytes, int device, tdx_wespk** out);
int tdx_wespk_destroy(tdx_wespk* h);
size_t tdx_wespk_workspace_bytes(const tdx_wespk* h, int B, int F, int S);
int tdx_wespk_forward(tdx_wespk* h, const float* feat_dev, int B, int F, const float* weights_dev, int S, int Fw,
                      float* emb_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * N9   SenseVoiceSmall — replaces `self.asr['sensevoice'].generate(input=wav, language=..., use_itn=True)`
 *      ASRProcessor.py:398-402 (funasr SenseVoiceSmall: third-party, absent; parity unpinned [upstream-recall], LayerNorm eps
 *      1e-12, the prompt order and the id tables included).  Rows per utterance: [embed[lid], embed[1], embed[2], embed[textnorm],
 *      feats(0..T-1)], S = T + 4; x sqrt(512) + sinusoidal positions 1..S; encoders0 + (num_blocks - 1) encoders (the SANM layer
 *      of tdx_pfenc: d 512, 4 heads, FSMN memory k = 11, FFN 2048), after_norm, tp_blocks tp_encoders, tp_norm; CTC head
 *      log_softmax(Linear(512, vocab)) with blank = 0 and a greedy decode over all S frames (the four prompt frames yield the
 *      language / emotion / event / text-norm tags).
 *      blob: TDXW container with funasr's names (embed.weight [16,560], encoder.encoders0.0.*, encoder.encoders.{i}.*,
 *      encoder.after_norm.*, encoder.tp_encoders.{i}.*, encoder.tp_norm.*, ctc.ctc_lo.weight [vocab,512], ctc.ctc_lo.bias); a
 *      missing tensor is TDX_E_BLOB with its name in tdx_last_error(); other tensors of the checkpoint are ignored.
 *      feats_dev [B,T,560] = tdx_lfr_cmvn output; the utterances of a call share T (callers bucket by length; no padding mask).
 *      prompt_host: 4 ids in [0,16) = {lid, 1, 2, textnorm}, read during the call (not kept).
 *      enc_dev: NULL or [B,S,512], the tp_norm output.  frame_ids_dev int32 [B,S] = argmax per frame (ties: the lowest id),
 *      frame_score_dev [B,S] = log-softmax at the argmax.  tok_ids_dev / tok_frames_dev int32 [B,S], counts_dev int32 [B]: the
 *      collapse below of frame_ids_dev with blank 0.  B * S < 2^22 (workspace_bytes returns 0 outside).
 *      The head never stores the logits of a whole call; TDX_SV_HEAD in the environment of tdx_sv_create picks how (a property
 *      of the handle): 1 = the fused kernel (64 rows staged in LDS, exact-fp32 MFMA sweep over 512-column vocabulary slices, one
 *      (max, argmax, sum exp) triple per row and slice, merged by a second kernel: 12 * ceil(vocab / 512) workspace bytes per
 *      row); 0 = chunks of TDX_SV_LOGITS_ROWS rows through the split-f16 x3 Linear into ONE logits buffer of that many rows, then
 *      a row kernel; unset = the default as measured.  All launches go on the caller's stream, no host wait.
 *
 *      tdx_ctc_collapse: frame_ids_dev int32 [B,S] -> per utterance the ids left after dropping every frame whose id equals the
 *      previous frame's and then every `blank`, compacted at the front of tok_ids_dev [B,S] (the rest `blank`), the first frame
 *      of each kept run in tok_frames_dev [B,S] (the rest -1), their number in counts_dev [B].  Runs never merge across
 *      utterances.  One launch, no host wait.
 * ---------------------------------------------------------------------------------- */
#define TDX_SV_LOGITS_ROWS 1024      /* cap of the TDX_SV_HEAD=0 logits buffer, in rows of up(vocab, 256) floats */
typedef struct tdx_sv tdx_sv;
int tdx_sv_create(int num_blocks, int tp_blocks, int vocab, const void* weights_blob, size_t blob_bytes, int device, tdx_sv** out);
int tdx_sv_destroy(tdx_sv* h);
size_t tdx_sv_workspace_bytes(const tdx_sv* h, int B, int T);
double tdx_sv_flops(const tdx_sv* h, int B, int T);
int tdx_sv_forward(tdx_sv* h, const float* feats_dev, int B, int T, const int* prompt_host, float* enc_dev, int* frame_ids_dev,
                   float* frame_score_dev, int* tok_ids_dev, int* tok_frames_dev, int* counts_dev, void* workspace_dev,
                   size_t workspace_bytes, void* stream);
int tdx_ctc_collapse(const int* frame_ids_dev, int B, int S, int blank, int* tok_ids_dev, int* tok_frames_dev, int* counts_dev,
                     void* stream);

/* ------------------------------------------------------------------------------------
 * N10  Whisper — replaces `AutoModelForSpeechSeq2Seq.from_pretrained(dir)` + `generate(input_features, task="transcribe",
 *      language="chinese", num_beams=1, prompt_ids=...)` (ASRProcessor.py:244-251, 489-514; Hugging Face transformers'
 *      WhisperForConditionalGeneration, pinned by tests/test_whisper_host.py).  fp32 throughout (the reference runs .half()),
 *      greedy decoding, one prefix per call or, in tdx_whisper_decode_ts, one per row; sampled decoding
 *      in tdx_whisper_decode_ts_sample.  No beam search.
 *      create enforces, each with its own message: d_model / heads == 64 (encoder and decoder), gelu != 0 (activation_function
 *      "gelu", the exact erf form), n_mels 80 or 128, 1 <= n_audio_ctx, n_text_ctx <= 32768, vocab >= 2, layers >= 1, the FFN
 *      widths positive multiples of 64.
 *      blob: TDXW container with transformers' names (model.encoder.*, model.decoder.*; proj_out.weight optional and then equal
 *      to model.decoder.embed_tokens.weight); strict both ways, by shape, before any device work.
 *      1 <= B <= 32 in every call (workspace_bytes returns 0 outside); one workspace size serves the three entry points
 *      (tdx_whisper_decode_ts_sample asks for tdx_whisper_decode_sample_workspace_bytes).
 *
 *      tdx_whisper_logmel: WhisperFeatureExtractor.  wav_dev [B,N] 16 kHz in [-1,1]; lens_dev NULL or int32 [B] on the DEVICE,
 *      the valid samples of each row (clamped to [0,N]).  Each clip is cut or zero-padded to 320 * n_audio_ctx samples, reflect-
 *      padded by 200, framed (periodic Hann 400, hop 160, the last frame dropped), power spectrum, Slaney mel bank, log10 of
 *      max(., 1e-10), clamped at the clip's own maximum - 8, (x + 4) / 4.  feat_dev [B, n_mels, 2 * n_audio_ctx].
 *      tdx_whisper_encode: feat_dev -> enc_dev (NULL or [B, n_audio_ctx, d_model], the encoder's final LayerNorm output) and
 *      enc_state_dev (NULL or [dec_layers][2][B][n_audio_ctx][d_model]: the cross-attention K and V of every decoder layer).
 *      tdx_whisper_decode: greedy decoding of B clips from enc_state_dev.  prefix_host: prefix_len >= 1 ids common to the clips,
 *      fed one per step through the same kernels as generated tokens (no batched prefill).  Step p reads the token at position p;
 *      step_ids_dev / step_scores_dev [B, n_text_ctx] receive at [b][p] the argmax over the unsuppressed vocabulary (ties: the
 *      lowest id) and its log-softmax; positions no step reached are left untouched.  suppress_host ids are masked at every
 *      step, begin_suppress_host ids at step prefix_len - 1 only.  min(max_new, n_text_ctx - prefix_len) tokens are generated
 *      at most (positions prefix_len ...); counts_dev [B] = tokens generated per clip, a final `eos` included; with max_new = 0
 *      the prefix is scored whole and nothing is generated.  A clip that emitted eos stops writing and does not disturb the
 *      others; a clip's results do not depend on the other clips of its batch (the Linear is one kernel for B <= 8 and another from
 *      9 rows on: across that line they agree to fp32 rounding).  The [B, vocab] logits are never stored.  Arguments
 *      are validated before the device is touched.  The call enqueues 16 steps at a time and then waits for one pinned word,
 *      the number of finished clips: it returns after the stream has drained and cannot be captured into a graph.
 *      tdx_whisper_decode_xattn: tdx_whisper_decode plus the cross-attention of the alignment heads (word timestamps).
 *      heads_host int32 [nh][2]: (decoder layer, head) pairs, 1 <= nh <= 64; xattn_dev float [B][nh][max_rows][n_audio_ctx].
 *      When step p feeds the token at position p and first_row <= p < first_row + max_rows, row p - first_row of every listed
 *      head receives that step's softmax probabilities over the n_audio_ctx encoder positions (a full softmax in one workgroup,
 *      recomputed from q and the layer's cross K: the decode's own attention kernels are not involved).  A clip that has finished
 *      receives no more rows; rows no step reached are left untouched.  step_ids_dev, step_scores_dev and counts_dev are
 *      bit-identical to tdx_whisper_decode's on the same inputs.  Rejected before any device call, each with its own message: nh
 *      outside [1, 64], max_rows < 1, first_row < 0, a NULL heads_host / xattn_dev, a (layer, head) pair outside the decoder.
 *
 *      Long-form transcription with timestamp tokens (whisper.transcribe / transformers' long-form generate):
 *      tdx_whisper_logmel_long: WhisperFeatureExtractor with truncation=False on ONE clip of N samples (1 <= N <= 2^30) on the
 *      device: no cut or pad to 320 * n_audio_ctx samples, F = N / 160 frames, and the clamp at maximum - 8 is taken over the whole
 *      clip.  feat_dev [n_mels, F].  N < 160: no frame, nothing is written.  The reflect padding mirrors as often as a short clip
 *      needs (numpy's "reflect").  The frames go through the same window x DFT and mel GEMMs in blocks of 4096, so the workspace
 *      (tdx_whisper_logmel_long_workspace_bytes; 0 for a bad argument) does not grow with N beyond one block.
 *      tdx_whisper_decode_ts: tdx_whisper_decode with per-row prefixes, Whisper's timestamp rules, the no-speech probability and
 *      an optional capture of the alignment heads.  prefix_host [B][max_prefix], prefix_len_host [B] (1 <= len <= max_prefix, len
 *      < n_text_ctx): row b feeds its own prefix one id per step and then generates at most min(max_new_host[b], n_text_ctx -
 *      prefix_len[b]) ids from position prefix_len[b]; outputs at [b][p] as in tdx_whisper_decode.  begin_host NULL or [B], 1 <=
 *      begin[b] <= prefix_len[b] (NULL: prefix_len): the ids of row b from position begin[b] on are its history `seq` (transformers'
 *      begin_index); with begin < prefix_len the tail of the prefix counts as already generated.  Per step, after the static
 *      suppress / begin_suppress masks (begin_suppress at the step that predicts position begin[b]), with tb = no_timestamps_id + 1:
 *      no_timestamps_id is denied; seq ends in a timestamp and the id before it is one too (or len(seq) < 2): every id >= tb is
 *      denied; seq ends in a timestamp after a text id: every id < eos is denied; seq holds a timestamp: ids in [tb, last) are
 *      denied, last = the last timestamp if seq ends in a timestamp that follows a text id, else that id + 1; at the step that
 *      predicts position begin[b]: every id < tb is denied, and every id > tb + max_initial_timestamp_index when that is >= 0;
 *      then, over what is still allowed, if the log-sum-exp of the logits >= tb exceeds (strictly) the largest logit < tb, every
 *      id < tb is denied.  The result is the argmax of what remains (ties: the lowest id) and its log-softmax over what remains
 *      (WhisperTimeStampLogitsProcessor applied last, as _retrieve_logit_processors orders it).  A max_initial_timestamp_index past
 *      the last timestamp id is clamped to it (negative: no limit).  If the masks and the rules leave no id at all (a suppress list
 *      that covers a whole class, say), the row emits eos with score +inf, as tdx_whisper_decode does.  Steps that predict a position
 *      below begin[b] score the prefix under an empty history.  The head keeps two running (max, argmax, sum exp) triples per row
 *      and 64-column slice, one per class of ids; the [B, vocab] logits are never stored.  nospeech_dev NULL or float [B]: the
 *      softmax probability of no_speech_id over the whole vocabulary, no mask, at the step that feeds position sot_pos_host[b]
 *      (the row's <|startoftranscript|>).  heads_host NULL (no capture) or as in tdx_whisper_decode_xattn, with first_row_host NULL
 *      or [B] (NULL: prefix_len[b]).  A row's results do not depend on the other rows of its batch.  Rejected before the device
 *      is touched, each with its own message: a prefix that leaves no room (prefix_len >= n_text_ctx), tb outside the vocabulary,
 *      eos >= tb, sot_pos outside the prefix, begin outside [1, prefix_len], a negative max_new or first_row, and
 *      tdx_whisper_decode_xattn's capture checks.  tdx_whisper_decode and tdx_whisper_decode_xattn are unchanged: the three share
 *      the decoder-layer launches, and each has its own head and step kernels.
 *      tdx_whisper_decode_ts_sample: tdx_whisper_decode_ts with a draw from softmax(logits / T) per row (whisper.transcribe's
 *      temperature fallback).  temperature_host float [B] (0: the row decodes greedily and gives tdx_whisper_decode_ts's
 *      bits; all 0: the call launches tdx_whisper_decode_ts's kernels), stream_host uint64 [B] (a row's own noise stream), seed.  The draw is the Gumbel-max trick inside the head, so the
 *      logits are still never stored: id n at context position p gets g = -logf(-logf(u)), u = ((w >> 9) + 0.5) 2^-23, w = word
 *      n & 3 of Philox4x32-10 under the key (seed & 0xffffffff, seed >> 32) and the counter (n >> 2, p, stream & 0xffffffff,
 *      stream >> 32); the head keeps, per class, the largest z = v / T + g over the ids the rules admit (ties: the lowest id).
 *      The mass rule is decided on the untempered logits as in tdx_whisper_decode_ts; if the timestamps win the id is the timestamp
 *      class's winner, otherwise the larger z of the two classes; the score is the id's untempered log-softmax over the allowed set.
 *      A row's results depend on (seed, stream, its inputs) alone.  The workspace is tdx_whisper_decode_sample_workspace_bytes(h, B):
 *      the common workspace (tdx_whisper_workspace_bytes, unchanged) with the rows' records behind it; 0 for a bad argument.
 *      Rejected, each with its own message: a NULL temperature_host or stream_host, a temperature that is negative, NaN or
 *      infinite (the row is named), and everything tdx_whisper_decode_ts rejects.
 *
 *      tdx_token_align: token times from those rows, as transformers' _extract_token_timestamps (no model handle; the current
 *      device).  xattn_dev [B][nh][max_rows][n_audio_ctx]; per clip on the DEVICE nrows_dev[b] (0 .. max_rows, clamped) and
 *      nframes_dev[b] (1 .. n_audio_ctx, clamped).  Over W[h][i][j], i < nrows, j < nframes: mean and population standard deviation
 *      over i for each (h, j) (two passes, fp64 sums), z = (W - mean) / std, the median of median_width (odd, 1 .. 31; the product
 *      passes 7) along j with reflect padding (skipped when nframes <= median_width / 2), the mean over the heads -> M[i][j]
 *      (matrix_dev, NULL or [B][max_rows][n_audio_ctx]), then dynamic time warping on -M exactly as _dynamic_time_warping: fp32
 *      cost, cost[i][j] = -M[i-1][j-1] + min as one fp32 addition, strict comparisons with ties going left, upstream's borders,
 *      the backtrace from the last cell.  frames_dev int32 [B][max_rows]: at [b][i] the frame at which the path first enters
 *      token row i (upstream's time_indices[jumps]); entries i >= nrows are left untouched.  nrows 0: nothing is written;
 *      nrows 1: frame 0 (matrix_dev untouched); a column whose std is 0 contributes 0 (upstream: NaN).  1 <= max_rows <= 2048,
 *      1 <= nh <= 64, 1 <= B <= 65535; every violation has its own message.  One workgroup per clip walks the anti-diagonals.
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_whisper_config {
    int32_t n_mels, n_audio_ctx, d_model, enc_heads, enc_layers, enc_ffn;
    int32_t n_text_ctx, dec_heads, dec_layers, dec_ffn, vocab, gelu;
    int32_t reserved[4];
} tdx_whisper_config;
typedef struct tdx_whisper tdx_whisper;
int tdx_whisper_create(const tdx_whisper_config* cfg, const void* weights_blob, size_t blob_bytes, int device, tdx_whisper** out);
int tdx_whisper_destroy(tdx_whisper* h);
size_t tdx_whisper_workspace_bytes(const tdx_whisper* h, int B);
double tdx_whisper_flops(const tdx_whisper* h, int B, int steps);
int tdx_whisper_logmel(tdx_whisper* h, const float* wav_dev, const int* lens_dev, int B, long N, float* feat_dev, void* workspace_dev,
                       size_t workspace_bytes, void* stream);
int tdx_whisper_encode(tdx_whisper* h, const float* feat_dev, int B, float* enc_dev, float* enc_state_dev, void* workspace_dev,
                       size_t workspace_bytes, void* stream);
int tdx_whisper_decode(tdx_whisper* h, const float* enc_state_dev, int B, const int* prefix_host, int prefix_len, const int* suppress_host,
                       int n_suppress, const int* begin_suppress_host, int n_begin, int eos, int max_new, int* step_ids_dev,
                       float* step_scores_dev, int* counts_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int tdx_whisper_decode_xattn(tdx_whisper* h, const float* enc_state_dev, int B, const int* prefix_host, int prefix_len, const int* suppress_host,
                             int n_suppress, const int* begin_suppress_host, int n_begin, int eos, int max_new, const int* heads_host, int nh,
                             int first_row, int max_rows, float* xattn_dev, int* step_ids_dev, float* step_scores_dev, int* counts_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream);
size_t tdx_whisper_logmel_long_workspace_bytes(const tdx_whisper* h, long N);
int tdx_whisper_logmel_long(tdx_whisper* h, const float* wav_dev, long N, float* feat_dev, void* workspace_dev, size_t workspace_bytes,
                            void* stream);
int tdx_whisper_decode_ts(tdx_whisper* h, const float* enc_state_dev, int B, const int* prefix_host, int max_prefix, const int* prefix_len_host,
                          const int* begin_host, const int* suppress_host, int n_suppress, const int* begin_suppress_host, int n_begin, int eos,
                          int no_timestamps_id, int max_initial_timestamp_index, const int* max_new_host, int no_speech_id,
                          const int* sot_pos_host, float* nospeech_dev, const int* heads_host, int nh, const int* first_row_host, int max_rows,
                          float* xattn_dev, int* step_ids_dev, float* step_scores_dev, int* counts_dev, void* workspace_dev,
                          size_t workspace_bytes, void* stream);
size_t tdx_whisper_decode_sample_workspace_bytes(const tdx_whisper* h, int B);
int tdx_whisper_decode_ts_sample(tdx_whisper* h, const float* enc_state_dev, int B, const int* prefix_host, int max_prefix,
                                 const int* prefix_len_host, const int* begin_host, const int* suppress_host, int n_suppress,
                                 const int* begin_suppress_host, int n_begin, int eos, int no_timestamps_id, int max_initial_timestamp_index,
                                 const int* max_new_host, int no_speech_id, const int* sot_pos_host, float* nospeech_dev, const int* heads_host,
                                 int nh, const int* first_row_host, int max_rows, float* xattn_dev, int* step_ids_dev, float* step_scores_dev,
                                 int* counts_dev, const float* temperature_host, const unsigned long long* stream_host, unsigned long long seed,
                                 void* workspace_dev, size_t workspace_bytes, void* stream);
size_t tdx_token_align_workspace_bytes(int B, int nh, int max_rows, int n_audio_ctx);
int tdx_token_align(const float* xattn_dev, int B, int nh, int max_rows, int n_audio_ctx, const int* nrows_dev, const int* nframes_dev,
                    int median_width, int* frames_dev, float* matrix_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * N6  noisereduce's spectral gate — replaces `nr.reduce_noise(y=audio_data, sr=sampling_rate)`   AudioProcessor.py:655
 *     (third-party noisereduce, non-stationary mode with its defaults; restated from upstream).
 *      STFT 1024 / hop 256 / periodic Hann with scipy's boundary="zeros", padded=False frame grid; |S| smoothed along time by
 *      filtfilt([b], [1, b - 1]) (forward and backward, each pass seeded with the steady state of its first sample); mask =
 *      sigmoid(((|S| - s) / s - thresh) * slope), 0 where s == 0 (upstream: NaN on digital silence); the mask smoothed by the
 *      normalised triangles of 2 nf + 1 bins and 2 nt + 1 frames with zero boundaries; mask * prop_decrease + (1 - prop_decrease);
 *      inverse STFT.  No model: create takes the device alone and builds the two DFT bases in double.
 *      A call gates nbuf buffers: x_dev [n_total] holds the clips packed back to back, y_dev [n_total] receives the kept samples
 *      (nothing else of it is written).  The table has 8 int64 per buffer — src_off, v0, v1, k0, k1, dst_off, L, row0 — and is
 *      passed twice with equal contents: table_host is validated and planned from, table_dev is what the kernels read.
 *      Buffer sample i is x[src_off + i] for v0 <= i < v1 and zero elsewhere in [0, L); F = 1 + L / 256 frames; samples [k0, k1)
 *      go to y[dst_off ...], and each needs its four frames: 256 <= k0, k1 <= 256 * (L / 256 - 1).  A buffer takes
 *      tdx_ngate_rows(L) = F + 3 rows; buffers fill rounds in order, a round is closed when the next buffer would take it past
 *      rows_per_launch, and row0 is the buffer's first row in its round.  The workspace is sized by the rows of the largest
 *      round.  Seven launches per round whatever nbuf.  The result of a buffer does not depend on the other buffers, on
 *      rows_per_launch or on the call.  1 <= nbuf <= 65535, F <= 32768, 0 <= nf, nt <= 128, 0 < b <= 1, 0 <= prop_decrease <= 1;
 *      every table entry is checked against n_total and L before the device is touched, each violation with its own message.
 *      Taps (NULL or [F, 513] of buffer 0): |S|, the smoothed |S|, the mask before and after its smoothing.
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_ngate tdx_ngate;
int tdx_ngate_create(int device, tdx_ngate** out);
int tdx_ngate_destroy(tdx_ngate* h);
long tdx_ngate_rows(long L);
size_t tdx_ngate_workspace_bytes(const tdx_ngate* h, long rows);
int tdx_ngate_forward(tdx_ngate* h, const float* x_dev, long n_total, const int64_t* table_host, const int64_t* table_dev, int nbuf,
                      long rows_per_launch, double b, int nf, int nt, float thresh, float slope, float prop_decrease, float* y_dev,
                      float* tap_mag_dev, float* tap_smooth_dev, float* tap_mask_dev, float* tap_msmooth_dev, void* workspace_dev,
                      size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * N11  emotion2vec — replaces funasr's `AutoModel(model=emotion_model_dir)` + `self.emotion(wav, granularity="utterance",
 *      extract_embedding=False)`   ASRProcessor.py:277-283, :945.  A data2vec 2.0 audio encoder and a linear head, fp32,
 *      restated from upstream (parity with iic/emotion2vec_plus_large is unpinned).
 *      Clip normalisation (x - mean) / sqrt(var + 1e-5) (digital silence gives zeros); n_conv strided convolutions without
 *      bias, each followed by LayerNorm over the C channels and erf-GELU; LayerNorm + Linear C -> D; x + P(x) with P =
 *      pos_layers x [Conv1d(D, D, pos_k, groups pos_groups) -> LayerNorm without affine -> GELU]; E learned prefix rows; a
 *      LayerNorm, then prenet_depth + depth post-LN blocks with head width 64 whose scores carry the symmetric ALiBi bias
 *      -slope_h max(alibi_scale_h, 0) |i - j| between frames and none to or from a prefix row; outputs: the T frame rows
 *      [B][T][D], their mean [B][D], softmax(head(mean)) [B][n_classes] — each optional (NULL).
 *      The blob holds the tensors under the short names of targetdiarization_amd/emotion.py PARAM_NAMES: conv.{i}.weight,
 *      conv.{i}.ln.{weight,bias}, proj.ln.*, proj.*, pos.{l}.{weight,bias}, extra_tokens, alibi_scale, prenet.norm.*,
 *      prenet.blocks.{l}.* and blocks.{l}.* with attn.qkv, attn.proj, norm1, mlp.fc1, mlp.fc2, norm2, head.*; shapes are strict
 *      and a tensor nobody asked for is an error.  create refuses D != 64 H, D % pos_groups != 0 and a group width that is not
 *      a multiple of 4 (or above 64), C not a multiple of 64 in [64, 1024], each with its own message.
 *      A launch takes B clips of the same length N; T = tdx_emo2v_frames(h, N) must be >= 1 (N >= 400 with the published
 *      kernels).  forward_taps also returns (each NULL or a buffer): the projection [B][T][D], x + P(x) [B][T][D], and the
 *      qkv [B][S][3 D] and attention output [B][S][D] of the first block, S = E + T.
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_emo2v tdx_emo2v;
typedef struct tdx_emo2v_config {
    int32_t C, D, H, E, prenet_depth, depth, n_conv;
    int32_t conv_k[8], conv_s[8];
    int32_t pos_layers, pos_k, pos_groups, n_classes;
    int32_t reserved[4];
} tdx_emo2v_config;
int tdx_emo2v_create(const tdx_emo2v_config* cfg, const void* weights_blob, size_t blob_bytes, int device, tdx_emo2v** out);
int tdx_emo2v_destroy(tdx_emo2v* h);
long tdx_emo2v_frames(const tdx_emo2v* h, long N);
size_t tdx_emo2v_workspace_bytes(const tdx_emo2v* h, int B, long N);
int tdx_emo2v_forward(tdx_emo2v* h, const float* wav_dev, int B, long N, float* feats_dev, float* emb_dev, float* scores_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream);
int tdx_emo2v_forward_taps(tdx_emo2v* h, const float* wav_dev, int B, long N, float* feats_dev, float* emb_dev, float* scores_dev,
                           float* tap_proj_dev, float* tap_pos_dev, float* tap_qkv_dev, float* tap_attn_dev, void* workspace_dev,
                           size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Probabilistic YIN pitch tracking (librosa.pyin, restated from upstream; parity with the package is unpinned) — DESIGN 8.21.
 *      x_dev holds the clips back to back (n_total floats).  The table has one entry of 4 int64 per clip: off (index of the
 *      clip's sample 0 in x_dev), n (samples), frame0 (first row of the clip in every per-frame output: the frames of the clips
 *      before it), T (frames: 1 + n / hop_length with center, 1 + (n - frame_length) / hop_length without).  It is passed twice
 *      with equal contents: table_host is validated, table_dev is what the kernels read.  The parameters are the host-side
 *      plan of the call (pitch.pyin_plan): periods, bins and the transition width are NOT recomputed here.  tables_dev, fp64:
 *          thr[n_thresholds + 1] | beta_probs[n_thresholds] | cumulative beta_probs [n_thresholds + 1] |
 *          Boltzmann factor (1 - e^-l) / (1 - e^(-l n)) [n_lags + 1] | e^(-l pos) [n_lags + 1] |
 *          log triangle [width] | -log of the sum of each source row of the band [n_pitch_bins]
 *      with n_lags = max_period - min_period + 1; tables_len is their total length.  Outputs per frame: states (int32; below
 *      n_pitch_bins voiced, bin = state % n_pitch_bins) and voiced_prob.  Taps (NULL, or all frames of the call): yin
 *      [frames][n_lags], shifts [frames][n_lags], obs [frames][2 n_pitch_bins].  Three launches whatever nclips; the result of a
 *      clip does not depend on the other clips of the call.  The difference function is summed directly in fp32 (upstream: FFT
 *      autocorrelation with values below 1e-6 flushed to 0); the padding is zeros.
 *      Limits, each rejected with its own message before the device is touched: frame_length 4 .. 8192, 1 <= win_length <
 *      frame_length, max_period <= min(frame_length - win_length - 1, 4096), max_period - min_period >= 2, 2 n_pitch_bins <= 4096,
 *      width odd and <= n_pitch_bins, n_thresholds 1 .. 254, 1 <= nclips <= 65535, every table entry.
 *
 *      tdx_pyin_viterbi: the decoding stage alone over obs_dev [T][2 n_pitch_bins] (probabilities, fp32); only n_pitch_bins,
 *      width, the three logs and the last two tables are read, the layout of tables_dev is the same.  tdx_pyin_forward runs
 *      the same kernel.  The path is the dense librosa.sequence.viterbi's: scores in fp64, first maximum on ties.
 * ---------------------------------------------------------------------------------- */
typedef struct tdx_pyin tdx_pyin;
typedef struct tdx_pyin_params {
    int32_t frame_length, win_length, hop_length, center;
    int32_t min_period, max_period, n_pitch_bins, n_thresholds;
    int32_t width;
    int32_t reserved[3];
    double sr, fmin, bins_per_octave;                  /* bins_per_octave = 12 * ceil(1 / resolution) */
    double no_trough_prob;
    double log_stay, log_switch, log_init_unvoiced;    /* log(1 - switch_prob + tiny), log(switch_prob + tiny), log(1 / n_pitch_bins + tiny) */
} tdx_pyin_params;
int tdx_pyin_create(int device, tdx_pyin** out);
int tdx_pyin_destroy(tdx_pyin* h);
size_t tdx_pyin_workspace_bytes(const tdx_pyin* h, const tdx_pyin_params* params, long total_frames);
int tdx_pyin_forward(tdx_pyin* h, const float* x_dev, long n_total, const int64_t* table_host, const int64_t* table_dev, int nclips,
                     const tdx_pyin_params* params, const double* tables_dev, size_t tables_len, int* states_dev, float* voiced_prob_dev,
                     float* tap_yin_dev, float* tap_shifts_dev, float* tap_obs_dev, void* workspace_dev, size_t workspace_bytes,
                     void* stream);
int tdx_pyin_viterbi(tdx_pyin* h, const float* obs_dev, long T, const tdx_pyin_params* params, const double* tables_dev, size_t tables_len,
                     int* states_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Phase-vocoder time stretch, pitch shift and EQ match (librosa 0.10's stft / phase_vocoder / istft and resample's role,
 * restated from upstream; parity with the package is unpinned) — AudioProcessor.py:452-546, DESIGN 8.22.
 *      Transforms: periodic Hann of n_fft points, center=True with ZERO padding of n_fft / 2 on both sides, T = 1 + n / hop
 *      frames.  tdx_pvoc_stretch is fixed at n_fft 2048, hop 512 (librosa's defaults); the others take (n_fft, hop) under the
 *      rule of the GEMM core: n_fft a multiple of 128 in [128, 4096] (the synthesis GEMM's N in tiles of 128, its K n_fft + 32),
 *      hop a multiple of 4 (the analysis rows overlap with pitch hop and are read 16 bytes at a time) with n_fft / 16 <= hop <=
 *      n_fft (the gather sums at most 16 frames per sample).  Anything else is TDX_E_INVALID with its own message.  create
 *      builds the bases of n_fft 2048 in double; tdx_pvoc_prepare builds those of another n_fft (allocates and copies: not for
 *      a captured stream), and a call with an n_fft nobody prepared is TDX_E_INVALID.
 *      Spectra that cross the ABI are complex64 [C][frames][n_fft / 2 + 1] (re, im interleaved), frames major.
 *
 *      tdx_pvoc_stretch: x_dev [C][n] -> y_dev [C][length].  The plan (effects.stretch_plan) is steps = arange(0, T, rate) in
 *      float64: idx[t] = int(steps[t]) (int32, passed twice: idx_host is validated, idx_dev is read by the kernel), alpha[t] =
 *      steps[t] mod 1 (fp64), Tout entries.  Output frame t: mag = (1 - alpha) |D[idx]| + alpha |D[idx + 1]| in fp32, columns
 *      >= T being exact zeros (magnitude 0, angle 0); phase acc[t] with acc[0] = angle(D[0]), acc[t + 1] = acc[t] + phi_k +
 *      wrap(angle(D[idx + 1]) - angle(D[idx]) - phi_k), phi_k = 2 pi k hop / n_fft, wrap(d) = d - 2 pi rint(d / 2 pi): all in
 *      fp64 (atan2, wrap, running sum, sincos).  The running sum is cut into segments of TDX_PVOC_SEG frames, TDX_PVOC_SLOTS of
 *      them per sweep, so its order depends on the clip alone.  Synthesis: inverse DFT x Hann, then every sample is the sum of
 *      the entries of the frames that cover it (first frame first) divided by the sum of Hann^2 of the same frames unless that
 *      is <= FLT_MIN; min(Tout, ceil((length + n_fft) / hop)) frames are used and samples beyond them are 0.
 *      Taps (NULL or complex64): the analysis spectrum [C][T][1025], the stretched spectrum [C][Tout][1025].
 *      Channel c of a call is computed exactly as a call with that channel alone.
 *      tdx_pvoc_vocode: the phase vocoder alone on D_dev complex64 [T][nbin] -> out_dev [Tout][nbin], n_fft = 2 (nbin - 1).
 *      tdx_pvoc_istft: D_dev complex64 [T][n_fft / 2 + 1] -> y_dev [length]; length < 0 means hop (T - 1).
 *      tdx_pvoc_eq_match: gain[k] = clip(mean_t |S_tgt[k]| / mean_t |S_src[k]|, 0.1, 10) with the means summed in fp64 in a
 *      fixed order; a source mean of exactly 0 gives gain 10 (the bin's output is 0 either way; upstream: 0 / 0 = NaN through
 *      the whole clip).  y_dev [hop (T_src - 1)] = istft(S_src gain).  The target is samples (tgt_dev, n_tgt) or a spectrum
 *      (tgt_stft_dev complex64 [T_tgt][n_fft / 2 + 1]), one of the two.  Taps (NULL or): the source spectrum, the two mean
 *      curves (fp64 [n_fft / 2 + 1]) and the gain (fp32).
 *      tdx_pvoc_workspace_bytes(h, n_fft, hop, C, n, Tout): stretch (2048, 512, C, n, Tout); istft (n_fft, hop, 1, 0, T);
 *      eq_match (n_fft, hop, 1, max(n_src, n_tgt), 0).  0 for arguments outside the limits.
 *      Limits, each rejected with its own message before the device is touched: 1 <= C <= 65535, 1 <= n, length <= 2^36, at
 *      most 2e9 frame rows per call, 1 <= Tout <= 2^30, every plan entry in [0, T).
 *
 *      tdx_resample_sinc: resampling by any ratio rho = target / orig in [1/64, 64], no handle.  n_out =
 *      tdx_resample_sinc_length(n_in, rho) = ceil(n_in rho).  Output m lies at the input position p = m / rho (fp64); with c =
 *      min(1, rho) and H = 10 / c, h(d) = c sinc(c d) I0(5 sqrt(1 - (d / H)^2)) / I0(5) for |d| <= H — the continuous form of
 *      the Kaiser(5.0) design with 10 zero crossings that tdx_resample_poly's filters sample — and y[m] = sum_j h(j - p) x[j] /
 *      sum_j h(j - p) over all integer j in the window, samples outside the clip being zero.  Taps and sums in fp64 (I0 by
 *      its power series).  x_dev [C][n_in] -> y_dev [C][n_store]: the first min(n_out, n_store) samples, zeros after them
 *      (librosa.util.fix_length in the same launch).
 * ---------------------------------------------------------------------------------- */
#define TDX_PVOC_SEG 16
#define TDX_PVOC_SLOTS 32
typedef struct tdx_pvoc tdx_pvoc;
int tdx_pvoc_create(int device, tdx_pvoc** out);
int tdx_pvoc_destroy(tdx_pvoc* h);
int tdx_pvoc_prepare(tdx_pvoc* h, int n_fft);
size_t tdx_pvoc_workspace_bytes(const tdx_pvoc* h, int n_fft, int hop, int C, long n, long Tout);
int tdx_pvoc_stretch(tdx_pvoc* h, const float* x_dev, int C, long n, const int32_t* idx_host, const int32_t* idx_dev, const double* alpha_dev,
                     int Tout, long length, float* y_dev, float* tap_spec_dev, float* tap_stretched_dev, void* workspace_dev,
                     size_t workspace_bytes, void* stream);
int tdx_pvoc_vocode(tdx_pvoc* h, const float* D_dev, int nbin, int T, int hop, const int32_t* idx_host, const int32_t* idx_dev,
                    const double* alpha_dev, int Tout, float* out_dev, void* stream);
int tdx_pvoc_istft(tdx_pvoc* h, const float* D_dev, int T, int n_fft, int hop, long length, float* y_dev, void* workspace_dev,
                   size_t workspace_bytes, void* stream);
int tdx_pvoc_eq_match(tdx_pvoc* h, const float* src_dev, long n_src, const float* tgt_dev, long n_tgt, const float* tgt_stft_dev, int T_tgt,
                      int n_fft, int hop, float* y_dev, float* tap_spec_dev, double* tap_mean_src_dev, double* tap_mean_tgt_dev,
                      float* tap_gain_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
long tdx_resample_sinc_length(long n_in, double ratio);
int tdx_resample_sinc(const float* x_dev, int C, long n_in, double ratio, float* y_dev, long n_store, void* stream);

/* ------------------------------------------------------------------------------------
 * Spectral clustering, the dense part (clustering.spectral_labels up to the eigenvectors) — DESIGN 8.24.  Stateless, all
 * arithmetic in fp64, no floating-point atomics and fixed reduction orders: a call returns the same bits every time.
 *      1 <= n <= 8192 (element indices are int, byte offsets size_t: L alone is 512 MiB at the cap), 1 <= d <= 65536.
 *
 *      tdx_spectral_laplacian: emb_dev [n][d] f32 -> L_dev [n][n] f64.  Rows are scaled to unit length, u = x / max(|x|, 1e-12);
 *      A = U U^T, summed over d in ascending order with fma (A is symmetric to the bit); A_tap_dev (NULL or [n][n] f64) receives
 *      this unpruned affinity.  Per row the `drop` smallest entries become 0, exactly those that
 *      np.argsort(A, axis=1, kind="stable")[:, :drop] names: among equal values the lower column index is the smaller one, -0.0
 *      equals 0.0, and the diagonal (= 1) takes part.  0 <= drop < n.  Then A <- (A + A^T) / 2, diagonal 0, and
 *      L = diag(row sums) - A, each row sum in a fixed tree order.
 *
 *      tdx_symeig_lowest: the m lowest eigenpairs of the symmetric M_dev [n][n] (row-major, full storage, OVERWRITTEN),
 *      1 <= m <= min(n, 16): w_dev [m] ascending, V_dev [n][m] row-major with orthonormal columns.  The direct route of LAPACK:
 *      unblocked Householder tridiagonalisation (dsytd2; two launches per column, so about 2 n launches — a column with nothing
 *      below its subdiagonal is skipped, H = I), bisection on Sturm counts from the Gershgorin interval (dstebz' pivmin rule, at
 *      most 128 halvings), inverse iteration with partial pivoting (a zero pivot becomes eps |T|; computed eigenvalues closer
 *      than 10 eps |T| are moved apart; start vectors are a fixed hash of (row, index); 5 iterations, after each one modified
 *      Gram-Schmidt against all earlier vectors of the m), back-transformation by the stored reflectors.  M = 0 gives w = 0 and
 *      the first m unit vectors.  Eigenvectors of a multiple eigenvalue are an orthonormal basis of its space, no particular one.
 *
 *      tdx_spectral_workspace_bytes(n, d, m): one size for both entries (symeig ignores d: pass 1); 0 for arguments outside
 *      the limits.  Bad arguments are TDX_E_INVALID, a short workspace TDX_E_WORKSPACE, both before anything is launched.
 * ---------------------------------------------------------------------------------- */
size_t tdx_spectral_workspace_bytes(int n, int d, int m);
int tdx_spectral_laplacian(const float* emb_dev, int n, int d, int drop, double* L_dev, double* A_tap_dev, void* workspace_dev,
                           size_t workspace_bytes, void* stream);
int tdx_symeig_lowest(double* M_dev, int n, int m, double* w_dev, double* V_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * FFT of any length n — prime, odd or a power of two — and the band mix of AudioProcessor.mix_audio_by_freq
 * (AudioProcessor.py:845-882) on top of it — DESIGN 8.27.  Stateless: no handle, no allocation, no synchronisation, nothing but
 * kernel launches on the caller's stream (capturable).  No floating-point atomics: a result depends on (n, data) alone, row b of
 * a batch equals a call with that row alone bit for bit, and so does a repeated call.
 *      Layout: complex64, re / im interleaved, [batch][n]; a half spectrum is [batch][n / 2 + 1].  numpy's conventions: the
 *      forward transform is unnormalised, the inverse is scaled by 1 / n.
 *      Powers of two: Stockham autosort, up to TDX_FFT_TILE points in one workgroup's LDS, longer ones in several passes that
 *      each read and write the data once.  Any other n: Bluestein's chirp-z over the power of two M >= 2n - 1, the chirp
 *      evaluated in fp64 from k^2 mod 2n and rounded once, rebuilt in the workspace on every call (up to 64 points: the DFT sum
 *      itself in fp64; the band mix of a clip of up to 64 samples runs in fp64 throughout and is rounded once).
 *
 *      tdx_fft_c2c: x_dev [batch][n] complex -> y_dev [batch][n] complex, inverse != 0 for the inverse.
 *      tdx_fft_r2c: x_dev [batch][n] real -> X_dev [batch][n / 2 + 1] complex (np.fft.rfft).  Even n: one complex transform of
 *      n / 2 points and a split; odd n: the complex path.
 *      tdx_fft_c2r: X_dev [batch][n / 2 + 1] complex -> y_dev [batch][n] real (np.fft.irfft(X, n)); the imaginary parts of bin 0
 *      and, for even n, of bin n / 2 are ignored.
 *      tdx_fft_band_mix: two real clips of n samples -> y_dev [2 (n / 2)].  Z = DFT_n(main + i aux) is one complex transform;
 *      F_main[k] = (Z[k] + conj Z[n - k]) / 2, F_aux[k] = (Z[k] - conj Z[n - k]) / 2i for the bins k <= n / 2.  ranges = the bin
 *      ranges [lo, hi) of main, aux and their overlap (fft.band_mix_plan): mix[k] = F_main[k] in main's range, then F_aux[k] in
 *      aux's, then F_main[k] w + F_aux[k] (1 - w) in the overlap, w = np.linspace(1, 0, count)[k - lo] formed in fp64 (j step +
 *      1, the last one exactly 0, [1.0] for one bin), blended in fp64 and rounded once; a bin in no range is exactly 0.
 *      y = np.fft.irfft(mix): the n / 2 + 1 bins read as the spectrum of m = 2 (n / 2) samples (an odd n comes back one sample
 *      shorter), the imaginary parts of bin 0 and of the last bin dropped, through one inverse complex transform of m / 2
 *      points.  Taps (each NULL or complex64 [n / 2 + 1]): F_main, F_aux and mix (with all its imaginary parts).
 *
 *      Limits, each TDX_E_INVALID with its own message before the device is touched: 1 <= n <= 2^26 (band mix: 2 <= n),
 *      1 <= batch <= 65535, bin ranges 0 <= lo <= hi <= n / 2 + 1, no null pointer (taps excepted), every pointer 8-byte
 *      aligned (the kernels move pairs of floats; a real row of even length is read as n / 2 complex), the workspace at least tdx_fft_workspace_bytes(n, batch) (one size for the three transforms) or
 *      tdx_fft_band_mix_workspace_bytes(n); both are 0 for arguments outside the limits.  In-place operation (the output is the
 *      input) is rejected; input and output must not overlap.
 * ---------------------------------------------------------------------------------- */
#define TDX_FFT_TILE 4096
size_t tdx_fft_workspace_bytes(long n, int batch);
int tdx_fft_c2c(const float* x_dev, long n, int batch, int inverse, float* y_dev, void* ws, size_t ws_bytes, void* stream);
int tdx_fft_r2c(const float* x_dev, long n, int batch, float* X_dev, void* ws, size_t ws_bytes, void* stream);
int tdx_fft_c2r(const float* X_dev, long n, int batch, float* y_dev, void* ws, size_t ws_bytes, void* stream);
size_t tdx_fft_band_mix_workspace_bytes(long n);
int tdx_fft_band_mix(const float* main_dev, const float* aux_dev, long n, const long ranges[6], float* y_dev, float* tap_main, float* tap_aux,
                     float* tap_mix, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TDX_H */
