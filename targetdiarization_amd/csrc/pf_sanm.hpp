// pf_sanm.hpp — what the two models that stack funasr's SANM encoder layer share: Paraformer (paraformer.hip, where the layer,
// its kernels and its dispatch thresholds live) and SenseVoiceSmall (sensevoice.hip).  ONE layer loop (pf_run_layers), ONE weight
// staging (pf_stage_layer / pf_queue_planes), ONE workspace layout (PfWork); the functions are defined in paraformer.hip and are
// internal to libtdx.so (C++ linkage: not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "epilogues.hpp"
#include "tdx_common.hpp"
#include "weight_planes.hpp"

// one layer: d = 512, 4 heads, FFN 2048, FSMN memory of 11 taps, pre-LN (eps 1e-12); fp32 weights and the x3 planes of the Linears
struct PfLayer {
    const float *Wqkv = nullptr, *bqkv = nullptr, *fsmnT = nullptr, *Wo = nullptr, *bo = nullptr, *W1 = nullptr, *b1 = nullptr, *W2 = nullptr,
        *b2 = nullptr, *n1g = nullptr, *n1b = nullptr, *n2g = nullptr, *n2b = nullptr;
    tdx::H3W hqkv, ho, h1, h2;
};
// a layer's tensors under the funasr prefix p ("encoder.encoders.3.") into the Loader's image, bound to w (an element of the handle's
// vector at its final size: Loader::bind); wide: the 560 -> 512 layer (K padded to 576)
void pf_stage_layer(tdx::Loader& ld, const std::string& p, bool wide, PfLayer& w);
// after finish(): the layer's four Linears queued for split_weight_planes
void pf_queue_planes(bool wide, PfLayer& w, std::vector<tdx::PlaneJob>& jobs);

// the activations of a layer stack over M = B * T rows
struct PfWork { float *x, *xin, *qkv, *sc, *ctx, *mem, *ffn; unsigned char* hp; float *hs, *hs8, *slab; };
size_t pf_work_floats(size_t B, size_t T);
PfWork pf_carve(float* ws, long M, int B, int T);
// n layers over the residual stream x [B*T][512], in place; wide_first: layer 0 reads k.xin [B*T][576] and has no attention residual.
// Rows <= 512 take the split-K Linears, short sequences the one-launch attention, as for Paraformer.
int pf_run_layers(const PfLayer* layers, int n, bool wide_first, float* x, const PfWork& k, int B, int T, hipStream_t st);
struct PfPrompt { int id[4]; };      // rows of the prompt embedding table in front of an utterance's features (by value into the launch)
int pf_embed_rows(const float* feats, const float* embed, PfPrompt pr, int nprompt, float* x, int B, int T, hipStream_t st);
int pf_layernorm_rows(const float* x, const float* g, const float* b, float* out, long M, hipStream_t st);
int pf_argmax_rows(const float* logits, long ld, int V, int* ids, float* score, long M, hipStream_t st);
