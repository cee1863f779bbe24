// pf_timestamps.hpp — the second head of funasr's CifPredictorV3 (BiCifParaformer, the "paraformer-large-vad-punc" bundle): a x3
// transposed convolution, a bidirectional LSTM (hidden 512) and a one-column Linear give "upsampled alphas" on a 20 ms grid, from
// which the host builds one [start_ms, end_ms] per token (targetdiarization_amd/pf_timestamps.py).  Third-party, parity unpinned.
// The functions are defined in pf_timestamps.hip and are internal to libtdx.so (C++ linkage); the C-ABI entry points
// (tdx_pfdec_timestamps*) live with the handle in paraformer.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "epilogues.hpp"
#include "tdx_common.hpp"
#include "weight_pack.hpp"
#include "weight_planes.hpp"

struct PfTsHead {
    bool present = false;
    float smooth = 0.25f, noise = 0.01f;       // smooth_factor2, noise_threshold2
    tdx::H3W hup, hih;                         // x3 planes of the two GEMM weights
    const float *Wup = nullptr, *bup = nullptr, *Wih = nullptr, *bih = nullptr, *whhT = nullptr, *w2 = nullptr, *b2 = nullptr;
};
// Stages the head's tensors when the blob holds any of them (a partial set leaves the first missing name in the Loader, so that
// finish() fails with it) and binds them to w, which sits in the heap-allocated handle (Loader::bind); returns whether the head is there.
bool pfts_stage(tdx::Loader& ld, PfTsHead& w);
// after finish(): marks the head present and queues its two GEMM weights for split_weight_planes
void pfts_queue_planes(PfTsHead& w, std::vector<tdx::PlaneJob>& jobs);
size_t pfts_work_floats(size_t B, size_t T);
// enc [B,T,512], counts int32 [B] -> us_alphas [B,3T], us_peaks [B,3T]; tap (or NULL) [B,3T,1024] = the BLSTM output.
// The first B*3T floats of ws hold the alphas before the re-normalisation on return.
int pfts_forward(const PfTsHead& w, const float* enc, int B, int T, const int* counts, float* us_alphas, float* us_peaks, float* tap,
                 float* ws, hipStream_t st);
