"""Functional PyTorch restatement of FSMN-VAD (funasr/models/fsmn_vad_streaming/encoder.py with the
speech_fsmn_vad_zh-cn-16k-common-pytorch config) [upstream-recall: the source is not vendored, parity with the published
checkpoint is unpinned] — the reference the device forward (csrc/fsmn_vad.hip) is compared against, in fp64 by default.
Nothing is folded here: six separate linears, the memory as a causal depthwise convolution with a zero history per clip.
Also the seeded voiced / silent test clips and the calibrated weights the tests use."""
from __future__ import annotations

import json
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as Fn

import campplus_oracle as corc
from oracle import frontend_oracle as fo
from targetdiarization_amd.weights import recipe_fsmn_vad_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
CALIBRATION = os.path.join(HERE, "golden", "fsmn_vad_calibration.json")
SR = 16000
LAYERS, TAPS = 4, 20


def lfr_features(wave: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """funasr WavFrontend for this model: fbank80(hamming, wave * 32768) -> LFR 5/1 -> (x + shift) * scale; [T,400]"""
    f = fo.kaldi_fbank(wave, "hamming", 32768.0)
    if f.shape[0] == 0:
        return torch.empty(0, 400, dtype=wave.dtype)
    return (fo.apply_lfr(f, 5, 1) + shift.to(wave.dtype)) * scale.to(wave.dtype)


def encoder(sd, x: torch.Tensor, upto: str = "logits") -> torch.Tensor:
    """x [T,400] of ONE clip -> logits [T,248] (upto="out_linear1": that layer's activations [T,140])"""
    def lin(p, v):
        return Fn.linear(v, sd[p + "weight"], sd.get(p + "bias"))
    h = lin("encoder.in_linear1.linear.", x)
    h = torch.relu(lin("encoder.in_linear2.linear.", h))
    for i in range(LAYERS):
        p = f"encoder.fsmn.{i}."
        q = lin(p + "linear.linear.", h)                                          # [T,128], no bias
        w = sd[p + "fsmn_block.conv_left.weight"][:, 0, :, 0]                     # [128,20]
        pad = Fn.pad(q.t()[None], (TAPS - 1, 0))                                  # zero history before the clip's first frame
        m = q + Fn.conv1d(pad, w[:, None, :], groups=w.shape[0])[0].t()           # m[t] = q[t] + sum_j w[:,j] q[t-19+j]
        h = torch.relu(lin(p + "affine.linear.", m))
    h = lin("encoder.out_linear1.linear.", h)
    if upto == "out_linear1":
        return h
    return lin("encoder.out_linear2.linear.", h)


def forward(sd, cmvn, wave, dtype=torch.float64):
    """one clip (1-D array) -> (p0 [T], posterior [T,248]) in `dtype`; T = 0 below 400 samples"""
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    w = torch.as_tensor(np.asarray(wave), dtype=dtype)
    x = lfr_features(w, torch.as_tensor(cmvn[0]).to(dtype), torch.as_tensor(cmvn[1]).to(dtype))
    if x.shape[0] == 0:
        return torch.empty(0, dtype=dtype), torch.empty(0, 248, dtype=dtype)
    post = torch.softmax(encoder(sdd, x), dim=-1)
    return post[:, 0], post


def calibration():
    with open(CALIBRATION) as f:
        return json.load(f)


def calibrated_state_dict(seed: int = 0):
    """-> (state dict, (shift, scale)): recipe weights with row 0 of out_linear2 and the CMVN from
    tests/golden/fsmn_vad_calibration.json (tools/make_goldens_fsmn_vad.py); the plain recipe gives p0 ~ 1/248 everywhere"""
    sd = recipe_fsmn_vad_state_dict(seed)
    cal = calibration()
    assert cal["seed"] == seed
    sd = OrderedDict((k, v.clone()) for k, v in sd.items())
    sd["encoder.out_linear2.linear.weight"][0] = torch.tensor(cal["row0_weight"], dtype=torch.float64).to(torch.float32)
    sd["encoder.out_linear2.linear.bias"][0] = float(np.float32(cal["row0_bias"]))
    cmvn = (torch.tensor(cal["cmvn_shift"], dtype=torch.float64).to(torch.float32),
            torch.tensor(cal["cmvn_scale"], dtype=torch.float64).to(torch.float32))
    return sd, cmvn


# ------------------------------------------------------------------------------------------------------------
# test clips: silence (1e-4 N(0,1)) alternating with bursts of campplus_oracle's synthetic voices
# ------------------------------------------------------------------------------------------------------------
def mix(n: int, bursts, seed: int) -> np.ndarray:
    """n samples of silence with voiced bursts [(start_sample, end_sample, voice), ...]"""
    rng = np.random.default_rng(seed)
    x = (1e-4 * rng.standard_normal(n)).astype(np.float32)
    for a, b, vid in bursts:
        b = min(b, n)
        if b > a:
            x[a:b] += corc.voice(vid, b - a, rng)
    return x


def frames_to_samples(T: int) -> int:
    return 400 + 160 * (T - 1)


POSTERIOR_FRAMES = (1, 5, 19, 20, 21, 77, 129, 300)
# per clip: (burst start as a fraction of the clip or None for no burst, voice, seed); the burst lasts half the clip (the whole of the
# 1-frame clip).  Positions and seeds are chosen so that no frame's oracle p0 lies within 0.02 of the decision point 0.2 and every
# clip of >= 19 frames has at least 20 % of its frames on either side (tests/test_fsmn_vad_host.py checks both); the single frame
# is speech, the 5-frame clip silence.
POSTERIOR_PLAN = ((0.0, 2, 125), (None, 0, 101), (0.25, 2, 101), (0.15, 0, 175), (0.10, 2, 100), (0.25, 2, 105), (0.15, 0, 114), (0.20, 1, 123))


def posterior_clips():
    """the eight clips of the posterior test, T = 1 ... 300 frames"""
    out = []
    for T, (frac, vid, seed) in zip(POSTERIOR_FRAMES, POSTERIOR_PLAN):
        n = frames_to_samples(T)
        if frac is None:
            bursts = []
        elif T == 1:
            bursts = [(0, n, vid)]
        else:
            a = int(n * frac)
            bursts = [(a, a + n // 2, vid)]
        out.append(mix(n, bursts, seed))
    return out


def leak_pair():
    """[loud voice, silence]: the second clip's first 19 frames read the first one's tail if the memory crosses the boundary"""
    rng = np.random.default_rng(142)
    loud = corc.voice(1, frames_to_samples(60), rng, amp=0.5)
    silent = mix(frames_to_samples(40), [], 141)
    return [loud, silent]


def e2e_clips():
    """4-6 s, three voiced bursts each, one of them under 150 ms; the second clip ends in speech"""
    s = lambda sec: int(round(sec * SR))
    a = mix(s(5.2), [(s(0.5), s(1.7), 0), (s(2.4), s(2.5), 1), (s(3.0), s(4.4), 2)], 150)
    b = mix(s(4.6), [(s(0.3), s(0.42), 2), (s(0.9), s(2.2), 1), (s(3.3), s(4.6), 0)], 151)
    return [a, b]
