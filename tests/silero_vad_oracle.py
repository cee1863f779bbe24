"""Functional PyTorch restatement of silero-VAD v5's 16 kHz branch (the `silero_vad` package's model) [upstream-recall: the
source is not vendored, parity with the published weights is unpinned] — the reference the device forward
(csrc/silero_vad.hip) is compared against, in fp64 by default.  Nothing is folded here: an explicit reflect pad, F.conv1d for
the STFT and the four convolutions, a Python loop over chunks with the LSTM cell written out.
Also the seeded voiced / silent test clips and the calibrated weights the tests use.  Bursts start and end on chunk
boundaries, so every chunk is wholly voiced or wholly silent."""
from __future__ import annotations

import json
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as Fn

import campplus_oracle as corc
from targetdiarization_amd.weights import recipe_silero_vad_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
CALIBRATION = os.path.join(HERE, "golden", "silero_vad_calibration.json")
SR = 16000
W, CTX = 512, 64
STRIDES = (1, 2, 2, 1)


def windows(wave: torch.Tensor) -> torch.Tensor:
    """one clip [n] -> [N,640]: per chunk 64 samples of context (zeros for the first chunk), the chunk, and a right reflect
    pad of 64 (the mirror of the chunk's own tail without the edge sample); the clip is zero-padded to whole chunks"""
    n = int(wave.shape[0])
    N = (n + W - 1) // W
    x = Fn.pad(wave, (0, N * W - n)).reshape(N, W)
    ctx = torch.cat([torch.zeros(1, CTX, dtype=wave.dtype), x[:-1, -CTX:]])
    return Fn.pad(torch.cat([ctx, x], dim=1)[:, None, :], (0, CTX), mode="reflect")[:, 0, :]


def encoder(sd, win: torch.Tensor) -> torch.Tensor:
    """[N,640] -> [N,128]: STFT magnitude [N,129,4], then Conv1d(k=3, pad=1) + ReLU with strides 1, 2, 2, 1"""
    y = Fn.conv1d(win[:, None, :], sd["stft.forward_basis_buffer"], stride=128)           # [N,258,4]
    x = torch.sqrt(y[:, :129] ** 2 + y[:, 129:] ** 2)
    for i, s in enumerate(STRIDES):
        x = torch.relu(Fn.conv1d(x, sd[f"encoder.{i}.reparam_conv.weight"], sd[f"encoder.{i}.reparam_conv.bias"], stride=s, padding=1))
    return x[:, :, 0]


def forward(sd, wave, dtype=torch.float64):
    """one clip (1-D array) -> (p [N], feat [N,128], h [N,128]) in `dtype`; N = ceil(n / 512), 0 for an empty clip"""
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    w = torch.as_tensor(np.asarray(wave), dtype=dtype).reshape(-1)
    if w.shape[0] == 0:
        return torch.empty(0, dtype=dtype), torch.empty(0, 128, dtype=dtype), torch.empty(0, 128, dtype=dtype)
    feat = encoder(sdd, windows(w))
    wih, whh = sdd["decoder.rnn.weight_ih"], sdd["decoder.rnn.weight_hh"]
    bih, bhh = sdd["decoder.rnn.bias_ih"], sdd["decoder.rnn.bias_hh"]
    h = torch.zeros(128, dtype=dtype); c = torch.zeros(128, dtype=dtype)
    hs = []
    for t in range(feat.shape[0]):
        g = wih @ feat[t] + bih + whh @ h + bhh
        i, f, gg, o = g[:128], g[128:256], g[256:384], g[384:]
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        hs.append(h)
    hs = torch.stack(hs)
    logit = torch.relu(hs) @ sdd["decoder.decoder.2.weight"][0, :, 0] + sdd["decoder.decoder.2.bias"][0]
    return torch.sigmoid(logit), feat, hs


def calibration():
    with open(CALIBRATION) as f:
        return json.load(f)


def calibrated_state_dict(seed: int = 0):
    """recipe weights with the head (decoder.decoder.2.*) from tests/golden/silero_vad_calibration.json
    (tools/make_goldens_silero_vad.py); the plain recipe's head does not separate voiced from silent chunks"""
    sd = OrderedDict((k, v.clone()) for k, v in recipe_silero_vad_state_dict(seed).items())
    cal = calibration()
    assert cal["seed"] == seed
    sd["decoder.decoder.2.weight"] = torch.tensor(cal["head_weight"], dtype=torch.float64).to(torch.float32).reshape(1, 128, 1)
    sd["decoder.decoder.2.bias"] = torch.tensor([cal["head_bias"]], dtype=torch.float64).to(torch.float32)
    return sd


# ------------------------------------------------------------------------------------------------------------
# test clips: silence (1e-4 N(0,1)) alternating with bursts of campplus_oracle's synthetic voices (fsmn_vad_oracle's mix, with
# the bursts given in chunks)
# ------------------------------------------------------------------------------------------------------------
def mix(n: int, bursts, seed: int) -> np.ndarray:
    """n samples of silence with voiced bursts [(first_chunk, end_chunk, voice), ...]"""
    rng = np.random.default_rng(seed)
    x = (1e-4 * rng.standard_normal(n)).astype(np.float32)
    for a, b, vid in bursts:
        a, b = a * W, min(b * W, n)
        if b > a:
            x[a:b] += corc.voice(vid, b - a, rng)
    return x


def labels(n: int, bursts) -> np.ndarray:
    """per chunk: 1 where a burst covers it"""
    lab = np.zeros((n + W - 1) // W, np.int64)
    for a, b, _ in bursts:
        lab[a:b] = 1
    return lab


PROB_SAMPLES = (1, 511, 512, 513, 1024, 1537, 33 * 512 - 7, 160000)          # 1, 1, 1, 2, 2, 4, 33, 313 chunks
# per clip: (bursts in chunks, seed)
PROB_PLAN = (((), 201), (((0, 1, 0),), 202), ((), 203), (((1, 2, 1),), 204), (((0, 1, 2),), 205), (((1, 3, 0),), 206),
             (((4, 13, 1), (20, 29, 2)), 207), (((10, 70, 0), (100, 160, 1), (200, 235, 2), (260, 313, 0)), 208))


def prob_clips():
    """the eight clips of the probability test"""
    return [mix(n, b, seed) for n, (b, seed) in zip(PROB_SAMPLES, PROB_PLAN)]


def prob_labels():
    return [labels(n, b) for n, (b, _) in zip(PROB_SAMPLES, PROB_PLAN)]


def leak_pair():
    """[loud voice, silence]: the second clip's first chunk reads the first one's tail, and starts from its (h, c), if context
    or state crosses the boundary"""
    rng = np.random.default_rng(242)
    loud = corc.voice(1, 20 * W, rng, amp=0.5)
    silent = mix(12 * W, [], 241)
    return [loud, silent]


def causal_pair(k: int):
    """two clips of 12 chunks, identical through chunk k, different after it"""
    a = mix(12 * W, [(0, 12, 0)], 250 + k)
    b = a.copy()
    rng = np.random.default_rng(260 + k)
    b[(k + 1) * W:] = corc.voice(2, (11 - k) * W, rng, amp=0.4)
    return a, b


E2E_PLAN = ((5 * SR + 3200, ((16, 52, 0), (75, 81, 1), (94, 138, 2)), 250),            # 5.2 s; the middle burst is 192 ms
            (144 * W - 200, ((9, 14, 2), (28, 69, 1), (103, 144, 0)), 251))            # 4.6 s; first burst 160 ms; ends in speech


def e2e_clips():
    """4-6 s, three voiced bursts each, one of them under 250 ms; the second clip ends in speech"""
    return [mix(n, b, seed) for n, b, seed in E2E_PLAN]


def e2e_labels():
    return [labels(n, b) for n, b, _ in E2E_PLAN]


CAL_PLAN = (400 * W, ((12, 60, 0), (90, 96, 1), (130, 200, 2), (230, 300, 1), (340, 345, 0), (360, 400, 2)), 299)


def calibration_clip():
    n, b, seed = CAL_PLAN
    return mix(n, b, seed), labels(n, b)
