"""Plain-torch restatement of WeSpeaker ResNet34 with pyannote's masked statistics pooling (wespeaker `ResNet34`:
m_channels 32, feat_dim 80, embed_dim 256, TSTP, two_emb_layer False; pyannote.audio `WeSpeakerResNet34`, `StatsPool`)
[upstream-recall]: the package is absent and no checkpoint is at hand, so this file and DESIGN §8.14 govern where memory of
upstream differs.  BatchNorm is applied unfolded, in eval mode."""
from __future__ import annotations

import json
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as Fn

from oracle.frontend_oracle import kaldi_fbank
from targetdiarization_amd.weights import recipe_wespeaker_state_dict
from pyannet_oracle import voice

HERE = os.path.dirname(os.path.abspath(__file__))
CALIBRATION = os.path.join(HERE, "golden", "wespeaker_calibration.json")
BLOCKS = (3, 4, 6, 3)
EPS = 1e-5
REL_BAR, COS_BAR = 1e-4, 1e-3        # the project's embedding bars (tests/test_gpu_campplus.py)


def features(wave) -> torch.Tensor:
    """1-D wave in [-1,1] -> [F,80]: fbank80 (hamming, input x32768, dither 0) minus the utterance mean over time"""
    wave = torch.as_tensor(wave)
    f = kaldi_fbank(wave, "hamming", 32768.0)
    return f - f.mean(dim=0, keepdim=True)


def resample_nearest(w: torch.Tensor, T: int) -> torch.Tensor:
    """[..., Fw] -> [..., T]: w'[i] = w[(i * Fw) // T]"""
    Fw = w.shape[-1]
    idx = (torch.arange(T, dtype=torch.int64) * Fw) // T
    return w[..., idx]


def stats_pool(x: torch.Tensor, w: torch.Tensor | None = None) -> torch.Tensor:
    """x [B,D,T], w None | [B,S,T] (already on x's frames) -> [B,S,2D] (S = 1 without weights): pyannote StatsPool
        v1 = sum w, v2 = sum w^2, mean = sum w x / v1, var = sum w (x - mean)^2 / (v1 - v2/v1 + 1e-8), [mean | sqrt(var)]"""
    if w is None:
        w = torch.ones(x.shape[0], 1, x.shape[2], dtype=x.dtype)
    w = w.to(x.dtype)[:, :, None, :]                    # [B,S,1,T]
    xs = x[:, None]                                     # [B,1,D,T]
    v1 = w.sum(dim=-1)
    v2 = (w * w).sum(dim=-1)
    mean = (w * xs).sum(dim=-1) / v1
    var = (w * (xs - mean[..., None]) ** 2).sum(dim=-1) / (v1 - v2 / v1 + 1e-8)
    return torch.cat([mean, var.sqrt()], dim=-1)


def _bn(sd, p, x, dtype, collect):
    if collect is not None:                             # calibration pass: this batch's statistics become the running ones
        mu, var = x.mean(dim=(0, 2, 3)), x.var(dim=(0, 2, 3), unbiased=False)
        collect[p + "running_mean"], collect[p + "running_var"] = mu.float(), var.float()
    else:
        mu, var = sd[p + "running_mean"].to(dtype), sd[p + "running_var"].to(dtype)
    s = sd[p + "weight"].to(dtype) / torch.sqrt(var + EPS)
    return (x - mu[None, :, None, None]) * s[None, :, None, None] + sd[p + "bias"].to(dtype)[None, :, None, None]


def trunk(sd, feat, dtype=torch.float64, collect=None) -> torch.Tensor:
    """feat [B,F,80] -> [B,2560,T'] with feature index c*10 + h"""
    x = torch.as_tensor(feat).to(dtype).transpose(1, 2)[:, None]           # [B,1,h=mel,w=time]
    cv = lambda name, x, stride, pad: Fn.conv2d(x, sd[name].to(dtype), stride=stride, padding=pad)
    x = torch.relu(_bn(sd, "resnet.bn1.", cv("resnet.conv1.weight", x, 1, 1), dtype, collect))
    for li, nb in enumerate(BLOCKS):
        for i in range(nb):
            p = f"resnet.layer{li + 1}.{i}."
            stride = 2 if (i == 0 and li > 0) else 1
            y = torch.relu(_bn(sd, p + "bn1.", cv(p + "conv1.weight", x, stride, 1), dtype, collect))
            y = _bn(sd, p + "bn2.", cv(p + "conv2.weight", y, 1, 1), dtype, collect)
            if p + "shortcut.0.weight" in sd:
                x = _bn(sd, p + "shortcut.1.", cv(p + "shortcut.0.weight", x, stride, 0), dtype, collect)
            x = torch.relu(y + x)
    return x.reshape(x.shape[0], -1, x.shape[3])


def head(sd, tr, weights=None, dtype=torch.float64) -> torch.Tensor:
    """trunk output [B,2560,T'] + weights None | [B,S,Fw] -> [B,S,256] ([B,256] without weights)"""
    w = None if weights is None else resample_nearest(torch.as_tensor(weights).to(dtype), tr.shape[2])
    st = stats_pool(tr, w)
    emb = st @ sd["resnet.seg_1.weight"].to(dtype).T + sd["resnet.seg_1.bias"].to(dtype)
    return emb[:, 0] if weights is None else emb


def forward(sd, feat, weights=None, dtype=torch.float64) -> torch.Tensor:
    with torch.no_grad():
        return head(sd, trunk(sd, feat, dtype), weights, dtype)


def embed_masked(sd, chunks, masks, dtype=torch.float64) -> np.ndarray:
    """chunks [n,N] waves, masks [n,S,Fw] -> [n,S,256] (the `embed_masked` of overlap.diarize over the oracle)"""
    out = []
    for c, m in zip(np.asarray(chunks), np.asarray(masks)):
        f = features(torch.from_numpy(np.ascontiguousarray(c)).to(dtype))[None]
        out.append(forward(sd, f, torch.from_numpy(np.ascontiguousarray(m))[None], dtype)[0].numpy())
    return np.stack(out)


# ---- test inputs and weights ------------------------------------------------------------------------------------------
_cache = {}


def shape_feat(B: int, F: int, seed: int = 0) -> torch.Tensor:
    """[B,F,80] float32: the first F frames of the features of B synthetic voices of at least 64 frames (cut AFTER the mean
    removal, so that F = 1 is not a row of zeros)"""
    key = ("feat", B, F, seed)
    if key not in _cache:
        n = 400 + 160 * (max(F, 64) - 1)
        rows = [features(torch.from_numpy(voice(n, b % 3, 100 * seed + 7 * B + b)))[:F] for b in range(B)]
        _cache[key] = torch.stack(rows).float().contiguous()
    return _cache[key]


def calibration_voices() -> torch.Tensor:
    """[6,150,80] float64: the batch whose statistics the BatchNorms are calibrated on"""
    n = 400 + 160 * 149
    return torch.stack([features(torch.from_numpy(voice(n, b % 3, 900 + b))) for b in range(6)])


def calibrate(sd):
    """-> {bn running_mean / running_var name: float32 tensor} from one fp64 pass over calibration_voices()"""
    got = OrderedDict()
    with torch.no_grad():
        trunk(sd, calibration_voices(), torch.float64, collect=got)
    return got


def calibration():
    if "cal" not in _cache:
        with open(CALIBRATION) as f:
            _cache["cal"] = json.load(f)
    return _cache["cal"]


def calibrated_state_dict(seed: int = 0):
    if ("sd", seed) not in _cache:
        c = calibration()
        assert c["seed"] == seed
        sd = recipe_wespeaker_state_dict(seed)
        for k, v in c["bn"].items():
            assert k in sd and sd[k].numel() == len(v), k
            sd[k] = torch.tensor(v, dtype=torch.float32)
        _cache[("sd", seed)] = sd
    return _cache[("sd", seed)]


def reference_trunk(feat: torch.Tensor, key) -> torch.Tensor:
    """fp64 trunk output of the calibrated weights on `feat`, computed once per key"""
    k = ("trunk", key)
    if k not in _cache:
        with torch.no_grad():
            _cache[k] = trunk(calibrated_state_dict(), feat, torch.float64)
    return _cache[k]


def rel_l2(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def cos_dist(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return float(1.0 - a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-300))


def shape_masks(B: int, S: int, Fw: int, Tp: int, seed: int = 0) -> np.ndarray:
    """[B,S,Fw] float32.  Per chunk: mask 0 binary on the first half, mask 1 (if any) binary on the second half — disjoint —
    and mask 2 fractional everywhere.  Chunk 0 gets special rows when there is room: its LAST mask is all zero, and with
    S >= 3 and Fw > Tp its mask 1 is one frame that nearest resampling to Tp frames never reads (it vanishes there)."""
    rng = np.random.default_rng([seed, B, S, Fw])
    m = np.zeros((B, S, Fw), dtype=np.float32)
    for b in range(B):
        for s in range(S):
            if s % 3 == 0:
                m[b, s, : max(Fw // 2, 1)] = 1.0
            elif s % 3 == 1:
                m[b, s, Fw // 2:] = 1.0
            else:
                m[b, s] = rng.uniform(0.05, 1.0, Fw).astype(np.float32)
    if S >= 2:
        m[0, S - 1] = 0.0
    if S >= 3 and Fw > Tp:
        read = set(((np.arange(Tp) * Fw) // Tp).tolist())
        lone = next(i for i in range(Fw) if i not in read)
        m[0, 1] = 0.0
        m[0, 1, lone] = 1.0
    return m


