"""Oracle of emotion2vec (funasr `Emotion2vec`, a data2vec 2.0 audio encoder + a linear head) in plain torch, written from the
model contract, float64 by default.  It reads a state dict in UPSTREAM names (weights.emotion2vec_param_shapes)
and one clip at a time.  Steps 2-4 (conv extractor, projection, positional stack) are pinned against transformers'
Data2VecAudio modules by tests/test_emotion2vec_host.py; the ALiBi blocks and the head are restated from upstream recall."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from targetdiarization_amd.weights import emotion2vec_config, emotion2vec_upstream_name as up, recipe_wave

EPS = 1e-5
# max |p32 - p64| over the 9 probabilities of the score clips (clip(), small config, recipe seed 1): the oracle run in float32
# against itself in float64, measured by test_emotion2vec_host.py::test_score_gap_constant (2.6e-7 .. 4.4e-7 with 1 .. 8 threads
# under torch; the largest is kept).  GPU probabilities are bounded by 10 x SCORE_GAP (the LOGMEL_BAR convention).
SCORE_GAP = 4.4e-7
SMALL = dict(C=64, D=128, H=2, E=10, prenet_depth=1, depth=2)
SCORE_CLIP_FRAMES = (9, 55, 129)


def samples_for_frames(T: int, extra: int = 0) -> int:
    """the shortest clip of T frames with the published kernels and strides, plus `extra` samples (< 320 keeps T)"""
    return 400 + 320 * (T - 1) + extra


def clip(n: int, name: str = "") -> np.ndarray:
    """the test clip of n samples: Philox noise under a slow envelope plus two tones, float32"""
    x = recipe_wave(f"emotion2vec:{name}:{n}", 1, n, seed=1, amp=0.05)[0].astype(np.float64)
    t = np.arange(n) / 16000.0
    x = x * (0.3 + np.sin(2 * np.pi * 1.7 * t) ** 2) + 0.05 * np.sin(2 * np.pi * 220.0 * t) + 0.02 * np.sin(2 * np.pi * 1234.5 * t + 1.0)
    return x.astype(np.float32)


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def frames(n: int, kernels=(10, 3, 3, 3, 3, 2, 2), strides=(5, 2, 2, 2, 2, 2, 2)) -> int:
    L = n
    for k, s in zip(kernels, strides):
        L = (L - k) // s + 1 if L >= k else 0
    return L


def normalize(x):
    """(x - mean) / sqrt(var + 1e-5), biased variance, over the clip"""
    return (x - x.mean()) / torch.sqrt(x.var(unbiased=False) + EPS)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def layer_norm(x, w=None, b=None):
    return F.layer_norm(x, (x.shape[-1],), w, b, EPS)


def feature_extractor(x, sd, cfg):
    """normalised samples [N] -> [T, C]: conv (no bias) -> LayerNorm over channels -> GELU, per layer"""
    h = x[None, None, :]
    for i, (k, s) in enumerate(zip(cfg["conv_kernels"], cfg["conv_strides"])):
        h = F.conv1d(h, sd[up("conv.{n}.weight", i)], None, stride=s)
        h = layer_norm(h.transpose(1, 2), sd[up("conv.{n}.ln.weight", i)], sd[up("conv.{n}.ln.bias", i)]).transpose(1, 2)
        h = gelu(h)
    return h[0].transpose(0, 1)


def project(f, sd):
    """[T, C] -> [T, D]: LayerNorm, Linear"""
    return F.linear(layer_norm(f, sd[up("proj.ln.weight")], sd[up("proj.ln.bias")]), sd[up("proj.weight")], sd[up("proj.bias")])


def positional(x, sd, cfg):
    """P(x): pos_layers x [grouped Conv1d with zero padding -> LayerNorm without affine -> GELU]; [T, D] -> [T, D]"""
    h = x.transpose(0, 1)[None]
    for l in range(cfg["pos_layers"]):
        h = F.conv1d(h, sd[up("pos.{n}.weight", l)], sd[up("pos.{n}.bias", l)], padding=cfg["pos_k"] // 2, groups=cfg["pos_groups"])
        h = gelu(layer_norm(h.transpose(1, 2)).transpose(1, 2))
    return h[0].transpose(0, 1)


def alibi_slopes(n: int):
    """the standard get_slopes(n)"""
    def pow2(m):
        start = 2.0 ** (-(2.0 ** -(math.log2(m) - 3)))
        return [start * start ** i for i in range(m)]
    if math.log2(n).is_integer():
        return pow2(n)
    c = 2 ** math.floor(math.log2(n))
    return pow2(c) + alibi_slopes(2 * c)[0::2][: n - c]


def alibi_bias(scale, E: int, T: int, dtype=torch.float64):
    """[H, S, S]: -slope_h max(scale_h, 0) |i - j| between frames, zero rows and columns for the E prefix tokens"""
    scale = scale.reshape(-1).to(dtype)
    H = scale.numel()
    pos = torch.arange(T, dtype=dtype)
    dist = (pos[:, None] - pos[None, :]).abs()
    sl = torch.tensor(alibi_slopes(H), dtype=dtype) * scale.clamp(min=0)
    b = torch.zeros(H, E + T, E + T, dtype=dtype)
    b[:, E:, E:] = -sl[:, None, None] * dist[None]
    return b


def attention(qkv, bias, H: int):
    """qkv [S, 3 D] (rows q | k | v, heads contiguous) -> [S, D]; bias [H, S, S] or None"""
    S, D3 = qkv.shape
    D = D3 // 3
    dk = D // H
    q, k, v = (qkv[:, i * D:(i + 1) * D].reshape(S, H, dk).transpose(0, 1) for i in range(3))
    s = (q * dk ** -0.5) @ k.transpose(1, 2)
    if bias is not None:
        s = s + bias
    return (torch.softmax(s, dim=-1) @ v).transpose(0, 1).reshape(S, D)


def block(x, sd, prefix: str, bias, H: int, taps=None):
    lin = lambda t, n: F.linear(t, sd[prefix + n + ".weight"], sd[prefix + n + ".bias"])
    ln = lambda t, n: layer_norm(t, sd[prefix + n + ".weight"], sd[prefix + n + ".bias"])
    qkv = lin(x, "attn.qkv")
    a = attention(qkv, bias, H)
    if taps is not None:
        taps["qkv"], taps["attn"] = qkv, a
    x = x + lin(a, "attn.proj")
    r = x = ln(x, "norm1")
    return ln(r + lin(gelu(lin(x, "mlp.fc1")), "mlp.fc2"), "norm2")


def forward(sd, wav, cfg=None, dtype=torch.float64, use_bias: bool = True, zero_extra: bool = False):
    """one clip [N] -> {"feats" [T, D], "emb" [D], "scores" [classes], "proj", "pos" (x + P(x)), "qkv", "attn" (first block)}"""
    cfg = emotion2vec_config(cfg)
    sd = cast(sd, dtype)
    x = normalize(torch.as_tensor(np.asarray(wav)).to(dtype).reshape(-1))
    out = {}
    out["proj"] = x = project(feature_extractor(x, sd, cfg), sd)
    out["pos"] = x = x + positional(x, sd, cfg)
    T, E, H = x.shape[0], cfg["E"], cfg["H"]
    extra = sd[up("extra_tokens")][0]
    x = torch.cat([torch.zeros_like(extra) if zero_extra else extra, x], dim=0)
    bias = alibi_bias(sd[up("alibi_scale")], E, T, dtype) if use_bias else None
    x = layer_norm(x, sd[up("prenet.norm.weight")], sd[up("prenet.norm.bias")])
    taps = {}
    prefixes = [up("prenet.blocks.{n}.", i) for i in range(cfg["prenet_depth"])] + [up("blocks.{n}.", i) for i in range(cfg["depth"])]
    for i, p in enumerate(prefixes):
        x = block(x, sd, p, bias, H, taps if i == 0 else None)
    out.update(taps)
    out["feats"] = x[E:]
    out["emb"] = out["feats"].mean(dim=0)
    out["scores"] = torch.softmax(F.linear(out["emb"], sd[up("head.weight")], sd[up("head.bias")]), dim=-1)
    return out
