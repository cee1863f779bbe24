"""Apollo band-split RoFormer restorer (look2hear/models/apollo.py) restated in plain torch, for the tests.

Independent of the reference's text: token layout [clip, frame, band, 256] (the device layout), the STFT / iSTFT as framed
rfft / irfft with an explicit reflect pad, window envelope and C2R synthesis.  The dtype of the state dict decides the
arithmetic: float64 for the oracle, float32 to compare with the reference's float32 run.  (The reference's RMSNorm casts to
float32 whatever the model dtype; the oracle does not, and its float64 pin runs the reference with that cast made an identity.)
Pinned against the reference by tools/make_goldens_apollo.py.

Imported by the tests as a sibling module (tests/ has no __init__.py).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

SR, NFFT, HOP, NBIN = 44100, 882, 441, 442
BANDS = [5] * 79 + [47]
EPS = float(torch.finfo(torch.float32).eps)


def frames_of(n: int) -> int:
    return 1 + n // HOP


def _window(dtype):
    k = torch.arange(NFFT, dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(2.0 * math.pi * k / NFFT)).to(dtype)       # periodic hann


def _rms(x, g, eps=1e-5):
    """RMSNorm over the last axis, times the gain"""
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * g


def _w(t):
    return t.reshape(t.shape[0], -1)                                            # Conv1d k=1 weight [out, in, 1] -> [out, in]


def stft(x):
    """x [N, n] -> complex [N, T, 442]"""
    xp = F.pad(x.unsqueeze(1), (NFFT // 2, NFFT // 2), mode="reflect").squeeze(1)
    fr = xp.unfold(-1, NFFT, HOP) * _window(x.dtype)
    return torch.fft.rfft(fr, dim=-1)


def istft(spec, n: int):
    """complex [N, T, 442] -> [N, n] (C2R frames, windowed overlap-add divided by the squared-window envelope, center trim)"""
    N, T, _ = spec.shape
    w = _window(spec.real.dtype)
    fr = torch.fft.irfft(spec, n=NFFT, dim=-1) * w                               # [N, T, 882]
    L = (T - 1) * HOP + NFFT
    y = torch.zeros(N, L, dtype=fr.dtype)
    env = torch.zeros(L, dtype=fr.dtype)
    for t in range(T):
        y[:, t * HOP:t * HOP + NFFT] += fr[:, t]
        env[t * HOP:t * HOP + NFFT] += w * w
    return (y / env)[:, NFFT // 2:NFFT // 2 + n]


def band_features(spec, sd):
    """complex [N, T, 442] -> tokens [N, T, 80, 256]"""
    out, b0 = [], 0
    for i, bw in enumerate(BANDS):
        s = spec[..., b0:b0 + bw]
        p = torch.sqrt((s.real ** 2 + s.imag ** 2).sum(-1, keepdim=True) + EPS)
        f = torch.cat([s.real / p, s.imag / p, torch.log(p)], -1)                # [N, T, 2bw+1]
        f = _rms(f, sd[f"BN.{i}.0.weight"])
        out.append(f @ _w(sd[f"BN.{i}.1.weight"]).t() + sd[f"BN.{i}.1.bias"])
        b0 += bw
    return torch.stack(out, 2)


def _rope(x, cos, sin):
    """x [..., P, 32]: pairs (x0, x1) -> (x0 c - x1 s, x1 c + x0 s), tables [P, 32]"""
    xr = torch.stack([-x[..., 1::2], x[..., 0::2]], -1).reshape(x.shape)
    return x * cos + xr * sin


def band_roformer(x, sd, p):
    """attention across the 80 bands of every frame; x [N, T, 80, 256]"""
    N, T, P, D = x.shape
    qkv = _rms(x, sd[p + "input_norm.weight"]) @ _w(sd[p + "weight.weight"]).t()          # [N, T, P, 768]
    qkv = qkv.reshape(N, T, P, 8, 96).permute(0, 1, 3, 2, 4)                              # head-interleaved q | k | v
    cos, sin = sd[p + "cos_freq"][:P], sd[p + "sin_freq"][:P]
    q, k, v = _rope(qkv[..., :32], cos, sin), _rope(qkv[..., 32:64], cos, sin), qkv[..., 64:]
    a = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(32.0), -1) @ v                 # [N, T, 8, P, 32]
    x = x + a.permute(0, 1, 3, 2, 4).reshape(N, T, P, D) @ _w(sd[p + "output.weight"]).t()
    h = F.silu(_rms(x, sd[p + "MLP.0.weight"]) @ _w(sd[p + "MLP.1.weight"]).t())
    gate, z = h[..., :4 * D], h[..., 4 * D:]
    return x + (F.silu(gate) * z) @ _w(sd[p + "MLP_output.weight"]).t()


def seq_icb(x, sd, p):
    """three ConvActNorm1d blocks along the frames of every (clip, band); x [N, T, 80, 256]"""
    N, T, P, D = x.shape
    for b in range(3):
        q = f"{p}blocks.{b}.conv."
        w = sd[q + "0.weight"][:, 0, :]                                                   # [256, 7]
        xp = F.pad(x, (0, 0, 0, 0, 3, 3))                                                 # zero pad the frame axis
        y = sum(xp[:, j:j + T] * w[:, j] for j in range(7)) + sd[q + "0.bias"]
        y = _rms(y, sd[q + "1.weight"])
        y = F.silu(y @ _w(sd[q + "2.weight"]).t() + sd[q + "2.bias"])
        x = x + y @ _w(sd[q + "4.weight"]).t() + sd[q + "4.bias"]
    return x


def heads(x, sd):
    """tokens [N, T, 80, 256] -> complex spectrum [N, T, 442]"""
    out = []
    for i, bw in enumerate(BANDS):
        h = _rms(x[:, :, i], sd[f"output.{i}.0.weight"]) @ _w(sd[f"output.{i}.1.weight"]).t() + sd[f"output.{i}.1.bias"]
        g = h[..., :2 * bw] * torch.sigmoid(h[..., 2 * bw:])
        out.append(torch.complex(g[..., :bw], g[..., bw:]))
    return torch.cat(out, -1)


def apollo_forward(x, sd, num_layers: int | None = None, taps: dict | None = None):
    """x [N, n] (clips as batch items, n >= 442) -> [N, n].  `taps`: filled with "features", "net.{l}" and "spec"."""
    n = x.shape[-1]
    if num_layers is None:
        num_layers = sum(1 for k in sd if k.endswith("band_net.cos_freq"))
    h = band_features(stft(x), sd)
    if taps is not None:
        taps["features"] = h
    for l in range(num_layers):
        h = seq_icb(band_roformer(h, sd, f"net.{l}.band_net."), sd, f"net.{l}.seq_net.")
        if taps is not None:
            taps[f"net.{l}"] = h
    spec = heads(h, sd)
    if taps is not None:
        taps["spec"] = spec
    return istft(spec, n)


def cast_state_dict(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}
