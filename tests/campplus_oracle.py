"""Functional PyTorch restatement of CAM++ (3D-Speaker speakerlab/models/campplus/{DTDNN,layers}.py) [upstream-recall:
the source is not vendored, parity with the published checkpoint is unpinned] — the reference the device forward
(csrc/campplus.hip) is compared against, in fp64 by default — plus the seeded synthetic voices and conversations the
diarizer tests use.  Every BatchNorm is eval-mode with eps 1e-5."""
from __future__ import annotations

import json
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as Fn

from oracle import frontend_oracle as fo
from targetdiarization_amd.weights import recipe_campplus_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
CALIBRATION = os.path.join(HERE, "golden", "campplus_calibration.json")
SR = 16000
LAYERS, DILATION = (12, 24, 16), (1, 2, 2)


def _bn(x, sd, p, affine=True):
    shape = [1, -1] + [1] * (x.ndim - 2)
    y = (x - sd[p + "running_mean"].view(shape)) / torch.sqrt(sd[p + "running_var"].view(shape) + 1e-5)
    if affine:
        y = y * sd[p + "weight"].view(shape) + sd[p + "bias"].view(shape)
    return y


def seg_pooling(x, seg_len=100):
    """[B,C,T] -> [B,C,T]: mean over consecutive seg_len-frame segments (the last, shorter one over its own length),
    repeated over the segment's frames (avg_pool1d(ceil_mode=True) + expand)."""
    T = x.shape[-1]
    out = torch.empty_like(x)
    for t0 in range(0, T, seg_len):
        out[..., t0:t0 + seg_len] = x[..., t0:t0 + seg_len].mean(dim=-1, keepdim=True)
    return out


def _res_block(x, sd, p, stride):
    out = torch.relu(_bn(Fn.conv2d(x, sd[p + "conv1.weight"], stride=(stride, 1), padding=1), sd, p + "bn1."))
    out = _bn(Fn.conv2d(out, sd[p + "conv2.weight"], padding=1), sd, p + "bn2.")
    sc = x
    if stride != 1:
        sc = _bn(Fn.conv2d(x, sd[p + "shortcut.0.weight"], stride=(stride, 1)), sd, p + "shortcut.1.")
    return torch.relu(out + sc)


def forward(sd, feat, dtype=torch.float64, pre_bn=False):
    """feat [B,F,80] -> [B,192] (pre_bn: the dense layer's output before its affine-free BatchNorm)."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x = feat.to(dtype).permute(0, 2, 1).unsqueeze(1)                     # [B,1,80,F]
    x = torch.relu(_bn(Fn.conv2d(x, sd["head.conv1.weight"], padding=1), sd, "head.bn1."))
    for li in (1, 2):
        x = _res_block(x, sd, f"head.layer{li}.0.", 2)
        x = _res_block(x, sd, f"head.layer{li}.1.", 1)
    x = torch.relu(_bn(Fn.conv2d(x, sd["head.conv2.weight"], stride=(2, 1), padding=1), sd, "head.bn2."))
    x = x.reshape(x.shape[0], x.shape[1] * x.shape[2], x.shape[3])      # [B, 320 (c*10 + f), F]
    x = torch.relu(_bn(Fn.conv1d(x, sd["xvector.tdnn.linear.weight"], stride=2, padding=2), sd, "xvector.tdnn.nonlinear.batchnorm."))
    for bi, (nl, dil) in enumerate(zip(LAYERS, DILATION), start=1):
        for i in range(nl):
            p = f"xvector.block{bi}.tdnnd{i + 1}."
            h = torch.relu(_bn(x, sd, p + "nonlinear1.batchnorm."))
            h = torch.relu(_bn(Fn.conv1d(h, sd[p + "linear1.weight"]), sd, p + "nonlinear2.batchnorm."))
            y = Fn.conv1d(h, sd[p + "cam_layer.linear_local.weight"], padding=dil, dilation=dil)
            ctx = h.mean(dim=-1, keepdim=True) + seg_pooling(h)
            ctx = torch.relu(Fn.conv1d(ctx, sd[p + "cam_layer.linear1.weight"], sd[p + "cam_layer.linear1.bias"]))
            m = torch.sigmoid(Fn.conv1d(ctx, sd[p + "cam_layer.linear2.weight"], sd[p + "cam_layer.linear2.bias"]))
            x = torch.cat([x, y * m], dim=1)
        p = f"xvector.transit{bi}."
        x = Fn.conv1d(torch.relu(_bn(x, sd, p + "nonlinear.batchnorm.")), sd[p + "linear.weight"])
    x = torch.relu(_bn(x, sd, "xvector.out_nonlinear.batchnorm."))
    stats = torch.cat([x.mean(dim=-1), x.std(dim=-1, unbiased=True)], dim=-1)       # [B,1024]
    e = Fn.conv1d(stats.unsqueeze(-1), sd["xvector.dense.linear.weight"])
    if not pre_bn:
        e = _bn(e, sd, "xvector.dense.nonlinear.batchnorm.", affine=False)
    return e.squeeze(-1)


def calibrated_state_dict(seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Recipe weights with the final BatchNorm's running statistics taken from tests/golden/campplus_calibration.json
    (tools/make_goldens_campplus.py): with the plain recipe statistics every input lands on nearly the same embedding."""
    sd = recipe_campplus_state_dict(seed)
    with open(CALIBRATION) as f:
        cal = json.load(f)
    assert cal["seed"] == seed
    sd["xvector.dense.nonlinear.batchnorm.running_mean"] = torch.tensor(cal["running_mean"], dtype=torch.float64).to(torch.float32)
    sd["xvector.dense.nonlinear.batchnorm.running_var"] = torch.tensor(cal["running_var"], dtype=torch.float64).to(torch.float32)
    return sd


def oracle_embedder(sd, dtype=torch.float64, batch=16):
    """embed(list of equal-length 1-D waveforms) -> [n,192] float64 array: Fbank("sv") oracle chained with forward()."""
    def embed(windows):
        out = []
        for c in range(0, len(windows), batch):
            feats = torch.stack([fo.sv_features(torch.as_tensor(np.asarray(w), dtype=dtype)) for w in windows[c:c + batch]])
            out.append(forward(sd, feats, dtype).to(torch.float64).numpy())
        return np.concatenate(out) if out else np.zeros((0, 192))
    return embed


# ------------------------------------------------------------------------------------------------------------
# synthetic voices: a harmonic source with its own f0 and three formant bumps, slow vibrato and amplitude
# modulation, a little noise
# ------------------------------------------------------------------------------------------------------------
VOICES = {
    0: dict(f0=105.0, formants=((650.0, 90.0), (1100.0, 110.0), (2500.0, 160.0)), vib=5.0, am=3.1),
    1: dict(f0=215.0, formants=((320.0, 70.0), (2300.0, 150.0), (3100.0, 200.0)), vib=6.2, am=2.3),
    2: dict(f0=150.0, formants=((480.0, 80.0), (1650.0, 130.0), (3500.0, 220.0)), vib=4.1, am=4.0),
}


def voice(vid: int, n: int, rng: np.random.Generator, amp: float = 0.1) -> np.ndarray:
    """n samples of voice `vid` at 16 kHz; phases, vibrato phase and the noise come from rng."""
    v = VOICES[vid]
    t = np.arange(n) / SR
    f0 = v["f0"] * (1.0 + 0.02 * np.sin(2 * np.pi * v["vib"] * t + rng.uniform(0, 2 * np.pi)))
    phase = 2 * np.pi * np.cumsum(f0) / SR
    x = np.zeros(n)
    for k in range(1, int(3800.0 / v["f0"]) + 1):
        fk = k * v["f0"]
        g = 0.02 + sum(np.exp(-0.5 * ((fk - fc) / bw) ** 2) for fc, bw in v["formants"])
        x += g / np.sqrt(k) * np.sin(k * phase + rng.uniform(0, 2 * np.pi))
    x *= 1.0 + 0.3 * np.sin(2 * np.pi * v["am"] * t + rng.uniform(0, 2 * np.pi))
    x = x / np.max(np.abs(x)) * amp
    return (x + 0.002 * rng.standard_normal(n)).astype(np.float32)


# (voice, seconds) turns; every turn is 3-10 s
CONVERSATIONS = {
    "three": dict(seed=11, turns=((0, 6.0), (1, 4.5), (2, 7.5), (0, 3.75), (1, 6.0), (2, 4.5), (0, 7.5))),      # 39.75 s
    "two": dict(seed=12, turns=((0, 6.0), (1, 7.5), (0, 4.5), (1, 9.0), (0, 6.0))),                             # 33.0 s
}


def conversation(name: str):
    """-> (audio float32, turns [(start_sample, end_sample, voice)])"""
    c = CONVERSATIONS[name]
    rng = np.random.default_rng(c["seed"])
    parts, turns, pos = [], [], 0
    for vid, sec in c["turns"]:
        n = int(round(sec * SR))
        parts.append(voice(vid, n, rng))
        turns.append((pos, pos + n, vid))
        pos += n
    return np.concatenate(parts), turns


def pure_window_truth(windows, turns):
    """per window [st, ed) in samples: the voice whose turn contains it wholly, or -1 for a window that straddles a change"""
    out = []
    for st, ed in windows:
        lab = -1
        for a, b, vid in turns:
            if st >= a and ed <= b:
                lab = vid
        out.append(lab)
    return np.array(out)


def consistent_up_to_permutation(labels, truth) -> bool:
    """over the windows with truth >= 0: labels and truth induce the same partition"""
    keep = truth >= 0
    l, t = np.asarray(labels)[keep], truth[keep]
    pairs = set(zip(l.tolist(), t.tolist()))
    return len(pairs) == len(set(l.tolist())) == len(set(t.tolist()))
