"""Plain-torch restatement of Whisper (Hugging Face transformers' WhisperFeatureExtractor and WhisperForConditionalGeneration) in
a chosen precision, fp64 by default: the log-mel front end, the encoder, one decoder forward over given ids, and a greedy loop
with the suppression rules of `generate`.  tests/test_whisper_host.py pins every function here to the installed upstream; the
GPU tests use only this file.  `cfg` is targetdiarization_amd.weights.whisper_config's dict, `sd` a state dict in upstream's names."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

EPS = 1e-5


def mel_filters(n_mels: int, dtype=torch.float64) -> torch.Tensor:
    """Slaney-scale, Slaney-normalised bank [n_mels, 201] over 0..8000 Hz (transformers.audio_utils.mel_filter_bank)"""
    def hz_to_mel(f):
        return 3.0 * f / 200.0 if f < 1000.0 else 15.0 + math.log(f / 1000.0) * 27.0 / math.log(6.4)

    def mel_to_hz(m):
        return 200.0 * m / 3.0 if m < 15.0 else 1000.0 * math.exp(math.log(6.4) / 27.0 * (m - 15.0))
    m0, m1 = hz_to_mel(0.0), hz_to_mel(8000.0)
    ff = torch.tensor([mel_to_hz(m0 + (m1 - m0) * i / (n_mels + 1)) for i in range(n_mels + 2)], dtype=torch.float64)
    f = torch.linspace(0, 8000, 201, dtype=torch.float64)
    down = (f[None, :] - ff[:-2, None]) / (ff[1:-1] - ff[:-2])[:, None]
    up = (ff[2:, None] - f[None, :]) / (ff[2:] - ff[1:-1])[:, None]
    fb = torch.clamp(torch.minimum(down, up), min=0.0) * (2.0 / (ff[2:] - ff[:-2]))[:, None]
    return fb.to(dtype)


def logmel(clips, n_mels: int, n_audio_ctx: int, dtype=torch.float64) -> torch.Tensor:
    """list of 1-D clips -> [B, n_mels, 2 n_audio_ctx]"""
    P = 320 * n_audio_ctx
    out = []
    win = torch.hann_window(400, periodic=True, dtype=dtype)
    fb = mel_filters(n_mels, dtype)
    for c in clips:
        x = torch.zeros(P, dtype=dtype)
        c = torch.as_tensor(c).reshape(-1)[:P].to(dtype)
        x[: c.shape[0]] = c
        spec = torch.stft(x, 400, 160, window=win, center=True, pad_mode="reflect", return_complex=True)[:, :-1]
        power = spec.real ** 2 + spec.imag ** 2
        lm = torch.log10(torch.clamp(fb @ power, min=1e-10))
        lm = torch.maximum(lm, lm.max() - 8.0)
        out.append((lm + 4.0) / 4.0)
    return torch.stack(out)


# the fp32-vs-fp64 gap of logmel() on logmel_test_clips, by frames of context: measured and held to within 20 % by
# tests/test_whisper_host.py::test_logmel_fp32_gap; the GPU test's bar is 10 x this
LOGMEL_GAP = {1500: 1.1e-4, 100: 1.1e-5}


def logmel_test_clips(n_audio_ctx: int):
    """noise and a sine at 0.5 s, 3.3 s, exactly the window and a second more, then half a second of silence"""
    P = 320 * n_audio_ctx
    g = torch.Generator().manual_seed(5)
    out = []
    for n in (8000, 52800, P, P + 16000):
        out.append(0.1 * torch.randn(n, generator=g))
        out.append(0.5 * torch.sin(2 * math.pi * 440.0 * torch.arange(n) / 16000.0))
    out.append(torch.zeros(8000))
    return out


def cast(sd, dtype=torch.float64):
    return {k: v.detach().cpu().to(dtype) for k, v in sd.items()}


def _ln(x, sd, p):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], EPS)


def _attn(sd, p, xq, xkv, heads, causal=False, kv=None):
    B, Lq, d = xq.shape
    q = (xq @ sd[p + ".q_proj.weight"].T + sd[p + ".q_proj.bias"]) * 0.125
    if kv is None:
        k = xkv @ sd[p + ".k_proj.weight"].T
        v = xkv @ sd[p + ".v_proj.weight"].T + sd[p + ".v_proj.bias"]
    else:
        k, v = kv
    Lk = k.shape[1]
    q = q.view(B, Lq, heads, 64).transpose(1, 2)
    k = k.view(B, Lk, heads, 64).transpose(1, 2)
    v = v.view(B, Lk, heads, 64).transpose(1, 2)
    s = q @ k.transpose(-1, -2)
    if causal:
        s = s + torch.full((Lq, Lk), float("-inf"), dtype=s.dtype).triu(1)
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, Lq, d)
    return o @ sd[p + ".out_proj.weight"].T + sd[p + ".out_proj.bias"]


def _ffn(sd, p, x):
    h = F.gelu(_ln(x, sd, p + "final_layer_norm") @ sd[p + "fc1.weight"].T + sd[p + "fc1.bias"])
    return x + h @ sd[p + "fc2.weight"].T + sd[p + "fc2.bias"]


def encoder(sd, cfg, feats):
    """feats [B, n_mels, 2 S] -> [B, S, d]; sd and feats in one dtype"""
    x = F.gelu(F.conv1d(feats, sd["model.encoder.conv1.weight"], sd["model.encoder.conv1.bias"], padding=1))
    x = F.gelu(F.conv1d(x, sd["model.encoder.conv2.weight"], sd["model.encoder.conv2.bias"], stride=2, padding=1))
    x = x.transpose(1, 2) + sd["model.encoder.embed_positions.weight"]
    for l in range(cfg["enc_layers"]):
        p = f"model.encoder.layers.{l}."
        xn = _ln(x, sd, p + "self_attn_layer_norm")
        x = x + _attn(sd, p + "self_attn", xn, xn, cfg["enc_heads"])
        x = _ffn(sd, p, x)
    return _ln(x, sd, "model.encoder.layer_norm")


def cross_kv(sd, cfg, enc):
    """[dec_layers, 2, B, S, d]"""
    out = []
    for l in range(cfg["dec_layers"]):
        p = f"model.decoder.layers.{l}.encoder_attn"
        out.append(torch.stack([enc @ sd[p + ".k_proj.weight"].T, enc @ sd[p + ".v_proj.weight"].T + sd[p + ".v_proj.bias"]]))
    return torch.stack(out)


def decoder_hidden(sd, cfg, enc, ids):
    """ids int64 [B, L] -> the decoder's final LayerNorm output [B, L, d] (teacher forcing, causal)"""
    L = ids.shape[1]
    x = sd["model.decoder.embed_tokens.weight"][ids] + sd["model.decoder.embed_positions.weight"][:L]
    for l in range(cfg["dec_layers"]):
        p = f"model.decoder.layers.{l}."
        xn = _ln(x, sd, p + "self_attn_layer_norm")
        x = x + _attn(sd, p + "self_attn", xn, xn, cfg["dec_heads"], causal=True)
        x = x + _attn(sd, p + "encoder_attn", _ln(x, sd, p + "encoder_attn_layer_norm"), enc, cfg["dec_heads"])
        x = _ffn(sd, p, x)
    return _ln(x, sd, "model.decoder.layer_norm")


def decoder_logits(sd, cfg, enc, ids):
    return decoder_hidden(sd, cfg, enc, ids) @ sd["model.decoder.embed_tokens.weight"].T


def _top(logits, deny):
    """logits [..., V], deny bool [V] -> (argmax over the allowed ids, its log-softmax, the margin to the runner-up)"""
    lg = logits.masked_fill(deny, float("-inf"))
    top2 = lg.topk(2, dim=-1)
    return top2.indices[..., 0], top2.values[..., 0] - torch.logsumexp(lg, dim=-1), top2.values[..., 0] - top2.values[..., 1]


def _deny(V, ids):
    m = torch.zeros(V, dtype=torch.bool)
    if len(ids):
        m[torch.as_tensor(list(ids), dtype=torch.long)] = True
    return m


def step_outputs(sd, cfg, enc, ids, prefix_len, suppress=(), begin_suppress=()):
    """what the decode steps write when the tokens `ids` [B, L] are fed: per position p (ids, log-probs, margins) [B, L];
    `suppress` is masked everywhere, `begin_suppress` at p = prefix_len - 1 as well"""
    V = cfg["vocab"]
    out = [[], [], []]
    for b in range(ids.shape[0]):                          # a clip at a time: [L, V] logits
        lg = decoder_logits(sd, cfg, enc[b:b + 1], ids[b:b + 1])[0]
        i, s, m = _top(lg, _deny(V, suppress))
        p = prefix_len - 1
        if len(begin_suppress) and p < lg.shape[0]:
            i[p], s[p], m[p] = _top(lg[p], _deny(V, list(suppress) + list(begin_suppress)))
        for o, v in zip(out, (i, s, m)):
            o.append(v)
    return [torch.stack(o) for o in out]


def greedy(sd, cfg, enc, prefix, max_new, suppress=(), begin_suppress=(), eos=50257):
    """Greedy decoding of every clip of enc [B, S, d] under the common prefix.  Returns per clip a dict: "tokens" (the generated
    ids, a final eos included), "scores" (their log-probabilities), "margins" (top-2 margins of those steps)."""
    V, T = cfg["vocab"], cfg["n_text_ctx"]
    room = max(0, min(max_new, T - len(prefix)))
    d_all, d_begin = _deny(V, suppress), _deny(V, list(suppress) + list(begin_suppress))
    res = []
    for b in range(enc.shape[0]):
        ids = list(prefix)
        r = {"tokens": [], "scores": [], "margins": []}
        for n in range(room):
            h = decoder_hidden(sd, cfg, enc[b:b + 1], torch.tensor([ids]))[0, -1]
            i, s, m = _top(h @ sd["model.decoder.embed_tokens.weight"].T, d_begin if n == 0 else d_all)
            r["tokens"].append(int(i)); r["scores"].append(float(s)); r["margins"].append(float(m))
            ids.append(int(i))
            if int(i) == eos:
                break
        res.append(r)
    return res
