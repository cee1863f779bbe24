"""Plain torch / numpy restatement of Whisper's word-timestamp path (Hugging Face transformers' WhisperGenerationMixin.
_extract_token_timestamps, _median_filter, _dynamic_time_warping and the tokenizer's _combine_tokens_into_words), fp64 by default:
the cross-attention probabilities of listed heads from a teacher-forced pass, the token-axis normalisation, the median filter, the
head mean, the time warping in two rounding variants, the frame of every token row and the word grouping.
tests/test_whisper_timestamps_host.py pins every function here to the installed upstream; the GPU tests use only this file and
whisper_oracle.py.  The inputs of the alignment tests are made here too (align_case), so that the host test measures ALIGN_GAP on
exactly what the GPU test feeds."""
from __future__ import annotations

import numpy as np
import torch

import whisper_oracle as wo


# ---- cross-attention of listed heads
def cross_attention(sd, cfg, enc, ids, heads):
    """teacher forcing of ids int64 [B, L] over enc [B, S, d] -> softmax probabilities [B, len(heads), L, S] of the (layer, head)
    pairs `heads`: row p is what the step that feeds position p sees"""
    L = ids.shape[1]
    B, S, _ = enc.shape
    H = cfg["dec_heads"]
    x = sd["model.decoder.embed_tokens.weight"][ids] + sd["model.decoder.embed_positions.weight"][:L]
    probs = {}
    for l in range(cfg["dec_layers"]):
        p = f"model.decoder.layers.{l}."
        xn = wo._ln(x, sd, p + "self_attn_layer_norm")
        x = x + wo._attn(sd, p + "self_attn", xn, xn, H, causal=True)
        xn = wo._ln(x, sd, p + "encoder_attn_layer_norm")
        q = ((xn @ sd[p + "encoder_attn.q_proj.weight"].T + sd[p + "encoder_attn.q_proj.bias"]) * 0.125).view(B, L, H, 64).transpose(1, 2)
        k = (enc @ sd[p + "encoder_attn.k_proj.weight"].T).view(B, S, H, 64).transpose(1, 2)
        probs[l] = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
        x = x + wo._attn(sd, p + "encoder_attn", xn, enc, H)
        x = wo._ffn(sd, p, x)
    return torch.stack([probs[l][:, h] for l, h in heads], dim=1)


# ---- normalisation, median filter, head mean
def normalise(w, zero_std_to_zero=True):
    """(w - mean) / population std over the token axis (dim -2).  Upstream divides by a zero std (NaN); with zero_std_to_zero such a
    column is 0, the device's documented deviation"""
    std = torch.std(w, dim=-2, keepdim=True, unbiased=False)
    mean = torch.mean(w, dim=-2, keepdim=True)
    if zero_std_to_zero:
        return torch.where(std > 0, (w - mean) / torch.where(std > 0, std, torch.ones_like(std)), torch.zeros_like(w))
    return (w - mean) / std


def median_filter(x, width):
    """median of `width` (odd) along the last axis with reflect padding; unchanged when the axis is no longer than width // 2.
    A selection by compare-exchanges up to the middle element: the exact median, whatever the width"""
    pad = width // 2
    m = x.shape[-1]
    if width == 1 or m <= pad:
        return x
    idx = torch.arange(-pad, m + pad)
    idx = torch.where(idx < 0, -idx, idx)
    idx = torch.where(idx >= m, 2 * (m - 1) - idx, idx)
    xp = x[..., idx]
    v = [xp[..., t:t + m] for t in range(width)]
    for a in range(pad + 1):
        for c in range(a + 1, width):
            v[a], v[c] = torch.minimum(v[a], v[c]), torch.maximum(v[a], v[c])
    return v[pad]


def matrix(w, width=7):
    """w [nh, n, m] (one clip, already cropped to its rows and frames) -> M [n, m]"""
    return median_filter(normalise(w), width).mean(dim=0)


# ---- dynamic time warping
def dtw(neg, mode="fp32"):
    """transformers' _dynamic_time_warping on neg = -M (n x m) -> (text_indices, time_indices), walking anti-diagonals.
    mode "double": upstream's arithmetic, the matrix in fp64, cost[i][j] = float32(neg64 + float64(min));
    mode "fp32": the device's, neg rounded to fp32 first and one fp32 addition."""
    neg = np.asarray(neg, dtype=np.float64)
    n, m = neg.shape
    a = neg.astype(np.float32) if mode == "fp32" else neg
    trace = np.full((n + 1, m + 1), -1, dtype=np.int8)
    inf = np.float32(np.inf)
    d2 = np.full(n + 1, inf, dtype=np.float32); d2[0] = 0          # diagonal 0: the origin
    d1 = np.full(n + 1, inf, dtype=np.float32)                     # diagonal 1: two border cells
    for k in range(2, n + m + 1):
        lo, hi = max(1, k - m), min(n, k - 1)
        i = np.arange(lo, hi + 1)
        c0, c1, c2 = d2[i - 1], d1[i - 1], d1[i]
        t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2)).astype(np.int8)
        c = np.where(t == 0, c0, np.where(t == 1, c1, c2))
        cur = np.full(n + 1, inf, dtype=np.float32)
        with np.errstate(invalid="ignore"):
            cur[i] = (a[i - 1, k - i - 1] + (c if mode == "fp32" else c.astype(np.float64))).astype(np.float32)
        trace[i, k - i] = t
        d2, d1 = d1, cur
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j, ti, tj = n, m, [], []
    while i > 0 or j > 0:
        ti.append(i - 1); tj.append(j - 1)
        if trace[i, j] == 0:
            i -= 1; j -= 1
        elif trace[i, j] == 1:
            i -= 1
        else:
            j -= 1
    return np.array(ti)[::-1], np.array(tj)[::-1]


def jump_frames(text_indices, time_indices):
    """the frame at which the path first enters every token row (upstream's time_indices[jumps])"""
    jumps = np.pad(np.diff(text_indices), (1, 0), constant_values=1).astype(bool)
    return time_indices[jumps]


def token_frames(M, mode="fp32"):
    """M [n, m] (torch or numpy) -> int64 [n].  One row: 0 (upstream divides by a zero std there; its NaN path ends at 0 too)"""
    M = M.detach().cpu().numpy() if isinstance(M, torch.Tensor) else np.asarray(M)
    if M.shape[0] == 1:
        return np.zeros(1, dtype=np.int64)
    return jump_frames(*dtw(-M.astype(np.float64), mode)).astype(np.int64)


def token_times(frames, n_generated, precision=0.02):
    """upstream's timestamps of the generated ids: the frames of the n - 1 tokens that were fed back, the last id repeating"""
    if n_generated <= 1 or len(frames) == 0:
        return [0.0] * n_generated
    t = [float(f) * precision for f in frames]
    return t + [t[-1]]


# ---- the inputs of the alignment tests
# (rows, frames, heads, seed): rows = 1, rows > frames, frames <= 3 (no filter), more rows than one wave, the largest shape of the
# product (n_text_ctx - 1 rows over 1500 frames)
ALIGN_CASES = ((1, 50, 1, 0), (2, 4, 3, 0), (7, 3, 10, 0), (23, 100, 1, 0), (23, 100, 10, 0), (300, 37, 3, 0), (300, 37, 10, 0), (447, 1500, 3, 0))
# one call that mixes clips: (rows, frames) per clip in a buffer of 32 rows x 100 frames, 3 heads
ALIGN_MIXED = ((23, 100), (2, 4), (0, 10), (7, 3), (1, 50), (32, 61))
ALIGN_MIXED_ROWS, ALIGN_MIXED_FRAMES, ALIGN_MIXED_HEADS = 32, 100, 3


def align_case(rows, frames, nh, seed):
    """attention-like input float32 [nh, rows, frames]: a Gaussian bump per token on a monotone token-to-frame ramp (every head
    with its own small shift and width), plus 5 % uniform noise, every row normalised to sum 1"""
    g = torch.Generator().manual_seed(1000 * rows + frames + 17 * nh + 100003 * seed)
    j = torch.arange(frames, dtype=torch.float64)[None, None, :]
    centre = ((torch.arange(rows, dtype=torch.float64) + 0.5) * frames / max(rows, 1))[None, :, None]
    shift = (torch.rand(nh, 1, 1, generator=g, dtype=torch.float64) - 0.5) * 2.0
    sigma = max(1.5, 0.5 * frames / max(rows, 1)) * (1.0 + 0.5 * torch.rand(nh, 1, 1, generator=g, dtype=torch.float64))
    w = torch.exp(-0.5 * ((j - centre - shift) / sigma) ** 2) + 0.05 * torch.rand(nh, rows, frames, generator=g, dtype=torch.float64)
    return (w / w.sum(dim=-1, keepdim=True)).float()


# the fp32-vs-fp64 gap of matrix() on align_case(*case): max |M32 - M64|, measured and held to within a factor of 2 by
# tests/test_whisper_timestamps_host.py::test_align_fp32_gap; the GPU test's bar on matrix_dev is 10 x this.  One row: no matrix.
ALIGN_GAP = {(2, 4, 3, 0): 3.0e-7, (7, 3, 10, 0): 8.4e-7, (23, 100, 1, 0): 2.9e-7, (23, 100, 10, 0): 5.0e-7, (300, 37, 3, 0): 3.8e-7,
             (300, 37, 10, 0): 3.7e-7, (447, 1500, 3, 0): 1.9e-6}
ALIGN_MIXED_SEED = 1                                    # clip (rows, frames) of the mixed call is align_case(rows, frames, 3, 1)
ALIGN_MIXED_GAP = {(23, 100): 4.6e-7, (2, 4): 5.4e-7, (7, 3): 1.1e-6, (32, 61): 2.7e-7}


def matrix_gap(w32, width=7):
    return float((matrix(w32, width).double() - matrix(w32.double(), width)).abs().max())


# ---- word grouping (transformers' tokenization_whisper._combine_tokens_into_words)
UNSPACED = ("chinese", "japanese", "thai", "lao", "myanmar", "cantonese")
PUNCT = "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"


def group_words(ids, decode, language, eos, prepend="\"'“¡¿([{-", append="\"'.。,，!！?？:：”)]}、"):
    """ids -> (words, ids per word, indices per word); decode(list of ids) -> str with U+FFFD for incomplete UTF-8"""
    full = decode(ids)
    sub, cur, off = [], [], 0
    for k, t in enumerate(ids):
        cur.append(k)
        dec = decode([ids[i] for i in cur])
        at = dec.find("�")
        if at < 0 or off + at >= len(full) or full[off + at] == "�":
            sub.append((dec, cur)); cur = []; off += len(dec)
    if language in UNSPACED:
        words = [[w, list(ix)] for w, ix in sub]
    else:
        words = []
        for w, ix in sub:
            if ids[ix[0]] >= eos or w.startswith(" ") or w.strip() in PUNCT or not words:
                words.append([w, list(ix)])
            else:
                words[-1][0] += w; words[-1][1] += ix
    i, j = len(words) - 2, len(words) - 1
    while i >= 0:
        if words[i][0].startswith(" ") and words[i][0].strip() in prepend:
            words[j] = [words[i][0] + words[j][0], words[i][1] + words[j][1]]; words[i] = ["", []]
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(words):
        if not words[i][0].endswith(" ") and words[j][0] in append:
            words[i] = [words[i][0] + words[j][0], words[i][1] + words[j][1]]; words[j] = ["", []]
        else:
            i = j
        j += 1
    text = [w for w, _ in words if w]
    idx = [ix for _, ix in words if ix]
    return text, [[ids[k] for k in ix] for ix in idx], idx
