"""ORACLE — test infrastructure, not product code.

CPU restatement (functional PyTorch, run in fp64 by the tests) of funasr's SenseVoiceSmall as the reference reaches it through
`self.asr['sensevoice'].generate(...)` (ASRProcessor.py:398-402).  funasr is THIRD-PARTY: un-vendored, not installed, no weights
in the reference tree => PARITY UNPINNED [upstream-recall].  Restated from the published code (SenseVoiceSmall.inference /
SenseVoiceEncoderSmall.forward / CTC.log_softmax):
  * the prompt: rows [embed(lid), embed(1), embed(2), embed(textnorm)] in front of the LFR features (embed = Embedding(16, 560));
  * the encoder entry on ALL rows: x * sqrt(512) + SinusoidalPositionEncoder (positions 1..T+4);
  * encoders0 (560 -> 512), encoders, after_norm, tp_encoders, tp_norm — the EncoderLayerSANM of oracle/paraformer_oracle.py,
    LayerNorm eps 1e-12;
  * ctc_lo + log_softmax; greedy decode: argmax per frame, unique_consecutive, drop blank (id 0) — over all T+4 frames, whose
    first four yield the language / emotion / event / text-norm tag tokens.
All sequences of a batch have equal length (no padding mask)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.paraformer_oracle import LN_EPS, _layer, sinusoidal_pe

LID = {"auto": 0, "zh": 3, "en": 4, "yue": 7, "ja": 11, "ko": 12, "nospeech": 13}
TEXTNORM = {"withitn": 14, "woitn": 15}


def prompt_rows(sd, language: str = "auto", use_itn: bool = True):
    """[4, 560]: language query, the event and emotion queries (ids 1, 2), the text-norm query"""
    ids = torch.tensor([LID.get(language, 0), 1, 2, TEXTNORM["withitn" if use_itn else "woitn"]])
    return sd["embed.weight"][ids]


def encoder_input(feats, sd, language="auto", use_itn=True):
    """feats [B,T,560] -> [B,T+4,560] after the scale and the position encoding"""
    B = feats.shape[0]
    x = torch.cat((prompt_rows(sd, language, use_itn)[None].expand(B, -1, -1).to(feats.dtype), feats), dim=1)
    return x * (512 ** 0.5) + sinusoidal_pe(x.shape[1], x.shape[2], feats.dtype)[None]


def encoder_forward(feats, sd, num_blocks: int, tp_blocks: int, language="auto", use_itn=True):
    """-> [B,T+4,512] (the tp_norm output)"""
    x = encoder_input(feats, sd, language, use_itn)
    x = _layer(x, sd, "encoder.encoders0.0.")
    for i in range(num_blocks - 1):
        x = _layer(x, sd, f"encoder.encoders.{i}.")
    x = F.layer_norm(x, (512,), sd["encoder.after_norm.weight"], sd["encoder.after_norm.bias"], LN_EPS)
    for i in range(tp_blocks):
        x = _layer(x, sd, f"encoder.tp_encoders.{i}.")
    return F.layer_norm(x, (512,), sd["encoder.tp_norm.weight"], sd["encoder.tp_norm.bias"], LN_EPS)


def ctc_log_probs(enc, sd):
    return torch.log_softmax(F.linear(enc, sd["ctc.ctc_lo.weight"], sd["ctc.ctc_lo.bias"]), dim=-1)


def collapse(ids, blank: int = 0):
    """one utterance's frame ids -> (kept ids, first frame of each kept run)"""
    keep = [i for i, t in enumerate(ids) if t != blank and (i == 0 or ids[i - 1] != t)]
    return [int(ids[i]) for i in keep], keep


def greedy_decode(feats, sd, num_blocks, tp_blocks, language="auto", use_itn=True):
    """-> (enc [B,S,512], log-probs [B,S,V], frame ids [B,S], per utterance (token ids, frames))"""
    enc = encoder_forward(feats, sd, num_blocks, tp_blocks, language, use_itn)
    lp = ctc_log_probs(enc, sd)
    ids = lp.argmax(-1)
    return enc, lp, ids, [collapse(row.tolist()) for row in ids]
