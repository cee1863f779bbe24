"""Shared fixtures of the SenseVoice tests (test infrastructure): the seeded random model, the inputs and the fp64 reference of
every (depth, B, T) case, each computed once per process.

V = 1031: odd, three 512-column slices of the fused head with 7 columns in the last.  The CTC weight is scaled by 4 so that the
top-2 log-prob gaps of a random model are wide (a gap below 1e-3 then has a probability of about 0.2 % per frame: the 1 % cap on
frames the margin rule may exclude holds with room), and the blank bias is raised until about half of the frames are blank.
The features hold every random frame for three steps, so that neighbouring frames often agree and the collapse has repeats to drop."""
from __future__ import annotations

import functools

import torch

import sensevoice_oracle as orc

VOCAB = 1031
CTC_SCALE = 4.0
BLANK_BIAS = {"small": 7.9, "full": 10.0}      # the median gap between the best word logit and the blank logit of each model
DEPTHS = {"small": (2, 1), "full": (50, 20)}
# rows (T + 4 per utterance): 11 (below one tile), 123 (no multiple of a tile), 298 (the largest of the split-K path's cases), and
# 596 (> 512 rows: the plain x3 path with the planes-out FFN)
SHAPES = [(1, 7), (3, 37), (2, 145), (4, 145)]
# 1212 rows, at the small depth only: above TDX_SV_LOGITS_ROWS = 1024 and no multiple of it, so the row-chunk head takes a second,
# shorter turn (plane, scale, id and score offsets; the one logits buffer reused), and 19 row tiles of the fused head, the last partial
LONG_SHAPE = (3, 400)
MARGIN = 1e-3


@functools.lru_cache(maxsize=None)
def state_dict(depth: str, vocab: int = VOCAB):
    from targetdiarization_amd.weights import recipe_sensevoice_state_dict
    nb, tp = DEPTHS[depth] if depth in DEPTHS else depth
    sd = recipe_sensevoice_state_dict(7, nb, tp, vocab)
    sd["ctc.ctc_lo.weight"] = sd["ctc.ctc_lo.weight"] * CTC_SCALE
    sd["ctc.ctc_lo.bias"][0] += BLANK_BIAS.get(depth, 7.9)
    return sd


def feats(B: int, T: int):
    g = torch.Generator().manual_seed(1000 * B + T)
    base = torch.randn(B, (T + 2) // 3, 560, generator=g)
    return (base.repeat_interleave(3, dim=1)[:, :T] + 0.05 * torch.randn(B, T, 560, generator=g)).contiguous()


@functools.lru_cache(maxsize=None)
def reference(depth: str, B: int, T: int):
    """fp64: {"enc" [B,S,512], "ids" [B,S], "top" [B,S] (log-prob at the argmax), "margin" [B,S] (top-1 minus top-2), "tokens"}"""
    nb, tp = DEPTHS[depth]
    sd64 = {k: v.double() for k, v in state_dict(depth).items()}
    enc, lp, ids, toks = orc.greedy_decode(feats(B, T).double(), sd64, nb, tp)
    top2 = lp.topk(2, dim=-1).values
    return {"enc": enc, "ids": ids, "top": top2[..., 0], "margin": top2[..., 0] - top2[..., 1], "tokens": toks}
