"""The configurations and fp64 oracle results that tests/test_gpu_whisper_widths.py (device) and tests/test_whisper_host.py (the
oracle-only conditions, where no device is present) share.  Nothing here touches a device.

    W  d 1280, 20 heads, 1 + 1 layers, 128 mels, 100 audio positions: the large-v3 width; K = 1280 and 5120 in every skinny, MFMA,
       head, LayerNorm and encoder GEMM path
    V  d 320, 5 heads, 1 + 2 layers, 80 mels, 100 positions: the GEMM width pads 320 -> 384; a second `k += 256` trip with a partial
       wave; fc2 at K = 1280, the smallest K that takes the skinny loop round twice
    L  d 64, 1 head, 1 + 1 layers, 80 mels, 4160 positions: the smallest model create accepts, more positions than the alignment
       softmax keeps in LDS (4096), 17 key chunks of the single-query attention, 65 query tiles of the encoder's

The vocabulary 1031 = 16 * 64 + 7 gives 17 head slices, the last with 7 columns, 3 mod 4.  Recipe weights of seed 1, features
0.5 * randn of generator seed 11, a teacher-forced prefix of 64 ids below the vocabulary from seed 21.  Results are computed once per
process and never changed."""
import functools

import torch

import whisper_oracle as wo
import whisper_ts_oracle as ts
from targetdiarization_amd.weights import recipe_whisper_state_dict, whisper_config

VOCAB = 1031
CFGS = {"W": dict(d_model=1280, enc_heads=20, enc_layers=1, dec_layers=1, n_mels=128, vocab=VOCAB, n_audio_ctx=100),
        "V": dict(d_model=320, enc_heads=5, enc_layers=1, dec_layers=2, n_mels=80, vocab=VOCAB, n_audio_ctx=100),
        "L": dict(d_model=64, enc_heads=1, enc_layers=1, dec_layers=1, n_mels=80, vocab=VOCAB, n_audio_ctx=4160)}
NCLIPS = {"W": 12, "V": 32, "L": 9}
# clips per teacher-forced call.  W: wh_skinny_kernel<1>, <8> (5 and 8 clips) and the MFMA Linear at 12 rows; V: <2>, <4> and the
# MFMA Linear at 32 rows; with them wh_head_kernel<1, 2, 4, 8, 16, 32>.  L at 9 clips: the MFMA Linear at K = 64, where K / 32 caps
# the K split at 2 and every wave has exactly one k block
TEACHER = (("W", 1), ("W", 5), ("W", 8), ("W", 12), ("V", 2), ("V", 3), ("V", 32), ("L", 2), ("L", 9))
MARGIN = 1e-3                                            # the margin rule of tests/test_gpu_whisper.py
MIN_DISTINCT = 8                                         # ids the oracle emits at its clear positions: a constant head cannot pass
# free greedy: clips and the seed of the 4-id prefix.  Seed 21 was tried first: W's smallest oracle margin with it is 1.1e-2; V has
# a step at 4.9e-4 with it, under the margin, so V moved to the next seed, 22 (smallest margin 2.2e-3).  The oracle never emits
# VOCAB - 1, the end-of-text here, so every clip runs its 16 steps.  test_whisper_host.py::test_width_greedy_oracle_is_clear holds all
# of this without a device.
GREEDY = {"W": (3, 21), "V": (9, 22)}
GREEDY_NEW, GREEDY_EOS = 16, VOCAB - 1
CAPTURE = (("L", 2, ((0, 0),)), ("W", 1, ((0, 19), (0, 0))), ("W", 9, ((0, 19), (0, 0))))     # W: the last head of 20, FMA and MFMA q


@functools.lru_cache(maxsize=None)
def weights(name):
    cfg = whisper_config(CFGS[name])
    sd = recipe_whisper_state_dict(1, cfg)
    return cfg, sd, wo.cast(sd)


@functools.lru_cache(maxsize=None)
def ref(name):
    """the features of the configuration's clips and the oracle's encoder output"""
    cfg, _, sd64 = weights(name)
    g = torch.Generator().manual_seed(11)
    feats = 0.5 * torch.randn(NCLIPS[name], cfg["n_mels"], 2 * cfg["n_audio_ctx"], generator=g)
    with torch.no_grad():
        enc = torch.cat([wo.encoder(sd64, cfg, feats[b:b + 1].double()) for b in range(NCLIPS[name])])     # a clip at a time: L's score map
    return feats, enc


def teacher_prefix():
    return torch.randint(0, VOCAB, (64,), generator=torch.Generator().manual_seed(21)).tolist()


@functools.lru_cache(maxsize=None)
def teacher_all(name):
    """(ids, log-probs, margins) [NCLIPS, 64] of the oracle under the teacher-forced prefix: a clip's row does not depend on the others"""
    cfg, _, sd64 = weights(name)
    n = NCLIPS[name]
    with torch.no_grad():
        return wo.step_outputs(sd64, cfg, ref(name)[1], torch.tensor([teacher_prefix()] * n), 64)


def teacher_case(name, nb):
    ids, sc, mg = teacher_all(name)
    return teacher_prefix(), ids[:nb], sc[:nb], mg[:nb]


def distinct_clear_ids(ids, mg):
    return len(set(ids[mg > MARGIN].tolist()))


@functools.lru_cache(maxsize=None)
def greedy_case(name):
    cfg, _, sd64 = weights(name)
    nb, seed = GREEDY[name]
    prefix = torch.randint(0, VOCAB, (4,), generator=torch.Generator().manual_seed(seed)).tolist()
    with torch.no_grad():
        res = wo.greedy(sd64, cfg, ref(name)[1][:nb], prefix, GREEDY_NEW, (), (), GREEDY_EOS)
    return prefix, res


@functools.lru_cache(maxsize=None)
def capture_case(name, nb, heads):
    cfg, _, sd64 = weights(name)
    with torch.no_grad():
        return ts.cross_attention(sd64, cfg, ref(name)[1][:nb], torch.tensor([teacher_prefix()] * nb), [list(h) for h in heads])
