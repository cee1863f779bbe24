"""Inputs and fp64 reference of the gated attention launch for tests/test_gpu_attention_gate.py (and the CPU check of its bar in
tests/test_attention_paths.py): o = (att_u * v) * sigmoid(att_v * u) with att_v, att_u from oracle.mossformer2_oracle.cal_attention.
Everything is computed once per case on the CPU and shared, never modified."""
import functools

import torch

FREQS_SEED = 7


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(quad_q, lin_q, quad_k, lin_k [B,S,128], v, u [B,S,E], freqs [16]) in fp32, uniform in +-0.5 from a seeded CPU generator; the rotary
    frequencies are those of rotary_embedding_torch (dim 32, theta 10000).  With more than one (row, segment), v is zeroed over the last
    128-channel segment of the middle row of the last sample: an all-zero output segment."""
    B, S, E = case
    g = torch.Generator(device="cpu").manual_seed(100000 * B + 10 * S + E)
    ts = [torch.rand(B, S, 128, generator=g) - 0.5 for _ in range(4)] + [torch.rand(B, S, E, generator=g) - 0.5 for _ in range(2)]
    if S * (E // 128) > 1:
        ts[4][B - 1, S // 2, E - 128:] = 0.0
    freqs = 1.0 / (10000.0 ** (torch.arange(0, 32, 2)[:16].float() / 32))
    return tuple(ts) + (freqs,)


def zero_segment(case):
    """(global row, segment) of the all-zero output segment, or None"""
    B, S, E = case
    return ((B - 1) * S + S // 2, E // 128 - 1) if S * (E // 128) > 1 else None


def _gate(ts):
    from oracle import mossformer2_oracle as orc
    av, au = orc.cal_attention(*ts)
    v, u = ts[4], ts[5]
    return (au * v) * torch.sigmoid(av * u)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(o in fp64 [B*S, E], err32): err32 = rel-L2 of the same computation by the oracle in torch fp32 against fp64"""
    ts = inputs(case)
    o64 = _gate([t.double() for t in ts])
    o32 = _gate(list(ts))
    err32 = float((o32.double() - o64).norm() / o64.norm())
    E = case[2]
    return o64.reshape(-1, E), err32
