"""Dispatch map of csrc/paraformer.hip, checked on the CPU: which kernel path a Paraformer encoder / decoder launch of a given shape
takes, and that the shape matrices of tests/test_gpu_paraformer_scale.py cover every reachable path cell and both sides of every
threshold.  The thresholds are parsed from the kernel source, so a moved threshold moves the map with it (and fails here if the
matrix no longer straddles it) instead of silently sending every GPU comparison down one side."""
import os
import re
from typing import NamedTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "targetdiarization_amd", "csrc", "paraformer.hip")

D, FFN, H = 512, 2048, 4
DINP = 576                                 # the first encoder layer's padded input width (560 -> 576)


def _parse():
    src = open(HIP).read()

    def one(pat, what):
        m = re.findall(pat, src)
        assert len(m) == 1, f"paraformer.hip: cannot find {what} (pattern {pat!r} matched {len(m)} times): update tests/test_paraformer_paths.py"
        return m[0]
    c = {
        "PF_FA_MAXT": int(one(r"\bPF_FA_MAXT\s*=\s*(\d+)\s*;", "PF_FA_MAXT")),
        "PF_FA_WORK": 1 << int(one(r"\bPF_FA_WORK\s*=\s*1L\s*<<\s*(\d+)\s*;", "PF_FA_WORK")),
        "PF_SPLITK_ROWS": int(one(r"\bPF_SPLITK_ROWS\s*=\s*(\d+)\s*;", "PF_SPLITK_ROWS")),
        "SOFTMAX_ONEPASS_SP": int(one(r"pf_softmax_kernel\([^)]*\)\s*\{[^}]*?if\s*\(\s*Sp\s*==\s*(\d+)\s*\)", "the Sp == N branch of pf_softmax_kernel")),
    }
    # the predicates themselves: if their form changes, the mirrors below are stale
    one(r"pf_attn_small_fits\(int B, int Tq, int Tk\) \{ return Tk <= PF_FA_MAXT && \(long\)B \* H \* Tq \* Tk <= PF_FA_WORK; \}", "pf_attn_small_fits")
    one(r"if \(M > PF_SPLITK_ROWS \|\| K < 512\) return 1;", "the row test of pf_nsplit")
    one(r"pf_nsplit\(M, D\), ns2048 = pf_nsplit\(M, FFN\), nsT = pf_nsplit\(MT, D\)", "the decoder's split-K switches")
    one(r"if \(ns512 <= 1 && ns2048 <= 1\)", "the encoder's planes-out FFN switch")
    return c


C = _parse()


def pf_nsplit(M, K):
    """mirror of pf_nsplit (paraformer.hip)"""
    if M > C["PF_SPLITK_ROWS"] or K < 512:
        return 1
    ns = min(K // 128, 16)
    while ns > 1 and (K % ns or (K // ns) % 32):
        ns -= 1
    return ns


def attn_small(B, Tq, Tk):
    """mirror of pf_attn_small_fits"""
    return Tk <= C["PF_FA_MAXT"] and B * H * Tq * Tk <= C["PF_FA_WORK"]


class Paths(NamedTuple):
    lin: str        # "splitk" | "direct": the M-row Linears (encoder: qkv / out / FFN; decoder: FFN / q / out)
    attn: str       # "attn_small" | "attn_gemm"
    softmax: str    # encoder GEMM attention: "sp512" (one-pass register softmax) | "generic"; decoder GEMM attention: "rect"; else "n/a"
    kv: str         # decoder only: k|v projection of the B*T encoder rows, "splitk" | "direct"; encoder "n/a"


def pf_paths(kind, B, Tq, Tk):
    """the dispatch of tdx_pfenc_forward (kind "enc", Tq = Tk = T) / tdx_pfdec_decode (kind "dec", Tq = L, Tk = T)"""
    M = B * Tq
    if kind == "enc":
        assert Tq == Tk
        ns = (pf_nsplit(M, DINP), pf_nsplit(M, D), pf_nsplit(M, FFN))
        assert len({n > 1 for n in ns}) == 1          # one row count, K >= 512 everywhere: all of a layer's Linears take the same side
        small = attn_small(B, Tk, Tk)
        Sp = (Tk + 127) // 128 * 128
        sm = "n/a" if small else ("sp512" if Sp == C["SOFTMAX_ONEPASS_SP"] else "generic")
        return Paths("splitk" if ns[0] > 1 else "direct", "attn_small" if small else "attn_gemm", sm, "n/a")
    assert kind == "dec"
    ns = (pf_nsplit(M, D), pf_nsplit(M, FFN))
    assert ns[0] > 1 if ns[1] > 1 else ns[0] == 1     # ns512 and ns2048 switch together
    small = attn_small(B, Tq, Tk)
    return Paths("splitk" if ns[0] > 1 else "direct", "attn_small" if small else "attn_gemm", "n/a" if small else "rect",
                 "splitk" if pf_nsplit(B * Tk, D) > 1 else "direct")


# ---- the shape matrices of tests/test_gpu_paraformer_scale.py ----
ENC_SHAPES = [                     # (B, T), 3 layers vs the fp64 oracle
    (2, 512),                      # B*4*T^2 == PF_FA_WORK exactly: small attention, direct Linears
    (3, 512), (3, 500),            # GEMM attention, one-pass softmax (Sp 512; 500 = the benchmark's T)
    (4, 385),                      # one-pass softmax at its lower edge
    (6, 384), (8, 257),            # generic softmax, Sp 384 (8*4*257^2 just above PF_FA_WORK)
    (32, 129),                     # Sp 256
    (200, 64),                     # Sp 128, 12 800 rows
    (1, 512),                      # M == 512: split-K, small attention at Tk == PF_FA_MAXT
    (1, 513),                      # M == 513: direct, Tk > PF_FA_MAXT: GEMM attention, Sp 640
    (1, 1000),                     # a 60 s segment: Sp 1024
    (3, 171),                      # M == 513 with small attention
]
DEC_SHAPES = [                     # (B, L, T), 2 blocks vs the fp64 oracle through decode_embeds
    (2, 256, 500),                 # M == 512: split-K, small attention
    (2, 257, 500),                 # M == 514: direct, small attention
    (4, 128, 600),                 # M == 512 split-K, Tk > 512: GEMM attention
    (4, 300, 500),                 # direct, GEMM attention (4*4*300*500 > PF_FA_WORK)
    (6, 200, 437),                 # T not a multiple of 128, 6*4*200*437 just above PF_FA_WORK: GEMM attention
    (2, 512, 512),                 # B*4*L*T == PF_FA_WORK exactly: small attention
    (1, 40, 500),                  # B*T == 500: the k|v projection of the encoder rows split-K too
    (1, 40, 513),                  # B*T == 513: k|v direct, Tk > PF_FA_MAXT with split-K Linears
    (1, 513, 512),                 # L == T + 1 (the CIF maximum): M == 513 direct, k|v split (B*T == 512)
]
BENCH_SHAPE = (120, 500)           # BASELINE configs[3]: 120 x 30 s segments in one launch sequence


def _enc_reachable():
    cells = set()
    for B in list(range(1, 65)) + [96, 120, 128, 200, 256]:
        for T in range(1, 1101):
            cells.add(pf_paths("enc", B, T, T))
    return cells


def _dec_reachable():
    """L <= T + 1: CIF fires at most once per frame plus the tail frame (counts = floor(sum alphas), alphas <= 1)"""
    cells = set()
    for B in (1, 2, 3, 4, 6, 8, 16, 64, 120):
        for T in range(1, 1101):
            for L in {1, 2, 8, 40, 64, 100, 128, 200, 256, 257, 300, 400, 512, 513, T - 1, T, T + 1}:
                if 1 <= L <= T + 1:
                    cells.add(pf_paths("dec", B, L, T))
    return cells


def test_thresholds_parsed():
    assert all(v > 0 for v in C.values()), C
    assert C["SOFTMAX_ONEPASS_SP"] % 128 == 0       # Sp is T rounded up to 128


def test_shape_matrices_cover_every_path_and_threshold():
    # every reachable cell has a shape; the benchmark's shape is on the GEMM / direct / one-pass side
    enc_cells = {pf_paths("enc", B, T, T) for B, T in ENC_SHAPES}
    assert _enc_reachable() <= enc_cells, _enc_reachable() - enc_cells
    dec_cells = {pf_paths("dec", B, L, T) for B, L, T in DEC_SHAPES}
    assert _dec_reachable() <= dec_cells, _dec_reachable() - dec_cells
    assert pf_paths("enc", *BENCH_SHAPE, BENCH_SHAPE[1]) == ("direct", "attn_gemm", "sp512", "n/a")

    # both sides of every threshold, the exact boundary value on its inclusive side
    R, W, TK, SP = C["PF_SPLITK_ROWS"], C["PF_FA_WORK"], C["PF_FA_MAXT"], C["SOFTMAX_ONEPASS_SP"]

    def straddles(vals, lim):
        return lim in vals and any(v > lim for v in vals)
    enc_M = {B * T for B, T in ENC_SHAPES}
    enc_T = {T for _, T in ENC_SHAPES}
    enc_W = {B * H * T * T for B, T in ENC_SHAPES if T <= TK}
    assert straddles(enc_M, R) and R + 1 in enc_M
    assert straddles(enc_T, TK) and TK + 1 in enc_T
    assert straddles(enc_W, W)
    gemm_T = {T for B, T in ENC_SHAPES if not attn_small(B, T, T)}     # the Sp switch only matters on the GEMM path
    assert {SP - 128, SP - 127, SP, SP + 1} <= gemm_T, gemm_T
    dec_M = {B * L for B, L, T in DEC_SHAPES}
    dec_MT = {B * T for B, L, T in DEC_SHAPES}
    dec_T = {T for _, _, T in DEC_SHAPES}
    dec_W = {B * H * L * T for B, L, T in DEC_SHAPES if T <= TK}
    assert straddles(dec_M, R) and straddles(dec_MT, R) and straddles(dec_T, TK) and straddles(dec_W, W)
    assert any(T % 128 and not attn_small(B, L, T) for B, L, T in DEC_SHAPES)
    assert all(L <= T + 1 for _, L, T in DEC_SHAPES)


def test_unreachable_cells_are_recorded():
    """Split-K Linears never meet GEMM attention in the encoder: M = B*T <= 512 with T <= 512 gives B*4*T^2 <= 4*512*T <= 2^20 <=
    PF_FA_WORK, and T > 512 gives M > 512.  In the decoder (L <= T + 1) the k|v projection is split-K only when B*T <= 512, and then
    B*4*L*T <= 4*(B*T)*(T+1) <= 4*512*513 < PF_FA_WORK with T <= 512: split-K k|v always comes with small attention."""
    enc = _enc_reachable()
    assert not any(c.lin == "splitk" and c.attn == "attn_gemm" for c in enc)
    assert {c for c in enc if c.lin == "splitk"} == {("splitk", "attn_small", "n/a", "n/a")}
    dec = _dec_reachable()
    assert not any(c.kv == "splitk" and c.attn == "attn_gemm" for c in dec)
    assert len(enc) == 4 and len(dec) == 6, (sorted(enc), sorted(dec))
