"""Dispatch map of the stand-alone gated attention (csrc/mf2_attention.hpp), checked on the CPU: how attn_plan splits the token axis of
the lin_k^T [v|u] launch for a shape (B, S, E), and whether that launch then runs on the half-height kernel gemm_h3a or falls back to
the wide one (h3a_fits in csrc/gemm_h3a.hpp).  The case list of tests/test_gpu_attention_gate.py lives here, and the test below checks
that it reaches every side.  The constants are parsed from the source, so a moved threshold moves the map with it (and fails here if
the cases no longer cover a side) instead of silently sending every GPU comparison down one side."""
import os
import re
from typing import NamedTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "targetdiarization_amd", "csrc")


def _parse():
    att = open(os.path.join(CSRC, "mf2_attention.hpp")).read()
    h3a = open(os.path.join(CSRC, "gemm_h3a.hpp")).read()

    def one(src, pat, what):
        m = re.findall(pat, src)
        assert len(m) == 1, f"cannot find {what} (pattern {pat!r} matched {len(m)} times): update tests/test_attention_paths.py"
        return m[0]
    c = {}
    # attn_plan: workgroup target, longest chunk, chunk rounding
    t = one(att, r"int sp = \((\d+) \+ \(2 \* E / 128\) \* B - 1\) / \(\(2 \* E / 128\) \* B\); if \(sp < 1\) sp = 1;", "the workgroup target of attn_plan")
    c["TARGET"] = int(t)
    m = one(att, r"int maxsp = \(S \+ (\d+)\) / (\d+); if \(sp > maxsp\) sp = maxsp;", "the longest chunk of attn_plan")
    assert int(m[0]) == int(m[1]) - 1
    c["MAXCHUNK"] = int(m[1])
    m = one(att, r"kchunk = \(\(S \+ sp - 1\) / sp \+ (\d+)\) / (\d+) \* (\d+);", "the chunk rounding of attn_plan")
    assert int(m[0]) == int(m[1]) - 1 and m[1] == m[2]
    c["ROUND"] = int(m[1])
    one(att, r"splits = \(S \+ kchunk - 1\) / kchunk;", "the chunk count of attn_plan")
    # the lin_k^T [v|u] launch: its arguments and the switch
    one(att, r"g\.seg\[0\]\.kchunk = kchunk; g\.seg\[0\]\.ktotal = Sp;", "the split-K arguments of the lin_k^T [v|u] launch")
    one(att, r"g\.nseg = 1; g\.M = QK; g\.N = 2 \* E;", "the shape of the lin_k^T [v|u] launch")
    one(att, r"if \(h3a && tdx::h3a_fits<false>\(g, false\)\) \{", "the kernel switch of the lin_k^T [v|u] launch")
    # h3a_fits
    m = one(h3a, r"if \(g\.nseg != \(TWOSEG \? 2 : 1\) \|\| g\.M % (\d+) \|\| g\.N % \(gate \? (\d+) : (\d+)\)\) return false;", "the tile test of h3a_fits")
    c["TILE_M"], c["TILE_N"] = int(m[0]), int(m[2])
    m = one(h3a, r"if \(sg\.K < (\d+) \|\| sg\.K % (\d+) \|\| sg\.segk \|\| sg\.a_shift \|\| sg\.a_period\) return false;", "the K test of h3a_fits")
    c["KMIN"], c["KMOD"] = int(m[0]), int(m[1])
    m = one(h3a, r"if \(TWOSEG \|\| sg\.kchunk % (\d+) \|\| sg\.ktotal % (\d+) \|\| sg\.K != sg\.kchunk\) return false;", "the chunk test of h3a_fits")
    assert int(m[0]) == int(m[1]) == c["KMOD"]
    one(h3a, r"const int last = sg\.ktotal - \(sg\.zdiv - 1\) \* sg\.kchunk;", "the last chunk of h3a_fits")
    c["LASTMIN"] = int(one(h3a, r"if \(last < (\d+)\) return false;", "the last-chunk test of h3a_fits"))
    return c


C = _parse()
QK = 128


class Plan(NamedTuple):
    G: int          # 256-token groups per sample
    Sp: int         # padded tokens per sample
    splits: int     # split-K chunks of the lin_k^T [v|u] launch
    kchunk: int     # tokens per chunk
    last: int       # k rows the last chunk's blocks see (up to the end of the zero padding)
    kvu: str        # "h3a" | "wide": the kernel of the lin_k^T [v|u] launch when h3a is requested


def attn_plan(B, S, E):
    """mirror of attn_plan (mf2_attention.hpp) and of h3a_fits<false>(g, false) (gemm_h3a.hpp) for the launch it feeds"""
    G = (S + 255) // 256
    Sp = G * 256
    tiles = (2 * E // 128) * B
    sp = max(1, (C["TARGET"] + tiles - 1) // tiles)
    sp = min(sp, (S + C["MAXCHUNK"] - 1) // C["MAXCHUNK"])
    kchunk = ((S + sp - 1) // sp + C["ROUND"] - 1) // C["ROUND"] * C["ROUND"]
    splits = (S + kchunk - 1) // kchunk
    last = Sp - (splits - 1) * kchunk
    fits = (QK % C["TILE_M"] == 0 and (2 * E) % C["TILE_N"] == 0 and kchunk >= C["KMIN"] and kchunk % C["KMOD"] == 0
            and Sp % C["KMOD"] == 0 and last >= C["LASTMIN"])
    return Plan(G, Sp, splits, kchunk, last, "h3a" if fits else "wide")


# ---- the cases of tests/test_gpu_attention_gate.py: (B, S, E), the smallest shapes at which each edge exists ----
CASES = [
    (1, 1, 128),        # one real row in a 256-row group; kchunk = 32: lin_k^T [v|u] takes the wide fallback
    (1, 33, 128),       # kchunk = 64: the shortest split-K chunk gemm_h3a accepts (four k-tiles)
    (1, 255, 128),      # one row short of a group
    (1, 256, 256),      # exactly one group; two column segments
    (1, 257, 128),      # one row into the second group: kchunk = 288, one chunk clipped inside the 512-row pad
    (3, 600, 256),      # B*G = 9 batches in 16 block slots (the z >= batches exit, the XCD map); two chunks (320 + 448)
    (1, 1000, 256),     # four groups, two chunks of 512
    (2, 300, 1024),     # the model's E: eight segments in os / oss, the 8E-byte pitch of the gate's v operand
]


def test_constants_parsed():
    assert C == {"TARGET": 1536, "MAXCHUNK": 512, "ROUND": 32, "TILE_M": 128, "TILE_N": 256, "KMIN": 64, "KMOD": 16, "LASTMIN": 48}, C


def test_plans_of_the_cases():
    """what the comments of CASES claim"""
    P = {c: attn_plan(*c) for c in CASES}
    assert P[(1, 1, 128)] == (1, 256, 1, 32, 256, "wide")
    assert P[(1, 33, 128)] == (1, 256, 1, C["KMIN"], 256, "h3a")
    assert P[(1, 255, 128)].G == 1 and P[(1, 256, 256)].G == 1 and P[(1, 257, 128)].G == 2
    assert P[(1, 257, 128)] == (2, 512, 1, 288, 512, "h3a")
    assert P[(3, 600, 256)] == (3, 768, 2, 320, 448, "h3a")
    assert 3 * P[(3, 600, 256)].G == 9                         # 9 batches: the second round of 8 block slots holds one
    assert P[(1, 1000, 256)] == (4, 1024, 2, 512, 512, "h3a")
    assert P[(2, 300, 1024)] == (2, 512, 1, 320, 512, "h3a")


def test_cases_cover_both_kernels_and_chunk_counts():
    plans = [attn_plan(*c) for c in CASES]
    assert any(p.kvu == "wide" for p in plans)
    assert any(p.kvu == "h3a" and p.splits == 1 for p in plans)
    assert any(p.kvu == "h3a" and p.splits == 2 for p in plans)
    assert any(p.kvu == "h3a" and p.kchunk == C["KMIN"] for p in plans)          # the K limit on its inclusive side ...
    assert any(p.kchunk == C["KMIN"] - C["ROUND"] for p in plans)                # ... and the nearest plan below it
    assert all(E % 128 == 0 for _, _, E in CASES)
    assert {E // 128 for _, _, E in CASES} >= {1, 2, 8}                          # one, two and the model's eight column segments
    assert {p.G for p in plans} >= {1, 2, 3, 4}
    S_all = {S for _, S, _ in CASES}
    assert {1, 255, 256, 257} <= S_all                                           # both sides of the group edge


def test_last_chunk_limit_is_unreachable_from_attn_plan():
    """No plan of attn_plan trips the last-chunk test of h3a_fits (the last chunk's blocks see the rows up to the end of the padding,
    Sp - (splits - 1) * kchunk of them): the only reachable reason for the wide fallback is a chunk shorter than the K limit, which is
    why the case list has no "last chunk too short" case.  By enumeration over S <= 6000."""
    for B in (1, 2, 3, 8, 60):
        for E in (128, 256, 1024):
            for S in range(1, 6001):
                p = attn_plan(B, S, E)
                assert p.last >= C["LASTMIN"], (B, S, E, p)
                assert (p.kvu == "wide") == (p.kchunk < C["KMIN"]), (B, S, E, p)


def test_fp32_bar_of_every_case_is_positive():
    """tests/test_gpu_attention_gate.py holds the kernel to 3 * err32, err32 = the oracle's own fp32 error against fp64 for the case:
    a case whose fp32 run happened to be exact would make that bar unreachable.  (1.7e-7 for the one-row case up to 1.8e-6.)"""
    import attention_gate_ref as ref
    for case in CASES:
        o64, err32 = ref.reference(case)
        assert o64.shape == (case[0] * case[1], case[2]) and float(o64.norm()) > 0
        assert 1e-7 < err32 < 3e-6, (case, err32)
