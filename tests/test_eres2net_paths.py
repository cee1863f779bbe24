"""Dispatch map of csrc/eres2net.hip, checked on the CPU: which kernel path a tdx_eres2net_forward of a given (B, F) takes, and
that the shape matrices of tests/test_gpu_eres2net_scale.py cover every reachable path cell and both sides of every threshold.
The thresholds are parsed from the kernel source (and speaker.py / gemm_h3.hpp), so a moved threshold moves the map with it (and
fails here if the matrix no longer straddles it) instead of silently sending every GPU comparison down one side."""
import os
import re
from typing import NamedTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "targetdiarization_amd", "csrc")
HIP = os.path.join(CSRC, "eres2net.hip")
H3 = os.path.join(CSRC, "gemm_h3.hpp")
SPEAKER = os.path.join(ROOT, "targetdiarization_amd", "speaker.py")

NSTAGE, SCALE, H0 = 4, 4, 80


def _one(src, pat, what, where):
    m = re.findall(pat, src)
    assert len(m) == 1, f"{where}: cannot find {what} (pattern {pat!r} matched {len(m)} times): update tests/test_eres2net_paths.py"
    return m[0]


def _ints(s):
    return [int(v) for v in s.split(",")]


def _parse():
    src, h3, spk = open(HIP).read(), open(H3).read(), open(SPEAKER).read()

    def one(pat, what):
        return _one(src, pat, what, "eres2net.hip")

    def one_h3(pat, what):
        return _one(h3, pat, what, "gemm_h3.hpp")
    c = {
        "DS_SPLIT_ROWS": int(one(r"constexpr long DS_SPLIT_ROWS = (\d+);", "DS_SPLIT_ROWS")),
        "DS_SPLIT": int(one(r"constexpr int DS_SPLIT = (\d+);", "DS_SPLIT")),
        "AFF34_MIN": int(one(r"const long aff34_min = aff34_env \? atol\(aff34_env\) : (\d+);", "the default aff34_min")),
        "AFF34_CAP": int(one(r"2 \* M4 <= \(long\)B \* (\d+) &&", "the fuse34 capacity test")),
        "kBlocks": _ints(one(r"const int kBlocks\[NSTAGE\] = \{([\d, ]+)\};", "kBlocks")),
        "kPlanes": _ints(one(r"const int kPlanes\[NSTAGE\] = \{([\d, ]+)\};", "kPlanes")),
        "kStride": _ints(one(r"const int kStride\[NSTAGE\] = \{([\d, ]+)\};", "kStride")),
        "graph_frames": int(_one(spk, r"graph_frames: int = (\d+)", "the default graph_frames", "speaker.py")),
        "H3_BM": int(one_h3(r"constexpr int H3_BM = (\d+), H3_BN = \d+,", "H3_BM")),
        "H3_BN": int(one_h3(r"constexpr int H3_BM = \d+, H3_BN = (\d+),", "H3_BN")),
        "GW_KB": int(one_h3(r"return e \? atol\(e\) : (\d+)L; \}\(\);", "the default TDX_H3_GW_KB")),
        "MC_MB": int(one_h3(r"long mc = mc_env >= 0 \? mc_env : \((\d+)L \* 1024 \* 1024\) / \(256L \* ktot \* 4\);", "the chunk size")),
    }
    # the predicates themselves: if their form changes, the mirrors below are stale
    one(r"w\.slab = rows4 <= \(size_t\)DS_SPLIT_ROWS \? al\(DS_SPLIT \* rows4 \* 2048 \+ 4096\) : 0;", "the tap-split slab of ws_plan")
    one(r"if \(wp\.slab && h->ds\.taps == 9 && h->ds\.Npad == 2048\)\s+TRY\(conv_gemm_h3_tapsplit\(", "the layer3_ds switch")
    one(r"if \(M4 >= aff34_min && 2 \* M4 <= \(long\)B \* 40960 && h->fuse34\.c0\.hp && h->fuse34\.ipad == 512\)", "the fuse34 switch")
    one(r"run_aff34_x3\(h, h->fuse34, x, P\[i_ds\], tbuf, P\[i_fu\], M4, hx, hcat, stats, hin, stats \+ M4, inv20, st\)",
        "the ys / ts rows of fuse34 inside `stats`")
    one(r"w\.stats = al\(\(size_t\)B \* 40960\);", "the stats buffer")
    one(r"d\.H\[s \+ 1\] = kStride\[s\] == 1 \? d\.H\[s\] : \(d\.H\[s\] - 1\) / 2 \+ 1;", "make_dims")
    one(r"if \(s < 1\) \{ for \(int j = 0; j < SCALE; \+\+j\) jobs\.push_back\(&b\.convs\[j\]\); continue; \}", "the x3 weight planes")
    _one(spk, r"if self\.graph_frames and B \* F <= self\.graph_frames:", "the graph-replay test", "speaker.py")
    one_h3(r"if \(g\.tiles_m >= 16 && batches <= 4\) \{", "the grouped tile map switch")
    one_h3(r"g\.mp = \(g\.tiles_m \+ 7\) / 8;", "mp")
    one_h3(r"long gw = \(gw_kb \* 1024\) / \(256L \* ktot \* 4\);", "gw")
    one_h3(r"if \(g\.gw < g\.tiles_n\) \{", "the chunk switch")
    one_h3(r"if \(mc > 0 && mc < g\.mp\) g\.mc = \(int\)mc;", "mc")
    return c


C = _parse()


def up(n, m):
    return (n + m - 1) // m * m


def al(n):
    return (n + 63) // 64 * 64


def make_dims(F):
    """mirror of make_dims: H[s], W[s] for s = 0..4 (input, stage outputs)"""
    H, W = [H0], [F]
    for s in range(NSTAGE):
        st = C["kStride"][s]
        H.append(H[s] if st == 1 else (H[s] - 1) // 2 + 1)
        W.append(W[s] if st == 1 else (W[s] - 1) // 2 + 1)
    return H, W


class Block(NamedTuple):
    s: int
    i: int
    stride: int
    cin: int
    width: int
    wpad: int
    w4: int
    cout: int
    has_sc: bool
    is_aff: bool
    ipad: int


def blocks():
    """the BlockW list of tdx_eres2net_create"""
    out, cin = [], 64
    for s in range(NSTAGE):
        planes = C["kPlanes"][s]
        width, cout = planes * 24 // 64, planes * 4
        for i in range(C["kBlocks"][s]):
            stride = C["kStride"][s] if i == 0 else 1
            out.append(Block(s, i, stride, cin, width, up(width, 32), width * SCALE, cout, stride != 1 or cin != cout, s >= 2,
                             up(width // 4, 32)))
            cin = cout
    return out


BLOCKS = blocks()


def ws_plan(B, F):
    """mirror of ws_plan: buffer sizes in floats"""
    H, W = make_dims(F)
    mP, mo1, msp, mt, mhx, mhc, mhi = B * H0 * F * 64, 0, 0, 0, 0, 0, 0
    for b in BLOCKS:
        rows = B * H[b.s + 1] * W[b.s + 1]
        if b.s >= 1:
            rows_in = B * H[b.s] * W[b.s] if b.i == 0 else rows
            mhx, mhc, mhi = max(mhx, rows_in * b.cin), max(mhc, rows * b.w4), max(mhi, rows * b.wpad)
        mP, mo1, msp = max(mP, rows * b.cout), max(mo1, rows * b.w4), max(msp, rows * b.wpad)
        if b.is_aff:
            mt = max(mt, rows * b.ipad)
    rows3, rows4 = B * H[3] * W[3], B * H[4] * W[4]
    mt = max(mt, rows4 * 512)
    w = {"P": al(mP + 4096), "keep3": al(rows3 * 1024 + 4096), "o1": al(mo1 + 4096), "spin": al(msp + 4096), "tbuf": al(mt + 4096),
         "stats": al(B * 40960), "hx": al(max(mhx, rows3 * 1024) + 4096), "hcat": al(mhc + 4096), "hin": al(mhi + 4096),
         "slab": al(C["DS_SPLIT"] * rows4 * 2048 + 4096) if rows4 <= C["DS_SPLIT_ROWS"] else 0}
    w["total"] = 3 * w["P"] + w["keep3"] + 2 * w["o1"] + 2 * w["spin"] + w["tbuf"] + w["stats"] + w["hx"] + w["hcat"] + w["hin"] + w["slab"]
    return w


def workspace_bytes(B, F):
    """mirror of tdx_eres2net_workspace_bytes"""
    return ws_plan(B, F)["total"] * 4


def largest_buffer(B, F):
    """elements (floats) of the largest single workspace buffer"""
    return max(v for k, v in ws_plan(B, F).items() if k != "total")


def h3_chunked(M, N, ktot, batches=1):
    """mirror of launch_gemm_h3x's tile map (no H3Conv epilogue): True when the chunked block-to-tile map is on (g.mc > 0)"""
    tiles_m, tiles_n = (M + C["H3_BM"] - 1) // C["H3_BM"], (N + C["H3_BN"] - 1) // C["H3_BN"]
    if not (tiles_m >= 16 and batches <= 4):
        return False
    mp = (tiles_m + 7) // 8
    gw = min(max((C["GW_KB"] * 1024) // (256 * ktot * 4), 1), tiles_n)
    if gw >= tiles_n:
        return False
    mc = (C["MC_MB"] * 1024 * 1024) // (256 * ktot * 4)
    return 0 < mc < mp


def x3_conv_launches(B, F):
    """(stage, name, M, N, ktot) of every conv_gemm_h3 launch of stages 3-4 (conv1, shortcut, the chain convolutions, conv3)"""
    H, W = make_dims(F)
    out = []
    for b in BLOCKS:
        if b.s < 2:
            continue
        M = B * H[b.s + 1] * W[b.s + 1]
        out.append((b.s + 1, "conv1", M, up(b.w4, 128), up(b.cin, 32)))
        if b.has_sc:
            out.append((b.s + 1, "sc", M, up(b.cout, 128), up(b.cin, 32)))
        out += [(b.s + 1, "convs", M, up(b.width, 128), 9 * up(b.width, 32))] * SCALE
        out.append((b.s + 1, "conv3", M, up(b.cout, 128), up(b.w4, 32)))
    return out


class Paths(NamedTuple):
    ds: str         # layer3_ds: "tapsplit" (3 x 3 taps into slabs + reduce) | "direct" (one implicit-GEMM launch)
    fuse34: str     # "x3" | "fp32_rows" (M4 < aff34_min) | "fp32_capacity" (ys / ts would overrun `stats`)
    graph: bool     # ERes2NetV2.embed_features replays the shape as a HIP graph from its second call on
    chunk34: bool   # a stage-3/4 x3 convolution runs with the chunked block-to-tile map (g.mc > 0)
    chunk_ds: bool  # layer3_ds runs with the chunked tile map


def eres_paths(B, F, aff34_min=None, graph_frames=None):
    """the dispatch of tdx_eres2net_forward (+ ERes2NetV2.embed_features' graph switch) for B clips of F frames"""
    aff34_min = C["AFF34_MIN"] if aff34_min is None else aff34_min
    graph_frames = C["graph_frames"] if graph_frames is None else graph_frames
    H, W = make_dims(F)
    M4 = B * H[4] * W[4]
    split = ws_plan(B, F)["slab"] > 0
    if M4 < aff34_min:
        fuse = "fp32_rows"
    elif 2 * M4 > B * C["AFF34_CAP"]:
        fuse = "fp32_capacity"
    else:
        fuse = "x3"
    ds_k = (9 // C["DS_SPLIT"] if split else 9) * 1024
    return Paths("tapsplit" if split else "direct", fuse, bool(graph_frames) and B * F <= graph_frames,
                 any(h3_chunked(M, N, k) for _, _, M, N, k in x3_conv_launches(B, F)),
                 h3_chunked(M4, 2048, ds_k, C["DS_SPLIT"] if split else 1))


def m4(B, F):
    H, W = make_dims(F)
    return B * H[4] * W[4]


def clips_at_boundaries(B, F):
    """the clips of a B-clip launch whose rows hold element 2^31 or 2^32 of a stage-1 buffer (the stem output: 64 channels, conv1
    output o1: 96, block outputs P: 256), sorted"""
    rows = H0 * F
    out = set()
    for ld in (64, 96, 256):
        for e in (1 << 31, 1 << 32):
            b = e // ld // rows
            if b < B:
                out.add(b)
    return sorted(out)


# ---- the shape matrices of tests/test_gpu_eres2net_scale.py ----
PATH_SHAPES = [                    # (B, F) vs the fp64 oracle, no env override; the (layer3_ds, fuse34, graph) cell it must take
    ((1, 9), ("tapsplit", "fp32_rows", True)),         # the smallest F (two pooled frames)
    ((3, 1001), ("tapsplit", "fp32_rows", True)),      # odd F, B = 3: the tap split with the chunked tile map in stage 3
    ((1, 3272), ("tapsplit", "fp32_rows", True)),      # M4 = 4090: the last tap split
    ((1, 3273), ("direct", "fp32_rows", True)),        # M4 = 4100: direct layer3_ds, fp32 AFF (the middle cell)
    ((4, 1000), ("direct", "fp32_rows", True)),        # the middle cell at B = 4; B F = graph_frames: replayed
    ((1, 4001), ("direct", "fp32_rows", False)),       # B F = graph_frames + 1: eager
    ((1, 6552), ("direct", "fp32_rows", False)),       # M4 = 8190: fp32 AFF below the row threshold
    ((1, 6553), ("direct", "x3", False)),              # M4 = 8200: x3 AFF
    ((7, 939), ("direct", "x3", False)),               # x3 AFF over 7 clips, odd F
    ((1, 16384), ("direct", "x3", False)),             # W4 = 2048: ys / ts fill `stats` exactly
    ((1, 16385), ("direct", "fp32_capacity", False)),  # W4 = 2049: fp32 AFF over the capacity limit
]
SHAPES = [s for s, _ in PATH_SHAPES]
BENCH_SHAPE = (180, 998)           # bench.py --embed-frames-per-launch 180000: 180 ten-second clips in one launch
BIG_SHAPE = (360, 998)             # --embed-frames-per-launch 360000: past 2^32 elements
CAPACITY_EDGE = ((1, 16384), (1, 16385))


def _reachable():
    cells = set()
    for B in (1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 32, 60, 106, 180, 360):
        Fs = list(range(9, 1200)) + list(range(1200, 17000, 7 if B == 1 else 97)) + [16376, 16377, 16384, 16385, 16392, 16393]
        for F in Fs:
            cells.add(eres_paths(B, F))
    return cells


def test_thresholds_parsed():
    assert C["kBlocks"] == [3, 4, 6, 3] and C["kPlanes"] == [64, 128, 256, 512] and C["kStride"] == [1, 2, 2, 2], C
    assert C["DS_SPLIT"] == 3 and 9 % C["DS_SPLIT"] == 0
    assert all(v > 0 for v in (C["DS_SPLIT_ROWS"], C["AFF34_MIN"], C["AFF34_CAP"], C["graph_frames"], C["GW_KB"], C["MC_MB"]))
    H, W = make_dims(998)
    assert H == [80, 80, 40, 20, 10] and W == [998, 998, 499, 250, 125] and m4(1, 998) == 1250
    # the numbers the issue / DESIGN quote for the benchmark shape: 80 F rows of 256 channels per clip in stage 1
    assert ws_plan(1, 998)["P"] == al(80 * 998 * 256 + 4096) and 80 * 998 * 256 == 20439040


def test_shape_matrices_cover_every_path_and_threshold():
    assert [eres_paths(*sh)[:3] for sh in SHAPES] == [c for _, c in PATH_SHAPES], [eres_paths(*sh) for sh in SHAPES]
    cells = {eres_paths(B, F) for B, F in SHAPES}
    reach = _reachable()
    assert reach <= cells, reach - cells
    # the benchmark's launch: direct layer3_ds, x3 AFF, no graph, the largest buffer past 2^31 elements; 360 clips past 2^32
    assert eres_paths(*BENCH_SHAPE) == ("direct", "x3", False, True, False)
    assert largest_buffer(*BENCH_SHAPE) > 1 << 31 and largest_buffer(105, 998) < 1 << 31 < largest_buffer(106, 998)
    assert eres_paths(*BIG_SHAPE) == ("direct", "x3", False, True, False) and largest_buffer(*BIG_SHAPE) > 1 << 32
    assert clips_at_boundaries(*BIG_SHAPE) == [105, 210, 280], clips_at_boundaries(*BIG_SHAPE)

    # both sides of every threshold, as tightly as the geometry allows: M4 = 10 B W4 is a multiple of 10, so the neighbours of a row
    # threshold are the multiples of 10 next to it (every value between two of them gives the same map)
    R, A, G = C["DS_SPLIT_ROWS"], C["AFF34_MIN"], C["graph_frames"]
    M4s = {m4(B, F) for B, F in SHAPES}
    assert {R // 10 * 10, R // 10 * 10 + 10} <= M4s, sorted(M4s)                   # rows4 <= R: 4090 split, 4100 direct
    assert {(A - 1) // 10 * 10, (A - 1) // 10 * 10 + 10} <= M4s, sorted(M4s)     # M4 >= A: 8190 fp32, 8200 x3
    cap = [make_dims(F)[1][4] for B, F in CAPACITY_EDGE]
    assert all(B == 1 for B, _ in CAPACITY_EDGE) and cap == [C["AFF34_CAP"] // 20, C["AFF34_CAP"] // 20 + 1], cap
    assert [eres_paths(*s).fuse34 for s in CAPACITY_EDGE] == ["x3", "fp32_capacity"]
    assert set(CAPACITY_EDGE) <= set(SHAPES)
    BF = {B * F for B, F in SHAPES}
    assert {G, G + 1} <= BF, sorted(BF)
    # the tap split's and the x3 AFF's switches are reached at B = 1 and at B > 1
    assert {B > 1 for B, F in SHAPES if eres_paths(B, F).ds == "tapsplit"} == {False, True}
    assert {B > 1 for B, F in SHAPES if eres_paths(B, F).ds == "direct" and eres_paths(B, F).fuse34 == "fp32_rows"} == {False, True}
    assert {B > 1 for B, F in SHAPES if eres_paths(B, F).fuse34 == "x3"} == {False, True}
    assert any(F % 2 for _, F in SHAPES) and min(F for _, F in SHAPES) == 9


def test_unreachable_cells_are_recorded():
    """M4 = B * 10 * W4 and W4 >= F / 8, so M4 >= 1.25 B F:
    * the tap split (M4 <= 4096) always comes with the fp32 AFF (M4 < 8192) and with graph replay (B F <= 3277 < 4000): tap split
      + x3 AFF is reached only through TDX_ERES_AFF34_ROWS (test_gpu_eres2net.test_fuse34_on_the_x3_core_vs_oracle);
    * the x3 AFF and the capacity limit need M4 >= 8192, B F > 4000: never graph-replayed;
    * the direct layer3_ds (M4 > 4096: stage 3 has > 16 384 rows, 64 tiles of 256, mp >= 8) always has the chunked map in stage 3
      (conv1 of blocks 2-6, ktot 1024: mc = 6);
    * layer3_ds itself never runs chunked: direct, ktot = 9216 gives mc = 0; split, ktot = 3072 gives mc = 2 but at most 16 row
      tiles (mp <= 2)."""
    reach = _reachable()
    assert not any(c.ds == "tapsplit" and c.fuse34 != "fp32_rows" for c in reach)
    assert all(c.graph for c in reach if c.ds == "tapsplit")
    assert not any(c.graph for c in reach if c.fuse34 != "fp32_rows")
    assert all(c.chunk34 for c in reach if c.ds == "direct")
    assert not any(c.chunk_ds for c in reach)
    assert eres_paths(2, 206, aff34_min=1) == ("tapsplit", "x3", True, False, False)       # the env-forced cell
    assert len(reach) == 6, sorted(reach)


def test_workspace_mirror_matches_the_benchmark_figures():
    """the B = 180 launch needs 81 GB, B = 360 163 GB of workspace (the MI355X has 288 GB)"""
    assert 80e9 < workspace_bytes(*BENCH_SHAPE) < 83e9, workspace_bytes(*BENCH_SHAPE)
    assert 160e9 < workspace_bytes(*BIG_SHAPE) < 166e9, workspace_bytes(*BIG_SHAPE)
