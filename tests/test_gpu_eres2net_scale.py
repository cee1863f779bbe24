"""-m gpu: ERes2NetV2 at the benchmark's launch shape and on every dispatch path of csrc/eres2net.hip, against the fp64 oracle.

The path of a tdx_eres2net_forward (tap-split or direct layer3_ds, x3 or fp32 fuse34 AFF, HIP-graph replay, the chunked tile map) is
a function of its shape (test_eres2net_paths.eres_paths, thresholds parsed from the source); PATH_SHAPES puts every reachable cell
and both sides of every threshold under the oracle.  The benchmark embeds 180 ten-second clips as ONE launch (B = 180, F = 998:
the stage-1 buffers hold 3.7e9 elements, past 2^31) and 360 as one launch with --embed-frames-per-launch 360000 (past 2^32): those
are compared on a subset of clips with the fp64 oracle and clip by clip with the same clip launched alone (B = 1: the tap split
and the fp32 AFF, a different code path).  Bars: rel-L2 < 1e-4 and 1 - cos < 1e-3 per clip against the oracle, rel-L2 < 1e-5
against the lone launch (test_gpu_eres2net.py)."""
import gc
import os
import sys

import pytest
import torch

from test_eres2net_paths import BENCH_SHAPE, BIG_SHAPE, PATH_SHAPES, clips_at_boundaries, eres_paths, workspace_bytes

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")

WINDOW = 160000                   # 10 s at 16 kHz: the benchmark's embedding clip
SUB = [0, 61, 122, 179]           # clips of the B = 180 launch compared with the fbank + fp64 oracle


def rel_l2(a, b):
    a = torch.as_tensor(a).double().cpu().reshape(-1); b = torch.as_tensor(b).double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm())


def cosd(a, b):
    a = torch.as_tensor(a).double().cpu().reshape(-1); b = torch.as_tensor(b).double().cpu().reshape(-1)
    return 1.0 - float(torch.dot(a, b) / (a.norm() * b.norm()))


def _synth(nwin, seed):
    """the benchmark's audio (bench.synth_mixtures), as test_gpu_configs._synth builds it"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from bench import synth_mixtures
    return synth_mixtures(nwin, WINDOW, seed)


def _release(model):
    """drop the model's grow-only workspace and hand the cached blocks back (the B = 180 / 360 workspaces are 81 / 163 GB)"""
    torch.cuda.synchronize()
    model._guard._ws = None
    gc.collect()
    torch.cuda.empty_cache()


def _fits(model, B, F):
    nb = int(model._l.tdx_eres2net_workspace_bytes(model._h, B, F))
    assert nb == workspace_bytes(B, F)
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(dev)
    assert free > nb + (4 << 30), f"B = {B}, F = {F} needs {nb / 2**30:.1f} GiB of workspace, {free / 2**30:.1f} GiB free"


@pytest.fixture(scope="module")
def model_and_sd():
    from targetdiarization_amd.speaker import ERes2NetV2
    from targetdiarization_amd.weights import recipe_eres2netv2_state_dict
    sd = recipe_eres2netv2_state_dict(0)
    m = ERes2NetV2(sd, dev)
    yield m, {k: v.double() for k, v in sd.items()}
    _release(m)


@pytest.mark.parametrize("shape,cell", PATH_SHAPES, ids=[f"B{B}_F{F}" for (B, F), _ in PATH_SHAPES])
def test_path_matrix_vs_oracle(model_and_sd, monkeypatch, shape, cell):
    """every path cell against the fp64 oracle on its natural path (no override).  The path is checked from the outside too: the
    workspace size carries the tap split's slabs; forcing the claimed fuse34 path through TDX_ERES_AFF34_ROWS gives the same bits,
    forcing the other one other bits (over the capacity limit the x3 core stays off even when forced); a graph-replayed shape
    gives the eager bits on its second call."""
    from oracle import eres2netv2_oracle as eo
    model, sd64 = model_and_sd
    B, F = shape
    ds, fuse, graph = cell
    assert eres_paths(B, F)[:3] == cell
    monkeypatch.delenv("TDX_ERES_AFF34_ROWS", raising=False)
    assert int(model._l.tdx_eres2net_workspace_bytes(model._h, B, F)) == workspace_bytes(B, F)
    g = torch.Generator().manual_seed(1000 + 7 * B + F)
    feat = torch.randn(B, F, 80, generator=g) * 2.0
    feat += 1.5 * torch.sin(torch.arange(F)[None, :, None] / (13.0 + torch.arange(B)[:, None, None]))       # a trend per clip
    feat -= feat.mean(dim=1, keepdim=True)
    out = model.embed_features(feat.to(dev))                          # first call of the shape: eager
    assert out.shape == (B, 192) and bool(torch.isfinite(out).all())
    ref = eo.eres2netv2_forward(feat.double(), sd64)
    errs = [(rel_l2(out[b], ref[b]), cosd(out[b], ref[b])) for b in range(B)]
    print(f"eres2net path B={B} F={F} {cell}: worst rel-L2 {max(e[0] for e in errs):.2e}, 1-cos {max(e[1] for e in errs):.2e}")
    for b, (r, c) in enumerate(errs):
        assert r < 1e-4 and c < 1e-3, (shape, b, r, c)

    # the fuse34 path, seen from its outputs (graph replay off: the override is read by the eager forward)
    gf = model.graph_frames
    model.graph_frames = 0
    try:
        monkeypatch.setenv("TDX_ERES_AFF34_ROWS", "1")                # x3 wherever the capacity allows
        forced_x3 = model.embed_features(feat.to(dev))
        monkeypatch.setenv("TDX_ERES_AFF34_ROWS", str(1 << 40))      # fp32 everywhere
        forced_fp32 = model.embed_features(feat.to(dev))
    finally:
        monkeypatch.delenv("TDX_ERES_AFF34_ROWS")
        model.graph_frames = gf
    if fuse == "x3":
        assert torch.equal(forced_x3, out) and not torch.equal(forced_fp32, out)
    elif fuse == "fp32_rows":
        assert torch.equal(forced_fp32, out) and not torch.equal(forced_x3, out)
    else:
        assert torch.equal(forced_fp32, out) and torch.equal(forced_x3, out)

    # graph replay: the second call of a small shape is captured and replayed, bit for bit the eager result
    again = model.embed_features(feat.to(dev))
    assert ((B, F) in model._graphs._g) == graph
    assert torch.equal(again, out), (shape, rel_l2(again, out))


@pytest.fixture(scope="module")
def bench_clips():
    return torch.from_numpy(_synth(2 * BENCH_SHAPE[0], 11))          # 360 ten-second clips of the benchmark's audio


def test_benchmark_launch_of_180_clips(model_and_sd, bench_clips):
    """bench.py's default: 180 clips as ONE launch (B = 180, F = 998: direct layer3_ds, x3 fuse34, 3.7e9-element stage-1 buffers).
    Four clips against fbank + fp64 oracle, all 180 against the clip launched alone (B = 1, tap split + fp32 AFF), and the
    benchmark's own call, SpeakerEmbedder.embed_device with max_batch_frames = 180000 over 360 clips (two launches of 180)."""
    from oracle import eres2netv2_oracle as eo
    from oracle import frontend_oracle as fo
    from targetdiarization_amd.speaker import SpeakerEmbedder
    model, sd64 = model_and_sd
    B, F = BENCH_SHAPE
    wav = bench_clips.to(dev)
    feat = model.fbank(wav)
    assert feat.shape == (2 * B, F, 80)
    _fits(model, B, F)
    big = model.embed_features(feat[:B])
    assert big.shape == (B, 192) and bool(torch.isfinite(big).all())
    worst = 0.0
    for b in SUB:
        ref = eo.eres2netv2_forward(fo.sv_features(bench_clips[b].double())[None], sd64)[0]
        r, c = rel_l2(big[b], ref), cosd(big[b], ref)
        worst = max(worst, r)
        assert r < 1e-4 and c < 1e-3, (b, r, c)
    lone = torch.cat([model.embed_features(feat[b:b + 1]) for b in range(2 * B)])
    d = [rel_l2(big[b], lone[b]) for b in range(B)]
    print(f"eres2net B={B}: worst rel-L2 vs fp64 {worst:.2e}; vs lone launch {max(d):.2e} (clip {d.index(max(d))})")
    assert max(d) < 1e-5, (d.index(max(d)), max(d))
    _release(model)

    from targetdiarization_amd.weights import recipe_eres2netv2_state_dict
    se = SpeakerEmbedder(recipe_eres2netv2_state_dict(0), 0, max_batch_frames=180000)      # bench.py --embed-frames-per-launch
    emb = se.embed_device([wav[i] for i in range(2 * B)])
    assert emb.shape == (2 * B, 192)
    d2 = [rel_l2(emb[b], lone[b]) for b in range(2 * B)]
    print(f"eres2net embed_device 2 x {B}: worst rel-L2 vs lone launch {max(d2):.2e}")
    assert max(d2) < 1e-5, (d2.index(max(d2)), max(d2))
    _release(se.model)
    del se
    _release(model)


def test_launch_of_360_clips_crosses_2_32_elements(model_and_sd, bench_clips):
    """--embed-frames-per-launch 360000: ONE launch of 360 clips, the stage-1 block outputs 7.4e9 elements (past 2^32).  The first,
    a middle and the last clip and the clips holding element 2^31 / 2^32 of a stage-1 buffer against launches of their own."""
    model, _ = model_and_sd
    B, F = BIG_SHAPE
    wav = bench_clips.to(dev)
    feat = model.fbank(wav)
    assert feat.shape == (B, F, 80)
    _fits(model, B, F)
    big = model.embed_features(feat)
    assert big.shape == (B, 192) and bool(torch.isfinite(big).all())
    _release(model)
    worst = 0.0
    for b in sorted({0, B // 2, B - 1, *clips_at_boundaries(B, F)}):
        d = rel_l2(big[b], model.embed_features(feat[b:b + 1])[0])
        worst = max(worst, d)
        assert d < 1e-5, (b, d)
    print(f"eres2net B={B}: worst rel-L2 vs lone launch {worst:.2e}")
    _release(model)
