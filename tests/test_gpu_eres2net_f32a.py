"""-m gpu: ERes2NetV2's TDX_ERES_F32A switch (csrc/eres2net.hip): the 1x1 convolutions of stage 2 (level 1) and of stages 1-2 (level 2,
the default) on the fp32-A form of the x3 core (csrc/gemm_h3f.hpp) instead of split passes + planes GEMMs (stage 2) and the fp32-MFMA
core (stage 1).  Level 1 replaces launches by a bit-identical one, so the embedding keeps its bits; level 2 moves stage 1 from exact
fp32 products to split-f16 x3 ones and is held to the model's bars against the fp64 oracle (rel-L2 < 1e-4, cosine < 1e-3).  Odd F
exercises the stride-2 edges of stage 2's first block, F = 9 is the smallest legal size.  A fresh model per level: embed_features
replays a repeated shape as a HIP graph, which would freeze the switch."""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
SHAPES = [(1, 9), (2, 17), (1, 101), (3, 64)]


def rel_l2(a, b):
    a = torch.as_tensor(a).double().cpu().reshape(-1); b = torch.as_tensor(b).double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm())


def cosd(a, b):
    a = torch.as_tensor(a).double().cpu().reshape(-1); b = torch.as_tensor(b).double().cpu().reshape(-1)
    return 1.0 - float(torch.dot(a, b) / (a.norm() * b.norm()))


def _feat(B, F):
    return torch.randn(B, F, 80, generator=torch.Generator().manual_seed(F)) * 2.0


@pytest.fixture(scope="module")
def sd():
    from targetdiarization_amd.weights import recipe_eres2netv2_state_dict
    return recipe_eres2netv2_state_dict(0)


@pytest.fixture(scope="module")
def oracle(sd):
    """fp64 reference embeddings, computed once"""
    from oracle import eres2netv2_oracle as eo
    sd64 = {k: v.double() for k, v in sd.items()}
    return {(B, F): eo.eres2netv2_forward(_feat(B, F).double(), sd64) for (B, F) in SHAPES}


@pytest.fixture(scope="module")
def embeddings(sd):
    """embeddings of every shape at every level of the switch (one model per level, the environment restored afterwards)"""
    from targetdiarization_amd.speaker import ERes2NetV2
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        for level in (0, 1, 2):
            mp.setenv("TDX_ERES_F32A", str(level))
            model = ERes2NetV2(sd, dev)
            for (B, F) in SHAPES:
                out[level, B, F] = model.embed_features(_feat(B, F).to(dev)).cpu()
            del model
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_F%d" % s)
def test_level1_keeps_the_bits_of_level0(embeddings, shape):
    B, F = shape
    a, b = embeddings[0, B, F], embeddings[1, B, F]
    assert a.shape == (B, 192) and bool(torch.isfinite(a).all())
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} values differ, max |d| = {float((a - b).abs().max())}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_F%d" % s)
def test_levels_vs_oracle(embeddings, oracle, shape):
    B, F = shape
    ref = oracle[shape]
    r = {level: rel_l2(embeddings[level, B, F], ref) for level in (0, 1, 2)}
    print(f"(B, F) = {shape}: rel-L2 vs fp64 oracle: level 0 {r[0]:.3e}, level 1 {r[1]:.3e}, level 2 {r[2]:.3e}")
    for level in (0, 2):
        out = embeddings[level, B, F]
        assert r[level] < 1e-4 and cosd(out, ref) < 1e-3, (level, shape, r[level])


def test_default_is_level2(sd, embeddings, monkeypatch):
    from targetdiarization_amd.speaker import ERes2NetV2
    monkeypatch.delenv("TDX_ERES_F32A", raising=False)
    B, F = SHAPES[1]
    out = ERes2NetV2(sd, dev).embed_features(_feat(B, F).to(dev)).cpu()
    assert torch.equal(out, embeddings[2, B, F])
