"""CPU tests of the WeSpeaker ResNet34 port: the weight layout and packer, the oracle's resampling and pooling against
torch, the calibration conditions the device tests rest on, pyannote's masked step (4) of overlap.diarize on stubs, and the
wiring (build_od_pipeline, server.env_to_kwargs)."""
import struct

import numpy as np
import pytest
import torch

import wespeaker_oracle as orc
from targetdiarization_amd import overlap
from targetdiarization_amd.weights import (drop_num_batches_tracked, pack_blob, recipe_wespeaker_state_dict,
                                           wespeaker_param_shapes)


def test_layout_recipe_and_packer():
    shapes = wespeaker_param_shapes()
    sd = recipe_wespeaker_state_dict(0)
    assert list(sd) == list(shapes) and all(tuple(sd[k].shape) == shapes[k] for k in shapes)
    convs = [k for k in shapes if len(shapes[k]) == 4]
    bns = [k for k in shapes if k.endswith("running_var")]
    assert len(convs) == 1 + 2 * 16 + 3 == 36 and len([k for k in convs if "shortcut" not in k]) == 33 and len(bns) == 36
    assert shapes["resnet.conv1.weight"] == (32, 1, 3, 3) and shapes["resnet.layer2.0.conv1.weight"] == (64, 32, 3, 3)
    assert shapes["resnet.layer4.0.shortcut.0.weight"] == (256, 128, 1, 1) and shapes["resnet.seg_1.weight"] == (256, 5120)
    assert "resnet.layer1.0.shortcut.0.weight" not in shapes and "resnet.layer2.1.shortcut.0.weight" not in shapes
    narrow = [k for k in convs if shapes[k][2] == 3 and shapes[k][0] == shapes[k][1] and shapes[k][0] <= 64]
    assert len(narrow) == 13                                   # all of layer1, layer2 but layer2.0.conv1
    # pack_blob round-trips names, shapes and values
    blob = pack_blob(sd)
    assert blob[:8] == b"TDXW0001"
    n, = struct.unpack_from("<I", blob, 8)
    assert n == len(sd)
    pos, ents = 12, []
    for _ in range(n):
        nl, = struct.unpack_from("<H", blob, pos); pos += 2
        name = blob[pos:pos + nl].decode(); pos += nl
        nd = blob[pos]; pos += 1
        dims = struct.unpack_from(f"<{nd}I", blob, pos); pos += 4 * nd
        off, = struct.unpack_from("<Q", blob, pos); pos += 8
        ents.append((name, dims, off))
    data0 = (pos + 63) // 64 * 64
    assert [e[0] for e in ents] == list(sd)
    for name, dims, off in ents:
        assert tuple(dims) == shapes[name]
        got = np.frombuffer(blob, dtype="<f4", count=int(np.prod(dims)), offset=data0 + off)
        assert np.array_equal(got, sd[name].numpy().reshape(-1)), name
    withcount = dict(sd)
    withcount["resnet.bn1.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    withcount["resnet.layer3.5.bn2.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    assert list(drop_num_batches_tracked(withcount)) == list(sd)


@pytest.mark.parametrize("Fw,T", [(589, 125), (589, 1), (7, 38), (125, 125)])
def test_nearest_resampling_equals_torch(Fw, T):
    w = torch.arange(Fw, dtype=torch.float64)[None, None] + 0.5
    want = torch.nn.functional.interpolate(w, size=T, mode="nearest")
    assert torch.equal(orc.resample_nearest(w, T), want)


def test_pooling_by_the_formula():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 6, 11, generator=g, dtype=torch.float64)
    plain = orc.stats_pool(x)
    assert plain.shape == (2, 1, 12)
    ones = orc.stats_pool(x, torch.ones(2, 1, 11, dtype=torch.float64))
    want = torch.cat([x.mean(dim=-1), x.std(dim=-1, unbiased=True)], dim=-1)
    assert torch.allclose(plain[:, 0], want, rtol=0, atol=1e-9) and torch.allclose(ones[:, 0], want, rtol=0, atol=1e-9)
    w = torch.zeros(2, 3, 11, dtype=torch.float64)
    w[:, 0, 4] = 1.0                                           # one frame: its value, std 0
    w[:, 1, 2:9] = torch.rand(7, generator=g, dtype=torch.float64) + 0.1
    out = orc.stats_pool(x, w)                                 # mask 2 is all zero
    assert torch.equal(out[:, 0, :6], x[:, :, 4]) and torch.equal(out[:, 0, 6:], torch.zeros(2, 6, dtype=torch.float64))
    assert torch.isnan(out[:, 2]).all() and torch.isfinite(out[:, :2]).all()
    ww = w[0, 1]
    mean = (ww * x[0]).sum(-1) / ww.sum()
    var = (ww * (x[0] - mean[:, None]) ** 2).sum(-1) / (ww.sum() - (ww * ww).sum() / ww.sum() + 1e-8)
    assert torch.allclose(out[0, 1], torch.cat([mean, var.sqrt()]), rtol=0, atol=1e-12)
    assert torch.equal(orc.stats_pool(x[:, :, :1])[:, 0, 6:], torch.zeros(2, 6, dtype=torch.float64))      # T' = 1: std 0


def test_calibration_conditions():
    """what the device tests rest on: (a) the oracle's own fp32 run is within a tenth of the bar of its fp64 run on every test
    input; (b) the embeddings of two disjoint masks of one chunk differ by at least 100 bars.  The recorded figures are held
    to the conditions, and the small shapes are recomputed."""
    cal = orc.calibration()
    sd = orc.calibrated_state_dict()
    assert set(cal["bn"]) == {k for k in sd if k.endswith(("running_mean", "running_var"))}
    assert sum(len(v) for v in cal["bn"].values()) == 8512
    for key in ("1x1", "1x2", "2x9", "3x17", "2x298", "1x998", "2x298x3x589", "1x998x3x589", "3x17x2x7", "1x9x1x2"):
        print(f"fp32 vs fp64 {key}: {cal['fp32_vs_fp64'][key]:.3e}")
        assert cal["fp32_vs_fp64"][key] <= 0.1 * orc.REL_BAR
    assert set(cal["mask_separation"]) == {"2x298x3x589", "3x17x2x7"}
    for key, v in cal["mask_separation"].items():
        print(f"disjoint masks {key}: {v:.3e}")
        assert v >= 100 * orc.REL_BAR
    assert cal["e2e"]["gap"] > cal["e2e"]["margin"] == 1e-2
    # recomputed on the small shapes
    feat = orc.shape_feat(3, 17)
    e64, e32 = orc.forward(sd, feat, None, torch.float64), orc.forward(sd, feat, None, torch.float32)
    a = max(orc.rel_l2(e32[b], e64[b]) for b in range(3))
    m = torch.from_numpy(orc.shape_masks(3, 2, 7, 3))
    em = orc.forward(sd, feat, m, torch.float64).numpy()
    b = min(orc.rel_l2(em[i, 0], em[i, 1]) for i in range(1, 3))
    print(f"recomputed (3,17): fp32 vs fp64 {a:.3e}, disjoint masks {b:.3e}")
    assert a <= 0.1 * orc.REL_BAR and b >= 100 * orc.REL_BAR
    assert np.isnan(em[0, 1]).all() and np.isfinite(em[0, 0]).all()
    # the calibration is what one fp64 pass over the voices measures
    got = orc.calibrate(recipe_wespeaker_state_dict(0))
    k = "resnet.layer2.0.shortcut.1.running_var"
    assert torch.allclose(got[k], torch.tensor(cal["bn"][k]), rtol=1e-5, atol=0)


# ---- pyannote's step (4) on stubs ---------------------------------------------------------------------------------------
def _activity():
    """[3,589,3] for a 12 s clip (3 chunks), at most two speakers per frame"""
    act = np.zeros((3, 589, 3), dtype=np.int8)
    act[0, 0:300, 0] = 1; act[0, 200:400, 1] = 1                                   # slot 2 never active
    act[1, 0:300, 0] = 1; act[1, 250:281, 2] = 1; act[1, 400:501, 1] = 1            # slot 2 always overlapped
    act[2, 0:300, 0] = 1; act[2, 298:401, 1] = 1; act[2, 502:506, 1] = 1; act[2, 500:506, 2] = 1   # slot 2: two clean frames
    assert act.sum(axis=-1).max() == 2
    return act


def _segment_of(act):
    def segment(chunks):
        assert chunks.shape == (act.shape[0], 160000)
        out = np.full(act.shape[:2] + (7,), -10.0)
        for k in range(act.shape[0]):
            cls = [overlap.POWERSET.tolist().index(r) for r in act[k].tolist()]
            out[k, np.arange(589), cls] = -0.01
        return out
    return segment


def test_diarize_with_masked_embeddings():
    act = _activity()
    wave = np.zeros(12 * 16000, np.float32) + 0.01
    seen = []

    def embed_masked(chunks, masks, nan_at=((1, 1),)):
        assert chunks.shape == (3, 160000) and masks.shape == (3, 3, 589) and masks.dtype == np.float32
        seen.append(masks.copy())
        E = np.tile(np.eye(3), (3, 1, 1))                       # slot j -> e_j, also for the never-active (0, 2)
        for k, j in nan_at:
            E[k, j, 1] = np.nan
        return E

    tracks = overlap.diarize(wave, _segment_of(act), None, embed_masked=embed_masked)
    m = seen[0]
    a = act.astype(np.float32)
    clean = a * (a.sum(axis=-1, keepdims=True) < 2)
    for k in range(3):
        for j in range(3):
            want = clean[k, :, j] if (k, j) not in ((1, 2), (2, 2)) else a[k, :, j]
            assert np.array_equal(m[k, j], want), (k, j)
    assert m[0, 0].sum() == 200 and m[0, 1].sum() == 100 and m[0, 2].sum() == 0      # clean frames only
    assert clean[1, :, 2].sum() == 0 and m[1, 2].sum() == 31                          # always overlapped: all its frames
    assert clean[2, :, 2].sum() == 2 and m[2, 2].sum() == 6                           # two clean frames are not more than 2
    assert clean[2, :, 1].sum() == 101 and m[2, 1].sum() == 101
    # the NaN row and the never-active speaker are missing: the same tracks as assign_speakers on the present ones
    starts, total = overlap.chunk_plan(wave.shape[0])
    seg = act
    owner = [(k, j) for k in range(3) for j in range(3) if act[k, :, j].any() and (k, j) != (1, 1)]
    assert len(owner) == 7
    emb = np.stack([np.eye(3)[j] for _, j in owner])
    got_emb, got_owner = overlap.masked_embeddings(overlap.cut_chunks(wave, starts), seg, embed_masked)
    assert got_owner == owner and np.array_equal(got_emb, emb)
    clusters = overlap.assign_speakers(seg, starts, total, emb, owner)
    assert clusters[0, 2] == -1 and clusters[1, 1] >= 0                              # (1,1) is assigned from what the others hear
    want = overlap.tracks_of(overlap.reconstruct(seg, starts, total, clusters, overlap.speaker_count(seg, starts, total)), wave.shape[0])
    assert tracks == want and len({t[2] for t in tracks}) >= 2

    # without NaN rows, the old path fed the same one-hots gives the same tracks: the two differ in step (4) only
    new = overlap.diarize(wave, _segment_of(act), None, embed_masked=lambda c, mk: embed_masked(c, mk, nan_at=()))
    active = [(k, j) for k in range(3) for j in range(3) if act[k, :, j].any()]

    def embed(clips):
        assert len(clips) == len(active)
        return np.stack([np.eye(3)[j] for _, j in active])
    old = overlap.diarize(wave, _segment_of(act), embed, min_embed_sec=1e-6)
    assert new == old and new


def test_bad_embedder_directory_prints_and_falls_back(tmp_path, capsys, monkeypatch):
    """od_embed_model_dir that fails in any way leaves today's `embed` path; weights handed in directly fail loudly"""
    import targetdiarization_amd.segmentation as segmentation
    import targetdiarization_amd.speaker as speaker

    class FakeNet:
        def __init__(self, sd, device):
            self.device = device

        def close(self):
            pass

    class Loud:
        def __init__(self, sd, device):
            if "resnet.conv1.weight" not in sd:
                raise RuntimeError("tensor missing: resnet.conv1.weight")
            self.device = device

        def close(self):
            pass
    monkeypatch.setattr(segmentation, "PyanNet", FakeNet)
    monkeypatch.setattr(speaker, "WeSpeakerResNet34", Loud)
    junk = tmp_path / "junk"; junk.mkdir(); (junk / "pytorch_model.bin").write_bytes(b"not a checkpoint")
    wrong = tmp_path / "wrong"; wrong.mkdir(); torch.save({"state_dict": {"x": torch.zeros(1)}}, str(wrong / "pytorch_model.bin"))
    empty = tmp_path / "empty"; empty.mkdir()
    for d in (junk, wrong, empty, tmp_path / "absent"):
        od = overlap.build_od_pipeline({"w": 0}, None, embed=len, od_embed_model_dir=str(d))
        assert isinstance(od, overlap.PyannoteDiarizer) and od.embedder is None and od.embed is len
        assert f"Failed to load the overlap detector's embedder from {d}" in capsys.readouterr().out
    good = tmp_path / "good"; good.mkdir(); torch.save({"state_dict": {"resnet.conv1.weight": torch.zeros(1)}}, str(good / "pytorch_model.bin"))
    od = overlap.build_od_pipeline({"w": 0}, None, embed=len, od_embed_model_dir=str(good))
    assert isinstance(od.embedder, Loud) and capsys.readouterr().out == ""
    od = overlap.build_od_pipeline({"w": 0}, None, embed=None, od_embed_state_dict={"resnet.conv1.weight": 0})     # no `embed` needed
    assert isinstance(od.embedder, Loud) and od.embed is None
    with pytest.raises(RuntimeError):
        overlap.build_od_pipeline({"w": 0}, None, embed=len, od_embed_state_dict={"x": 0})
    with pytest.raises(ValueError):                                                # a failed directory and nothing to fall back to
        overlap.build_od_pipeline({"w": 0}, None, embed=None, od_embed_model_dir=str(junk))


def test_env_forwards_the_embedder_directory():
    from targetdiarization_amd.server import env_to_kwargs
    base = {"verbose_log": False, "is_vad_buffer": True, "use_asr_prompt": True}
    assert env_to_kwargs({}) == base
    assert env_to_kwargs({"OD_EMBED_MODEL_DIR": "x"}) == dict(base, od_embed_model_dir="x")
    assert env_to_kwargs({"OD_MODEL_DIR": "y"}) == dict(base, od_model_dir="y")


def test_flops_is_the_issues_arithmetic():
    from targetdiarization_amd.speaker import WeSpeakerResNet34
    f = WeSpeakerResNet34.flops(1, 998)
    print(f"{f / 1e9:.1f} GFLOP per 998-frame chunk")
    assert 45e9 < f < 49e9 and WeSpeakerResNet34.flops(3, 17) == 3 * WeSpeakerResNet34.flops(1, 17)
