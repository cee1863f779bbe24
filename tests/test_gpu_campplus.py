"""-m gpu: CAM++ on the device (csrc/campplus.hip) against the fp64 oracle (tests/campplus_oracle.py; third-party architecture
restated from upstream, parity unpinned; recipe weights with the calibrated final BatchNorm), and the diarizer behind
TargetDiarization.sd_pipeline.  Embedding bar of the project: rel-L2 < 1e-4 and cosine distance < 1e-3 per row."""
import numpy as np
import pytest
import torch

import campplus_oracle as orc

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")


def rel_l2(a, b):
    a = torch.as_tensor(a).double().cpu().reshape(-1); b = torch.as_tensor(b).double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm())


def cosd(a, b):
    a = torch.as_tensor(a).double().cpu().reshape(-1); b = torch.as_tensor(b).double().cpu().reshape(-1)
    return 1.0 - float(torch.dot(a, b) / (a.norm() * b.norm()))


@pytest.fixture(scope="module")
def sd():
    return orc.calibrated_state_dict()


@pytest.fixture(scope="module")
def model(sd):
    from targetdiarization_amd.speaker import CAMPPlus
    return CAMPPlus(sd, dev)


def _feat(B, F):
    g = torch.Generator().manual_seed(1000 * B + F)
    feat = torch.randn(B, F, 80, generator=g) * 2.0
    for b in range(B):          # rows differ in level and carry a slow trend
        feat[b] = feat[b] * (1.0 - 0.25 * b) + 1.5 * torch.sin(torch.arange(F)[:, None] / (23.0 + 7 * b) + b)
    return feat


@pytest.mark.parametrize("B,F", [(1, 9), (2, 17), (3, 101), (1, 148), (2, 298), (1, 998)])
def test_embed_features_vs_oracle(model, sd, B, F):
    """(2,298) and (1,998) cross one and four segment-pooling boundaries (T' = 149, 499)"""
    feat = _feat(B, F)
    ref = orc.forward(sd, feat, torch.float64)
    out = model.embed_features(feat.to(dev))
    assert out.shape == (B, 192) and torch.isfinite(out).all()
    for b in range(B):
        r, c = rel_l2(out[b], ref[b]), cosd(out[b], ref[b])
        print(f"B={B} F={F} row {b}: rel-L2 {r:.3e} cosine distance {c:.3e}")
        assert r < 1e-4 and c < 1e-3, (B, F, b, r, c)


def test_batch_independence(model):
    feat = _feat(3, 298).to(dev)
    out = model.embed_features(feat)
    for b in range(3):
        one = model.embed_features(feat[b:b + 1])
        print(f"row {b}: batch vs alone rel-L2 {rel_l2(out[b], one[0]):.3e}, bit-equal {bool(torch.equal(out[b], one[0]))}")
        assert rel_l2(out[b], one[0]) < 1e-5
    assert model.flops(3, 298) == 3 * model.flops(1, 298) > 0
    with pytest.raises(Exception):
        model.embed_features(feat[:, :8])


def test_wave_to_embedding(model, sd):
    """wav -> Fbank("sv") -> CAM++ against frontend_oracle.sv_features chained with the oracle"""
    from oracle import frontend_oracle as fo
    rng = np.random.default_rng(21)
    wavs = np.stack([orc.voice(v, 24000, rng) for v in (0, 1, 2)])
    ref = orc.forward(sd, torch.stack([fo.sv_features(torch.from_numpy(w).double()) for w in wavs]), torch.float64)
    out = model(torch.from_numpy(wavs).to(dev))
    for b in range(3):
        r, c = rel_l2(out[b], ref[b]), cosd(out[b], ref[b])
        print(f"voice {b}: rel-L2 {r:.3e} cosine distance {c:.3e}")
        assert r < 1e-4 and c < 1e-3


def test_speaker_embedder_ragged_and_target_asr(sd):
    from oracle import frontend_oracle as fo
    from targetdiarization_amd.speaker import SpeakerEmbedder
    from targetdiarization_amd.target_asr import TargetASR
    rng = np.random.default_rng(22)
    clips = [orc.voice(i % 3, n, rng) for i, n in enumerate((24000, 16000, 24000, 31234, 16000))]
    emb = SpeakerEmbedder(sd, cuda_device=0, arch="campplus")
    got = emb.get_speaker_embeddings(clips)
    assert got.shape == (5, 192)
    for i, c in enumerate(clips):
        ref = orc.forward(sd, fo.sv_features(torch.from_numpy(c).double())[None], torch.float64)[0]
        assert rel_l2(got[i], ref) < 1e-4 and cosd(got[i], ref) < 1e-3, i
    with pytest.raises(Exception):
        SpeakerEmbedder(sd, cuda_device=0, arch="xvector")
    asr = TargetASR(cuda_device=0, campp_state_dict=sd)
    assert set(asr.embedding) == {"campp"}
    e = asr.get_speaker_embedding(clips[3], "campp")
    assert e.shape == (192,) and rel_l2(e, got[3]) < 1e-5
    assert asr.get_speaker_embeddings(clips[:2], "campp").shape == (2, 192)
    lst = asr.get_target_embedding(clips[0], is_preprocess=False, embedding_model="campp")
    assert len(lst) >= 1 and all(v.shape == (192,) for v in lst)
    with pytest.raises(KeyError):
        asr.get_speaker_embedding(clips[0])                     # eres2netv2_large is not loaded


def test_benchmark_sized_launch(sd):
    """the 2 399 windows of an 1 800 s signal through embed_device (chunks of 270 windows); 32 of them against lone launches"""
    from targetdiarization_amd import diarization as dz
    from targetdiarization_amd.speaker import SpeakerEmbedder
    n = 1800 * 16000
    rng = np.random.default_rng(1800)
    audio = np.concatenate([orc.voice(i % 3, 15 * 16000, rng) for i in range(120)])
    windows = dz.plan_windows([[0.0, 1800.0]], n)
    assert len(windows) == 2399
    emb = SpeakerEmbedder(sd, cuda_device=0, arch="campplus")
    x = torch.from_numpy(audio).to(dev)
    out = emb.embed_device([x[st:ed] for st, ed in windows])
    assert out.shape == (2399, 192) and torch.isfinite(out).all()
    worst = 0.0
    for i in np.linspace(0, 2398, 32).astype(int):
        st, ed = windows[i]
        one = emb.model(x[st:ed][None])[0]
        worst = max(worst, rel_l2(out[i], one))
    print(f"benchmark-sized launch vs lone launches: worst rel-L2 {worst:.3e}")
    assert worst < 1e-5


@pytest.mark.parametrize("name", ["three", "two"])
def test_diarizer_matches_host_functions(sd, name):
    from targetdiarization_amd import diarization as dz
    audio, turns = orc.conversation(name)
    d = dz.CamppDiarizer(sd, cuda_device=0)
    res, windows, labels = d(audio, return_windows=True)
    want, _, want_labels = dz.diarize(audio, orc.oracle_embedder(sd), return_windows=True)
    assert np.array_equal(labels, want_labels) and res == want
    truth = orc.pure_window_truth(windows, turns)
    assert (truth < 0).mean() <= 0.35 and orc.consistent_up_to_permutation(labels, truth)
    assert d(audio) == res
    assert len({r[2] for r in d(audio, oracle_num=2)["text"]}) == 2


def test_target_diarization_builds_and_uses_the_diarizer(sd, sd2, tmp_path):
    from targetdiarization_amd.diarization import CamppDiarizer
    from targetdiarization_amd.target_diarization import TargetDiarization
    from targetdiarization_amd.weights import recipe_eres2netv2_state_dict
    audio, _ = orc.conversation("three")
    spk = recipe_eres2netv2_state_dict(0)
    td = TargetDiarization(cuda_device=0, sep_state_dict=sd2, spk_state_dict=spk, sd_state_dict=sd)
    assert isinstance(td.sd_pipeline, CamppDiarizer) and td.sd_pipeline.vad is td.vad
    target, results, _ = td.infer(audio, None)
    assert len({r["speaker"] for r in results}) > 1
    # without the weights: the one-segment default, exactly as before
    td0 = TargetDiarization(cuda_device=0, sep_state_dict=sd2, spk_state_dict=spk)
    assert td0.sd_pipeline is None
    _, res0, _ = td0.infer(audio, None)
    assert len(res0) == 1 and res0[0]["speaker"] == "0" and res0[0]["timerange"][1] == round(len(audio) / 16000, 3)
    # the reference's constructor argument: a directory holding campplus_cn_common.bin
    torch.save(dict(sd, **{"head.bn1.num_batches_tracked": torch.tensor(7)}), tmp_path / "campplus_cn_common.bin")
    td1 = TargetDiarization(str(tmp_path), cuda_device=0, sep_state_dict=sd2, spk_state_dict=spk)
    assert isinstance(td1.sd_pipeline, CamppDiarizer)
    assert td1.sd_pipeline(audio) == td.sd_pipeline(audio)
    assert TargetDiarization(str(tmp_path / "absent"), cuda_device=0, sep_state_dict=sd2, spk_state_dict=spk).sd_pipeline is None
