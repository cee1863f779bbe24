"""GPU tests of emotion2vec (tdx_emo2v_*, emotion.Emotion2vec, ASRProcessor.emotion_detection) against the float64 oracle
(tests/emotion2vec_oracle.py).  Recipe weights of seed 1.  Features: rel-L2 < 1e-4, the project's standing contract;
probabilities: 10 x SCORE_GAP, the oracle's own float32-versus-float64 gap."""
import numpy as np
import pytest
import torch

import emotion2vec_oracle as orc
from targetdiarization_amd.weights import emotion2vec_config, recipe_emotion2vec_state_dict

pytestmark = pytest.mark.gpu

FEAT_TOL = 1e-4
SCORE_BAR = 10 * orc.SCORE_GAP
# T = 1, 2: halos larger than the clip; 63, 64, 65: the 64-frame tile edge of the grouped convolution; 54, 55 and 118, 129:
# S = 10 + T at and across 64 and 128 in attention; N = 719, 961 = 3 x 320 + 1 and 3279: conv layers that drop trailing samples
FRAMES = (1, 2, 9, 10, 18, 19, 54, 55, 63, 64, 65, 118, 129)
LENGTHS = tuple(orc.samples_for_frames(T) for T in FRAMES) + (719, 961, orc.samples_for_frames(9, 319))


def rel(a, b):
    return float((a.double().cpu() - b).norm() / b.norm())


@pytest.fixture(scope="module")
def small():
    from targetdiarization_amd.emotion import Emotion2vec
    cfg = emotion2vec_config(orc.SMALL)
    sd = recipe_emotion2vec_state_dict(1, cfg)
    m = Emotion2vec(sd, "cuda:0")
    yield cfg, sd, m
    m.close()


@pytest.fixture(scope="module")
def runs(small):
    """every length once: the oracle in float64, and the device in ONE bucketed call with taps"""
    cfg, sd, m = small
    clips = [orc.clip(n, "len") for n in LENGTHS]
    want = [orc.forward(sd, c, cfg) for c in clips]
    taps = []
    feats = m.features(clips, taps=taps)
    gen = m.generate(clips, extract_embedding=True)
    return clips, want, feats, taps, gen


@pytest.mark.parametrize("i", range(len(LENGTHS)), ids=[str(n) for n in LENGTHS])
def test_small_config_lengths(runs, i):
    clips, want, feats, taps, gen = runs
    w = want[i]
    T = orc.frames(LENGTHS[i])
    assert feats[i].shape == w["feats"].shape == (T, 128)
    e_f, e_emb = rel(feats[i], w["feats"]), rel(torch.from_numpy(gen[i]["feats"]), w["emb"])
    e_p = float((torch.tensor(gen[i]["scores"], dtype=torch.float64) - w["scores"]).abs().max())
    print(f"N {LENGTHS[i]} T {T}: feats rel-L2 {e_f:.2e}, embedding {e_emb:.2e}, scores max abs {e_p:.2e} (bar {SCORE_BAR:.1e})")
    assert torch.isfinite(feats[i]).all()
    assert e_f < FEAT_TOL and e_emb < FEAT_TOL
    assert e_p <= SCORE_BAR
    assert gen[i]["key"] == f"rand_key_{i}" and len(gen[i]["labels"]) == 9 and abs(sum(gen[i]["scores"]) - 1.0) < 1e-5


@pytest.mark.parametrize("i", [0, 1, 5, 9, 10, 12, 13], ids=lambda i: str(LENGTHS[i]))
def test_positional_stack_alone(small, runs, i):
    """x + P(x) of the device's own projection: the grouped convolution cannot hide behind the end-to-end number"""
    cfg, sd, m = small
    clips, want, feats, taps, gen = runs
    x = taps[i]["proj"].double().cpu()
    ref = x + orc.positional(x, orc.cast(sd, torch.float64), cfg)
    e = rel(taps[i]["pos"], ref)
    print(f"N {LENGTHS[i]}: projection rel-L2 {rel(taps[i]['proj'], want[i]['proj']):.2e}, positional stack alone {e:.2e}")
    assert rel(taps[i]["proj"], want[i]["proj"]) < FEAT_TOL
    assert e < FEAT_TOL


@pytest.mark.parametrize("i", [0, 6, 7, 11, 12], ids=lambda i: str(LENGTHS[i]))
def test_attention_alone(small, runs, i):
    """the first block's attention of the device's own qkv, with the oracle's bias"""
    cfg, sd, m = small
    clips, want, feats, taps, gen = runs
    qkv = taps[i]["qkv"].double().cpu()
    T = qkv.shape[0] - cfg["E"]
    from targetdiarization_amd.weights import emotion2vec_upstream_name as up
    ref = orc.attention(qkv, orc.alibi_bias(sd[up("alibi_scale")], cfg["E"], T), cfg["H"])
    e = rel(taps[i]["attn"], ref)
    print(f"N {LENGTHS[i]} S {qkv.shape[0]}: attention alone rel-L2 {e:.2e}")
    assert e < FEAT_TOL
    if T > 1:                                        # the bias is there
        assert rel(taps[i]["attn"], orc.attention(qkv, None, cfg["H"])) > 100 * FEAT_TOL


def test_batch_of_three_against_single(small):
    """B = 3 against B = 1: a row's place in the GEMM tiles may move the last bit, no more"""
    cfg, sd, m = small
    for T in (9, 64, 129):
        n = orc.samples_for_frames(T)
        clips = [orc.clip(n, f"b{j}") for j in range(3)]
        together = m.features(clips)
        for j in range(3):
            alone = m.features([clips[j]])[0]
            d = float((alone - together[j]).abs().max())
            print(f"T {T} clip {j}: B = 3 against B = 1 max abs {d:.2e}")
            assert d <= 1e-6
            assert rel(together[j], orc.forward(sd, clips[j], cfg)["feats"]) < FEAT_TOL


def test_thirty_seconds(small):
    cfg, sd, m = small
    c = orc.clip(480000, "30s")
    w = orc.forward(sd, c, cfg)
    r = m.generate([c], granularity="frame", extract_embedding=True)[0]
    assert r["feats"].shape == (1499, 128)
    e_f = rel(torch.from_numpy(r["feats"]), w["feats"])
    e_p = float((torch.tensor(r["scores"], dtype=torch.float64) - w["scores"]).abs().max())
    print(f"30 s: feats rel-L2 {e_f:.2e}, scores max abs {e_p:.2e}")
    assert e_f < FEAT_TOL and e_p <= SCORE_BAR


def test_digital_silence(small):
    cfg, sd, m = small
    c = np.zeros(orc.samples_for_frames(20), dtype=np.float32)
    w = orc.forward(sd, c, cfg)
    r = m.generate([c], extract_embedding=True)[0]
    got = torch.tensor(r["scores"], dtype=torch.float64)
    assert np.isfinite(r["feats"]).all() and torch.isfinite(got).all()
    assert torch.argsort(got, descending=True).tolist() == torch.argsort(w["scores"], descending=True).tolist()
    assert float((got - w["scores"]).abs().max()) <= SCORE_BAR


@pytest.mark.parametrize("D,H", [(768, 12), (1024, 16)])
def test_real_widths(D, H):
    """C 512 with D 768 (group width 48) and D 1024 (group width 64), one prenet block + one main block, 2 s clips"""
    from targetdiarization_amd.emotion import Emotion2vec
    from targetdiarization_amd.weights import emotion2vec_upstream_name as up
    cfg = emotion2vec_config(C=512, D=D, H=H, prenet_depth=1, depth=1)
    sd = recipe_emotion2vec_state_dict(1, cfg)
    m = Emotion2vec(sd, "cuda:0")
    try:
        clips = [orc.clip(32000, f"w{j}") for j in range(2)]
        taps = []
        feats = m.features(clips, taps=taps)
        gen = m.generate(clips)
        sd64 = orc.cast(sd, torch.float64)
        for j, c in enumerate(clips):
            w = orc.forward(sd, c, cfg)
            e_f = rel(feats[j], w["feats"])
            x = taps[j]["proj"].double().cpu()
            e_pos = rel(taps[j]["pos"], x + orc.positional(x, sd64, cfg))
            qkv = taps[j]["qkv"].double().cpu()
            e_att = rel(taps[j]["attn"], orc.attention(qkv, orc.alibi_bias(sd[up("alibi_scale")], cfg["E"], qkv.shape[0] - cfg["E"]), H))
            e_p = float((torch.tensor(gen[j]["scores"], dtype=torch.float64) - w["scores"]).abs().max())
            print(f"D {D} clip {j}: feats {e_f:.2e}, positional alone {e_pos:.2e}, attention alone {e_att:.2e}, scores max abs {e_p:.2e}")
            assert feats[j].shape == (99, D)
            assert e_f < FEAT_TOL and e_pos < FEAT_TOL and e_att < FEAT_TOL
            assert e_p <= SCORE_BAR
    finally:
        m.close()


def test_top_one_label(small):
    cfg, sd, m = small
    clips = [orc.clip(orc.samples_for_frames(T), "score") for T in orc.SCORE_CLIP_FRAMES]
    want = [orc.forward(sd, c, cfg)["scores"] for c in clips]
    for w in want:                                   # before the device is looked at
        top = torch.sort(w, descending=True).values
        assert float(top[0] - top[1]) >= 100 * SCORE_BAR
    for r, w in zip(m.generate(clips), want):
        assert int(np.argmax(r["scores"])) == int(torch.argmax(w))
        assert float((torch.tensor(r["scores"], dtype=torch.float64) - w).abs().max()) <= SCORE_BAR


def test_asr_processor_emotion_detection(small):
    from targetdiarization_amd.asr_processor import ASRProcessor
    from targetdiarization_amd.emotion import DEFAULT_LABELS
    cfg, sd, _ = small
    p = ASRProcessor(is_emotion=True, emotion_state_dict=sd, verbose_log=False)
    assert p.is_emotion and p.emotion is not None
    try:
        a, b, c = (orc.clip(orc.samples_for_frames(T), "score") for T in (55, 9, 55))
        res = p.emotion_detection([a, b, c])
        assert len(res) == 3 and [r["key"] for r in res] == ["rand_key_0", "rand_key_1", "rand_key_2"]
        for r, clip in zip(res, (a, b, c)):
            w = orc.forward(sd, clip, cfg)["scores"]
            assert set(r) == {"key", "cls", "emotion", "label_score"} and r["cls"] in ("positive", "negative", "neutral")
            by_label = dict(r["label_score"])
            assert [s for _, s in r["label_score"]] == sorted(by_label.values(), reverse=True)
            for k, lab in enumerate(DEFAULT_LABELS):
                assert abs(by_label[lab] - float(w[k])) <= SCORE_BAR + 0.5e-6           # (+ the rounding to 6 places)
            assert r["emotion"] == DEFAULT_LABELS[int(torch.argmax(w))].split("/")[-1]
        one = p.emotion_detection(a, output_emotion_only=True)
        assert isinstance(one, str) and one == res[0]["emotion"]
        assert p.emotion_detection([a, b, c], output_emotion_only=True) == [r["emotion"] for r in res]
    finally:
        p.emotion.close()


def test_close_and_refusals():
    from targetdiarization_amd import _lib
    from targetdiarization_amd.emotion import Emotion2vec
    cfg = emotion2vec_config(orc.SMALL)
    sd = recipe_emotion2vec_state_dict(1, cfg)
    m = Emotion2vec(sd, "cuda:0")
    ok = orc.clip(orc.samples_for_frames(3), "ok")
    with pytest.raises(_lib.TdxError, match=r"clip 'short'.*399 samples"):
        m.generate([ok, ok[:399]], keys=["fine", "short"])
    tight = Emotion2vec(sd, "cuda:0", workspace_budget_bytes=1 << 16)
    with pytest.raises(_lib.TdxError, match=r"clip 'big'.*budget"):
        tight.generate([orc.clip(160000, "big")], keys=["big"])
    tight.close()
    assert len(m.generate([ok])) == 1
    m.close()
    m.close()
    with pytest.raises(_lib.TdxError):
        m.generate([ok])
    bad_cfg = emotion2vec_config(C=64, D=96, H=2, prenet_depth=1, depth=1)
    with pytest.raises(_lib.TdxError, match=r"D must be 64 x H"):
        Emotion2vec(recipe_emotion2vec_state_dict(1, bad_cfg), "cuda:0")
