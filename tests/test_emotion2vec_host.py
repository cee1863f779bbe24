"""CPU tests of emotion2vec's host side: the oracle's convolutional front end against transformers' Data2VecAudio modules, its
ALiBi bias, the sensitivity of the test clips to the bias and to the prefix tokens, the frame count, the loader, and
emotion_detection's post-processing with a stub model."""
import numpy as np
import pytest
import torch

import emotion2vec_oracle as orc
from targetdiarization_amd import _lib, emotion
from targetdiarization_amd.asr_processor import ASRProcessor
from targetdiarization_amd.weights import (emotion2vec_config, emotion2vec_frames, emotion2vec_param_shapes, emotion2vec_upstream_name as up,
                                           recipe_emotion2vec_state_dict)

FEAT_TOL = 1e-4                          # the GPU tests' rel-L2 bound on features
SCORE_BAR = 10 * orc.SCORE_GAP           # and their bound on probabilities


@pytest.fixture(scope="module")
def small():
    cfg = emotion2vec_config(orc.SMALL)
    return cfg, recipe_emotion2vec_state_dict(1, cfg)


@pytest.fixture(scope="module")
def score_runs(small):
    cfg, sd = small
    clips = [orc.clip(orc.samples_for_frames(T), "score") for T in orc.SCORE_CLIP_FRAMES]
    return clips, [orc.forward(sd, c, cfg) for c in clips]


def test_front_end_equals_transformers():
    """oracle steps 2-4 == Data2VecAudioFeatureEncoder, FeatureProjection, PositionalConvEmbedding in float64, 1e-10 relative"""
    tr = pytest.importorskip("transformers")
    from transformers.models.data2vec.modeling_data2vec_audio import (Data2VecAudioFeatureEncoder, Data2VecAudioFeatureProjection,
                                                                        Data2VecAudioPositionalConvEmbedding)
    cfg = emotion2vec_config(C=32, D=128, H=2, prenet_depth=1, depth=1)
    sd = orc.cast(recipe_emotion2vec_state_dict(3, cfg), torch.float64)
    hc = tr.Data2VecAudioConfig(conv_bias=False, num_conv_pos_embeddings=5, conv_pos_kernel_size=19, num_conv_pos_embedding_groups=16,
                                conv_dim=(32,) * 7, hidden_size=128, feat_proj_dropout=0.0, layer_norm_eps=1e-5)
    enc, proj, pos = (m(hc).double().eval() for m in (Data2VecAudioFeatureEncoder, Data2VecAudioFeatureProjection, Data2VecAudioPositionalConvEmbedding))
    with torch.no_grad():
        for i, layer in enumerate(enc.conv_layers):
            layer.conv.weight.copy_(sd[up("conv.{n}.weight", i)])
            layer.layer_norm.weight.copy_(sd[up("conv.{n}.ln.weight", i)])
            layer.layer_norm.bias.copy_(sd[up("conv.{n}.ln.bias", i)])
        proj.layer_norm.weight.copy_(sd[up("proj.ln.weight")])
        proj.layer_norm.bias.copy_(sd[up("proj.ln.bias")])
        proj.projection.weight.copy_(sd[up("proj.weight")])
        proj.projection.bias.copy_(sd[up("proj.bias")])
        for l, layer in enumerate(pos.layers):
            layer.conv.weight.copy_(sd[up("pos.{n}.weight", l)])
            layer.conv.bias.copy_(sd[up("pos.{n}.bias", l)])
        for n in (400 + 3 * 320, 719, 5000):
            x = orc.normalize(torch.from_numpy(orc.clip(n, "hf")).double())
            f = orc.feature_extractor(x, sd, cfg)
            ref_f = enc(x[None])[0].transpose(0, 1)
            assert f.shape == ref_f.shape == (orc.frames(n), 32)
            assert (f - ref_f).norm() <= 1e-10 * ref_f.norm()
            p = orc.project(f, sd)
            ref_p = proj(ref_f[None])[0][0]
            assert (p - ref_p).norm() <= 1e-10 * ref_p.norm()
            q = orc.positional(p, sd, cfg)
            ref_q = pos(ref_p[None])[0]
            assert (q - ref_q).norm() <= 1e-10 * ref_q.norm()
    assert orc.frames(400 + 3 * 320) == 4


@pytest.mark.parametrize("H", [2, 12, 16])
def test_alibi_slopes(H):
    s = orc.alibi_slopes(H)
    assert len(s) == H
    if H & (H - 1) == 0:
        assert np.allclose(s, [2.0 ** (-8.0 * (h + 1) / H) for h in range(H)], rtol=1e-15)
    else:                                  # 12: the 8 slopes of 8 heads, then every other one of the 16-head series
        assert np.allclose(s[:8], [2.0 ** (-(h + 1)) for h in range(8)], rtol=1e-15)
        assert np.allclose(s[8:], [2.0 ** (-0.5 * (2 * h + 1)) for h in range(4)], rtol=1e-15)


def test_alibi_bias_prefix_and_clamp():
    scale = torch.tensor([1.5, -0.5, 0.0, 2.0]).reshape(1, 1, 4, 1, 1)
    E, T = 3, 5
    b = orc.alibi_bias(scale, E, T)
    assert b.shape == (4, 8, 8)
    assert (b[:, :E, :] == 0).all() and (b[:, :, :E] == 0).all()          # bias-free prefix rows and columns
    assert (b[1] == 0).all() and (b[2] == 0).all()                        # the clamp at 0 from below
    sl = orc.alibi_slopes(4)
    for i in range(T):
        for j in range(T):
            assert b[0, E + i, E + j].item() == pytest.approx(-sl[0] * 1.5 * abs(i - j), rel=1e-15)
            assert b[3, E + i, E + j].item() == pytest.approx(-sl[3] * 2.0 * abs(i - j), rel=1e-15)
    assert torch.equal(b, b.transpose(1, 2))


def test_recipe_exercises_clamp_and_prefix(small):
    cfg, sd = small
    sc = sd[up("alibi_scale")].reshape(-1)
    assert (sc < 0).sum() == 1 and sc[sc > 0].min() >= 0.5 and sc.max() <= 2.0
    assert sd[up("extra_tokens")].abs().min() > 0 or sd[up("extra_tokens")].abs().mean() > 0.1
    big = recipe_emotion2vec_state_dict(1, emotion2vec_config(prenet_depth=1, depth=1))[up("alibi_scale")].reshape(-1)
    assert (big < 0).sum() == 1 and big.numel() == 16


def test_bias_and_prefix_matter(small, score_runs):
    """without the ALiBi bias, or with a zero prefix, the oracle moves by >= 100 x the GPU tolerances on the test clips: a
    device path that lacks either cannot pass the GPU tests"""
    cfg, sd = small
    clips, full = score_runs
    for c, ref in zip(clips, full):
        for kw in (dict(use_bias=False), dict(zero_extra=True)):
            alt = orc.forward(sd, c, cfg, **kw)
            rel = float((alt["feats"] - ref["feats"]).norm() / ref["feats"].norm())
            dp = float((alt["scores"] - ref["scores"]).abs().max())
            assert rel >= 100 * FEAT_TOL, (kw, rel)
            assert dp >= 100 * SCORE_BAR, (kw, dp)


def test_score_gap_constant(small, score_runs):
    """SCORE_GAP is the oracle's own float32-versus-float64 gap on the score clips (max abs over the probabilities).  The float32
    run depends on how torch's BLAS splits its sums: 2.6e-7 with one thread, 3.2e-7 with four, 4.4e-7 with eight and more were
    measured; the constant is the largest of them, and this test only keeps it honest to within that spread (x 1/4 .. x 2)."""
    cfg, sd = small
    clips, full = score_runs
    gap = max(float((orc.forward(sd, c, cfg, dtype=torch.float32)["scores"].double() - r["scores"]).abs().max()) for c, r in zip(clips, full))
    print(f"measured float32 - float64 score gap: {gap:.3e} (SCORE_GAP = {orc.SCORE_GAP:.1e})")
    assert 0.25 * orc.SCORE_GAP <= gap <= 2.0 * orc.SCORE_GAP


def test_top_two_gap_of_score_clips(score_runs):
    """the clips of the GPU top-1 test: the oracle's top two probabilities are >= 100 x the score bar apart"""
    for r in score_runs[1]:
        top = torch.sort(r["scores"], descending=True).values
        assert float(top[0] - top[1]) >= 100 * SCORE_BAR


@pytest.mark.parametrize("n,T", [(400, 1), (719, 1), (720, 2), (480000, 1499), (399, 0)])
def test_frame_count(n, T):
    assert emotion2vec_frames(n) == T == orc.frames(n)
    if T:
        assert T == (n - 400) // 320 + 1


def test_loader_infers_dimensions(small):
    cfg, sd = small
    got = emotion.infer_config(sd)
    assert got == cfg
    assert got["conv_strides"] == (5, 2, 2, 2, 2, 2, 2) and got["pos_groups"] == 16 and got["pos_k"] == 19 and got["n_classes"] == 9
    assert emotion.infer_config(sd, {"conv_strides": (5, 2, 2, 2, 2, 2, 1)})["conv_strides"][-1] == 1
    big = {k: torch.empty(s, device="meta") for k, s in emotion2vec_param_shapes(emotion2vec_config()).items()}
    c = emotion.infer_config(big)
    assert (c["C"], c["D"], c["H"], c["E"], c["prenet_depth"], c["depth"]) == (512, 1024, 16, 10, 4, 24)
    with pytest.raises(_lib.TdxError, match="config says D"):
        emotion.infer_config(sd, {"D": 256})


def test_loader_ignores_and_reports(small):
    cfg, sd = small
    extra = dict(sd)
    extra["modality_encoders.AUDIO.decoder.blocks.0.0.weight"] = torch.zeros(3)
    extra["_ema.blocks.0.attn.qkv.weight"] = torch.zeros(3)
    extra["modality_encoders.AUDIO.mask_emb"] = torch.zeros(3)
    blob = emotion.to_blob_state(extra, emotion.infer_config(extra))
    assert len(blob) == len(sd) and set(blob) == set(emotion.to_blob_state(sd, cfg))
    assert torch.equal(blob["pos.0.weight"], sd["modality_encoders.AUDIO.relative_positional_encoder.1.0.weight"])
    assert torch.equal(blob["head.weight"], sd["proj.weight"]) and torch.equal(blob["prenet.blocks.0.mlp.fc1.bias"],
                                                                               sd["modality_encoders.AUDIO.context_encoder.blocks.0.mlp.fc1.bias"])
    for name in ("blocks.1.mlp.fc2.bias", up("conv.{n}.ln.weight", 3), up("pos.{n}.bias", 4), up("prenet.norm.weight"), "proj.bias"):
        miss = {k: v for k, v in sd.items() if k != name}
        with pytest.raises(_lib.TdxError, match="tensor missing.*" + name.replace(".", r"\.")):
            emotion.to_blob_state(miss, emotion.infer_config(miss) if name != "blocks.1.mlp.fc2.bias" else cfg)
    bad = dict(sd)
    bad["blocks.0.attn.qkv.weight"] = sd["blocks.0.attn.qkv.weight"].t().contiguous()
    with pytest.raises(_lib.TdxError, match=r"wrong shape: blocks\.0\.attn\.qkv\.weight"):
        emotion.to_blob_state(bad, cfg)
    odd = dict(sd)
    odd["blocks.0.attn.extra"] = torch.zeros(1)
    with pytest.raises(_lib.TdxError, match=r"unexpected tensor: blocks\.0\.attn\.extra"):
        emotion.to_blob_state(odd, cfg)


def test_load_state_dict_reads_model_pt_and_tokens(tmp_path, small):
    cfg, sd = small
    torch.save({"model": dict(sd)}, tmp_path / "model.pt")
    (tmp_path / "tokens.txt").write_text("\n".join(emotion.DEFAULT_LABELS) + "\n", encoding="utf-8")
    got, labels = emotion.load_state_dict(str(tmp_path))
    assert set(got) == set(sd) and labels == list(emotion.DEFAULT_LABELS) and len(labels) == 9
    torch.save(dict(sd), tmp_path / "model.pt")
    assert set(emotion.load_state_dict(str(tmp_path))[0]) == set(sd)


class StubEmotion:
    """stands where funasr's model stands: fixed scores per clip"""
    def __init__(self, rows, labels=emotion.DEFAULT_LABELS):
        self.rows, self.labels, self.calls = rows, list(labels), 0

    def __call__(self, wavs, granularity="utterance", extract_embedding=False):
        assert granularity == "utterance" and extract_embedding is False and isinstance(wavs, list)
        self.calls += 1
        return [{"key": f"rand_key_{i}", "labels": list(self.labels), "scores": list(self.rows[i])} for i in range(len(wavs))]


def _proc(rows, **kw):
    p = ASRProcessor(verbose_log=False)
    p.is_emotion, p.emotion = True, StubEmotion(rows, **kw)
    return p


def _row(idx, top):
    r = [(1.0 - top) / 8] * 9
    r[idx] = top
    return r


def test_emotion_detection_postprocessing():
    wav = np.zeros(16000, dtype=np.float32)
    names = [l.split("/")[-1] for l in emotion.DEFAULT_LABELS]
    # 0.95 exactly -> the class; just below -> neutral
    assert _proc([_row(3, 0.95)]).emotion_detection(wav)[0]["cls"] == "positive"
    assert _proc([_row(3, 0.949999)]).emotion_detection(wav)[0]["cls"] == "neutral"
    assert _proc([_row(0, 0.9499996)]).emotion_detection(wav)[0]["cls"] == "negative"      # rounds to 0.95 at 6 places
    for i, n in enumerate(names):
        r = _proc([_row(i, 0.99)]).emotion_detection(wav)
        assert r[0]["emotion"] == n and r[0]["key"] == "rand_key_0"
        assert r[0]["cls"] == ("negative" if n in ("fearful", "disgusted", "sad", "angry") else "positive")
    assert {n for n in names if n in ("fearful", "disgusted", "sad", "angry")} == {"fearful", "disgusted", "sad", "angry"}
    r = _proc([_row(8, 0.99)]).emotion_detection(wav)[0]
    assert r["emotion"] == "<unk>" and r["cls"] == "positive"
    # label_score: (label, rounded score) sorted descending
    row = [0.1234564, 0.3, 0.05, 0.2, 0.0765436, 0.1, 0.05, 0.06, 0.04]
    ls = _proc([row]).emotion_detection(wav)[0]["label_score"]
    assert ls[0] == (emotion.DEFAULT_LABELS[1], 0.3) and ls[2] == (emotion.DEFAULT_LABELS[0], 0.123456)
    assert [s for _, s in ls] == sorted((round(v, 6) for v in row), reverse=True)
    # the "excited" exception
    assert _proc([[0.99, 0.01]], labels=["兴奋/excited", "难过/sad"]).emotion_detection(wav)[0]["cls"] == "neutral"
    assert _proc([[0.01, 0.99]], labels=["兴奋/excited", "难过/sad"]).emotion_detection(wav)[0]["cls"] == "negative"


def test_emotion_detection_one_clip_versus_list_and_not_loaded(capsys):
    wav = np.zeros(16000, dtype=np.float32)
    p = _proc([_row(6, 0.99), _row(3, 0.5), _row(4, 0.97)])
    assert p.emotion_detection(wav, output_emotion_only=True) == "sad"
    assert p.emotion_detection([wav], output_emotion_only=True) == "sad"
    assert p.emotion_detection([wav, wav, wav], output_emotion_only=True) == ["sad", "happy", "neutral"]
    calls = p.emotion.calls
    res = p.emotion_detection([wav, wav, wav])
    assert p.emotion.calls == calls + 1                                   # a list is one generate call
    assert [r["cls"] for r in res] == ["negative", "neutral", "positive"] and set(res[0]) == {"key", "cls", "emotion", "label_score"}
    with pytest.raises(ValueError, match="16 kHz float32"):
        p.emotion_detection("clip.wav")
    off = ASRProcessor(verbose_log=False)
    assert off.is_emotion is False and off.emotion_detection(wav) == [] and off.emotion_detection(wav, output_emotion_only=True) == ""
    failed = ASRProcessor(verbose_log=False, is_emotion=True, emotion_model_dir="/nonexistent/dir")
    assert failed.is_emotion is False and failed.emotion_detection(wav) == []
    assert "Failed to load Modelscope emotion detection model" in capsys.readouterr().out


def _cabi_create(**kw):
    """tdx_emo2v_create with a config alone: the refusals below come before the blob or the device is looked at"""
    import ctypes as C
    l = _lib.lib()
    cc = _lib.Emo2vConfig()
    base = dict(C=64, D=128, H=2, E=10, prenet_depth=1, depth=1, n_conv=7, pos_layers=5, pos_k=19, pos_groups=16, n_classes=9)
    base.update(kw)
    for k, v in base.items():
        setattr(cc, k, v)
    for i, (k, s) in enumerate(zip((10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2))):
        cc.conv_k[i], cc.conv_s[i] = k, s
    h = C.c_void_p()
    blob = (C.c_char * 64)()
    rc = l.tdx_emo2v_create(C.byref(cc), blob, 64, 0, C.byref(h))
    return rc, l.tdx_last_error().decode(), h.value


@pytest.mark.parametrize("kw,msg", [(dict(D=96, H=2), "D must be 64 x H"), (dict(D=128, H=2, pos_groups=24), "divisible by the group count"),
                                    (dict(D=192, H=3, pos_groups=32), "multiple of 4"), (dict(D=1024, H=16, pos_groups=8), "at most 64"),
                                    (dict(C=96), "multiple of 64")])
def test_create_refuses_with_a_message(kw, msg):
    rc, err, h = _cabi_create(**kw)
    assert rc != 0 and h is None and msg in err


def test_create_reaches_the_blob_with_a_good_config():
    rc, err, h = _cabi_create()
    assert rc != 0 and h is None and "malformed TDXW blob" in err
    l = _lib.lib()
    assert l.tdx_emo2v_workspace_bytes(None, 1, 16000) == 0 and l.tdx_emo2v_frames(None, 16000) == 0 and l.tdx_emo2v_destroy(None) == 0
