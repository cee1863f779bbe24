"""CPU tests of Whisper's word-timestamp path.  tests/whisper_ts_oracle.py is pinned to the installed transformers: the median
filter and the time warping on random matrices, the token times against generate(..., return_token_timestamps=True) at batch size 1
(uncropped, and cropped through the route upstream honours on this path: an attention_mask over the mel frames; the plain
num_frames= keyword is ignored there), the word grouping against tokenization_whisper's functions with a WhisperTokenizer built
offline from a small synthetic vocab.json + merges.txt (that route constructs without network access, so no hand-written cases are
needed).  Then the host side of the engine: the OpenAI name map (transformers.models.whisper.convert_openai_to_hf does not import
here, so there is no comparison with its mapping), the argument validation of the two new entry points, and the result shapes of
generate / asr_detection / recognise_whisper with stub models.

Measured here: the oracle's fp32-vs-fp64 gap on the GPU test's alignment inputs (test_align_fp32_gap), the constant ALIGN_GAP."""
import os

os.environ["HF_HUB_OFFLINE"] = "1"
os.environ["TRANSFORMERS_OFFLINE"] = "1"

import json

import numpy as np
import pytest
import torch

import whisper_oracle as wo
import whisper_ts_oracle as ts
from targetdiarization_amd import _lib
from targetdiarization_amd import whisper as W
from targetdiarization_amd.weights import recipe_whisper_state_dict, whisper_config

CFG_S = dict(d_model=128, enc_heads=2, enc_layers=2, dec_layers=2, n_mels=80, vocab=51865, n_audio_ctx=100)
HEADS = [[1, 1], [0, 0], [1, 0]]


def hf_model(cfg, sd, dtype):
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    c = whisper_config(cfg)
    hc = WhisperConfig(vocab_size=c["vocab"], num_mel_bins=c["n_mels"], d_model=c["d_model"], encoder_layers=c["enc_layers"],
                       decoder_layers=c["dec_layers"], encoder_attention_heads=c["enc_heads"], decoder_attention_heads=c["dec_heads"],
                       encoder_ffn_dim=c["enc_ffn"], decoder_ffn_dim=c["dec_ffn"], max_source_positions=c["n_audio_ctx"],
                       max_target_positions=c["n_text_ctx"], activation_function=c["activation"])
    m = WhisperForConditionalGeneration(hc).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(dtype)


# ---- the oracle against upstream
@pytest.mark.parametrize("n,m", [(5, 9), (9, 5), (1, 7), (6, 1), (4, 3), (7, 2), (40, 60), (60, 40)])        # rows > frames, rows = 1, frames <= 3
def test_median_filter_and_dtw_are_upstreams(n, m):
    gw = pytest.importorskip("transformers.models.whisper.generation_whisper")
    rng = np.random.default_rng(100 * n + m)
    M = rng.standard_normal((n, m))
    a, b = gw._dynamic_time_warping(-M)
    for mode in ("double", "fp32"):                       # on fp64 noise the two roundings walk the same path
        c, d = ts.dtw(-M, mode)
        assert np.array_equal(a, c) and np.array_equal(b, d)
    jumps = np.pad(np.diff(a), (1, 0), constant_values=1).astype(bool)
    assert np.array_equal(ts.jump_frames(c, d), b[jumps]) and np.array_equal(ts.token_frames(M, "double"), b[jumps] if n > 1 else [0])
    x = torch.from_numpy(rng.standard_normal((2, 3, n, m)))
    for width in (1, 3, 7):
        assert torch.equal(gw._median_filter(x, width), ts.median_filter(x, width))
    w = torch.from_numpy(rng.random((3, n, m)))
    if n > 1:
        std, mean = torch.std(w, dim=-2, keepdim=True, unbiased=False), torch.mean(w, dim=-2, keepdim=True)
        assert torch.equal(ts.matrix(w), gw._median_filter((w - mean) / std, 7).mean(dim=0))


def test_align_fp32_gap():
    """the bar of the GPU test's matrix check: 10 x the oracle's own fp32-vs-fp64 gap on the same inputs (3e-7 .. 2e-6: a few
    units of the last place of values that reach sqrt(rows))"""
    for case in ts.ALIGN_CASES:
        if case[0] > 1:
            gap = ts.matrix_gap(ts.align_case(*case))
            print(f"{case}: gap {gap:.3e}")
            assert 0.5 * ts.ALIGN_GAP[case] <= gap <= 2.0 * ts.ALIGN_GAP[case]
    for n, m in ts.ALIGN_MIXED:
        if n > 1:
            gap = ts.matrix_gap(ts.align_case(n, m, ts.ALIGN_MIXED_HEADS, ts.ALIGN_MIXED_SEED))
            print(f"mixed {(n, m)}: gap {gap:.3e}")
            assert 0.5 * ts.ALIGN_MIXED_GAP[(n, m)] <= gap <= 2.0 * ts.ALIGN_MIXED_GAP[(n, m)]


@pytest.mark.parametrize("nframes", [None, 60, 61])
def test_token_times_are_generates(nframes):
    pytest.importorskip("transformers")
    cfg = whisper_config(CFG_S)
    sd = recipe_whisper_state_dict(1, cfg)
    gen = W.default_generation_config(cfg["vocab"])
    m = hf_model(cfg, sd, torch.float64)
    for k, v in gen.items():
        setattr(m.generation_config, k, v)
    m.generation_config.pad_token_id = gen["eos_token_id"]
    m.generation_config.alignment_heads = HEADS
    feats = torch.randn(1, cfg["n_mels"], 2 * cfg["n_audio_ctx"], generator=torch.Generator().manual_seed(7)).double()
    kw = {}
    if nframes is not None:                                 # the crop upstream honours: the mask's length in mel frames, halved
        kw["attention_mask"] = torch.zeros(1, 2 * cfg["n_audio_ctx"], dtype=torch.long)
        kw["attention_mask"][:, :2 * nframes] = 1
    with torch.no_grad():
        out = m.generate(input_features=feats, language="chinese", task="transcribe", num_beams=1, do_sample=False, max_new_tokens=12,
                         return_token_timestamps=True, return_dict_in_generate=True, **kw)
        prefix = W.decode_prefix("chinese", "transcribe", None, gen, cfg["n_text_ctx"])
        sd64 = wo.cast(sd)
        enc = wo.encoder(sd64, cfg, feats)
        toks = wo.greedy(sd64, cfg, enc, prefix, 12, gen["suppress_tokens"], gen["begin_suppress_tokens"], gen["eos_token_id"])[0]["tokens"]
        probs = ts.cross_attention(sd64, cfg, enc, torch.tensor([prefix + toks[:-1]]), HEADS)[0][:, len(prefix):]
    n = len(toks)
    assert out["sequences"][0].tolist()[-n:] == toks
    want = out["token_timestamps"][0].tolist()[-n:]       # generated ids only; the first time is 0
    frames = ts.token_frames(ts.matrix(probs[..., :nframes] if nframes else probs), "double")
    got = ts.token_times(frames, n)
    assert want[0] == 0.0 and len(set(want)) >= 5
    assert np.allclose(got, want, rtol=0, atol=1e-6), (got, want)
    assert ts.token_times([], 1) == [0.0]                   # a lone id: upstream returns zeros


# ---- word grouping
@pytest.fixture(scope="module")
def tiny_tokenizer(tmp_path_factory):
    tr = pytest.importorskip("transformers")
    enc = {b: ch for ch, b in W._BYTE_DECODER.items()}
    P = lambda bs: "".join(enc[b] for b in bs)
    han, wen = "中".encode(), "文".encode()
    pieces = [P(b" hello"), P(b" wor"), P(b"ld"), P(b","), P(b" ("), P(b"ok"), P(b")"), P(b"."), P(han[:2]), P(han[2:]), P(wen), P("。".encode()),
              P(b" \""), P(b"hi"), P(b"\""), P(b"!"), P(b" -"), P(b"x"), P(han[:1])]
    d = tmp_path_factory.mktemp("tok")
    with open(d / "vocab.json", "w", encoding="utf-8") as f:
        json.dump({p: i for i, p in enumerate(pieces)}, f)
    with open(d / "merges.txt", "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n")
    return tr.WhisperTokenizer(str(d / "vocab.json"), str(d / "merges.txt")), pieces, str(d / "vocab.json")


@pytest.mark.parametrize("ids,language", [
    ([0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15], "english"),            # leading and trailing punctuation merges
    ([16, 17, 0, 15, 15, 3, 1, 2], "english"), ([1, 2], "german"), ([3, 0], "english"),
    ([8, 9, 10, 11, 8, 9], "chinese"),                                 # the unicode split; a character across two tokens
    ([8, 9, 10, 11, 8, 9], "english"), ([10, 18, 10, 8], "chinese"),   # an incomplete character in the middle and at the end
    ([0, 10, 3, 8, 9, 7], "japanese"), ([], "english")])
def test_word_grouping_is_upstreams(tiny_tokenizer, ids, language):
    tw = pytest.importorskip("transformers.models.whisper.tokenization_whisper")
    tok, pieces, _ = tiny_tokenizer
    want = tw._combine_tokens_into_words(tok, list(ids), language) if ids else ([], [], [])
    got = W.combine_tokens_into_words(ids, pieces, language, eos=tok.eos_token_id)
    assert tuple(got) == tuple(want)
    oracle = ts.group_words(list(ids), lambda t: tok.decode(t, decode_with_timestamps=True), language, tok.eos_token_id)
    assert tuple(oracle) == tuple(want)


def test_word_timestamps(tiny_tokenizer):
    _, pieces, vocab_json = tiny_tokenizer
    assert W.load_token_list(vocab_json) == pieces
    ids, eos = [0, 1, 2, 3, 8, 9, 100], 100
    times = [0.0, 0.5, 0.7, 0.9, 1.0, 1.2, 1.2]
    assert W.word_timestamps(ids, times, pieces, "en", eos) == [(" hello", [0.0, 0.5]), (" world", [0.5, 0.9]), (",中", [0.9, 1.2])]
    assert W.word_timestamps(ids, times, pieces, "zh", eos) == [(" hello", [0.0, 0.5]), (" wor", [0.5, 0.7]), ("ld,", [0.7, 1.0]), ("中", [1.0, 1.2])]
    assert W.word_timestamps([5, 100], [0.0, 0.0], None, "en", eos) == [("<5>", [0.0, 0.0])]
    assert W.word_timestamps([100], [0.0], pieces, "en", eos) == []


# ---- the OpenAI checkpoint
def to_openai(sd):
    """transformers' names -> openai/whisper's, written out independently of the map under test"""
    out = {}
    for k, v in sd.items():
        if k == "proj_out.weight":
            continue
        k = k[len("model."):]
        for a, b in ((".self_attn_layer_norm.", ".attn_ln."), (".encoder_attn_layer_norm.", ".cross_attn_ln."), (".final_layer_norm.", ".mlp_ln."),
                     (".self_attn.q_proj.", ".attn.query."), (".self_attn.k_proj.", ".attn.key."), (".self_attn.v_proj.", ".attn.value."),
                     (".self_attn.out_proj.", ".attn.out."), (".encoder_attn.q_proj.", ".cross_attn.query."), (".encoder_attn.k_proj.", ".cross_attn.key."),
                     (".encoder_attn.v_proj.", ".cross_attn.value."), (".encoder_attn.out_proj.", ".cross_attn.out."), (".fc1.", ".mlp.0."),
                     (".fc2.", ".mlp.2."), (".layers.", ".blocks."), ("encoder.layer_norm.", "encoder.ln_post."), ("decoder.layer_norm.", "decoder.ln."),
                     ("embed_tokens.", "token_embedding."), ("encoder.embed_positions.weight", "encoder.positional_embedding"),
                     ("decoder.embed_positions.weight", "decoder.positional_embedding")):
            k = k.replace(a, b)
        out[k] = v
    return out


def test_openai_checkpoint_round_trip(tmp_path):
    cfg = whisper_config(d_model=128, enc_heads=2, enc_layers=2, dec_layers=3, n_mels=128, vocab=51866, n_audio_ctx=100, n_text_ctx=64)
    sd = recipe_whisper_state_dict(1, cfg)
    oa = to_openai(sd)
    assert "decoder.blocks.2.cross_attn.query.weight" in oa and "encoder.blocks.1.mlp.2.bias" in oa and "decoder.ln.weight" in oa
    assert "encoder.positional_embedding" in oa and "decoder.token_embedding.weight" in oa and not any(k.startswith("model.") for k in oa)
    dims = {"n_mels": 128, "n_audio_ctx": 100, "n_audio_state": 128, "n_audio_head": 2, "n_audio_layer": 2, "n_vocab": 51866, "n_text_ctx": 64,
            "n_text_state": 128, "n_text_head": 2, "n_text_layer": 3}
    path = str(tmp_path / "whisper_large_v3.pt")
    torch.save({"dims": dims, "model_state_dict": oa}, path)
    got, got_cfg = W.load_openai_checkpoint(path)
    assert got_cfg == cfg
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert got["proj_out.weight"] is got["model.decoder.embed_tokens.weight"]
    torch.save({"weights": oa}, str(tmp_path / "other.pt"))
    with pytest.raises(ValueError):
        W.load_openai_checkpoint(str(tmp_path / "other.pt"))
    assert W.default_alignment_heads(cfg) == [[1, 0], [1, 1], [2, 0], [2, 1]]            # the upper half of 3 layers, every head


# ---- the C-ABI without a device
@pytest.fixture(scope="module")
def lib():
    from targetdiarization_amd.build import build_lib
    build_lib()
    return _lib.lib()


def test_argument_validation_without_gpu(lib):
    err = lambda: lib.tdx_last_error().decode()
    dec = lambda nh, first_row, max_rows: lib.tdx_whisper_decode_xattn(None, None, 1, None, 0, None, 0, None, 0, 0, 0, None, nh, first_row, max_rows,
                                                                        None, None, None, None, None, 0, None)
    assert dec(0, 0, 4) == 1 and "tdx_whisper_decode_xattn: nh must be" in err()
    assert dec(65, 0, 4) == 1 and "nh must be" in err()
    assert dec(1, 0, 0) == 1 and "max_rows must be" in err()
    assert dec(1, -1, 4) == 1 and "first_row" in err()
    assert dec(1, 0, 4) == 1 and "heads_host" in err()
    assert lib.tdx_token_align_workspace_bytes(0, 1, 1, 1) == 0 and lib.tdx_token_align_workspace_bytes(1, 65, 1, 1) == 0
    assert lib.tdx_token_align_workspace_bytes(1, 1, 2049, 1) == 0 and lib.tdx_token_align_workspace_bytes(1, 1, 1, 0) == 0
    assert lib.tdx_token_align_workspace_bytes(2, 10, 447, 1500) >= 2 * (2 * 10 * 1500 * 4 + 447 * 1500 * 5)
    al = lambda B, nh, rows, S, width: lib.tdx_token_align(None, B, nh, rows, S, None, None, width, None, None, None, 0, None)
    for args, text in (((1, 0, 4, 4, 7), "nh must be"), ((1, 65, 4, 4, 7), "nh must be"), ((1, 1, 0, 4, 7), "max_rows must be"),
                       ((1, 1, 2049, 4, 7), "max_rows must be"), ((1, 1, 4, 4, 0), "median_width must be"), ((1, 1, 4, 4, 6), "median_width must be"),
                       ((1, 1, 4, 4, 33), "median_width must be"), ((0, 1, 4, 4, 7), "1 <= B"), ((1, 1, 4, 0, 7), "n_audio_ctx"), ((1, 1, 4, 4, 7), "NULL")):
        assert al(*args) == 1 and "tdx_token_align: " in err() and text in err(), (args, err())


# ---- generate / asr_detection / recognise_whisper with stub models
class FakeASR(W.WhisperASR):
    """WhisperASR.generate over fakes of the device calls: clip b "speaks" LANGS[b]; its ids are 100 + 10 b + step"""
    LANGS = ["en", "zh", "en", "ja"]

    def __init__(self, token_list=None):
        self.cfg = whisper_config(CFG_S)
        self.gen_cfg = W.default_generation_config(self.cfg["vocab"])
        self.token_list, self.tokenizer = token_list, None
        self.alignment_heads = HEADS
        self.device, self._h, self.n_samples = "cpu", 1, 32000
        self.calls = []

    def features(self, wavs, lens=None):
        return torch.tensor([[float(np.asarray(w).reshape(-1)[0])] for w in wavs])        # a clip's first sample names it

    def encode(self, feats, with_state=False):
        return feats, feats.reshape(1, 1, -1, 1, 1).clone()

    def detect_language(self, state):
        return [self.LANGS[int(v)] for v in state[0, 0, :, 0, 0].tolist()]

    def _run(self, state, prefix, max_new):
        who = [int(v) for v in state[0, 0, :, 0, 0].tolist()]
        self.calls.append((list(prefix), who))
        T = self.cfg["n_text_ctx"]
        ids = torch.full((len(who), T), -1, dtype=torch.int32)
        for k, b in enumerate(who):
            ids[k, len(prefix) - 1:len(prefix) - 1 + 3] = torch.tensor([100 + 10 * b, 101 + 10 * b, 50257], dtype=torch.int32)
        return ids, torch.zeros(len(who), T), torch.full((len(who),), 3, dtype=torch.int32)

    def decode(self, state, prefix, max_new, suppress=(), begin_suppress=(), eos=None):
        return self._run(state, prefix, max_new)

    def decode_xattn(self, state, prefix, max_new, suppress=(), begin_suppress=(), eos=None, **kw):
        return (*self._run(state, prefix, max_new), torch.zeros(state.shape[2], 3, max(1, max_new - 1), self.cfg["n_audio_ctx"]))


@pytest.fixture()
def fake(monkeypatch):
    def align(xattn, nrows, nframes, median_width=7, want_matrix=False):
        assert list(nrows) == [2] * xattn.shape[0] and all(1 <= f <= 100 for f in nframes)
        return torch.tensor([[5, 9] + [-1] * (xattn.shape[2] - 2)] * xattn.shape[0], dtype=torch.int32)
    monkeypatch.setattr(W, "token_align", align)
    return FakeASR()


def test_generate_groups_by_detected_language(fake):
    wavs = [np.full(3200 * (b + 1), float(b), dtype=np.float32) for b in range(4)]
    res = fake.generate(wavs, language="auto", max_new_tokens=8, return_timestamps=True)
    g = fake.gen_cfg
    assert [(p[1], who) for p, who in fake.calls] == [(g["lang_to_id"]["<|en|>"], [0, 2]), (g["lang_to_id"]["<|ja|>"], [3]), (g["lang_to_id"]["<|zh|>"], [1])]
    assert [r["key"] for r in res] == ["clip_0", "clip_1", "clip_2", "clip_3"] and [r["language"] for r in res] == FakeASR.LANGS
    for b, r in enumerate(res):
        assert r["token_ids"] == [100 + 10 * b, 101 + 10 * b, 50257]
        assert r["token_times"] == [5 * 0.02, 9 * 0.02, 9 * 0.02]
        assert r["words"] == [(f"<{100 + 10 * b}>", [5 * 0.02, 9 * 0.02]), (f"<{101 + 10 * b}>", [9 * 0.02, 9 * 0.02])]
    fake.calls.clear()
    plain = fake.generate(wavs, language="chinese", max_new_tokens=8)
    assert len(fake.calls) == 1 and fake.calls[0][1] == [0, 1, 2, 3]
    assert [set(r) for r in plain] == [{"key", "text", "token_ids", "scores"}] * 4          # the call without the new argument is unchanged
    assert fake.generate(wavs, language=None, max_new_tokens=8)[1]["language"] == "zh"


def test_asr_detection_whisper_v3(fake, capsys):
    from targetdiarization_amd.asr_processor import ASRProcessor
    p = ASRProcessor.__new__(ASRProcessor)
    p.is_asr, p.asr, p.decoder, p.verbose_log = True, {"whisper_v3": fake}, None, False
    wavs = [np.full(16000, float(b), dtype=np.float32) for b in range(2)]
    res = p.asr_detection(wavs, asr_engine="whisper_v3", language="auto")
    assert [set(r) for r in res] == [{"key", "language", "text", "timestamp"}] * 2
    assert [r["language"] for r in res] == ["en", "zh"] and [r["key"] for r in res] == ["0", "1"]
    assert res[1]["timestamp"] == [("<110>", [0.1, 0.18]), ("<111>", [0.18, 0.18])] and res[1]["text"] == "<110><111>"
    fixed = p.asr_detection(wavs, asr_engine="whisper_v3", language="Chinese", prompt="hello")
    assert [r["language"] for r in fixed] == ["zh", "zh"] and "prompt is ignored" in capsys.readouterr().out
    raw = p.asr_detection(wavs, asr_engine="whisper_v3", output_raw_result=True)
    assert set(raw[0]) == {"key", "text", "token_ids", "scores", "language", "token_times", "words"}
    assert p.asr_detection(wavs, asr_engine="whisper_v3", output_text_only=True) == "<100><101><110><111>"


def test_recognise_whisper_offsets_segments(fake):
    from targetdiarization_amd.pipeline import HotPath
    hp = HotPath.__new__(HotPath)
    hp.whisper, hp.asr_segment, hp.device = fake, 16000, "cpu"
    streams = [torch.cat([torch.full((16000,), 0.0), torch.full((8000,), 1.0)]), torch.full((12000,), 2.0)]
    out = hp.recognise_whisper(streams, language="auto", timestamps=True)
    assert [len(o) for o in out] == [2, 1]
    assert [seg["offset"] for seg in out[0]] == [0.0, 1.0] and out[1][0]["offset"] == 0.0
    assert out[0][1]["words"] == [("<110>", [1.1, 1.18]), ("<111>", [1.18, 1.18])] and out[0][1]["token_times"] == [1.1, 1.18, 1.18]
    assert out[0][0]["words"] == [("<100>", [0.1, 0.18]), ("<101>", [0.18, 0.18])] and out[0][1]["language"] == "zh"
    plain = hp.recognise_whisper(streams)
    assert [len(o) for o in plain] == [2, 1] and all(set(seg) == {"key", "text", "token_ids", "scores"} for o in plain for seg in o)
