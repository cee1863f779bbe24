"""CPU tests of the SenseVoice host side: the fp64 oracle's own invariants, tag parsing, loader errors (no device is touched before
the blob is accepted), the server's environment keys, and that the default engine's construction is what it was."""
import ctypes as C

import pytest
import torch

import sensevoice_cases as sc
import sensevoice_oracle as orc


def test_oracle_prompt_order_and_positions():
    sd = {k: v.double() for k, v in sc.state_dict("small").items()}
    f = sc.feats(2, 7).double()
    x = orc.encoder_input(f, sd, "en", use_itn=False)
    assert x.shape == (2, 11, 560)
    pe = orc.sinusoidal_pe(11, 560, torch.float64)
    rows = (x - pe[None]) / 512 ** 0.5
    for s, i in enumerate([4, 1, 2, 15]):                      # [embed[lid], embed[1], embed[2], embed[textnorm], feats...]
        assert torch.allclose(rows[:, s], sd["embed.weight"][i].expand(2, -1), atol=1e-12)
    assert torch.allclose(rows[:, 4:], f, atol=1e-12)
    assert torch.equal(orc.prompt_rows(sd, "klingon", True), sd["embed.weight"][torch.tensor([0, 1, 2, 14])])      # unknown language: auto


def test_oracle_batch_equals_single_clips():
    sd = {k: v.double() for k, v in sc.state_dict("small").items()}
    f = sc.feats(3, 37).double()
    enc, lp, ids, toks = orc.greedy_decode(f, sd, 2, 1)
    for b in range(3):
        e1, l1, i1, t1 = orc.greedy_decode(f[b:b + 1], sd, 2, 1)
        assert float((e1[0] - enc[b]).abs().max()) < 1e-10 and torch.equal(i1[0], ids[b]) and t1[0] == toks[b]


def test_oracle_collapse():
    assert orc.collapse([0, 0, 0]) == ([], [])
    assert orc.collapse([7, 7, 0, 7]) == ([7, 7], [0, 3])
    assert orc.collapse([3, 3, 5, 5, 2]) == ([3, 5, 2], [0, 2, 4])
    assert orc.collapse([5]) == ([5], [0])


@pytest.mark.parametrize("depth", ["small"])
def test_oracle_margin_cap_of_the_cases(depth):
    """the seeds of the GPU cases: the fp64 oracle alone leaves at most 1 % of a case's frames under the 1e-3 margin rule, about
    half of the frames are blank and the collapse has repeats to drop (the full-depth cases assert the cap on the GPU run)"""
    for (B, T) in sc.SHAPES + [sc.LONG_SHAPE]:
        r = sc.reference(depth, B, T)
        n = r["ids"].numel()
        assert int((r["margin"] <= sc.MARGIN).sum()) <= n // 100
        if n > 100:
            assert 0.25 < float((r["ids"] == 0).float().mean()) < 0.75
            rows = r["ids"].tolist()
            assert sum(1 for row in rows for i in range(1, len(row)) if row[i] == row[i - 1] and row[i] != 0) > 0


def test_tag_parsing_and_fallback():
    from targetdiarization_amd.sensevoice import join_text_only, parse_tagged_text
    assert parse_tagged_text("<|EN|><|NEUTRAL|><|Speech|><|withitn|>Hello, World.") == ("en", "neutral", "Hello, World.")
    assert parse_tagged_text("<|EN|><|NEUTRAL|><|Speech|><|withitn|>Hello, World.", no_punc=True) == ("en", "neutral", "hello world")
    assert parse_tagged_text("<|zh|><|SAD|><|Speech|><|woitn|>你 好 <|zh|><|SAD|><|Speech|><|woitn|>吗") == ("zh", "sad", "你好吗")
    assert parse_tagged_text("no tags here") == ("", "", "no tags here")
    assert parse_tagged_text("<|en|><|HAPPY|><|Speech|><|withitn|>") == ("", "", "<|en|><|HAPPY|><|Speech|><|withitn|>")   # nothing after the tags
    assert join_text_only([{"text": "a."}, {"text": ""}, {"text": "b"}, {"text": "c,"}]) == "a. bc, "


def test_prompt_id_tables():
    from targetdiarization_amd.sensevoice import SenseVoiceSmall
    ids = {l: SenseVoiceSmall.prompt_ids(l)[0] for l in ("auto", "zh", "en", "yue", "ja", "ko", "nospeech", "fr")}
    assert ids == {"auto": 0, "zh": 3, "en": 4, "yue": 7, "ja": 11, "ko": 12, "nospeech": 13, "fr": 0}
    assert SenseVoiceSmall.prompt_ids("EN", True) == [4, 1, 2, 14] and SenseVoiceSmall.prompt_ids("en", False) == [4, 1, 2, 15]


def test_loader_reports_a_missing_tensor():
    from targetdiarization_amd import _lib
    from targetdiarization_amd.build import build_lib
    from targetdiarization_amd.weights import pack_blob
    build_lib()
    l = _lib.lib()
    for name in ("embed.weight", "encoder.tp_norm.bias", "encoder.tp_encoders.0.feed_forward.w_2.weight", "ctc.ctc_lo.weight"):
        sd = dict(sc.state_dict((1, 1)))
        sd.pop(name)
        blob = pack_blob(sd)
        h = C.c_void_p()
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        assert l.tdx_sv_create(1, 1, sc.VOCAB, buf, len(blob), 0, C.byref(h)) == 2
        assert name.encode() in l.tdx_last_error()
    sd = dict(sc.state_dict((1, 1)))
    sd["ctc.ctc_lo.weight"] = sd["ctc.ctc_lo.weight"].t().contiguous()       # transposed: right size, wrong shape
    blob = pack_blob(sd)
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    h = C.c_void_p()
    assert l.tdx_sv_create(1, 1, sc.VOCAB, buf, len(blob), 0, C.byref(h)) == 2 and b"ctc.ctc_lo.weight" in l.tdx_last_error()
    assert l.tdx_sv_create(0, 1, sc.VOCAB, buf, len(blob), 0, C.byref(h)) == 1
    assert l.tdx_sv_workspace_bytes(None, 1, 10) == 0
    assert l.tdx_ctc_collapse(None, 1, 1, 0, None, None, None, None) == 1


def test_env_to_kwargs_keys(tmp_path):
    from targetdiarization_amd.sensevoice import load_token_list
    from targetdiarization_amd.server import env_to_kwargs
    base = env_to_kwargs({})
    assert "sensevoice_model_dir" not in base and "sensevoice_token_file" not in base
    assert env_to_kwargs({"SENSEVOICE_MODEL_DIR": "d", "SENSEVOICE_TOKEN_FILE": "t"}) == dict(base, sensevoice_model_dir="d", sensevoice_token_file="t")
    j, t = tmp_path / "tokens.json", tmp_path / "tokens.txt"
    j.write_text('["<|zh|>", "\\u2581a", "b"]', encoding="utf-8")
    t.write_text("<|zh|>\n▁a\nb\n", encoding="utf-8")
    assert load_token_list(str(j)) == load_token_list(str(t)) == ["<|zh|>", "▁a", "b"]
    assert load_token_list(str(tmp_path / "absent")) is None and load_token_list(None) is None


def test_default_engine_construction_unchanged(capsys):
    """no SenseVoice weights: nothing is loaded, asr_engine stays a stored name, and asr_detection without models answers as before"""
    import inspect
    from targetdiarization_amd.asr_processor import ASRProcessor
    from targetdiarization_amd.sensevoice import build_sensevoice
    from targetdiarization_amd.target_diarization import TargetDiarization
    assert build_sensevoice() is None and build_sensevoice(model_dir="no/such/dir") is None
    sig = inspect.signature(TargetDiarization.__init__).parameters
    assert sig["asr_engine"].default == "paraformer" and sig["sensevoice_state_dict"].default is None
    asr = ASRProcessor(is_asr=True, verbose_log=False)
    assert asr.asr == {} and asr.decoder is None
    assert asr.asr_detection(torch.zeros(16000).numpy(), asr_engine="sensevoice") == []
    assert asr.asr_detection(torch.zeros(16000).numpy(), output_text_only=True) == ""
    assert "ASR models haven't been loaded" in capsys.readouterr().out
