"""CPU tests of the Whisper engine's host side.  tests/whisper_oracle.py is pinned to the installed transformers (the log-mel front
end, the encoder, teacher-forced logits, greedy decoding under decode_prefix() against generate()); the language table, the
parameter layout, decode_text, the loader's checks and the argument validation of the C-ABI run without a device.

Measured here (fp32-vs-fp64 gap of the oracle's log-mel on the GPU test's inputs): see test_logmel_fp32_gap."""
import os

os.environ["HF_HUB_OFFLINE"] = "1"
os.environ["TRANSFORMERS_OFFLINE"] = "1"

import ctypes as C

import numpy as np
import pytest
import torch

import whisper_oracle as wo
import whisper_widths_cases as wc
from targetdiarization_amd import _lib
from targetdiarization_amd import whisper as W
from targetdiarization_amd.weights import pack_blob, recipe_whisper_state_dict, whisper_config, whisper_param_shapes

CFG_S = dict(d_model=128, enc_heads=2, enc_layers=2, dec_layers=2, n_mels=80, vocab=51865, n_audio_ctx=100)
CFG_T = dict(d_model=192, enc_heads=3, enc_layers=1, dec_layers=1, n_mels=128, vocab=51866, n_audio_ctx=100)


def hf_config(cfg):
    from transformers import WhisperConfig
    c = whisper_config(cfg)
    return WhisperConfig(vocab_size=c["vocab"], num_mel_bins=c["n_mels"], d_model=c["d_model"], encoder_layers=c["enc_layers"],
                         decoder_layers=c["dec_layers"], encoder_attention_heads=c["enc_heads"], decoder_attention_heads=c["dec_heads"],
                         encoder_ffn_dim=c["enc_ffn"], decoder_ffn_dim=c["dec_ffn"], max_source_positions=c["n_audio_ctx"],
                         max_target_positions=c["n_text_ctx"], activation_function=c["activation"])


def hf_model(cfg, sd, dtype):
    from transformers import WhisperForConditionalGeneration
    m = WhisperForConditionalGeneration(hf_config(cfg)).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(dtype)


clips_for_logmel = wo.logmel_test_clips


@pytest.fixture(scope="module")
def small():
    cfg = whisper_config(CFG_S)
    return cfg, recipe_whisper_state_dict(1, cfg)


def test_language_table_is_upstreams():
    tw = pytest.importorskip("transformers.models.whisper.tokenization_whisper")
    assert list(tw.LANGUAGES.items()) == list(W.LANGUAGES)
    for name, code in tw.TO_LANGUAGE_CODE.items():
        assert W.language_code(name) == code
    assert W.language_code("<|zh|>") == "zh" and W.language_code("ZH") == "zh"
    with pytest.raises(ValueError):
        W.language_code("klingon")


@pytest.mark.parametrize("cfg", [CFG_S, CFG_T])
def test_param_shapes_are_upstreams(cfg):
    tr = pytest.importorskip("transformers")
    m = tr.WhisperForConditionalGeneration(hf_config(cfg))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(whisper_param_shapes(cfg))
    sd = recipe_whisper_state_dict(1, cfg)
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(whisper_param_shapes(cfg))
    assert sd["proj_out.weight"] is sd["model.decoder.embed_tokens.weight"]
    assert torch.equal(recipe_whisper_state_dict(1, cfg)["model.decoder.layers.0.fc1.weight"], sd["model.decoder.layers.0.fc1.weight"])


@pytest.mark.parametrize("n_mels,n_audio_ctx", [(80, 1500), (128, 1500), (80, 100)])
def test_logmel_matches_feature_extractor(n_mels, n_audio_ctx):
    tr = pytest.importorskip("transformers")
    fe = tr.WhisperFeatureExtractor(feature_size=n_mels, chunk_length=n_audio_ctx // 50)
    clips = clips_for_logmel(n_audio_ctx)
    ref = fe([c.numpy() for c in clips], sampling_rate=16000, return_tensors="pt").input_features.double()
    o64, o32 = wo.logmel(clips, n_mels, n_audio_ctx), wo.logmel(clips, n_mels, n_audio_ctx, torch.float32)
    gap = float((o32.double() - o64).abs().max())
    err = float((ref - o64).abs().max())
    print(f"logmel n_mels={n_mels} ctx={n_audio_ctx}: oracle fp32-vs-fp64 gap {gap:.3e}, oracle-vs-upstream {err:.3e}")
    assert ref.shape == o64.shape
    assert err <= 10 * gap
    assert torch.all(o64[-1] == -1.5)                      # silence: log10(1e-10) = -10 everywhere -> (-10 + 4) / 4


def test_logmel_fp32_gap():
    """the bar of the GPU log-mel test: the oracle's own fp32-vs-fp64 gap on its inputs (1.1e-4 at 3000 frames, 1.1e-5 at 200:
    the largest differences sit in the sine clips), times 10"""
    for n_mels, ctx in ((80, 1500), (128, 1500), (80, 100)):
        clips = clips_for_logmel(ctx)
        gap = float((wo.logmel(clips, n_mels, ctx, torch.float32).double() - wo.logmel(clips, n_mels, ctx)).abs().max())
        print(f"n_mels={n_mels} ctx={ctx}: gap {gap:.3e}")
        assert abs(gap - wo.LOGMEL_GAP[ctx]) <= 0.2 * wo.LOGMEL_GAP[ctx]        # the constant the GPU test's bar is built from


@pytest.mark.parametrize("cfg", [CFG_S, CFG_T])
def test_encoder_and_logits_match_upstream(cfg):
    pytest.importorskip("transformers")
    cfg = whisper_config(cfg)
    sd = recipe_whisper_state_dict(1, cfg)
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(2, cfg["n_mels"], 2 * cfg["n_audio_ctx"], generator=g)
    ids = torch.randint(0, 50257, (2, 64), generator=g)
    with torch.no_grad():
        m64, m32 = hf_model(cfg, sd, torch.float64), hf_model(cfg, sd, torch.float32)
        e64 = m64.model.encoder(feats.double()).last_hidden_state
        e32 = m32.model.encoder(feats).last_hidden_state
        l64 = m64(input_features=feats.double(), decoder_input_ids=ids).logits
        l32 = m32(input_features=feats, decoder_input_ids=ids).logits
        sd64 = wo.cast(sd)
        oe = wo.encoder(sd64, cfg, feats.double())
        ol = wo.decoder_logits(sd64, cfg, oe, ids)
    gap_e, gap_l = float((e32.double() - e64).abs().max()), float((l32.double() - l64).abs().max())
    print(f"upstream fp32-vs-fp64: encoder {gap_e:.3e}, logits {gap_l:.3e}; oracle-vs-upstream: {float((oe - e64).abs().max()):.3e}, {float((ol - l64).abs().max()):.3e}")
    assert float((oe - e64).abs().max()) <= 10 * gap_e
    assert float((ol - l64).abs().max()) <= 10 * gap_l
    # the recipe gives a decoder worth testing: distinct arg-max ids and clear margins
    top2 = l64.topk(2, dim=-1)
    assert float(((top2.values[..., 0] - top2.values[..., 1]) < 1e-3).double().mean()) <= 0.01      # the GPU test's margin rule and cap
    assert len(set(top2.indices[..., 0].flatten().tolist())) >= 16


@pytest.mark.parametrize("prompt_len", [0, 5, 300])
def test_greedy_with_decode_prefix_is_generate(small, prompt_len):
    pytest.importorskip("transformers")
    cfg, sd = small
    g = torch.Generator().manual_seed(7 + prompt_len)
    feats = torch.randn(2, cfg["n_mels"], 2 * cfg["n_audio_ctx"], generator=g)
    gen = W.default_generation_config(cfg["vocab"])
    m = hf_model(cfg, sd, torch.float64)
    for k, v in gen.items():
        setattr(m.generation_config, k, v)
    m.generation_config.pad_token_id = gen["eos_token_id"]
    prompt = None
    if prompt_len:
        prompt = torch.cat([torch.tensor([gen["prev_sot_token_id"]]), torch.randint(0, 50257, (prompt_len,), generator=g)])
    with torch.no_grad():
        ref = m.generate(input_features=feats.double(), language="chinese", task="transcribe", prompt_ids=prompt, num_beams=1, do_sample=False,
                         max_new_tokens=12)
        prefix = W.decode_prefix("chinese", "transcribe", prompt, gen, cfg["n_text_ctx"])
        assert len(prefix) == (4 if not prompt_len else 5 + prompt_len)        # fed whole, beyond n_text_ctx // 2 - 1 too
        sd64 = wo.cast(sd)
        enc = wo.encoder(sd64, cfg, feats.double())
        res = wo.greedy(sd64, cfg, enc, prefix, W.new_token_limit(len(prefix), 12, gen, cfg["n_text_ctx"]), gen["suppress_tokens"],
                        gen["begin_suppress_tokens"], gen["eos_token_id"])
    for b, r in enumerate(res):
        got = ref[b].tolist()
        got = got[-12:] if len(got) > 12 else got            # (version 5 returns the new tokens only)
        n = len(r["tokens"])
        assert r["tokens"] == got[:n]
        assert all(t == gen["eos_token_id"] for t in got[n:])
        assert min(r["margins"]) > 1e-6


def test_new_token_limit():
    gen = W.default_generation_config(51865)
    assert W.new_token_limit(4, None, gen) == 444
    assert W.new_token_limit(300, None, gen) == 148
    assert W.new_token_limit(440, 32, gen) == 8
    assert W.new_token_limit(4, 24, gen) == 24
    with pytest.raises(ValueError):
        W.decode_prefix("zh", "transcribe", list(range(443)), gen)
    g3 = W.default_generation_config(51866)
    assert g3["lang_to_id"]["<|yue|>"] == 50358 and g3["task_to_id"]["transcribe"] == 50360 and g3["no_timestamps_token_id"] == 50364
    assert gen["task_to_id"]["transcribe"] == 50359 and gen["no_timestamps_token_id"] == 50363 and gen["prev_sot_token_id"] == 50361
    with pytest.raises(ValueError):
        W.default_generation_config(1000)


def test_decode_text():
    enc = {b: ch for ch, b in W._BYTE_DECODER.items()}
    assert len(enc) == 256
    pieces = lambda bs: "".join(enc[b] for b in bs)
    han = "中".encode("utf-8")                                # three bytes, split over two tokens
    tl = [pieces(b"hi"), pieces(han[:2]), pieces(han[2:]), pieces(b" ok"), pieces(han[:1])]
    assert W.decode_text([0, 1, 2, 3], tl, eos=100) == "hi中 ok"
    assert W.decode_text([0, 100, 1, 150, 2, 101, 3], tl, eos=100) == "hi中 ok"          # special ids interleaved
    assert W.decode_text([0, 4], tl, eos=100) == "hi�"                              # an invalid tail
    assert W.decode_text([3, 7, 100], None, eos=100) == "<3><7>"
    tw = pytest.importorskip("transformers.models.gpt2.tokenization_gpt2")
    if hasattr(tw, "bytes_to_unicode"):
        assert {v: k for k, v in tw.bytes_to_unicode().items()} == W._BYTE_DECODER


# ---- the loader and the C-ABI without a device
@pytest.fixture(scope="module")
def lib():
    from targetdiarization_amd.build import build_lib
    build_lib()
    return _lib.lib()


TINY = dict(d_model=64, enc_heads=1, enc_layers=1, dec_layers=1, n_mels=80, vocab=300, n_audio_ctx=4, n_text_ctx=8)


def _create(lib, cfg, sd, **over):
    c = whisper_config(cfg)
    f = dict(n_mels=c["n_mels"], n_audio_ctx=c["n_audio_ctx"], d_model=c["d_model"], enc_heads=c["enc_heads"], enc_layers=c["enc_layers"],
             enc_ffn=c["enc_ffn"], n_text_ctx=c["n_text_ctx"], dec_heads=c["dec_heads"], dec_layers=c["dec_layers"], dec_ffn=c["dec_ffn"],
             vocab=c["vocab"], gelu=1)
    f.update(over)
    cc = _lib.WhisperConfig(**f)
    blob = pack_blob(sd)
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    h = C.c_void_p()
    rc = lib.tdx_whisper_create(C.byref(cc), buf, len(blob), 0, C.byref(h))
    msg = lib.tdx_last_error().decode() if rc else ""
    if rc == 0:
        lib.tdx_whisper_destroy(h)
    return rc, msg


@pytest.mark.parametrize("over,text", [
    (dict(enc_heads=2), "d_model / heads"), (dict(dec_heads=2), "d_model / heads"), (dict(gelu=0), "activation_function"),
    (dict(n_mels=64), "n_mels"), (dict(n_audio_ctx=0), "n_audio_ctx"), (dict(n_text_ctx=0), "n_text_ctx"), (dict(vocab=1), "vocab"),
    (dict(dec_layers=0), "dec_layers"), (dict(enc_ffn=100), "enc_ffn")])
def test_create_reports_every_contract_violation(lib, over, text):
    rc, msg = _create(lib, TINY, recipe_whisper_state_dict(1, TINY), **over)
    assert rc == 1 and text in msg, (rc, msg)


def test_loader_is_strict_both_ways(lib):
    sd = dict(recipe_whisper_state_dict(1, TINY))
    del sd["proj_out.weight"]
    miss = {k: v for k, v in sd.items() if k != "model.decoder.layers.0.encoder_attn.k_proj.weight"}
    rc, msg = _create(lib, TINY, miss)
    assert rc == 2 and "model.decoder.layers.0.encoder_attn.k_proj.weight" in msg
    extra = dict(sd)
    extra["model.encoder.layers.0.self_attn.k_proj.bias"] = torch.zeros(64)
    rc, msg = _create(lib, TINY, extra)
    assert rc == 2 and "unexpected tensor: model.encoder.layers.0.self_attn.k_proj.bias" in msg
    tr = dict(sd)
    tr["model.encoder.layers.0.fc1.weight"] = sd["model.encoder.layers.0.fc1.weight"].T.contiguous()
    rc, msg = _create(lib, TINY, tr)
    assert rc == 2 and "shape: model.encoder.layers.0.fc1.weight" in msg
    rc, msg = _create(lib, TINY, sd, vocab=301)
    assert rc == 2 and "model.decoder.embed_tokens.weight" in msg


def test_proj_out_absent_tied_or_different(lib):
    sd = dict(recipe_whisper_state_dict(1, TINY))
    diff = dict(sd)
    diff["proj_out.weight"] = sd["proj_out.weight"] + 1.0
    rc, msg = _create(lib, TINY, diff)
    assert rc == 2 and "proj_out.weight differs" in msg
    # absent or tied: the blob is accepted — without a device the call then stops at the upload (TDX_E_HIP), with one it succeeds
    tied = dict(sd)
    tied["proj_out.weight"] = sd["proj_out.weight"].clone()
    absent = {k: v for k, v in sd.items() if k != "proj_out.weight"}
    for case in (tied, absent):
        rc, msg = _create(lib, TINY, case)
        assert rc in (0, 3), (rc, msg)


def test_argument_validation_without_gpu(lib):
    assert lib.tdx_whisper_destroy(None) == 0
    assert lib.tdx_whisper_workspace_bytes(None, 1) == 0
    assert lib.tdx_whisper_flops(None, 1, 1) == 0.0
    assert lib.tdx_whisper_create(None, None, 0, 0, None) == 1
    assert lib.tdx_whisper_logmel(None, None, None, 1, 16000, None, None, 0, None) == 1
    assert lib.tdx_whisper_encode(None, None, 1, None, None, None, 0, None) == 1
    assert lib.tdx_whisper_decode(None, None, 1, None, 0, None, 0, None, 0, 0, 0, None, None, None, None, 0, None) == 1
    assert b"tdx_whisper_decode" in lib.tdx_last_error()


# ---- the wide, padded and long configurations of tests/test_gpu_whisper_widths.py: what that module asserts about the oracle alone
@pytest.mark.parametrize("name,nb", wc.TEACHER)
def test_width_oracle_stays_within_the_margin_cap(name, nb):
    _, ids, _, mg = wc.teacher_case(name, nb)
    share, distinct = float((mg <= wc.MARGIN).double().mean()), wc.distinct_clear_ids(ids, mg)
    print(f"{name} B={nb}: {100 * share:.2f} % of the positions under the margin, {distinct} distinct ids at the clear ones")
    assert ids.shape == (nb, 64) and int(ids.max()) < wc.VOCAB and max(wc.teacher_prefix()) < wc.VOCAB
    assert share <= 0.01
    assert distinct >= wc.MIN_DISTINCT


@pytest.mark.parametrize("name", sorted(wc.GREEDY))
def test_width_greedy_oracle_is_clear(name):
    prefix, res = wc.greedy_case(name)
    low = min(min(r["margins"]) for r in res)
    print(f"{name}: prefix {prefix} (seed {wc.GREEDY[name][1]}), smallest margin {low:.2e}, {len({t for r in res for t in r['tokens']})} distinct ids")
    assert len(prefix) == 4 and len(res) == wc.GREEDY[name][0]
    assert low > wc.MARGIN
    assert all(len(r["tokens"]) == wc.GREEDY_NEW and wc.GREEDY_EOS not in r["tokens"] for r in res)        # end-of-text is never emitted
    assert len({t for r in res for t in r["tokens"]}) >= wc.MIN_DISTINCT


@pytest.mark.parametrize("name", sorted(wc.CFGS))
def test_width_configs_are_accepted(lib, name):
    cfg, sd, _ = wc.weights(name)
    assert cfg["d_model"] == 64 * cfg["enc_heads"] == 64 * cfg["dec_heads"]     # tdx_whisper_create's rule, from whisper_config's defaults
    assert cfg["enc_ffn"] == cfg["dec_ffn"] == 4 * cfg["d_model"] and cfg["n_text_ctx"] == 448
    shapes = dict(whisper_param_shapes(cfg))
    assert {k: tuple(v.shape) for k, v in sd.items()} == shapes
    assert shapes["model.decoder.embed_tokens.weight"] == (wc.VOCAB, cfg["d_model"])
    assert shapes["model.encoder.embed_positions.weight"] == (cfg["n_audio_ctx"], cfg["d_model"])
    rc, msg = _create(lib, cfg, sd)                      # every contract check and the strict loader pass: without a device the call
    assert rc in (0, 3), (rc, msg)                       # then stops at the upload (TDX_E_HIP), with one it succeeds
    rc, msg = _create(lib, cfg, sd, enc_heads=cfg["enc_heads"] + 1)
    assert rc == 1 and "d_model / heads" in msg


def test_no_cpu_path(small):
    cfg, sd = small
    with pytest.raises(_lib.TdxError):
        W.WhisperASR(sd, cfg, device="cpu")
    assert W.build_whisper(None, None, model_dir="/nonexistent") is None
