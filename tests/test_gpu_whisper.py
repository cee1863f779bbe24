"""Whisper on the device (csrc/whisper.hip, targetdiarization_amd/whisper.py) against tests/whisper_oracle.py in fp64.

Three configurations with the recipe weights of seed 1: A = (d 128, 2 heads, 2 + 2 layers, 80 mels, vocabulary 51865, 1500 audio
positions), B = (d 192, 3 heads, 1 + 1 layers, 128 mels, vocabulary 51866, 1500), C = A with 100 audio positions.  The oracle's
results are computed once per module (`ref`) and never changed; every assertion about the oracle alone (margins, caps) is made
before the device's output is looked at."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import whisper_oracle as wo
from targetdiarization_amd import _lib
from targetdiarization_amd import whisper as W
from targetdiarization_amd.weights import recipe_whisper_state_dict, whisper_config

pytestmark = pytest.mark.gpu

CFGS = {"A": dict(d_model=128, enc_heads=2, enc_layers=2, dec_layers=2, n_mels=80, vocab=51865, n_audio_ctx=1500),
        "B": dict(d_model=192, enc_heads=3, enc_layers=1, dec_layers=1, n_mels=128, vocab=51866, n_audio_ctx=1500),
        "C": dict(d_model=128, enc_heads=2, enc_layers=2, dec_layers=2, n_mels=80, vocab=51865, n_audio_ctx=100)}
NCLIPS = {"A": 3, "B": 5, "C": 32}
# 10 x the oracle's own fp32-vs-fp64 gap on logmel_test_clips (tests/test_whisper_host.py::test_logmel_fp32_gap)
LOGMEL_BAR = {ctx: 10 * gap for ctx, gap in wo.LOGMEL_GAP.items()}
MARGIN, SCORE_TOL = 1e-3, 1e-3


@functools.lru_cache(maxsize=None)
def weights(name):
    cfg = whisper_config(CFGS[name])
    sd = recipe_whisper_state_dict(1, cfg)
    return cfg, sd, wo.cast(sd)


@functools.lru_cache(maxsize=None)
def ref(name):
    """the features of the configuration's clips and the oracle's encoder output"""
    cfg, _, sd64 = weights(name)
    g = torch.Generator().manual_seed(11)
    feats = 0.5 * torch.randn(NCLIPS[name], cfg["n_mels"], 2 * cfg["n_audio_ctx"], generator=g)
    with torch.no_grad():
        enc = wo.encoder(sd64, cfg, feats.double())
    return feats, enc


def teacher_case(name, nb):
    cfg, _, sd64 = weights(name)
    g = torch.Generator().manual_seed(21)
    prefix = torch.randint(0, 50257, (64,), generator=g).tolist()
    with torch.no_grad():
        ids, sc, mg = wo.step_outputs(sd64, cfg, ref(name)[1][:nb], torch.tensor([prefix] * nb), 64)
    return prefix, ids, sc, mg


@functools.lru_cache(maxsize=None)
def greedy_case(name):
    """a real prefix (A: with a 5-id prompt, B: without); the default suppress list plus the id the oracle would emit first; the
    default begin list plus X, the id clip 0 would then emit first, and Y, an id clip 0 then emits at its second step: a head that
    ignored the begin list would emit X, one that applied it at every step could not emit Y"""
    cfg, _, sd64 = weights(name)
    gen = W.default_generation_config(cfg["vocab"])
    prompt = [gen["prev_sot_token_id"], 1212, 318, 257, 1332, 13] if name == "A" else None
    prefix = W.decode_prefix("chinese", "transcribe", prompt, gen, cfg["n_text_ctx"])
    enc = ref(name)[1][:3]
    sup, beg = list(gen["suppress_tokens"]), list(gen["begin_suppress_tokens"])
    with torch.no_grad():
        first = wo.greedy(sd64, cfg, enc, prefix, 1, sup, beg, gen["eos_token_id"])[0]["tokens"][0]
        sup.append(first)
        x = wo.greedy(sd64, cfg, enc, prefix, 1, sup, beg, gen["eos_token_id"])[0]["tokens"][0]
        beg.append(x)
        y = wo.greedy(sd64, cfg, enc[:1], prefix, 2, sup, beg, gen["eos_token_id"])[0]["tokens"][1]
        beg.append(y)
        res = wo.greedy(sd64, cfg, enc, prefix, 24, sup, beg, gen["eos_token_id"])
    return prefix, sup, beg, gen["eos_token_id"], first, res


@functools.lru_cache(maxsize=None)
def model(name):
    cfg, sd, _ = weights(name)
    return W.WhisperASR(sd, cfg, device="cuda:0")


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


# ---- 1. log-mel
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_logmel(name):
    cfg, _, _ = weights(name)
    m = model(name)
    clips = wo.logmel_test_clips(cfg["n_audio_ctx"])
    want = wo.logmel(clips, cfg["n_mels"], cfg["n_audio_ctx"])
    got = torch.cat([m.features(clips[i:i + 3]) for i in range(0, 9, 3)]).cpu().double()
    err = (got - want).abs().amax(dim=(1, 2))
    print(f"logmel {name}: max error per clip {[f'{e:.2e}' for e in err.tolist()]} (bar {LOGMEL_BAR[cfg['n_audio_ctx']]:.1e})")
    assert torch.isfinite(got).all()
    assert float(err.max()) <= LOGMEL_BAR[cfg["n_audio_ctx"]]
    assert torch.all(got[8] == want[8]) and torch.all(got[8] == -1.5)          # silence: exact
    for i in (0, 5, 8):                             # B = 1 against the batch of three: a row's place in the shared GEMM's tiles moves
        alone = m.features([clips[i]]).cpu().double()[0]                        # the last bit of a few values (2.4e-7 measured), no more
        assert float((alone - got[i]).abs().max()) <= 1e-6 and float((alone - want[i]).abs().max()) <= LOGMEL_BAR[cfg["n_audio_ctx"]]


# ---- 2. encoder
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_encoder(name):
    feats, want = ref(name)
    m = model(name)
    got3 = m.encode(feats[:3]).cpu().double()
    got1 = m.encode(feats[:1]).cpu().double()
    e3, e1 = rel_l2(got3, want[:3]), rel_l2(got1, want[:1])
    first, last = rel_l2(got3[:, 0], want[:3, 0]), rel_l2(got3[:, -1], want[:3, -1])
    print(f"encoder {name}: rel-L2 B=3 {e3:.2e}, B=1 {e1:.2e}, first row {first:.2e}, last row {last:.2e}")
    assert max(e3, e1, first, last) < 1e-4


def check_steps(got_ids, got_sc, ids, sc, mg, cols):
    """ids equal wherever the oracle's top-2 margin exceeds MARGIN, scores within SCORE_TOL where the ids agree"""
    clear = mg[:, cols] > MARGIN
    same = got_ids[:, cols] == ids[:, cols]
    assert bool((same | ~clear).all()), f"{int((~same & clear).sum())} clear positions differ"
    d = (got_sc[:, cols] - sc[:, cols]).abs()[same]
    print(f"  {int(same.sum())} positions agree, {int((~clear).sum())} under the margin, max score error {float(d.max()):.2e}, "
          f"{len(set(ids[:, cols].flatten().tolist()))} distinct ids")
    assert float(d.max()) <= SCORE_TOL


# ---- 3. teacher-forced decode
@pytest.mark.parametrize("name,nb", [("A", 2), ("B", 5), ("C", 2), ("C", 12), ("C", 32)])        # 12, 32: the MFMA Linear of 9..32 rows
def test_teacher_forced(name, nb):
    prefix, ids, sc, mg = teacher_case(name, nb)
    assert float((mg <= MARGIN).double().mean()) <= 0.01                       # the oracle alone stays within the cap
    m = model(name)
    _, state = m.encode(ref(name)[0][:nb], with_state=True)
    gi, gs, cnt = m.decode(state, prefix, 0)
    gi, gs = gi.cpu().long(), gs.cpu().double()
    assert cnt.cpu().tolist() == [0] * nb
    assert bool((gi[:, 64:] == -1).all())                                       # nothing past the prefix
    check_steps(gi, gs, ids, sc, mg, slice(0, 64))


def run_greedy(m, state, prefix, sup, beg, eos, max_new=24):
    gi, gs, cnt = m.decode(state, prefix, max_new, sup, beg, eos)
    gi, gs, cnt = gi.cpu().long(), gs.cpu().double(), cnt.cpu().tolist()
    p0 = len(prefix) - 1
    return [gi[b, p0:p0 + n].tolist() for b, n in enumerate(cnt)], [gs[b, p0:p0 + n] for b, n in enumerate(cnt)], cnt


# ---- 4. free greedy
@pytest.mark.parametrize("name", ["A", "B"])
def test_greedy(name):
    prefix, sup, beg, eos, first, res = greedy_case(name)
    assert min(min(r["margins"]) for r in res) > MARGIN                        # the oracle has no step under the margin
    assert all(first not in r["tokens"] for r in res) and len({t for r in res for t in r["tokens"]}) >= 8
    x, y = beg[-2], beg[-1]
    assert all(r["tokens"][0] not in (x, y) for r in res) and res[0]["tokens"][1] == y      # begin list: the first position only
    m = model(name)
    _, state = m.encode(ref(name)[0][:3], with_state=True)
    toks, scs, cnt = run_greedy(m, state, prefix, sup, beg, eos)
    assert cnt == [len(r["tokens"]) for r in res]
    for b, r in enumerate(res):
        assert toks[b] == r["tokens"]
        assert float((scs[b] - torch.tensor(r["scores"], dtype=torch.float64)).abs().max()) <= SCORE_TOL


# ---- 5. EOS and independence
def test_eos_and_independence():
    cfg, _, sd64 = weights("A")
    prefix, sup, beg, _, _, res = greedy_case("A")
    t0 = res[0]["tokens"]
    k = next(i for i in range(2, len(t0)) if t0[i] not in t0[:i])              # the first id at a step >= 2 that clip 0 has not emitted before
    eos, stop = t0[k], k + 1
    with torch.no_grad():
        want = wo.greedy(sd64, cfg, ref("A")[1][:3], prefix, 24, sup, beg, eos)
    assert len(want[0]["tokens"]) == stop and want[0]["tokens"] == res[0]["tokens"][:stop]
    m = model("A")
    _, state = m.encode(ref("A")[0][:3], with_state=True)
    toks, scs, cnt = run_greedy(m, state, prefix, sup, beg, eos)
    assert cnt[0] == stop and toks[0] == want[0]["tokens"]
    for b in (1, 2):
        assert toks[b] == want[b]["tokens"]
        if eos not in res[b]["tokens"]:
            assert toks[b] == res[b]["tokens"]                                  # unchanged by clip 0 stopping
    for b in range(3):                                                           # every clip alone
        t1, s1, c1 = run_greedy(m, state[:, :, b:b + 1].contiguous(), prefix, sup, beg, eos)
        assert c1 == [cnt[b]] and t1[0] == toks[b]
        assert float((s1[0] - scs[b]).abs().max()) <= 1e-5


# ---- 6. the end of the cache
def test_cache_end():
    cfg, _, sd64 = weights("C")
    T, d = cfg["n_text_ctx"], cfg["d_model"]
    g = torch.Generator().manual_seed(31)
    prefix = torch.randint(0, 50257, (440,), generator=g).tolist()
    enc = ref("C")[1][:2]
    with torch.no_grad():
        want = wo.greedy(sd64, cfg, enc, prefix, 32, (), (), 50257)
        full = torch.tensor([prefix + w["tokens"] for w in want])
        ids, sc, mg = wo.step_outputs(sd64, cfg, enc, full, 440)
    assert [len(w["tokens"]) for w in want] == [8, 8] and full.shape[1] == T
    assert min(min(w["margins"]) for w in want) > MARGIN
    assert float((mg <= MARGIN).double().mean()) <= 0.01
    m = model("C")
    _, state = m.encode(ref("C")[0][:2], with_state=True)
    # the C-ABI directly, with a guard band behind the workspace (the cache is its last part) and behind the id and score buffers
    nb, guard = m.workspace_bytes(2), 4096
    ws = torch.full((nb + guard,), 0x5A, dtype=torch.uint8, device="cuda:0")
    gi = torch.full((2 * T + 1024,), -7, dtype=torch.int32, device="cuda:0")
    gs = torch.full((2 * T + 1024,), -7.0, device="cuda:0")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    pre = (C.c_int * 440)(*prefix)
    none = (C.c_int * 1)(0)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(m._l.tdx_whisper_decode(m._h, state.data_ptr(), 2, pre, 440, none, 0, none, 0, 50257, 32, gi.data_ptr(), gs.data_ptr(), cnt.data_ptr(),
                                       ws.data_ptr(), nb, st))
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [8, 8]
    assert bool((ws[nb:] == 0x5A).all()) and bool((gi[2 * T:] == -7).all()) and bool((gs[2 * T:] == -7.0).all())
    gi2, gs2 = gi[:2 * T].view(2, T).cpu().long(), gs[:2 * T].view(2, T).cpu().double()
    assert bool((gi2[:, 447] == -7).all())                                      # the last step run is 446: it wrote the token of position 447
    for b in range(2):
        assert gi2[b, 439:447].tolist() == want[b]["tokens"]                    # positions 440 .. 447
    check_steps(gi2, gs2, ids, sc, mg, slice(0, 447))


# ---- 7. the public surface
def test_public_surface(capsys):
    from targetdiarization_amd.asr_processor import ASRProcessor
    cfg, sd, _ = weights("C")
    enc = {b: ch for ch, b in W._BYTE_DECODER.items()}
    token_list = ["".join(enc[b] for b in (" t%d" % i).encode()) for i in range(50257)]
    g = torch.Generator().manual_seed(41)
    wavs = [0.1 * torch.randn(n, generator=g).numpy() for n in (16000, 40000)]
    p = ASRProcessor(is_asr=True, whisper_state_dict=sd, whisper_config=cfg, whisper_token_list=token_list, verbose_log=False)
    assert list(p.asr) == ["whisper_finetune"]
    m = p.asr["whisper_finetune"]
    raw = p.asr_detection(wavs, asr_engine="whisper_finetune", output_raw_result=True)
    assert [set(r) for r in raw] == [{"key", "text", "token_ids", "scores"}] * 2 and all(r["token_ids"] for r in raw)
    res = p.asr_detection(wavs, asr_engine="whisper_finetune")
    assert [set(r) for r in res] == [{"key", "language", "text"}] * 2
    for r, w in zip(res, raw):
        assert r["text"] == w["text"].strip() and w["text"].startswith(" t") and r["language"] == ASRProcessor.detect_language(w["text"])
        assert r["text"] == W.decode_text(w["token_ids"], token_list).strip()
    assert p.asr_detection(wavs, asr_engine="whisper_finetune", output_text_only=True) == "".join(r["text"] for r in res)
    capsys.readouterr()
    again = p.asr_detection(wavs, asr_engine="whisper_finetune", prompt="hello")
    assert "prompt is ignored" in capsys.readouterr().out and again == res
    assert p.asr_detection(wavs, asr_engine="sensevoice") == res                # an engine that is not loaded falls back
    # HotPath.recognise_whisper on two speakers' streams: one item each (the <= 30 s bucket of a stream)
    from targetdiarization_amd.pipeline import HotPath
    hp = HotPath.__new__(HotPath)
    hp.whisper, hp.asr_segment, hp.device = m, 480000, m.device
    out = hp.recognise_whisper([torch.from_numpy(w) for w in wavs])
    assert [len(o) for o in out] == [1, 1] and [o[0]["token_ids"] for o in out] == [w["token_ids"] for w in raw]
    m.close()
    m.close()
    with pytest.raises(_lib.TdxError):
        m.generate(wavs)


def test_target_diarization_whisper_engine(gold, sd2):
    import os
    import wave as wavmod
    from targetdiarization_amd.target_diarization import TargetDiarization
    from targetdiarization_amd.weights import recipe_eres2netv2_state_dict, recipe_paraformer_state_dict

    def wave(fn):
        with wavmod.open(os.path.join(gold, fn), "rb") as w:
            return np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16).astype(np.float32) / 32768.0
    mix, tgt = wave("chat_mix.wav"), wave("female_a.wav")
    sd_rows = {"text": [[0.0, 3.0, 0], [2.4, 5.5, 1], [5.5, 8.6, 0]]}
    od = [(0.0, 3.0, "SPEAKER_00"), (2.4, 5.5, "SPEAKER_01"), (5.5, 8.6, "SPEAKER_00")]
    cfg, sd, _ = weights("C")
    enc = {b: ch for ch, b in W._BYTE_DECODER.items()}
    token_list = ["".join(enc[b] for b in b" ab")] * 50257            # every piece is Latin text: detect_language gives "en"
    td = TargetDiarization(cuda_device=0, sep_state_dict=sd2, spk_state_dict=recipe_eres2netv2_state_dict(0),
                           asr_state_dict=recipe_paraformer_state_dict(0, 2), sd_pipeline=lambda a: sd_rows, od_pipeline=lambda a: od,
                           asr_engine="whisper_finetune", whisper_state_dict=sd, whisper_config=cfg, whisper_token_list=token_list)
    assert td.hp.whisper is not None
    spk, res, aud = td.infer(mix, tgt)
    singles = [r for r in res if r["type"] == "single"]
    assert singles and len(singles) == len(res) == len({r["speaker"] for r in res})     # no timestamps: one item per speaker
    assert all(set(r) >= {"speaker", "timerange", "text", "type", "language"} for r in singles)
    assert all(r["language"] == "en" and r["text"].startswith("ab") and r["text"] == r["text"].strip() for r in singles)
    td.asr_engine = "paraformer"                                          # the default engine is untouched by the Whisper weights
    _, res_pf, _ = td.infer(mix, tgt)
    assert all("language" not in r for r in res_pf)
