"""CPU tests of Whisper's long-form transcription: tests/whisper_longform_oracle.py and the host side of
WhisperASR.transcribe pinned to the installed transformers on the tiny models of whisper_longform_cases.py, the switches over stub
models, and the argument checks of the new C-ABI entry points."""
import numpy as np
import pytest
import torch

import whisper_longform_cases as lc
import whisper_longform_oracle as lo
import whisper_oracle as wo
import whisper_ts_oracle as ts
from targetdiarization_amd import _lib
from targetdiarization_amd import whisper as W


# ---- 1. the rule function is WhisperTimeStampLogitsProcessor
def hf_rules(name, max_initial):
    from transformers import GenerationConfig
    from transformers.generation.logits_process import WhisperTimeStampLogitsProcessor
    g = lc.gen_config(name)
    gc = GenerationConfig(eos_token_id=g["eos_token_id"], no_timestamps_token_id=g["no_timestamps_token_id"])
    if max_initial is not None:
        gc.max_initial_timestamp_index = max_initial
    return WhisperTimeStampLogitsProcessor(gc, begin_index=3)


@pytest.mark.parametrize("name", ["S", "M"])
@pytest.mark.parametrize("max_initial", [None, 0, 5])
def test_rules_are_upstreams(name, max_initial):
    pytest.importorskip("transformers")
    I, V = lc.ids_of(name), lc.CFGS[name]["vocab"]
    proc = hf_rules(name, max_initial)
    g = torch.Generator().manual_seed(3)
    n = 0
    for seq in lc.histories(name):
        for trial in range(6):
            lg = 2.0 * torch.randn(V, generator=g)
            if trial >= 4:                          # the timestamp mass just above / just below the best text logit
                ok = lo.history_rules(V, seq, len(seq) == 0, I["tb"], I["eos"], max_initial)
                if ok[:I["tb"]].any() and ok[I["tb"]:].any():
                    m = lg.double().masked_fill(~ok, float("-inf"))
                    gap = float(torch.logsumexp(m[I["tb"]:], 0) - m[:I["tb"]].max())
                    lg[I["tb"]:] += -gap + (1e-3 if trial == 4 else -1e-3)
            ids = torch.tensor([[I["sot"], I["en"], I["transcribe"]] + seq])
            want = ~torch.isinf(proc(ids, lg[None].clone())[0])
            got = lo.ts_rules(lg, seq, len(seq) == 0, I["tb"], I["eos"], max_initial)
            assert torch.equal(got, want), (seq, trial)
            n += int((got != lo.history_rules(V, seq, len(seq) == 0, I["tb"], I["eos"], max_initial)).any())
    assert n >= 4                                   # the mass rule changed the set in several of the trials


# ---- 2. the long feature extractor is WhisperFeatureExtractor(truncation=False)
@pytest.mark.parametrize("n", [160 * 128 + 37, 160 * 40 + 159, 160 * 300 + 1, 417, 201])      # (upstream raises at N <= 200: its reflect pad)
def test_logmel_long_is_feature_extractor(n):
    tr = pytest.importorskip("transformers")
    fe = tr.WhisperFeatureExtractor(feature_size=80, chunk_length=1)
    x = lc.noise(n, 5, 0.2) + 0.3 * torch.sin(2 * np.pi * 300.0 * torch.arange(n) / 16000.0)
    want = fe(x.numpy(), sampling_rate=16000, truncation=False, padding="longest", return_tensors="pt")["input_features"][0].double()
    got = lo.logmel_long(x, 80)
    assert got.shape == want.shape == (80, n // 160)
    assert float((got - want).abs().max()) < 2e-4   # upstream computes in fp32 / numpy fp64 mixed: its own rounding
    assert lo.logmel_long(x[:159], 80).shape == (80, 0) and lo.logmel_long(x[:1], 80).shape == (80, 0)


def test_logmel_long_clamp_is_clip_wide():
    x = torch.cat([1e-4 * lc.noise(160 * 200, 1), lc.noise(160 * 60, 2, 0.5)])
    whole = lo.logmel_long(x, 80)
    assert float(whole[:, :150].min()) == float(whole.min()) and float(whole.min()) == pytest.approx(float(whole.max()) - 2.0, abs=1e-9)
    quiet_alone = lo.logmel_long(x[:160 * 200], 80)
    assert float((quiet_alone[:, :150] - whole[:, :150]).abs().max()) > 0.1      # a per-window clamp would give other values


# ---- 3. the segment cutting is _retrieve_segment
def hf_cut(tokens, tb, seek, nfr):
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin
    seq = torch.tensor(tokens)
    segs, step = WhisperGenerationMixin._retrieve_segment(
        seek_sequence=seq, seek_outputs=[{}], time_offset=torch.tensor([seek * 0.02 / 2], dtype=torch.float64), timestamp_begin=tb,
        seek_num_frames=torch.tensor([nfr]), time_precision=0.02, time_precision_features=0.01, input_stride=2, prev_idx=0, idx=0,
        return_token_timestamps=False, decoder_input_ids=torch.zeros(1, 3, dtype=torch.long))
    return [(s["tokens"].tolist(), float(s["start"]), float(s["end"])) for s in segs], int(step)


def test_segments_are_upstreams():
    pytest.importorskip("transformers")
    tb = lc.ids_of("S")["tb"]
    cases = [[tb, 3, 4, tb + 10, tb + 10, 5, tb + 30, tb + 30, 6, 7],             # pairs, no closing timestamp: seek to the last pair
             [tb, 3, 4, tb + 10, tb + 10, 5, tb + 30],                             # pairs and a single closing timestamp: the whole window
             [tb + 2, 3, 4, tb + 10, tb + 10],                                     # the ids end in a pair
             [tb + 2, 3, 4, 5],                                                    # no pair, one timestamp
             [tb, 3, 4, 5],                                                        # no pair, only <|0.00|>: the window's end
             [tb + 2, 3, 4, tb + 40],                                              # no pair, a closing timestamp
             [tb + 5]]                                                             # a lone timestamp
    for toks in cases:
        for seek, nfr in ((0, 128), (256, 90)):
            want = hf_cut(toks, tb, seek, nfr)
            for cut in (lo.cut_segments, W.cut_segments):
                segs, step = cut(toks, tb, seek, nfr)
                assert step == want[1], (toks, cut)
                assert [s["tokens"] for s in segs] == [w[0] for w in want[0]]
                assert [(s["start"], s["end"]) for s in segs] == [pytest.approx((w[1], w[2]), abs=1e-12) for w in want[0]]


# ---- 4. the whole loop is generate(return_timestamps=True, return_segments=True)
class OracleASR(W.WhisperASR):
    """WhisperASR.transcribe with the device calls answered by the fp64 oracle model: what is tested is the host loop"""

    def __init__(self, name, sd, alignment=False):
        from targetdiarization_amd.weights import whisper_config
        self.cfg = whisper_config(lc.CFGS[name])
        self.gen_cfg = lc.gen_config(name)
        self.sd64 = wo.cast(sd)
        self.token_list, self.tokenizer, self.alignment_heads = None, None, [[1, 0]]
        self.device, self._h = "cpu", 1
        self.log = []

    def features_long(self, wav):
        return lo.logmel_long(torch.as_tensor(wav), self.cfg["n_mels"]).float()

    def encode(self, feats, with_state=False):
        with torch.no_grad():
            enc = wo.encoder(self.sd64, self.cfg, feats.double())
        return enc, enc[None, None].expand(self.cfg["dec_layers"], 2, *enc.shape).contiguous()

    def detect_language(self, state):
        return (["en", "zh"] * state.shape[2])[:state.shape[2]]

    def decode_ts(self, state, prefixes, max_new, suppress=(), begin_suppress=(), eos=None, no_timestamps_id=None, max_initial_timestamp_index=None,
                  begin=None, sot_pos=None, no_speech_id=None, heads=None, first_row=None, max_rows=None):
        B, T = state.shape[2], self.cfg["n_text_ctx"]
        ids, sc = torch.full((B, T), -1, dtype=torch.int32), torch.zeros(B, T)
        cnt, nosp = torch.zeros(B, dtype=torch.int32), torch.zeros(B)
        self.log.append({"prefixes": [list(p) for p in prefixes], "max_new": list(max_new), "sot_pos": list(sot_pos)})
        for b in range(B):
            with torch.no_grad():
                r = lo.greedy_ts(self.sd64, self.cfg, state[0, 0, b:b + 1], prefixes[b], max_new[b], no_timestamps_id + 1, eos, suppress, begin_suppress,
                                 None, None, no_timestamps_id - 1, sot_pos[b])
            n, p0 = len(r["tokens"]), len(prefixes[b]) - 1
            ids[b, p0:p0 + n] = torch.tensor(r["tokens"], dtype=torch.int32)
            sc[b, p0:p0 + n] = torch.tensor(r["scores"])
            cnt[b], nosp[b] = n, r["no_speech_prob"]
        xattn = None
        if heads is not None:                       # the capture: row p - prefix_len of the step that fed position p, all generated ids but the last
            xattn = torch.zeros(B, len(heads), max(1, max(max_new) - 1), self.cfg["n_audio_ctx"], dtype=torch.float64)
            for b in range(B):
                n, pl = int(cnt[b]), len(prefixes[b])
                if n > 1:
                    fed = torch.tensor([list(prefixes[b]) + ids[b, pl - 1:pl - 1 + n - 1].tolist()])
                    with torch.no_grad():
                        xattn[b, :, :n - 1] = ts.cross_attention(self.sd64, self.cfg, state[0, 0, b:b + 1], fed, heads)[0][:, pl:]
        return ids, sc, cnt, nosp, xattn


LOOP_CASES = {"plain": dict(cond=False), "conditioned": dict(cond=True), "prompt": dict(cond=True, prompt=True),
              "skip": dict(cond=False, thr={"S": (0.6, -1.3), "M": (0.6, -1.0)}, scale=2.0, boost=7.0)}      # some windows are silent to this model


@pytest.mark.parametrize("name", ["S", "M"])
@pytest.mark.parametrize("case", list(LOOP_CASES))
def test_loop_is_generate(name, case):
    pytest.importorskip("transformers")
    k = LOOP_CASES[case]
    I, g = lc.ids_of(name), lc.gen_config(name)
    cfg, sd = lc.weights(name, 1, k.get("scale", 3.0), k.get("boost", 0.0))
    nframes = 700
    wav = torch.cat([lc.noise(160 * 300, 101), torch.zeros(160 * 256), lc.noise(160 * 144 + 77, 102)])
    feats = lo.logmel_long(wav, cfg["n_mels"]).float()
    prompt = [I["prev"], 5, 6, 7] if k.get("prompt") else None
    thr = k["thr"][name] if "thr" in k else None
    kw = dict(return_timestamps=True, return_segments=True, language="en", task="transcribe", condition_on_prev_tokens=k["cond"], temperature=0.0)
    if thr:
        kw.update(no_speech_threshold=thr[0], logprob_threshold=thr[1])
    if prompt:
        kw.update(prompt_ids=torch.tensor(prompt), prompt_condition_type="first-segment")
    with torch.no_grad():
        out = lc.hf_model(name, sd).generate(feats[None], attention_mask=torch.ones(1, nframes, dtype=torch.long), **kw)
    want = [(s["tokens"].tolist(), float(s["start"]), float(s["end"])) for s in out["segments"][0]]
    # the oracle loop over the fp64 oracle model
    sd64 = wo.cast(sd)

    def dec(seek, nfr, prefix, max_new):
        with torch.no_grad():
            enc = wo.encoder(sd64, cfg, lo.window(feats.double(), seek, 128)[None])
            return lo.greedy_ts(sd64, cfg, enc, prefix, max_new, I["tb"], I["eos"], g["suppress_tokens"], g["begin_suppress_tokens"], None, None,
                                I["nospeech"], len(prefix) - 3)
    r = lo.transcribe_loop(dec, nframes, 128, [I["sot"], I["en"], I["transcribe"]], I["tb"], I["eos"], I["prev"], cfg["n_text_ctx"], g["max_length"],
                           prompt, k["cond"], thr[0] if thr else None, thr[1] if thr else None)
    assert [s["tokens"] for s in r["segments"]] == [w[0] for w in want]
    assert [(s["start"], s["end"]) for s in r["segments"]] == [pytest.approx((w[1], w[2]), abs=1e-9) for w in want]
    wins = r["windows"]
    assert len(wins) >= 5 and sum(w["step"] for w in wins) >= nframes
    if case == "skip":
        assert 0 < sum(w["skip"] for w in wins) < len(wins)
    if case == "conditioned" and name == "S":
        assert any(w["step"] < min(128, nframes - w["seek"]) for w in wins) and any(w["step"] == 128 for w in wins)     # both seek branches
    if case == "prompt":
        assert wins[0]["prefix"][:4] == prompt
    if k["cond"]:
        assert any(len(w["prefix"]) > 3 for w in wins[1:]) and all(len(w["prefix"]) <= cfg["n_text_ctx"] // 2 + 3 for w in wins)
    # WhisperASR.transcribe's host loop over the same model: the same segments, seeks, prefixes and budgets
    m = OracleASR(name, sd)
    res = m.transcribe([wav], language="en", prompt_ids=prompt, condition_on_prev_tokens=k["cond"], no_speech_threshold=thr[0] if thr else None,
                       logprob_threshold=thr[1] if thr else None, word_timestamps=False)[0]
    assert [s["tokens"] for s in res["segments"]] == [w[0] for w in want]
    assert [(s["start"], s["end"]) for s in res["segments"]] == [pytest.approx((w[1], w[2]), abs=1e-9) for w in want]
    assert [c["prefixes"][0] for c in m.log] == [w["prefix"] for w in wins] and [c["max_new"][0] for c in m.log] == [w["max_new"] for w in wins]
    kept = [w for w in wins if not w["skip"]]
    assert sorted({s["seek"] for s in res["segments"]}) == sorted({w["seek"] for w in kept if w["tokens"]})
    assert set(res) == {"key", "language", "text", "segments"} and res["language"] == "en"
    assert all(set(s) == {"id", "seek", "start", "end", "text", "tokens", "avg_logprob", "no_speech_prob", "words"} for s in res["segments"])
    assert [s["id"] for s in res["segments"]] == list(range(len(want)))
    by_seek = {w["seek"]: w for w in wins}
    for s in res["segments"]:
        assert s["avg_logprob"] == pytest.approx(by_seek[s["seek"]]["avg_logprob"], abs=1e-5)
        assert s["no_speech_prob"] == pytest.approx(by_seek[s["seek"]]["no_speech_prob"], abs=1e-6)


def oracle_token_align(xattn, nrows, nframes, median_width=7, want_matrix=False):
    """tdx_token_align answered by tests/whisper_ts_oracle.py in upstream's arithmetic"""
    out = torch.full(xattn.shape[:1] + xattn.shape[2:3], -1, dtype=torch.int32)
    for b, (n, m) in enumerate(zip(nrows, nframes)):
        if n >= 1:
            out[b, :n] = torch.as_tensor(ts.token_frames(ts.matrix(xattn[b, :, :n, :m].double(), median_width), "double"), dtype=torch.int32)
    return out


@pytest.mark.parametrize("condition", [False, True])
def test_word_times_are_generates(monkeypatch, condition):
    """which rows, how many positions, the repeat of the last time, the slicing by segment and the window's offset: transcribe's
    word times against generate(return_token_timestamps=True)'s per-segment token_timestamps.  Without a piece table every
    ordinary id is its own word, so a word's start is its token's time."""
    pytest.importorskip("transformers")
    name = "S"
    I = lc.ids_of(name)
    cfg, sd = lc.weights(name, 1, 3.0)
    nframes = 500
    wav = torch.cat([lc.noise(160 * 300, 101), 0.3 * torch.sin(2 * np.pi * 500.0 * torch.arange(160 * 200 + 9) / 16000.0)])
    feats = lo.logmel_long(wav, cfg["n_mels"]).float()
    with torch.no_grad():
        out = lc.hf_model(name, sd).generate(feats[None], attention_mask=torch.ones(1, nframes, dtype=torch.long), return_timestamps=True,
                                             return_segments=True, return_token_timestamps=True, language="en", task="transcribe",
                                             condition_on_prev_tokens=condition, temperature=0.0)
    want = out["segments"][0]
    monkeypatch.setattr(W, "token_align", oracle_token_align)
    res = OracleASR(name, sd).transcribe([wav], language="en", condition_on_prev_tokens=condition, no_speech_threshold=None, logprob_threshold=None)[0]
    assert [s["tokens"] for s in res["segments"]] == [w["tokens"].tolist() for w in want] and len(want) >= 6
    seen = set()
    for s, w in zip(res["segments"], want):
        times = w["token_timestamps"].double().tolist()
        keep = [k for k, t in enumerate(s["tokens"]) if t < I["eos"]]
        assert [x for x, _ in s["words"]] == [f"<{s['tokens'][k]}>" for k in keep]
        assert [a for _, (a, _b) in s["words"]] == [pytest.approx(times[k], abs=1e-6) for k in keep]
        ends = [times[k] for k in keep[1:]] + [times[-1]]                          # a word ends where the next begins, the last at the segment's last time
        assert [b for _, (_a, b) in s["words"]] == [pytest.approx(e, abs=1e-6) for e in ends]
        seen.update(round(a - s["seek"] / 100.0, 6) for _, (a, _b) in s["words"])
    assert len(seen) >= 4 and any(s["seek"] > 0 and s["words"] for s in res["segments"])       # several distinct times, and windows with an offset


def test_zero_seek_step_guard():
    """_retrieve_segment gives a seek step of 0 for ids whose last pair is <|0.00|><|0.00|>, and upstream's loop would then not
    end.  The rules cannot produce such ids (after <|0.00|> text, <|0.00|> is denied: checked here against upstream's processor);
    cut_segments consumes the whole window instead, which is the one place it departs from _retrieve_segment."""
    pytest.importorskip("transformers")
    tb, V = lc.ids_of("S")["tb"], lc.CFGS["S"]["vocab"]
    toks = [tb, 5, tb, tb, 6]
    want = hf_cut(toks, tb, 256, 90)
    assert want[1] == 0 and lo.cut_segments(toks, tb, 256, 90)[1] == 0
    segs, step = W.cut_segments(toks, tb, 256, 90)
    assert step == 90 and [s["tokens"] for s in segs] == [w[0] for w in want[0]]
    I = lc.ids_of("S")
    allowed = ~torch.isinf(hf_rules("S", None)(torch.tensor([[I["sot"], I["en"], I["transcribe"], tb, 5]]), torch.zeros(1, V))[0])
    assert not bool(allowed[tb]) and bool(allowed[tb + 1])
    assert not bool(lo.history_rules(V, [tb, 5], False, tb, I["eos"])[tb])


def test_transcribe_batches_clips_of_different_lengths():
    """two clips in one call: one decode_ts call per round with one row per live clip; each clip's result is what it gets alone"""
    cfg, sd = lc.weights("S", 1, 3.0)
    wavs = [lc.noise(160 * 300, 7), lc.noise(160 * 520 + 3, 8)]
    m = OracleASR("S", sd)
    both = m.transcribe(wavs, language=None, word_timestamps=False)
    assert [r["language"] for r in both] == ["en", "zh"]                                  # two languages in the same decode_ts calls
    rows = [len(c["prefixes"]) for c in m.log]
    assert rows[0] == 2 and rows[-1] == 1 and sorted(rows, reverse=True) == rows
    assert any(len(c["prefixes"]) == 2 and c["prefixes"][0] != c["prefixes"][1] for c in m.log)      # each row under its own prefix
    for i, w in enumerate(wavs):
        alone = OracleASR("S", sd).transcribe([w], language=["en", "zh"][i], word_timestamps=False)[0]
        assert [s["tokens"] for s in alone["segments"]] == [s["tokens"] for s in both[i]["segments"]]
    assert [r["key"] for r in both] == ["clip_0", "clip_1"]


# ---- 5. the switches, over stub models
class StubLong:
    """a Whisper engine that records what reaches it"""
    tokenizer = None

    def __init__(self):
        self.calls = []

    def generate(self, clips, **kw):
        self.calls.append(("generate", [int(np.asarray(c).reshape(-1).shape[0]) for c in clips], kw))
        return [{"key": kw["keys"][i] if kw.get("keys") else f"clip_{i}", "text": "short", "token_ids": [1], "scores": [0.0], "language": "en",
                 "token_times": [0.0], "words": [("short", [0.0, 0.5])]} for i in range(len(clips))]

    def transcribe(self, wavs, **kw):
        n = [int(torch.as_tensor(np.asarray(w) if not isinstance(w, torch.Tensor) else w).reshape(-1).shape[0]) for w in wavs]
        self.calls.append(("transcribe", n, kw))
        out = []
        for i, ni in enumerate(n):
            segs = [{"id": k, "seek": 3000 * k, "start": 30.0 * k, "end": min(30.0 * (k + 1), ni / 16000.0), "text": f" part{k}", "tokens": [10 + k],
                     "avg_logprob": -0.1, "no_speech_prob": 0.0, "words": [(f" part{k}", [30.0 * k + 1.0, 30.0 * k + 2.0])]}
                    for k in range(-(-ni // 480000))]
            out.append({"key": kw["keys"][i] if kw.get("keys") else f"clip_{i}", "language": "en", "text": "".join(s["text"] for s in segs), "segments": segs})
        return out


def _processor(stub, **kw):
    from targetdiarization_amd.asr_processor import ASRProcessor
    p = ASRProcessor.__new__(ASRProcessor)
    p.is_asr, p.asr, p.decoder, p.verbose_log = True, {"whisper_v3": stub, "whisper_finetune": stub}, None, False
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_asr_detection_long_form_switch():
    clip = np.zeros(70 * 16000, dtype=np.float32)
    off = StubLong()
    res = _processor(off).asr_detection([clip], asr_engine="whisper_v3", language="en")
    assert [c[0] for c in off.calls] == ["generate"] and off.calls[0][1] == [480000]          # default: today's one-window call
    assert res[0]["text"] == "short"
    on = StubLong()
    p = _processor(on, whisper_long_form=True)
    res = p.asr_detection([clip], asr_engine="whisper_v3", language="en")
    assert [c[0] for c in on.calls] == ["transcribe"] and on.calls[0][1] == [70 * 16000]     # the 70 s clip arrives whole
    assert [set(r) for r in res] == [{"key", "language", "text", "timestamp"}]
    assert res[0]["text"] == " part0 part1 part2" and res[0]["language"] == "en" and res[0]["key"] == "0"
    assert res[0]["timestamp"] == [(" part0", [1.0, 2.0]), (" part1", [31.0, 32.0]), (" part2", [61.0, 62.0])]      # the text goes on after 30 s
    raw = p.asr_detection([clip], asr_engine="whisper_v3", output_raw_result=True)
    assert set(raw[0]) == {"key", "language", "text", "segments"} and len(raw[0]["segments"]) == 3
    assert p.asr_detection([clip], asr_engine="whisper_v3", output_text_only=True) == " part0 part1 part2"
    on.calls.clear()
    p.asr_detection([clip[:16000]], asr_engine="whisper_v3")                                 # nothing over 30 s: the one-window path
    p.asr_detection([clip], asr_engine="whisper_finetune")                                   # whisper_finetune keeps its one-window path
    assert [c[0] for c in on.calls] == ["generate", "generate"] and on.calls[1][1] == [480000]


def test_asr_processor_constructor_switch_defaults_off():
    from targetdiarization_amd.asr_processor import ASRProcessor
    assert ASRProcessor(verbose_log=False).whisper_long_form is False
    assert ASRProcessor(verbose_log=False, whisper_long_form=True).whisper_long_form is True


def test_recognise_whisper_long_form_switch():
    from targetdiarization_amd.pipeline import HotPath
    hp = HotPath.__new__(HotPath)
    stub = StubLong()
    hp.whisper, hp.asr_segment, hp.device = stub, 480000, "cpu"
    streams = [torch.zeros(70 * 16000), torch.zeros(20 * 16000)]
    out = hp.recognise_whisper(streams, language="auto", timestamps=True)
    assert [c[0] for c in stub.calls] == ["generate"] and stub.calls[0][1] == [480000, 480000, 160000, 320000]     # default: cut every 30 s
    assert [len(o) for o in out] == [3, 1]
    stub.calls.clear()
    out = hp.recognise_whisper(streams, language="auto", timestamps=True, long_form=True)
    assert [c[0] for c in stub.calls] == ["transcribe"] and stub.calls[0][1] == [70 * 16000, 20 * 16000]
    assert stub.calls[0][2]["language"] is None and stub.calls[0][2]["word_timestamps"] is True
    assert [len(o) for o in out] == [3, 1] and [s["offset"] for s in out[0]] == [0.0, 30.0, 60.0]
    assert out[0][1]["words"] == [(" part1", [31.0, 32.0])] and out[0][1]["token_ids"] == [11] and out[0][1]["language"] == "en"


def test_target_diarization_switch_defaults_off():
    import inspect
    from targetdiarization_amd.target_diarization import TargetDiarization
    assert inspect.signature(TargetDiarization.__init__).parameters["whisper_long_form"].default is False


# ---- 6. the C-ABI without a device
@pytest.fixture(scope="module")
def lib():
    from targetdiarization_amd.build import build_lib
    build_lib()
    return _lib.lib()


def test_argument_validation_without_gpu(lib):
    import ctypes as C
    err = lambda: lib.tdx_last_error().decode()
    assert lib.tdx_whisper_logmel_long_workspace_bytes(None, 16000) == 0
    assert lib.tdx_whisper_logmel_long(None, None, 16000, None, None, 0, None) == 1 and "tdx_whisper_logmel_long: NULL argument" in err()
    arr = lambda v: (C.c_int * len(v))(*v)
    assert lib.tdx_whisper_decode_ts(None, None, 1, arr([1]), 1, arr([1]), None, None, 0, None, 0, 0, 5, -1, arr([1]), 0, None, None, None, 0, None, 0,
                                     None, None, None, None, None, 0, None) == 1 and "tdx_whisper_decode_ts: bad argument" in err()
