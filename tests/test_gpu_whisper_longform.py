"""Whisper long-form transcription on the device: tdx_whisper_logmel_long, tdx_whisper_decode_ts and
WhisperASR.transcribe against tests/whisper_longform_oracle.py in fp64, on the tiny models of whisper_longform_cases.py.

The decode tests feed the oracle the device's own encoder output.  Every decision of the oracle (an argmax, or the mass-versus-
best-text test) must keep a margin above MARGIN, which each test asserts by recomputing the margins before it looks at the device's
ids: no step is excluded.  MARGIN and SCORE_TOL are those of tests/test_gpu_whisper.py."""
import functools
import os

import numpy as np
import pytest
import torch

import whisper_longform_cases as lc
import whisper_longform_oracle as lo
import whisper_oracle as wo
from targetdiarization_amd import _lib
from targetdiarization_amd import whisper as W

pytestmark = pytest.mark.gpu

MARGIN, SCORE_TOL = 1e-3, 1e-3
# a probability whose logarithm is within SCORE_TOL is within p (e^SCORE_TOL - 1) <= 1.001e-3
NOSPEECH_TOL = 1.001e-3
# 10 x the oracle's own fp32-vs-fp64 gap, as in tests/test_gpu_whisper.py: by frames of context
LOGMEL_BAR = {ctx: 10 * gap for ctx, gap in wo.LOGMEL_GAP.items()}


@functools.lru_cache(maxsize=None)
def model(name, scale=lc.SCALE, boost=0.0):
    cfg, sd = lc.weights(name, 1, scale, boost)
    return W.WhisperASR(sd, cfg, device="cuda:0", generation_config=lc.gen_config(name)), cfg, wo.cast(sd)


def run_rows(m, name, state, rows, max_initial=None, eos=None, nospeech=True, heads=None):
    g = lc.gen_config(name)
    begin = [r.get("begin", len(r["prefix"])) for r in rows]
    ids, sc, cnt, nosp, xattn = m.decode_ts(state, [r["prefix"] for r in rows], [r["max_new"] for r in rows], suppress=g["suppress_tokens"],
                                            begin_suppress=g["begin_suppress_tokens"], eos=eos, max_initial_timestamp_index=-1 if max_initial is None else max_initial,
                                            begin=begin, sot_pos=[r["sot_pos"] for r in rows] if nospeech else None, heads=heads)
    return ids.cpu(), sc.cpu(), cnt.cpu().tolist(), (nosp.cpu() if nosp is not None else None), xattn


def generated(ids, sc, cnt, rows):
    toks, scs = [], []
    for b, r in enumerate(rows):
        p0 = len(r["prefix"]) - 1
        toks.append(ids[b, p0:p0 + cnt[b]].tolist()); scs.append(sc[b, p0:p0 + cnt[b]].double())
    return toks, scs


def check_against_oracle(name, got, rows, want):
    ids, sc, cnt, nosp, _ = got
    toks, scs = generated(ids, sc, cnt, rows)
    for b, (r, w) in enumerate(zip(rows, want)):
        assert toks[b] == w["tokens"], (b, toks[b], w["tokens"])
        err = float((scs[b] - torch.tensor(w["scores"], dtype=torch.float64)).abs().max())
        assert err <= SCORE_TOL, (b, err)
        if nosp is not None:
            assert abs(float(nosp[b]) - w["no_speech_prob"]) <= NOSPEECH_TOL, (b, float(nosp[b]), w["no_speech_prob"])
        assert bool((ids[b, len(r["prefix"]) - 1 + cnt[b]:] == -1).all())             # nothing after the row's last step


# ---- 1. decode_ts against the oracle: B = 1, 3, 9 (the skinny Linear changes kernels at 9 rows), prefixes of different lengths
@pytest.mark.parametrize("name,B", [("S", 1), ("S", 3), ("S", 9), ("M", 3)])
def test_decode_ts(name, B):
    m, cfg, sd64 = model(name)
    feats, rows = lc.decode_case(name, B)
    enc, state = m.encode(feats, with_state=True)
    want = lc.oracle_rows(name, sd64, cfg, enc.cpu().double(), rows)
    assert min(min(w["margins"]) for w in want) > MARGIN                              # no decision of the oracle is close: nothing to exclude
    T = cfg["n_text_ctx"]
    assert [len(w["tokens"]) for w in want] == [min(r["max_new"], T - len(r["prefix"])) if w["tokens"][-1] != lc.ids_of(name)["eos"] else len(w["tokens"])
                                                for r, w in zip(rows, want)]
    if B >= 3:
        assert len({len(r["prefix"]) for r in rows}) >= 3 and any(len(w["tokens"]) == 2 for w in want) and any(len(w["tokens"]) == 4 for w in want)
    got = run_rows(m, name, state, rows)
    print(f"decode_ts {name} B={B}: counts {got[2]}, no-speech {[round(float(v), 4) for v in got[3]]}")
    check_against_oracle(name, got, rows, want)
    # a row's results do not depend on its batch: alone (B <= 8 share one Linear kernel), or at another place among other rows
    # (9 rows and more run the MFMA Linear, which a lone row would not)
    toks, scs = generated(*got[:3], rows)
    if 1 < B <= 8:
        for b in range(B):
            one = run_rows(m, name, state[:, :, b:b + 1].contiguous(), rows[b:b + 1])
            t1, s1 = generated(*one[:3], rows[b:b + 1])
            assert t1[0] == toks[b] and torch.equal(s1[0], scs[b]) and float(one[3][0]) == float(got[3][b])
    if B > 8:
        perm = list(reversed(range(B)))
        other = run_rows(m, name, state[:, :, perm].contiguous(), [rows[b] for b in perm])
        t2, s2 = generated(*other[:3], [rows[b] for b in perm])
        for k, b in enumerate(perm):
            assert t2[k] == toks[b] and torch.equal(s2[k], scs[b]) and float(other[3][k]) == float(got[3][b])


# ---- 2. one row per branch of the rules, reached through `begin`; with and without max_initial_timestamp_index
@pytest.mark.parametrize("name", ["S", "M"])
@pytest.mark.parametrize("max_initial", [None, 5])
def test_rule_branches(name, max_initial):
    m, cfg, sd64 = model(name)
    I, g, V = lc.ids_of(name), lc.gen_config(name), cfg["vocab"]
    feats, rows = lc.branch_case(name)
    enc, state = m.encode(feats, with_state=True)
    enc64 = enc.cpu().double()
    want = lc.oracle_rows(name, sd64, cfg, enc64, rows, max_initial)
    assert min(min(w["margins"]) for w in want) > MARGIN
    flips = 0
    with torch.no_grad():
        for b, (r, w) in enumerate(zip(rows, want)):                                   # the first decision lies in the set the rules allow
            seq = r["prefix"][3:]
            lg = wo.decoder_hidden(sd64, cfg, enc64[b:b + 1], torch.tensor([r["prefix"]]))[0, -1] @ sd64["model.decoder.embed_tokens.weight"].T
            deny = wo._deny(V, g["suppress_tokens"] + (g["begin_suppress_tokens"] if not seq else []))
            pre = lo.history_rules(V, seq, not seq, I["tb"], I["eos"], max_initial, deny)
            assert bool(pre[w["tokens"][0]])
            flips += int(lg.masked_fill(~pre, float("-inf")).argmax()) != w["tokens"][0]
    first = want[0]["tokens"][0]
    assert first >= I["tb"] and (max_initial is None or first <= I["tb"] + max_initial)
    if name == "M":                                                                    # S's decisions hardly depend on the audio and no seed made one flip:
        assert flips >= 1                                                              # only M's case is sure to hold a result the mass rule changed
    got = run_rows(m, name, state, rows, max_initial)
    print(f"rule branches {name} max_initial={max_initial}: first ids {[w['tokens'][0] for w in want]}, mass flips {flips}")
    check_against_oracle(name, got, rows, want)
    sub = [0, 1, 2, 5, 7]                                                              # and through the B <= 8 kernels: empty, text only, text then a timestamp, a pair
    got3 = run_rows(m, name, state[:, :, sub].contiguous(), [rows[b] for b in sub], max_initial)
    check_against_oracle(name, got3, [rows[b] for b in sub], [want[b] for b in sub])


# ---- 3. eos ends a row and leaves the others alone
def test_eos_stops_a_row():
    name = "S"
    m, cfg, sd64 = model(name)
    I = lc.ids_of(name)
    feats, rows = lc.decode_case(name, 3)
    enc, state = m.encode(feats, with_state=True)
    enc64 = enc.cpu().double()
    base = lc.oracle_rows(name, sd64, cfg, enc64, rows)
    t0 = base[0]["tokens"]
    k = next(i for i in range(2, len(t0)) if t0[i] < I["eos"] and t0[i] not in t0[:i] and t0[i] > 3)
    eos = t0[k]                                                                        # row 0 emits this id at step k: as eos it ends the row there
    want = lc.oracle_rows(name, sd64, cfg, enc64, rows, eos=eos)
    assert min(min(w["margins"]) for w in want) > MARGIN and want[0]["tokens"][-1] == eos and len(want[0]["tokens"]) < len(t0)
    got = run_rows(m, name, state, rows, eos=eos)
    check_against_oracle(name, got, rows, want)
    assert got[2][0] == len(want[0]["tokens"]) and got[2][1:] == [len(w["tokens"]) for w in want[1:]]


# ---- 4. no-speech off and capture on / off leave ids and scores alone, bit for bit; the captured rows are the decode's
def test_nospeech_and_capture_do_not_touch_the_result():
    name = "S"
    m, cfg, sd64 = model(name)
    feats, rows = lc.decode_case(name, 3)
    _, state = m.encode(feats, with_state=True)
    full = run_rows(m, name, state, rows, heads=[[1, 0], [0, 0]])
    plain = run_rows(m, name, state, rows, nospeech=False)
    assert plain[3] is None and plain[4] is None
    assert torch.equal(full[0], plain[0]) and torch.equal(full[1], plain[1]) and full[2] == plain[2]
    x = full[4].cpu()
    assert x.shape == (3, 2, max(1, max(r["max_new"] for r in rows) - 1), cfg["n_audio_ctx"])
    for b, r in enumerate(rows):                     # row p - prefix_len[b]: one softmax row per generated id but the last, zeros after
        n = max(0, full[2][b] - 1)
        assert bool((x[b, :, n:] == 0).all())
        if n:
            assert float((x[b, :, :n].sum(-1) - 1.0).abs().max()) < 1e-5
    # row 0's rows are what tdx_whisper_decode_xattn captures when the same ids are fed as a prefix (a row depends on the ids up to
    # its position only): bit for bit
    g, p0, n = lc.gen_config(name), rows[0]["prefix"], full[2][0] - 1
    fed = p0 + full[0][0, len(p0) - 1:len(p0) - 1 + n].tolist()
    _, _, _, x2 = m.decode_xattn(state[:, :, :1].contiguous(), fed, 0, g["suppress_tokens"], (), None, first_row=len(p0), max_rows=n, heads=[[1, 0], [0, 0]])
    assert n >= 8 and torch.equal(x2.cpu()[0], x[0, :, :n])


# ---- 5. the long log-mel
def long_clips():
    blk = 4096 * 160                                 # samples per internal block of frames
    loud_last = torch.cat([1e-4 * lc.noise(2 * blk + 160 * 50, 3), lc.noise(160 * 200 + 7, 4, 0.5)])
    return {"one": lc.noise(1, 1), "short": lc.noise(159, 2), "window": lc.noise(160 * 128 + 37, 5) + 0.3 * torch.sin(2 * np.pi * 440.0 * torch.arange(160 * 128 + 37) / 16000.0),
            "hop": lc.noise(160, 6), "tiny": lc.noise(201, 7), "blocks": lc.noise(2 * blk + 160 * 77 + 13, 8), "loud_last": loud_last}


@pytest.mark.parametrize("clip", ["one", "short", "hop", "tiny", "window", "blocks", "loud_last"])
def test_logmel_long(clip):
    m, cfg, _ = model("S")
    x = long_clips()[clip]
    want = lo.logmel_long(x, cfg["n_mels"])
    got = m.features_long(x).cpu().double()
    assert got.shape == want.shape == (cfg["n_mels"], x.shape[0] // 160)
    if clip in ("one", "short"):
        return                                       # no frame: nothing to compare, and nothing was written
    bar = LOGMEL_BAR[100] if want.shape[1] <= 200 else LOGMEL_BAR[1500]
    err = float((got - want).abs().max())
    print(f"logmel_long {clip}: {want.shape[1]} frames, max error {err:.2e} (bar {bar:.1e})")
    assert torch.isfinite(got).all() and err <= bar
    if clip == "loud_last":                          # the clamp is the clip's: the quiet blocks sit on the floor the last block sets
        assert float(got[:, :8192].max()) == float(got.min()) and float(want[:, :8192].max()) == float(want.min())
    if clip == "window":                             # against tdx_whisper_logmel on the same 128 frames: the clip is its own window
        old = m.features([x[:160 * 128]]).cpu().double()[0]
        assert float((old - lo.logmel_long(x[:160 * 128], cfg["n_mels"])).abs().max()) <= bar


def test_logmel_long_workspace_does_not_grow():
    m, _, _ = model("S")
    ws = lambda n: int(m._l.tdx_whisper_logmel_long_workspace_bytes(m._h, n))
    assert ws(16000 * 1800) == ws(16000 * 60) == ws(4096 * 160) > ws(160 * 100) > 0 and ws(0) == 0


# ---- 6. transcribe end to end
TRANSCRIBE_SEEDS = (25, 26)


@pytest.mark.parametrize("condition", [False, True])
def test_transcribe(condition):
    name = "S"
    m, cfg, sd64 = model(name)
    I, g, T = lc.ids_of(name), lc.gen_config(name), cfg["n_text_ctx"]
    wavs = [lc.noise(5 * 16000, TRANSCRIBE_SEEDS[0]), lc.noise(9 * 16000 + 55, TRANSCRIBE_SEEDS[1])]
    log = []
    real_encode, real_decode = m.encode, m.decode_ts

    def encode(feats, with_state=False):
        out = real_encode(feats, with_state)
        log.append({"enc": out[0].cpu().double()})
        return out

    def decode_ts(state, prefixes, max_new, *a, **k):
        out = real_decode(state, prefixes, max_new, *a, **k)
        log[-1].update(prefixes=[list(p) for p in prefixes], max_new=list(max_new), ids=out[0].cpu(), scores=out[1].cpu(), counts=out[2].cpu().tolist(),
                       nosp=out[3].cpu().tolist())
        return out
    m.encode, m.decode_ts = encode, decode_ts
    try:
        res = m.transcribe(wavs, language="en", condition_on_prev_tokens=condition, no_speech_threshold=0.6, logprob_threshold=-1.0)
    finally:
        del m.encode, m.decode_ts
    F = [w.shape[0] // 160 for w in wavs]
    assert len(log[0]["prefixes"]) == 2 and len(log[-1]["prefixes"]) == 1            # both clips share the calls while both run
    # (a) the oracle loop, its windows answered by the device's own decode results: segments, seeks, prefixes, budgets, skips
    for i in range(2):
        rounds = iter([r for r in log if len(r["prefixes"]) == 2 or i == 1])           # clip 1 is row 1, or row 0 once clip 0 has left
        used = []

        def dec(seek, nfr, prefix, max_new):
            r = next(rounds)
            k = i if len(r["prefixes"]) == 2 else 0
            assert r["prefixes"][k] == prefix and r["max_new"][k] == max_new
            p0, n = len(prefix) - 1, r["counts"][k]
            used.append((r, k))
            return {"tokens": r["ids"][k, p0:p0 + n].tolist(), "scores": r["scores"][k, p0:p0 + n].double().tolist(), "no_speech_prob": r["nosp"][k]}
        want = lo.transcribe_loop(dec, F[i], 128, [I["sot"], I["en"], I["transcribe"]], I["tb"], I["eos"], I["prev"], T, g["max_length"], None, condition, 0.6, -1.0)
        assert next(rounds, None) is None             # the clip was in exactly these calls
        segs = res[i]["segments"]
        assert [s["tokens"] for s in segs] == [s["tokens"] for s in want["segments"]] and len(want["windows"]) >= 4
        assert [(s["seek"], s["start"], s["end"]) for s in segs] == [(s["seek"], pytest.approx(s["start"]), pytest.approx(s["end"])) for s in want["segments"]]
        assert [s["avg_logprob"] for s in segs] == [pytest.approx(s["avg_logprob"], abs=1e-6) for s in want["segments"]]
        for s in segs:                               # words: over the non-timestamp ids, inside the clip, in order
            assert [w for w, _ in s["words"]] == [f"<{t}>" for t in s["tokens"] if t < I["eos"]]
            assert all(0.0 <= a <= b <= F[i] / 100.0 + 0.02 for _, (a, b) in s["words"])
            assert all(s["seek"] / 100.0 - 1e-9 <= a for _, (a, _b) in s["words"])
        # (b) the ids of every window against the fp64 oracle model on the device's encoder output
        for r, k in used:
            with torch.no_grad():
                w = lo.greedy_ts(sd64, cfg, r["enc"][k:k + 1], r["prefixes"][k], r["max_new"][k], I["tb"], I["eos"], g["suppress_tokens"], g["begin_suppress_tokens"],
                                 None, None, I["nospeech"], len(r["prefixes"][k]) - 3)
            assert min(w["margins"]) > MARGIN
            p0, n = len(r["prefixes"][k]) - 1, r["counts"][k]
            assert r["ids"][k, p0:p0 + n].tolist() == w["tokens"]
            assert float((r["scores"][k, p0:p0 + n].double() - torch.tensor(w["scores"], dtype=torch.float64)).abs().max()) <= SCORE_TOL
            assert abs(r["nosp"][k] - w["no_speech_prob"]) <= NOSPEECH_TOL
    assert res[0]["text"] == "".join(s["text"] for s in res[0]["segments"]) and [r["key"] for r in res] == ["clip_0", "clip_1"]


# ---- 7. the argument checks that need a model
def test_decode_ts_argument_validation():
    name = "S"
    m, cfg, _ = model(name)
    I, T = lc.ids_of(name), cfg["n_text_ctx"]
    state = torch.zeros(cfg["dec_layers"], 2, 1, cfg["n_audio_ctx"], cfg["d_model"], device="cuda:0")
    init = [I["sot"], I["en"], I["transcribe"]]

    def msg(prefix=init, max_new=4, **kw):
        args = dict(eos=I["eos"], no_timestamps_id=I["tb"] - 1, sot_pos=[0])
        args.update(kw)
        with pytest.raises(_lib.TdxError) as e:
            m.decode_ts(state, [prefix], max_new, **args)
        return str(e.value)
    assert "leaves no room" in msg(prefix=[5] * (T - 3) + init)
    assert "first timestamp id" in msg(no_timestamps_id=cfg["vocab"] - 1) and "first timestamp id" in msg(no_timestamps_id=-1)
    assert "eos must be below" in msg(eos=I["tb"])
    assert "sot_pos of row 0 outside its prefix" in msg(sot_pos=[3])
    assert "begin of row 0" in msg(begin=[0]) and "begin of row 0" in msg(begin=[4])
    assert "max_new of row 0 is negative" in msg(max_new=-1)
    assert "alignment head" in msg(heads=[[2, 0]]) and "prefix id outside" in msg(prefix=[cfg["vocab"]] + init)
    ids, _, cnt, _, _ = m.decode_ts(state, [init], 0, eos=I["eos"], no_timestamps_id=I["tb"] - 1)        # nothing to generate: the prefix is scored
    assert cnt.cpu().tolist() == [0] and bool((ids[0, :3] >= 0).all()) and bool((ids[0, 3:] == -1).all())
    # a max_initial_timestamp_index past the last timestamp id is no limit (clamped on the host: tb + index cannot overflow)
    free = m.decode_ts(state, [init], 3, eos=I["eos"], no_timestamps_id=I["tb"] - 1, max_initial_timestamp_index=-1)
    huge = m.decode_ts(state, [init], 3, eos=I["eos"], no_timestamps_id=I["tb"] - 1, max_initial_timestamp_index=2 ** 31 - 1)
    assert torch.equal(free[0], huge[0]) and torch.equal(free[1], huge[1]) and int(huge[0][0, 2]) >= I["tb"] and bool(torch.isfinite(huge[1]).all())


# ---- 8. tdx_whisper_decode gives what it gave before tdx_whisper_decode_ts shared its decoder-layer launches
@pytest.mark.parametrize("nb", [3, 12])
def test_old_decode_is_unchanged(gold, nb):
    z = np.load(os.path.join(gold, "whisper_decode_golden.npz"))
    ids, sc, cnt = lc.old_decode_run(W, nb)
    assert cnt.tolist() == z[f"counts{nb}"].tolist() and int(cnt.min()) >= 1
    assert np.array_equal(ids.numpy(), z[f"ids{nb}"]) and np.array_equal(sc.numpy(), z[f"scores{nb}"])          # bit for bit


# ---- 9. tdx_whisper_decode_ts gives what it gave before the three decode entry points shared one loop: every kernel path of the
# smallest shapes that reach them (the B <= 8 and B > 8 Linear, tb inside the first and the second head slice, a partial last slice,
# every rule branch, the mass-rule flip, the no-speech pair, the per-clip capture row)
def test_decode_ts_is_unchanged(gold):
    z = np.load(os.path.join(gold, "whisper_decode_ts_golden.npz"))
    got = lc.decode_ts_golden_run(lambda name: model(name)[0])
    assert sorted(got) == sorted(k for k in z.files if k != "commit") and len(got) == 17 and len(str(z["commit"])) == 40
    for k, v in got.items():
        assert v.dtype == z[k].dtype and np.array_equal(v, z[k]), k                                              # bit for bit
