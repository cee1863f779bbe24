"""Whisper's sampled decoding and temperature fallback on the device: the noise hook, tdx_whisper_decode_ts_sample and
WhisperASR.transcribe(temperature=(...)) against tests/whisper_sample_oracle.py in fp64, on the tiny models of
whisper_longform_cases.py.

The decode tests feed the oracle the device's own encoder output.  Every decision of the oracle must keep a margin, which each test
asserts by recomputing the margins before it looks at the device's ids; no step is excluded: a draw's z gap above MARGIN / T + 2
NOISE_TOL (the device's logit error, bounded by MARGIN as in tests/test_gpu_whisper.py, is amplified by 1 / T, and each of the two
z carries one noise error), a mass-rule margin and a greedy top-2 gap above MARGIN.  The noise seeds were searched on the CPU (on the
oracle's own encoder output) so that these hold."""
import functools

import numpy as np
import pytest
import torch

import whisper_longform_cases as lc
import whisper_longform_oracle as lo
import whisper_oracle as wo
import whisper_sample_oracle as so
from targetdiarization_amd import _lib
from targetdiarization_amd import whisper as W

pytestmark = pytest.mark.gpu

MARGIN, SCORE_TOL = 1e-3, 1e-3
NOSPEECH_TOL = 1.001e-3                                  # as tests/test_gpu_whisper_longform.py
# 10 x the oracle's own fp32-vs-fp64 gap of g over all 2^23 uniforms (so.noise_gap() = 6.009e-07, pinned by the host test): the
# project's convention for a bar on fp32 arithmetic (LOGMEL_BAR)
NOISE_TOL = 10 * so.NOISE_GAP
TEMPS = [0.0, 0.2, 1.0, 0.6, 0.4, 0.8, 1.0, 0.0, 0.2]
DECODE_SEEDS = {("S", 1): 1, ("S", 3): 1, ("S", 9): 1, ("M", 3): 1}
BRANCH_SEEDS = {"S": 1, "M": 1}


def temps_of(B):
    return [1.0] if B == 1 else TEMPS[:B]


def stream_of(b):
    return ((b + 1) << 32) | (7 * b + 3)


@functools.lru_cache(maxsize=None)
def model(name):
    cfg, sd = lc.weights(name, 1, lc.SCALE)
    return W.WhisperASR(sd, cfg, device="cuda:0", generation_config=lc.gen_config(name)), cfg, wo.cast(sd)


def run_rows(m, name, state, rows, temps=None, streams=None, seed=0, max_initial=None, heads=None):
    g = lc.gen_config(name)
    kw = {} if temps is None else dict(temperature=temps, streams=streams, seed=seed)
    ids, sc, cnt, nosp, xattn = m.decode_ts(state, [r["prefix"] for r in rows], [r["max_new"] for r in rows], suppress=g["suppress_tokens"],
                                            begin_suppress=g["begin_suppress_tokens"], max_initial_timestamp_index=-1 if max_initial is None else max_initial,
                                            begin=[r.get("begin", len(r["prefix"])) for r in rows], sot_pos=[r["sot_pos"] for r in rows], heads=heads, **kw)
    return ids.cpu(), sc.cpu(), cnt.cpu(), nosp.cpu(), xattn


def oracle_rows(name, sd64, cfg, enc64, rows, temps, streams, seed, max_initial=None):
    I, g = lc.ids_of(name), lc.gen_config(name)
    out = []
    with torch.no_grad():
        for b, r in enumerate(rows):
            out.append(so.sample_ts(sd64, cfg, enc64[b:b + 1], r["prefix"], r["max_new"], I["tb"], I["eos"], g["suppress_tokens"], g["begin_suppress_tokens"],
                                    max_initial, r.get("begin"), I["nospeech"], r["sot_pos"], temps[b], streams[b], seed))
    return out


def assert_margins(want, temps):
    for w, T in zip(want, temps):
        bound = MARGIN if T == 0 else MARGIN / T + 2 * NOISE_TOL
        assert min(w["draw_margins"]) > bound, (T, min(w["draw_margins"]), bound)
        assert min(w["mass_margins"]) > MARGIN, (T, min(w["mass_margins"]))


def generated(got, rows):
    ids, sc, cnt = got[:3]
    toks, scs = [], []
    for b, r in enumerate(rows):
        p0, n = len(r["prefix"]) - 1, int(cnt[b])
        toks.append(ids[b, p0:p0 + n].tolist()); scs.append(sc[b, p0:p0 + n].double())
    return toks, scs


def check_against_oracle(got, rows, want):
    toks, scs = generated(got, rows)
    for b, (r, w) in enumerate(zip(rows, want)):
        assert toks[b] == w["tokens"], (b, toks[b], w["tokens"])
        err = float((scs[b] - torch.tensor(w["scores"], dtype=torch.float64)).abs().max())
        assert err <= SCORE_TOL, (b, err)
        assert abs(float(got[3][b]) - w["no_speech_prob"]) <= NOSPEECH_TOL, (b, float(got[3][b]), w["no_speech_prob"])
        assert bool((got[0][b, len(r["prefix"]) - 1 + int(got[2][b]):] == -1).all())


def same_row(a, ka, b, kb, ra, rb):
    (ta, sa), (tb_, sb) = generated(a, ra), generated(b, rb)
    return ta[ka] == tb_[kb] and torch.equal(sa[ka], sb[kb]) and int(a[2][ka]) == int(b[2][kb]) and float(a[3][ka]) == float(b[3][kb])


# ---- 1. the noise: words bit for bit, g within NOISE_TOL; 130 ids span a slice edge and the text / timestamp edge
@pytest.mark.parametrize("n0", [0, 61, lc.ids_of("S")["tb"] - 2])
def test_noise(n0):
    d, count = _lib.diag(), 130
    worst = 0.0
    for seed, stream, p in [(0, 0, 0), (1, stream_of(2), 5), (0x9e3779b97f4a7c15, (0xfffffff1 << 32) | 0xfffffff3, 447)]:
        g = torch.zeros(count, device="cuda:0")
        w = torch.zeros(count, dtype=torch.int32, device="cuda:0")
        assert d.tdx_test_whisper_noise(seed, stream, p, n0, count, g.data_ptr(), w.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        want = so.noise_words(seed, stream, p, np.arange(n0, n0 + count))
        assert np.array_equal(w.cpu().numpy().view(np.uint32), want)
        worst = max(worst, float(np.abs(g.cpu().numpy().astype(np.float64) - so.gumbel64(want)).max()))
    print(f"noise n0={n0}: max |g - g64| {worst:.2e} (NOISE_TOL {NOISE_TOL:.2e})")
    assert worst <= NOISE_TOL
    assert d.tdx_test_whisper_noise(0, 0, 0, 0, 0, g.data_ptr(), w.data_ptr(), None) != 0 and d.tdx_test_whisper_noise(0, 0, 0, 0, 4, None, w.data_ptr(), None) != 0


# ---- 2. decode_ts with sampling against sample_ts, temperatures mixed within the batch
@pytest.mark.parametrize("name,B", [("S", 1), ("S", 3), ("S", 9), ("M", 3)])
def test_decode_ts_sampled(name, B):
    m, cfg, sd64 = model(name)
    feats, rows = lc.decode_case(name, B)
    temps, streams, seed = temps_of(B), [stream_of(b) for b in range(B)], DECODE_SEEDS[(name, B)]
    enc, state = m.encode(feats, with_state=True)
    want = oracle_rows(name, sd64, cfg, enc.cpu().double(), rows, temps, streams, seed)
    assert_margins(want, temps)
    moved = sum(a != c for w, T in zip(want, temps) if T == 1.0 for a, c in zip(w["tokens"], w["greedy"]))
    assert moved >= 1                                    # at T = 1 some draw is not the argmax: the noise decides something
    if B >= 3:
        assert len({len(r["prefix"]) for r in rows}) >= 3
    got = run_rows(m, name, state, rows, temps, streams, seed)
    print(f"decode_ts sampled {name} B={B}: counts {got[2].tolist()}, {moved} draws at T=1 differ from the argmax")
    check_against_oracle(got, rows, want)
    # a row's result depends on (seed, stream, its inputs) alone: a same-seed rerun, a row alone (B <= 8 share one Linear kernel), the
    # reversed order (9 rows and more run the MFMA Linear); another seed changes an id
    again = run_rows(m, name, state, rows, temps, streams, seed)
    assert all(torch.equal(a, b) for a, b in zip(got[:4], again[:4]))
    if 1 < B <= 8:
        for b in range(B):
            one = run_rows(m, name, state[:, :, b:b + 1].contiguous(), rows[b:b + 1], temps[b:b + 1], streams[b:b + 1], seed)
            assert same_row(one, 0, got, b, rows[b:b + 1], rows)
    if B > 8:
        perm = list(reversed(range(B)))
        other = run_rows(m, name, state[:, :, perm].contiguous(), [rows[b] for b in perm], [temps[b] for b in perm], [streams[b] for b in perm], seed)
        for k, b in enumerate(perm):
            assert same_row(other, k, got, b, [rows[q] for q in perm], rows)
    reseeded = run_rows(m, name, state, rows, temps, streams, seed + 1)
    assert generated(reseeded, rows)[0] != generated(got, rows)[0]
    for b, T in enumerate(temps):                        # ... but never one of a greedy row
        if T == 0:
            assert same_row(reseeded, b, got, b, rows, rows)


# ---- 3. a temp = 0 row inside a sampling launch, and a launch whose temperatures are all 0: the greedy entry point's bits
@pytest.mark.parametrize("name,B", [("S", 3), ("S", 9)])
def test_greedy_rows_of_a_sampling_launch(name, B):
    m, cfg, _ = model(name)
    feats, rows = lc.decode_case(name, B)
    _, state = m.encode(feats, with_state=True)
    old = run_rows(m, name, state, rows, heads=[[1, 0]])
    temps, streams = temps_of(B), [stream_of(b) for b in range(B)]
    mixed = run_rows(m, name, state, rows, temps, streams, 5, heads=[[1, 0]])
    zeros = run_rows(m, name, state, rows, [0.0] * B, streams, 5, heads=[[1, 0]])
    assert all(torch.equal(a, b) for a, b in zip(old[:4], zeros[:4])) and torch.equal(old[4], zeros[4])
    greedy = [b for b, T in enumerate(temps) if T == 0]
    assert greedy and len(greedy) < B
    for b in greedy:
        assert all(torch.equal(a[b], c[b]) for a, c in zip(old[:4], mixed[:4])) and torch.equal(old[4][b], mixed[4][b])
    assert any(not torch.equal(old[0][b], mixed[0][b]) for b in range(B) if b not in greedy)
    ws = lambda n: int(m._l.tdx_whisper_decode_sample_workspace_bytes(m._h, n))
    assert ws(B) > m.workspace_bytes(B) and ws(0) == 0 and ws(33) == 0


# ---- 4. every branch of the rules at T = 0.6
@pytest.mark.parametrize("name", ["S", "M"])
def test_rule_branches_sampled(name):
    m, cfg, sd64 = model(name)
    I, g, V = lc.ids_of(name), lc.gen_config(name), cfg["vocab"]
    feats, rows = lc.branch_case(name)
    B = len(rows)
    temps, streams, seed = [0.6] * B, [stream_of(b) for b in range(B)], BRANCH_SEEDS[name]
    enc, state = m.encode(feats, with_state=True)
    enc64 = enc.cpu().double()
    want = oracle_rows(name, sd64, cfg, enc64, rows, temps, streams, seed)
    assert_margins(want, temps)
    flips = 0
    with torch.no_grad():
        for b, (r, w) in enumerate(zip(rows, want)):     # the first decision lies in the set the rules allow
            seq = r["prefix"][3:]
            lg = wo.decoder_hidden(sd64, cfg, enc64[b:b + 1], torch.tensor([r["prefix"]]))[0, -1] @ sd64["model.decoder.embed_tokens.weight"].T
            deny = wo._deny(V, g["suppress_tokens"] + (g["begin_suppress_tokens"] if not seq else []))
            pre = lo.history_rules(V, seq, not seq, I["tb"], I["eos"], None, deny)
            assert bool(pre[w["tokens"][0]])
            if int(lg.masked_fill(~pre, float("-inf")).argmax()) < I["tb"] and not bool(lo.ts_rules(lg, seq, not seq, I["tb"], I["eos"], None, deny)[:I["tb"]].any()):
                flips += 1                               # the best allowed id is text, yet the timestamps hold more mass:
                assert w["tokens"][0] >= I["tb"]         # the draw is still among the timestamps
    assert want[0]["tokens"][0] >= I["tb"]
    if name == "M":                                      # (as in tests/test_gpu_whisper_longform.py: only M's case holds a flipped row)
        assert flips >= 1
    got = run_rows(m, name, state, rows, temps, streams, seed)
    print(f"rule branches sampled {name}: first ids {[w['tokens'][0] for w in want]}, mass flips {flips}")
    check_against_oracle(got, rows, want)
    sub = [0, 1, 2, 5, 7]                                # and through the B <= 8 kernels
    got5 = run_rows(m, name, state[:, :, sub].contiguous(), [rows[b] for b in sub], [temps[b] for b in sub], [streams[b] for b in sub], seed)
    check_against_oracle(got5, [rows[b] for b in sub], [want[b] for b in sub])


# ---- 5. transcribe with the fallback.  The thresholds were chosen from the oracle's own per-attempt values on these clips (printed
# below), with gaps far above SCORE_TOL, so that one window stops at 0.0, one at a later temperature and one exhausts the list
FB_TEMPS = (0.0, 0.4, 1.0)
FB_SEEDS = (25, 26)                                      # the clips of tests/test_gpu_whisper_longform.py
FB = dict(seed=1, logprob_threshold=-2.02, compression_ratio_threshold=4.0, no_speech_threshold=0.6)


def transcribe_logged(m, wavs, **kw):
    log = []
    real_encode, real_decode = m.encode, m.decode_ts

    def encode(feats, with_state=False):
        out = real_encode(feats, with_state)
        log.append({"enc": out[0].cpu().double(), "calls": []})
        return out

    def decode_ts(state, prefixes, max_new, *a, **k):
        out = real_decode(state, prefixes, max_new, *a, **k)
        log[-1]["calls"].append({"prefixes": [list(p) for p in prefixes], "max_new": list(max_new), "temperature": k.get("temperature"),
                                 "streams": k.get("streams"), "seed": k.get("seed"), "heads": k.get("heads"), "ids": out[0].cpu(), "scores": out[1].cpu(),
                                 "counts": out[2].cpu().tolist(), "nosp": out[3].cpu().tolist()})
        return out
    m.encode, m.decode_ts = encode, decode_ts
    try:
        res = m.transcribe(wavs, **kw)
    finally:
        del m.encode, m.decode_ts
    return res, log


def test_transcribe_fallback():
    name = "S"
    m, cfg, sd64 = model(name)
    I, g, T = lc.ids_of(name), lc.gen_config(name), cfg["n_text_ctx"]
    wavs = [lc.noise(5 * 16000, FB_SEEDS[0]), lc.noise(9 * 16000 + 55, FB_SEEDS[1])]
    thr = {k: FB[k] for k in ("logprob_threshold", "compression_ratio_threshold", "no_speech_threshold")}
    res, log = transcribe_logged(m, wavs, language="en", temperature=FB_TEMPS, seed=FB["seed"], **thr)
    F = [w.shape[0] // 160 for w in wavs]
    both = lambda r: len(r["calls"][0]["prefixes"]) == 2
    stopped = []
    for i in range(2):
        rounds = iter([r for r in log if both(r) or i == 1])                           # clip 1 is row 1, or row 0 once clip 0 has left
        used = []

        def dec(seek, nfr, prefix, max_new, temp, attempt, stream, i=i):
            r = next(rounds) if attempt == 0 else dec.round
            dec.round = r
            c = r["calls"][attempt]
            if c["streams"] is None:
                assert attempt == 0 and temp == 0.0 and c["temperature"] is None
                j = i if both(r) else 0
            else:
                j = c["streams"].index(stream)
                assert c["temperature"][j] == temp and c["seed"] == FB["seed"]
            assert c["prefixes"][j] == prefix and c["max_new"][j] == max_new and c["heads"] == m.alignment_heads
            p0, n = len(prefix) - 1, c["counts"][j]
            used.append((r, i if both(r) else 0, c, j, temp, stream))
            return {"tokens": c["ids"][j, p0:p0 + n].tolist(), "scores": c["scores"][j, p0:p0 + n].double().tolist(), "no_speech_prob": c["nosp"][j]}
        want = so.transcribe_loop_fallback(dec, F[i], 128, [I["sot"], I["en"], I["transcribe"]], I["tb"], I["eos"], I["prev"], T, g["max_length"], FB_TEMPS,
                                           m.text_of, clip=i, condition=True, **thr)
        assert next(rounds, None) is None
        for w in want["windows"]:
            print(f"clip {i} seek {w['seek']}: " + ", ".join(f"T={a['temperature']} avg {a['avg_logprob']:.3f} ratio {a['compression_ratio']:.3f}" for a in w["attempts"]))
        stopped += [(len(w["attempts"]), W.needs_fallback(w["attempts"][-1]["compression_ratio"], w["avg_logprob"], w["no_speech_prob"],
                                                           (thr["compression_ratio_threshold"], thr["logprob_threshold"], thr["no_speech_threshold"])))
                    for w in want["windows"]]
        segs = res[i]["segments"]
        assert [s["tokens"] for s in segs] == [s["tokens"] for s in want["segments"]]
        assert [(s["seek"], s["temperature"], s["compression_ratio"]) for s in segs] == [(s["seek"], s["temperature"], s["compression_ratio"]) for s in want["segments"]]
        assert [(s["start"], s["end"]) for s in segs] == [(pytest.approx(s["start"]), pytest.approx(s["end"])) for s in want["segments"]]
        assert [s["avg_logprob"] for s in segs] == [pytest.approx(s["avg_logprob"], abs=1e-6) for s in want["segments"]]
        for s in segs:
            assert [w for w, _ in s["words"]] == [f"<{t}>" for t in s["tokens"] if t < I["eos"]]
            assert all(s["seek"] / 100.0 - 1e-9 <= a <= b <= F[i] / 100.0 + 0.02 for _, (a, b) in s["words"])
        for w, nxt in zip(want["windows"], want["windows"][1:]):                       # a window decoded above 0.5 does not condition the next one
            if w["reset"]:
                assert nxt["prefix"] == [I["sot"], I["en"], I["transcribe"]]
        # every attempt's ids against the fp64 oracle model on the device's encoder output
        for r, k, c, j, temp, stream in used:
            with torch.no_grad():
                w = so.sample_ts(sd64, cfg, r["enc"][k:k + 1], c["prefixes"][j], c["max_new"][j], I["tb"], I["eos"], g["suppress_tokens"],
                                 g["begin_suppress_tokens"], None, None, I["nospeech"], len(c["prefixes"][j]) - 3, temp, stream, FB["seed"])
            assert_margins([w], [temp])
            p0, n = len(c["prefixes"][j]) - 1, c["counts"][j]
            assert c["ids"][j, p0:p0 + n].tolist() == w["tokens"]
            assert float((c["scores"][j, p0:p0 + n].double() - torch.tensor(w["scores"], dtype=torch.float64)).abs().max()) <= SCORE_TOL
            assert abs(c["nosp"][j] - w["no_speech_prob"]) <= NOSPEECH_TOL
    # on the oracle loop: a window that stops at 0.0, one that stops at a later temperature, one that exhausts the list in need
    assert any(n == 1 for n, _ in stopped) and any(1 < n and not need for n, need in stopped) and any(n == len(FB_TEMPS) and need for n, need in stopped)
    assert any(s["temperature"] > 0.5 for r in res for s in r["segments"])
    # one encode per round however many attempts; the rows in need share one decode call per attempt
    assert all(1 <= len(r["calls"]) <= len(FB_TEMPS) for r in log) and any(len(r["calls"]) > 1 for r in log)
    for r in log:
        for a, c in enumerate(r["calls"][1:], 1):
            assert c["temperature"] == [FB_TEMPS[a]] * len(c["prefixes"]) and [(s >> 32) % 16 for s in c["streams"]] == [a] * len(c["prefixes"])
            assert len(c["prefixes"]) <= len(r["calls"][a - 1]["prefixes"])
    assert any(len(c["prefixes"]) == 2 for r in log for c in r["calls"][1:])             # two clips fell back together


# ---- 6. the defaults are today's transcribe
def test_transcribe_defaults():
    m, _, _ = model("S")
    wavs = [lc.noise(5 * 16000, FB_SEEDS[0]), lc.noise(9 * 16000 + 55, FB_SEEDS[1])]
    plain, log0 = transcribe_logged(m, wavs, language="en")
    zero, log1 = transcribe_logged(m, wavs, language="en", temperature=0.0)
    assert plain == zero and len(plain[0]["segments"]) >= 1 and "temperature" not in plain[0]["segments"][0]
    assert all(len(r["calls"]) == 1 and r["calls"][0]["temperature"] is None for r in log0 + log1)


# ---- 7. the argument checks
def test_sampling_argument_validation():
    name = "S"
    m, cfg, _ = model(name)
    I = lc.ids_of(name)
    state = torch.zeros(cfg["dec_layers"], 2, 2, cfg["n_audio_ctx"], cfg["d_model"], device="cuda:0")
    init = [I["sot"], I["en"], I["transcribe"]]

    def msg(**kw):
        with pytest.raises(_lib.TdxError) as e:
            m.decode_ts(state, [init, init], 2, eos=I["eos"], no_timestamps_id=I["tb"] - 1, sot_pos=[0, 0], **kw)
        return str(e.value)
    assert "temperature of row 1" in msg(temperature=[0.0, -0.1]) and "temperature of row 0" in msg(temperature=[float("nan"), 0.5])
    assert "temperature of row 1" in msg(temperature=[1.0, float("inf")])
    assert "temperature has 3 entries for 2 rows" in msg(temperature=[0.1, 0.2, 0.3])
    assert "streams has 1 entries for 2 rows" in msg(temperature=0.5, streams=[4])
    assert "begin of row 0" in msg(temperature=0.5, begin=[0, 1])                        # and the greedy entry point's checks
    ok = m.decode_ts(state, [init, init], 2, eos=I["eos"], no_timestamps_id=I["tb"] - 1, sot_pos=[0, 0], temperature=0.5, streams=[2 ** 64 - 1, 0], seed=2 ** 64 - 1)
    assert ok[2].cpu().tolist() == [2, 2] and bool(torch.isfinite(ok[1]).all())
    # NULL arrays are refused at the C boundary, by name
    l = m._l
    rc = l.tdx_whisper_decode_ts_sample(m._h, state.data_ptr(), 2, None, 3, None, None, None, 0, None, 0, I["eos"], I["tb"] - 1, -1, None, 0, None, None, None, 0,
                                        None, 0, None, None, None, None, None, None, 0, None, 0, None)
    assert rc != 0 and "temperature_host must not be NULL" in l.tdx_last_error().decode()
