"""Whisper word timestamps on the device (csrc/whisper.hip: tdx_whisper_decode_xattn, tdx_token_align; targetdiarization_amd/whisper.py)
against tests/whisper_ts_oracle.py in fp64.

Configurations C (100 audio positions) and A (1500) of tests/test_gpu_whisper.py with the recipe weights of seed 1.  Every assertion
about the oracle alone (rounding variants, stability of a path) is made on the CPU before the device's output is compared."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import whisper_oracle as wo
import whisper_ts_oracle as ts
from targetdiarization_amd import _lib
from targetdiarization_amd import whisper as W
from targetdiarization_amd.weights import recipe_whisper_state_dict, whisper_config

pytestmark = pytest.mark.gpu

CFGS = {"A": dict(d_model=128, enc_heads=2, enc_layers=2, dec_layers=2, n_mels=80, vocab=51865, n_audio_ctx=1500),
        "C": dict(d_model=128, enc_heads=2, enc_layers=2, dec_layers=2, n_mels=80, vocab=51865, n_audio_ctx=100)}
NCLIPS = {"A": 3, "C": 32}
HEADS = [[1, 1], [0, 0], [1, 0]]                        # both decoder layers, head 0 and the last head, not in layer order
CANARY = 7.0


@functools.lru_cache(maxsize=None)
def weights(name):
    cfg = whisper_config(CFGS[name])
    sd = recipe_whisper_state_dict(1, cfg)
    return cfg, sd, wo.cast(sd)


@functools.lru_cache(maxsize=None)
def ref(name):
    cfg, _, sd64 = weights(name)
    g = torch.Generator().manual_seed(11)
    feats = 0.5 * torch.randn(NCLIPS[name], cfg["n_mels"], 2 * cfg["n_audio_ctx"], generator=g)
    with torch.no_grad():
        enc = wo.encoder(sd64, cfg, feats.double())
    return feats, enc


@functools.lru_cache(maxsize=None)
def model(name):
    cfg, sd, _ = weights(name)
    return W.WhisperASR(sd, cfg, device="cuda:0")


def teacher_prefix():
    return torch.randint(0, 50257, (64,), generator=torch.Generator().manual_seed(21)).tolist()


# ---- 1. capture
@pytest.mark.parametrize("name,nb", [("C", 1), ("C", 9), ("C", 32), ("A", 3)])        # 1: the FMA Linear, 9 and 32: the MFMA one
def test_capture_teacher_forced(name, nb):
    cfg, _, sd64 = weights(name)
    prefix = teacher_prefix()
    with torch.no_grad():
        want = ts.cross_attention(sd64, cfg, ref(name)[1][:nb], torch.tensor([prefix] * nb), HEADS)
    m = model(name)
    _, state = m.encode(ref(name)[0][:nb], with_state=True)
    gi, gs, cnt = m.decode(state, prefix, 0)
    xi, xs, xc, xa = m.decode_xattn(state, prefix, 0, first_row=0, max_rows=64, heads=HEADS)
    assert torch.equal(gi, xi) and torch.equal(gs, xs) and torch.equal(cnt, xc)          # bit for bit
    got = xa.cpu().double()
    assert got.shape == want.shape == (nb, 3, 64, cfg["n_audio_ctx"])
    sums = got.sum(dim=-1)
    err = (got - want).norm(dim=-1) / want.norm(dim=-1)
    print(f"capture {name} B={nb}: row sums within {float((sums - 1).abs().max()):.2e}, per-row rel-L2 max {float(err.max()):.2e}")
    assert float((sums - 1).abs().max()) <= 1e-5
    assert float(err.max()) < 1e-4
    # a window of the positions: rows 0..3 are the steps 60..63, the rest of the buffer keeps its canary
    buf = torch.full((nb, 3, 8, cfg["n_audio_ctx"]), CANARY, device="cuda:0")
    m.decode_xattn(state, prefix, 0, first_row=60, max_rows=8, heads=HEADS, xattn=buf)
    assert torch.equal(buf[:, :, :4], xa[:, :, 60:64]) and bool((buf[:, :, 4:] == CANARY).all())


def test_capture_stops_with_the_clip():
    cfg, _, _ = weights("C")
    m = model("C")
    _, state = m.encode(ref("C")[0][:3], with_state=True)
    prefix = teacher_prefix()[:4]
    ids, _, cnt = m.decode(state, prefix, 12, eos=50257)
    assert cnt.cpu().tolist() == [12, 12, 12]
    t = ids[:, 3:15].cpu().tolist()
    k = next(i for i in range(2, 10) if t[0][i] not in t[0][:i] and t[0][i] not in t[1] and t[0][i] not in t[2])
    eos = t[0][k]                                        # clip 0 now ends at its step k, the others run on
    buf = torch.full((3, 3, 11, cfg["n_audio_ctx"]), CANARY, device="cuda:0")
    xi, xs, xc, _ = m.decode_xattn(state, prefix, 12, eos=eos, heads=HEADS, xattn=buf)
    gi, gs, gc = m.decode(state, prefix, 12, eos=eos)
    assert torch.equal(gi, xi) and torch.equal(gs, xs) and torch.equal(gc, xc)
    assert xc.cpu().tolist() == [k + 1, 12, 12]
    for b, n in enumerate(xc.cpu().tolist()):            # n ids generated: the n - 1 that were fed back have a row each
        assert float((buf[b, :, :n - 1].sum(dim=-1) - 1).abs().max()) <= 1e-5
        assert bool((buf[b, :, n - 1:] == CANARY).all())


def test_capture_argument_checks():
    m = model("C")
    _, state = m.encode(ref("C")[0][:1], with_state=True)
    for kw, text in ((dict(heads=[[2, 0]]), "alignment head (2, 0)"), (dict(heads=[[0, 2]]), "alignment head (0, 2)"), (dict(heads=[]), "nh must be"),
                     (dict(heads=[[0, 0]] * 65), "nh must be"), (dict(max_rows=0), "max_rows"), (dict(first_row=-1), "first_row")):
        with pytest.raises(_lib.TdxError, match="tdx_whisper_decode_xattn") as e:
            m.decode_xattn(state, [1, 2, 3], 0, **{"heads": HEADS, "max_rows": 4, "xattn": None, **kw})
        assert text in str(e.value)


# ---- 2. alignment on synthetic sharp attention
def embed(clips, max_rows, S, nh):
    """clips: list of float32 [nh, n, m] -> a canary-filled buffer [B, nh, max_rows, S] holding every clip in its corner"""
    buf = torch.full((len(clips), nh, max_rows, S), CANARY)
    for b, w in enumerate(clips):
        buf[b, :, :w.shape[1], :w.shape[2]] = w
    return buf


def stable_path(w, width, bar):
    """the fp64 oracle's frames, or None when the path moves under a relative 1e-5 perturbation of W, under a perturbation of M
    by the bar of the matrix check (the device's M may differ by that much), or when the oracle run in fp32 takes another path
    (two rows normalise to +-1 exactly: ties that no random perturbation lands on, but rounding does)"""
    M = ts.matrix(w.double(), width)
    f = ts.token_frames(M, "double")
    if not np.array_equal(ts.token_frames(ts.matrix(w, width), "fp32"), f):
        return None
    g = torch.Generator().manual_seed(5)
    for _ in range(2):
        wp = w.double() * (1 + 1e-5 * (2 * torch.rand(w.shape, generator=g, dtype=torch.float64) - 1))
        Mp = M + bar * (2 * torch.rand(M.shape, generator=g, dtype=torch.float64) - 1)
        if not np.array_equal(ts.token_frames(ts.matrix(wp, width), "double"), f) or not np.array_equal(ts.token_frames(Mp, "double"), f):
            return None
    return f


def check_clip(w, width, gap, frames, matrix, label, need_stable):
    """frames int [max_rows], matrix [max_rows, S] of one clip of the device against the oracle on w float32 [nh, n, m]"""
    _, n, m = w.shape
    if n == 0:
        assert bool((frames == -1).all()) and bool((matrix == 0).all())
        return
    assert bool((frames[n:] == -1).all())
    if n == 1:
        assert int(frames[0]) == 0 and bool((matrix == 0).all())
        return
    want = ts.matrix(w.double(), width)
    stable = stable_path(w, width, 10 * gap)
    assert stable is not None or not need_stable, f"{label}: choose another seed"
    got = matrix[:n, :m].double()
    assert np.array_equal(ts.token_frames(got, "fp32"), ts.token_frames(got, "double")), f"{label}: the rounding variants differ on the device's matrix"
    err = float((got - want).abs().max())
    print(f"align {label}: matrix max error {err:.2e} (bar {10 * gap:.1e}), path stable: {stable is not None}")
    assert err <= 10 * gap                                                               # (a)
    assert bool((matrix[n:] == 0).all()) and bool((matrix[:, m:] == 0).all())            # nothing outside the clip's corner
    assert np.array_equal(frames[:n].numpy(), ts.token_frames(got, "fp32"))              # (b)
    if stable is not None:
        assert np.array_equal(frames[:n].numpy(), stable)                                # (c)


@pytest.mark.parametrize("case", ts.ALIGN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_align_cases(case):
    rows, frames, nh, _ = case
    w = ts.align_case(*case)
    big = rows == 447
    buf = embed([w], rows if big else rows + 3, frames if big else frames + 5, nh).cuda()
    f, M = W.token_align(buf, [rows], [frames], 7, want_matrix=True)
    check_clip(w, 7, ts.ALIGN_GAP.get(case, 0.0), f[0].cpu().long(), M[0].cpu(), str(case), need_stable=rows > 2)


@pytest.mark.parametrize("max_rows", [600, 1100])                                       # two and four rows per thread
def test_align_rows_per_thread(max_rows):
    case = (300, 37, 3, 0)
    w = ts.align_case(*case)
    f, M = W.token_align(embed([w], max_rows, 40, 3).cuda(), [300], [37], 7, want_matrix=True)
    check_clip(w, 7, ts.ALIGN_GAP[case], f[0].cpu().long(), M[0].cpu(), f"{case} in {max_rows} rows", need_stable=True)
    f2 = W.token_align(embed([w], 303, 40, 3).cuda(), [300], [37], 7)
    assert torch.equal(f2[0, :300], f[0, :300])


def test_align_mixed_batch():
    clips = [ts.align_case(n, m, ts.ALIGN_MIXED_HEADS, ts.ALIGN_MIXED_SEED) for n, m in ts.ALIGN_MIXED]
    buf = embed(clips, ts.ALIGN_MIXED_ROWS, ts.ALIGN_MIXED_FRAMES, ts.ALIGN_MIXED_HEADS).cuda()
    f, M = W.token_align(buf, [n for n, _ in ts.ALIGN_MIXED], [m for _, m in ts.ALIGN_MIXED], 7, want_matrix=True)
    for b, (n, m) in enumerate(ts.ALIGN_MIXED):
        check_clip(clips[b], 7, ts.ALIGN_MIXED_GAP.get((n, m), 0.0), f[b].cpu().long(), M[b].cpu(), f"mixed {(n, m)}", need_stable=False)
    alone = W.token_align(buf[:1].contiguous(), [23], [100], 7)                          # a clip's frames do not depend on its batch
    assert torch.equal(alone[0], f[0])


def test_align_degenerate():
    case = (23, 100, 10, 0)
    w = ts.align_case(*case)
    w0 = w.clone()
    w0[:, :, 40] = 0.01                                                                  # a column without spread: it contributes 0
    w0[:3, :, 77] = 0.0
    for ww, width, label in ((w0, 7, "zero-std columns"), (w, 1, "median_width 1"), (w, 3, "median_width 3"), (w, 31, "median_width 31")):
        gap = ts.matrix_gap(ww, width)                                                   # the oracle's own gap on this very input
        f, M = W.token_align(embed([ww], 26, 105, 10).cuda(), [23], [100], width, want_matrix=True)
        assert bool(torch.isfinite(M).all())
        check_clip(ww, width, gap, f[0].cpu().long(), M[0].cpu(), label, need_stable=False)
    assert bool((ts.normalise(w0.double())[:, :, 40] == 0).all())                        # (the oracle treats such a column the same way)
    # clamped counts, and the argument checks
    f = W.token_align(embed([w], 23, 100, 10).cuda(), [99], [1000], 7)
    assert torch.equal(f, W.token_align(embed([w], 23, 100, 10).cuda(), [23], [100], 7))
    x = embed([w], 23, 100, 10).cuda()
    for width, text in ((0, "median_width"), (4, "median_width"), (33, "median_width")):
        with pytest.raises(_lib.TdxError, match=text):
            W.token_align(x, [23], [100], width)
    with pytest.raises(_lib.TdxError, match="max_rows"):
        W.token_align(torch.zeros(1, 1, 2049, 4, device="cuda:0"), [1], [1], 7)
    with pytest.raises(_lib.TdxError, match="nh must be"):
        W.token_align(torch.zeros(1, 65, 4, 4, device="cuda:0"), [1], [1], 7)


# ---- 3. end to end
def test_generate_with_timestamps():
    cfg, sd, sd64 = weights("C")
    enc = {b: ch for ch, b in W._BYTE_DECODER.items()}
    token_list = ["".join(enc[b] for b in (" t%d" % i).encode()) for i in range(50257)]
    m = W.WhisperASR(sd, cfg, device="cuda:0", token_list=token_list, alignment_heads=HEADS)
    g = torch.Generator().manual_seed(41)
    wavs = [0.1 * torch.randn(n, generator=g).numpy() for n in (9000, 20000, 32000)]
    plain = m.generate(wavs, max_new_tokens=12)
    timed = m.generate(wavs, max_new_tokens=12, return_timestamps=True)
    gen = m.gen_cfg
    prefix = W.decode_prefix("chinese", "transcribe", None, gen, cfg["n_text_ctx"])
    _, state = m.encode(m.features(wavs), with_state=True)
    _, _, cnt, xa = m.decode_xattn(state, prefix, 12, gen["suppress_tokens"], gen["begin_suppress_tokens"])
    nframes = [29, 63, 100]
    assert [m.num_frames(len(w)) for w in wavs] == nframes
    frames = W.token_align(xa, [n - 1 for n in cnt.cpu().tolist()], nframes).cpu().tolist()
    for b, (p, t) in enumerate(zip(plain, timed)):
        assert set(t) == set(p) | {"token_times", "words"}
        assert t["token_ids"] == p["token_ids"] and t["scores"] == p["scores"] and t["text"] == p["text"]
        n = len(t["token_ids"])
        assert n >= 2 and len(t["token_times"]) == n
        assert t["token_times"][:n - 1] == [f * 0.02 for f in frames[b][:n - 1]] and t["token_times"][-1] == t["token_times"][-2]
        assert t["token_times"][0] == 0.0 and all(a <= b_ for a, b_ in zip(t["token_times"], t["token_times"][1:]))
        assert t["token_times"][-1] <= nframes[b] * 0.02
        ordinary = [i for i in t["token_ids"] if i < gen["eos_token_id"]]
        assert [w for w, _ in t["words"]] == [" t%d" % i for i in ordinary]             # every piece starts a word: all ids, in order
        assert all(s <= e for _, (s, e) in t["words"]) and t["words"][-1][1][1] == t["token_times"][-1]
    # language detection against the oracle's argmax over the language ids, where its margin is clear
    lang_ids = sorted(gen["lang_to_id"].values())
    with torch.no_grad():
        enc64 = wo.encoder(sd64, cfg, m.features(wavs).cpu().double())
        lg = wo.decoder_logits(sd64, cfg, enc64, torch.tensor([[gen["decoder_start_token_id"]]] * 3))[:, 0, lang_ids]
    top = lg.topk(2, dim=-1)
    by_id = {v: k for k, v in gen["lang_to_id"].items()}
    got = m.detect_language(state)
    assert len(got) == 3
    for b in range(3):
        if float(top.values[b, 0] - top.values[b, 1]) > 1e-3:
            assert got[b] == W.language_code(by_id[lang_ids[int(top.indices[b, 0])]])
    auto = m.generate(wavs, language="auto", max_new_tokens=6, return_timestamps=True)
    assert [r["language"] for r in auto] == got and [r["key"] for r in auto] == ["clip_0", "clip_1", "clip_2"]
    for b, r in enumerate(auto):                                                          # grouped by language: each clip as if decoded under its own
        alone = m.generate([wavs[b]], language=got[b], max_new_tokens=6, return_timestamps=True)[0]
        assert r["token_ids"] == alone["token_ids"] and r["token_times"] == alone["token_times"]
    m.close()


def test_target_diarization_whisper_v3_engine(gold, sd2):
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
    token_list = ["".join(enc[b] for b in b" ab")] * 50257            # every piece is the word " ab"
    kw = dict(cuda_device=0, sep_state_dict=sd2, spk_state_dict=recipe_eres2netv2_state_dict(0), asr_state_dict=recipe_paraformer_state_dict(0, 2),
              sd_pipeline=lambda a: sd_rows, od_pipeline=lambda a: od, whisper_state_dict=sd, whisper_config=cfg, whisper_token_list=token_list)
    td = TargetDiarization(asr_engine="whisper_v3", **kw)
    _, res, _ = td.infer(mix, tgt)
    td.asr_engine = "whisper_finetune"
    _, plain, _ = td.infer(mix, tgt)
    speakers = {r["speaker"] for r in plain}
    assert len(plain) == len(speakers)                                 # no timestamps: one item per speaker
    assert len(res) > len(speakers) and {r["speaker"] for r in res} == speakers      # word times: the diarization chunks keep their own texts
    words = 0
    for r in res:
        t = r["text"].replace(" ", "")
        assert t == "ab" * (len(t) // 2)
        words += len(t) // 2
    assert words >= len(res)                                           # the words landed in the chunks by their start times
