"""-m gpu: SenseVoiceSmall on the device (tdx_sv_*, csrc/sensevoice.hip) against tests/sensevoice_oracle.py in fp64, under both
head paths (TDX_SV_HEAD=1 the fused kernel, 0 row chunks through the x3 Linear).  Third-party architecture restated from upstream:
parity with the published checkpoint is unpinned; the weights are random and seeded (tests/sensevoice_cases.py).

Bars: encoder rel-L2 < 1e-4 (the bar of test_gpu_paraformer.py for this layer); frame ids equal the oracle's wherever its top-2
log-prob margin exceeds 1e-3 and scores within 1e-3 at agreeing frames (test_gpu_paraformer.py:96-102); at most 1 % of a case's
frames may fall under the margin rule; planted maxima and the collapse are exact."""
import ctypes as C
import os
import wave as wavmod

import numpy as np
import pytest
import torch

import sensevoice_cases as sc
import sensevoice_oracle as orc

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
HEADS = [1, 0]
_models, _runs = {}, {}


def _make(sd, head, **kw):
    """a model whose handle took `head` from TDX_SV_HEAD at create (a property of the handle)"""
    from targetdiarization_amd.sensevoice import SenseVoiceSmall
    old = os.environ.get("TDX_SV_HEAD")
    os.environ["TDX_SV_HEAD"] = str(head)
    try:
        return SenseVoiceSmall(sd, dev, **kw)
    finally:
        if old is None:
            del os.environ["TDX_SV_HEAD"]
        else:
            os.environ["TDX_SV_HEAD"] = old


def model(depth, head):
    if (depth, head) not in _models:
        _models[depth, head] = _make(sc.state_dict(depth), head)
    return _models[depth, head]


def run(depth, head, B, T):
    """one forward per case and head, shared by the tests: host copies of every output"""
    key = (depth, head, B, T)
    if key not in _runs:
        r = model(depth, head).forward(sc.feats(B, T).to(dev), with_enc=True)
        _runs[key] = {k: v.cpu() for k, v in r.items()}
    return _runs[key]


def rel_l2(a, b):
    a = a.double().reshape(-1); b = b.double().reshape(-1)
    return float((a - b).norm() / b.norm())


CASES = [(d, h, B, T) for d in sc.DEPTHS for h in HEADS for (B, T) in sc.SHAPES] + [("small", h) + sc.LONG_SHAPE for h in HEADS]


@pytest.mark.parametrize("depth,head,B,T", CASES)
def test_encoder_tap_vs_oracle(depth, head, B, T):
    ref = sc.reference(depth, B, T)["enc"]
    out = run(depth, head, B, T)["enc"]
    assert out.shape == (B, T + 4, 512)
    e_all, e_prompt, e_feat = rel_l2(out, ref), rel_l2(out[:, :4], ref[:, :4]), rel_l2(out[:, 4:], ref[:, 4:])
    print(f"enc rel-L2 {depth} head={head} {B}x{T}: all {e_all:.3g} prompt rows {e_prompt:.3g} feature rows {e_feat:.3g}")
    assert e_all < 1e-4 and e_feat < 1e-4
    assert e_prompt < 1e-4                                     # on their own: a position or scale error there cannot hide in the average
    for s in range(4):
        assert rel_l2(out[:, s], ref[:, s]) < 1e-4, s


@pytest.mark.parametrize("depth,head,B,T", CASES)
def test_head_frame_ids_scores_and_tokens(depth, head, B, T):
    ref, out = sc.reference(depth, B, T), run(depth, head, B, T)
    thin = ref["margin"] <= sc.MARGIN
    n = thin.numel()
    assert int(thin.sum()) <= n // 100, "the oracle alone must keep the margin rule's exclusions within 1 % of the frames"
    ids = out["frame_ids"].long()
    agree = ids == ref["ids"]
    err = (out["frame_scores"].double() - ref["top"])[agree].abs().max()
    print(f"head {depth} head={head} {B}x{T}: {int((~agree).sum())} of {n} ids differ, {int(thin.sum())} under the margin rule, score err {float(err):.3g}")
    assert bool(agree[~thin].all()), (torch.nonzero(~agree & ~thin)[:5].tolist())
    assert float(err) < 1e-3
    # the token outputs are the collapse of the device's own frame ids, and of the oracle's when no frame was excluded
    for b in range(B):
        cnt = int(out["counts"][b])
        tok, frm = orc.collapse(ids[b].tolist())
        assert out["token_ids"][b, :cnt].tolist() == tok and out["token_frames"][b, :cnt].tolist() == frm
        assert bool((out["token_ids"][b, cnt:] == 0).all()) and bool((out["token_frames"][b, cnt:] == -1).all())
        if not bool(thin.any()):
            assert (tok, frm) == ref["tokens"][b]


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("case", ["last_real_column", "first_column_of_a_slice", "runner_up_to_an_equal_lower_id"])
def test_head_planted_logits(head, case):
    """every row of ctc_lo but the last is the SAME vector, so that the GEMM adds one value c(frame) to every column and the bias
    alone orders them: the planted maximum must come back exactly.  Columns 1031..1535 of the last slice are padding: the fused kernel
    reads the LAST real row of the weight there, without a bias.  Where the maximum is planted elsewhere that row is poisoned: tp_norm
    is set so that channel 0 of every LN'd row is exactly 1, the last row gets + 50 in that channel and its bias - 50 — the real column
    1030 stays an ordinary one, a padding column that entered the maximum or the sum would carry c + 50 and win.  (The padded rows of the
    x3 Linear's weight are the loader's zeros: that layout cannot be poisoned from outside; there the score carries the check.)"""
    V = sc.VOCAB
    sd = dict(sc.state_dict((1, 0)))
    g = torch.Generator().manual_seed(3)
    sd["ctc.ctc_lo.weight"] = (torch.randn(512, generator=g) * 0.05)[None].repeat(V, 1).contiguous()
    bias = torch.zeros(V)
    want = {"last_real_column": V - 1, "first_column_of_a_slice": 512, "runner_up_to_an_equal_lower_id": 100}[case]
    bias[want] = 4.0
    if case == "runner_up_to_an_equal_lower_id":
        bias[700] = 4.0
    if want != V - 1:
        sd["encoder.tp_norm.weight"] = sd["encoder.tp_norm.weight"].clone(); sd["encoder.tp_norm.bias"] = sd["encoder.tp_norm.bias"].clone()
        sd["encoder.tp_norm.weight"][0], sd["encoder.tp_norm.bias"][0] = 0.0, 1.0
        sd["ctc.ctc_lo.weight"][V - 1, 0] += 50.0
        bias[V - 1] = -50.0
    sd["ctc.ctc_lo.bias"] = bias
    m = _make(sd, head, num_blocks=1, tp_blocks=0)
    r = m.forward(sc.feats(2, 37).to(dev))
    ids, score = r["frame_ids"].cpu(), r["frame_scores"].cpu().double()
    m.close()
    assert bool((ids == want).all()), ids.unique().tolist()
    nmax = 2 if case == "runner_up_to_an_equal_lower_id" else 1
    expect = 4.0 - np.log(nmax * np.exp(4.0) + (V - nmax))
    assert float((score - expect).abs().max()) < 1e-3


def _collapse_dev(ids, blank=0):
    from targetdiarization_amd import _lib
    l = _lib.lib()
    ids = torch.as_tensor(ids, dtype=torch.int32)
    B, S = ids.shape
    d = ids.to(dev).contiguous()
    tok = torch.full((B, S), -7, dtype=torch.int32, device=dev); frm = torch.full((B, S), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((B,), -7, dtype=torch.int32, device=dev)
    _lib.check(l.tdx_ctc_collapse(d.data_ptr(), B, S, blank, tok.data_ptr(), frm.data_ptr(), cnt.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return tok.cpu(), frm.cpu(), cnt.cpu()


def _collapse_ref(ids, blank=0):
    """the five-line restatement: per utterance, keep a frame whose id is not blank and differs from the previous frame's"""
    B, S = len(ids), len(ids[0])
    tok, frm, cnt = np.full((B, S), blank, np.int32), np.full((B, S), -1, np.int32), np.zeros(B, np.int32)
    for b, row in enumerate(ids):
        keep = [i for i, t in enumerate(row) if t != blank and (i == 0 or row[i - 1] != t)]
        tok[b, :len(keep)] = [row[i] for i in keep]; frm[b, :len(keep)] = keep; cnt[b] = len(keep)
    return tok, frm, cnt


def _rand_ids(B, S, seed):
    return torch.randint(0, 4, (B, S), generator=torch.Generator().manual_seed(seed)).tolist()


@pytest.mark.parametrize("name,ids", [
    ("all_blank", [[0] * 9]),
    ("no_blank", [[3, 3, 5, 5, 5, 2, 3]]),
    ("a_a_blank_a", [[7, 7, 0, 7]]),
    ("run_across_an_utterance_boundary", [[0, 4, 6, 6], [6, 6, 0, 1]]),
    ("S_1", [[5], [0], [5]]),
    ("1x5", _rand_ids(1, 5, 1)),
    ("3x149", _rand_ids(3, 149, 2)),
    ("2x600_three_scan_rounds", _rand_ids(2, 600, 3)),
])
def test_ctc_collapse_bit_exact(name, ids):
    tok, frm, cnt = _collapse_dev(ids)
    rt, rf, rc = _collapse_ref(ids)
    assert cnt.tolist() == rc.tolist()
    assert np.array_equal(tok.numpy(), rt) and np.array_equal(frm.numpy(), rf)
    if name == "a_a_blank_a":
        assert tok[0, :2].tolist() == [7, 7] and frm[0, :2].tolist() == [0, 3]
    if name == "run_across_an_utterance_boundary":
        assert tok[1, :2].tolist() == [6, 1] and cnt.tolist() == [2, 2]


@pytest.mark.parametrize("head", HEADS)
def test_workspace_grows_by_less_than_the_logits(head):
    """V = 25055: 32 more 30 s segments must cost less than their fp32 logits would"""
    sd = dict(sc.state_dict((2, 0)))
    g = torch.Generator().manual_seed(11)
    sd["ctc.ctc_lo.weight"] = torch.randn(25055, 512, generator=g) * 0.04
    sd["ctc.ctc_lo.bias"] = torch.zeros(25055)
    m = _make(sd, head, num_blocks=2, tp_blocks=0)
    w64, w32 = m.workspace_bytes(64, 500), m.workspace_bytes(32, 500)
    m.close()
    assert w32 > 0 and 0 < w64 - w32 < 32 * 504 * 4 * 25055


# ---- host ---------------------------------------------------------------------------------------------------------
TAGS = ["<|zh|>", "<|HAPPY|>", "<|Speech|>", "<|withitn|>"]


def _wave(gold, fn):
    with wavmod.open(os.path.join(gold, fn), "rb") as w:
        return np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16).astype(np.float32) / 32768.0


def test_asr_processor_sensevoice_engine(gold):
    """asr_detection(asr_engine="sensevoice") (ASRProcessor.py:398-421, :515-524) on two clips of different lengths.  Fails on the
    parent commit: the engine name was ignored there."""
    from targetdiarization_amd.asr_processor import ASRProcessor
    sd = sc.state_dict("small")
    toks = TAGS + [f"▁w{i}," if i % 5 == 0 else f"▁W{i}" for i in range(4, sc.VOCAB)]
    asr = ASRProcessor(is_asr=True, cuda_device=0, verbose_log=False, sensevoice_state_dict=sd, sensevoice_token_list=toks)
    assert list(asr.asr) == ["sensevoice"]
    tgt = _wave(gold, "female_a.wav")
    clips = [tgt[:16000], tgt[:26000]]
    raw = asr.asr_detection(clips, asr_engine="sensevoice", output_raw_result=True)
    assert [set(r) for r in raw] == [{"key", "text", "token_ids", "frames", "scores"}] * 2 and [r["key"] for r in raw] == ["clip_0", "clip_1"]
    sv = asr.asr["sensevoice"]
    for r, c in zip(raw, clips):
        S = ((1 + (len(c) - 400) // 160) + 5) // 6 + 4
        assert len(r["token_ids"]) >= 6 and len(r["token_ids"]) == len(r["frames"]) == len(r["scores"])
        assert r["frames"] == sorted(r["frames"]) and 0 <= r["frames"][0] and r["frames"][-1] < S and all(s <= 0.0 for s in r["scores"])
        assert r["text"] == sv.text_of(r["token_ids"])
        one = sv.generate([c])[0]                               # a batch of one gives the clip's own result
        assert one["token_ids"] == r["token_ids"]
    # random weights decode random pieces: such a text does not carry the four tags -> the fallback result
    res = asr.asr_detection(clips, asr_engine="sensevoice")
    assert [set(r) for r in res] == [{"key", "language", "text", "emotion"}] * 2
    for r, w in zip(res, raw):
        if not w["text"].startswith("".join(TAGS)):
            assert (r["language"], r["emotion"], r["text"]) == ("", "", w["text"])
    # a table whose pieces for the first clip's first four ids are tag tokens (other ids keep word pieces); an id that comes twice
    # among the four keeps the tag of its first place, which still reads as four tags
    first4 = raw[0]["token_ids"][:4]
    assert first4[0] != first4[1]
    table = [f"▁w{i}," if i % 5 == 0 else f"▁W{i}" for i in range(sc.VOCAB)]
    for t, i in reversed(list(zip(TAGS, first4))):
        table[i] = t
    sv.token_list = table
    r0 = asr.asr_detection(clips[0], asr_engine="sensevoice")[0]
    assert r0["key"] == "clip_0" and r0["language"] == "zh" and r0["emotion"] == "happy"
    # the four leading tags are gone (a lone tag piece further on stays, as in the reference: only groups of four are deleted); zh: no spaces
    assert r0["text"] == "".join(table[i] for i in raw[0]["token_ids"][4:]).replace("▁", "") and " " not in r0["text"] and "," in r0["text"]
    n0 = asr.asr_detection(clips[0], asr_engine="sensevoice", no_punc=True)[0]
    import re
    assert "," not in n0["text"] and n0["text"] == re.sub(r"[^\w\s]", "", r0["text"]).lower() and n0["language"] == "zh"
    both = asr.asr_detection(clips, asr_engine="sensevoice")
    text = asr.asr_detection(clips, asr_engine="sensevoice", output_text_only=True)
    assert text == "".join(r["text"] + (" " if r["text"][-1] in ",.?!" else "") for r in both if r["text"])
    assert asr.asr_detection(clips[0], asr_engine="whisper_v9")[0]["text"] == r0["text"]       # unknown engine: the first loaded one
    sv.close()
    from targetdiarization_amd._lib import TdxError
    with pytest.raises(TdxError):
        sv.generate([clips[0]])


def test_target_diarization_sensevoice_engine(gold, sd2):
    from targetdiarization_amd.target_diarization import TargetDiarization
    from targetdiarization_amd.weights import recipe_eres2netv2_state_dict, recipe_paraformer_state_dict
    mix, tgt = _wave(gold, "chat_mix.wav"), _wave(gold, "female_a.wav")
    sd_rows = {"text": [[0.0, 3.0, 0], [2.4, 5.5, 1], [5.5, 8.6, 0]]}
    od = [(0.0, 3.0, "SPEAKER_00"), (2.4, 5.5, "SPEAKER_01"), (5.5, 8.6, "SPEAKER_00")]
    # every piece is a tag token: whatever the random weights decode, a text of five or more pieces parses to language "en"
    td = TargetDiarization(cuda_device=0, sep_state_dict=sd2, spk_state_dict=recipe_eres2netv2_state_dict(0),
                           asr_state_dict=recipe_paraformer_state_dict(0, 2), sd_pipeline=lambda a: sd_rows, od_pipeline=lambda a: od,
                           asr_engine="sensevoice", sensevoice_state_dict=sc.state_dict("small"), sensevoice_token_list=["<|en|>"] * sc.VOCAB)
    assert td.hp.sv is not None
    spk, res, aud = td.infer(mix, tgt)
    assert spk in ("0", "1") and res and aud is not None
    singles = [r for r in res if r["type"] == "single"]
    assert singles and len(singles) == len(res) == len({r["speaker"] for r in res})     # the no-timestamp branch: one item per speaker
    assert all(set(r) >= {"speaker", "timerange", "text", "type", "score", "language"} for r in singles)
    assert all(r["language"] == "en" for r in singles)
    # the default engine on the same model object's inputs is untouched by the SenseVoice weights
    td.asr_engine = "paraformer"
    _, res_pf, _ = td.infer(mix, tgt)
    assert all("language" not in r for r in res_pf)
