"""-m gpu: Paraformer at the benchmark's batch shape and on every dispatch path of csrc/paraformer.hip, against the fp64 oracle.

The path of a launch (split-K or direct Linears, small or GEMM attention, one-pass or generic softmax, split-K k|v projection) is a
function of its shape (test_paraformer_paths.pf_paths, thresholds parsed from the kernel source); the shape matrices put every
reachable path cell under the oracle, and the default benchmark's ASR stage (120 x 30 s segments as ONE launch sequence: B = 120,
T = 500, the 50-layer encoder and the 16-block decoder) is compared at full depth on a subset of utterances (utterances are
independent, so the subset is exact) plus all 120 against the same utterance encoded alone.  Bars: encoder rel-L2 < 1e-4 per
utterance and < 1e-3 for the worst single row; decoder token ids equal the fp64 argmax wherever its top-2 log-prob margin exceeds
1e-3 and >= 98 % overall, scores within 1e-3 where the ids agree (the rule of test_gpu_paraformer.py)."""
import numpy as np
import pytest
import torch

from test_paraformer_paths import BENCH_SHAPE, DEC_SHAPES, ENC_SHAPES, pf_paths

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")

SEG = 480000                      # 30 s at 16 kHz: HotPath.asr_segment
SUB = [0, 41, 78, 119]            # the utterances of the B = 120 launch compared with the fp64 oracle at full depth


def _sd64(sd):
    return {k: v.double() for k, v in sd.items()}


def enc_errors(out, ref):
    """per-utterance rel-L2 [B] and per-row rel-L2 [B,T] of a device encoder output against the fp64 reference"""
    d = out.detach().double().cpu() - ref
    return d.flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1), d.norm(dim=-1) / ref.norm(dim=-1)


def check_ids(ids, score, logits, counts, what):
    """device ids / scores [B,L] vs fp64 logits [B,L,V] on rows < counts[b]: ids equal where the fp64 top-2 margin > 1e-3, >= 98 %
    agreement over all compared rows, scores within 1e-3 where the ids agree.  Returns (agreement, max score error)."""
    lp = torch.log_softmax(logits, -1)
    agree_all, err = [], 0.0
    for b, n in enumerate(counts):
        if n == 0:
            continue
        top2 = lp[b, :n].topk(2, dim=-1)
        margin = (top2.values[:, 0] - top2.values[:, 1]).numpy()
        agree = ids[b, :n].numpy() == top2.indices[:, 0].numpy()
        assert agree[margin > 1e-3].all(), (what, b, np.where(~agree)[0][:5], margin[~agree][:5])
        if agree.any():
            err = max(err, float(np.abs(score[b, :n].numpy()[agree] - top2.values[:, 0].numpy()[agree]).max()))
        agree_all.append(agree)
    agreement = float(np.concatenate(agree_all).mean())
    assert agreement >= 0.98 and err < 1e-3, (what, agreement, err)
    return agreement, err


def check_decoded(r, ids_ref, peaks_ref, lp, off_ms=0.0):
    """one utterance of ParaformerDecoder.decode (timestamps shifted by off_ms) vs paraformer_decode: the checks of
    test_gpu_paraformer.test_nar_decoder_vs_oracle.  Returns (agreement, max score error)."""
    assert len(r["token_ids"]) == len(ids_ref) and len(ids_ref) > 0
    top2 = lp[: len(ids_ref)].topk(2, dim=-1).values
    margin = (top2[:, 0] - top2[:, 1]).numpy()
    agree = np.array(r["token_ids"]) == np.array(ids_ref)
    assert agree[margin > 1e-3].all(), (np.where(~agree)[0][:5], margin[~agree][:5])
    assert agree.mean() > 0.98
    sc = np.array(r["scores"])
    err = float(np.abs(sc[agree] - top2[:, 0].numpy()[agree]).max())
    assert err < 1e-3
    ts = [[a - off_ms, b - off_ms] for a, b in r["timestamp"]]
    assert len(ts) == len(ids_ref) and all(s <= e for s, e in ts) and all(ts[i][1] <= ts[i + 1][0] + 1e-9 for i in range(len(ts) - 1))
    assert [int(round((p + 1) * 60.0)) for p in peaks_ref] == [e for _, e in ts][: len(peaks_ref)]
    return float(agree.mean()), err


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def enc3():
    from targetdiarization_amd.paraformer import ParaformerEncoder
    from targetdiarization_amd.weights import recipe_paraformer_state_dict
    sd = recipe_paraformer_state_dict(0, 3)
    return ParaformerEncoder(sd, dev), _sd64(sd)


@pytest.fixture(scope="module")
def dec2():
    from targetdiarization_amd.paraformer import ParaformerDecoder
    from targetdiarization_amd.weights import recipe_paraformer_decoder_state_dict
    sd = recipe_paraformer_decoder_state_dict(0, 2)
    return ParaformerDecoder(sd, dev), _sd64(sd)


@pytest.fixture(scope="module")
def bench():
    """the benchmark's ASR stage input: 120 x 30 s of bench.synth_mixtures audio (= two 1800 s streams), the benchmark's weights
    (50-layer encoder, 16-block decoder, identity CMVN), device features and the ONE B = 120 encoder launch"""
    from test_gpu_configs import _synth
    from targetdiarization_amd.paraformer import ParaformerDecoder, ParaformerEncoder
    from targetdiarization_amd.weights import recipe_paraformer_decoder_state_dict, recipe_paraformer_state_dict
    enc_sd = recipe_paraformer_state_dict(0, 50)
    dec_sd = recipe_paraformer_decoder_state_dict(0, 16)
    asr_sd = dict(enc_sd); asr_sd.update(dec_sd)
    audio = _synth(BENCH_SHAPE[0] * SEG // 160000, 11).reshape(BENCH_SHAPE[0], SEG)
    enc = ParaformerEncoder(enc_sd, dev)
    feats = enc.features(torch.from_numpy(audio).to(dev))
    assert tuple(feats.shape) == (*BENCH_SHAPE, 560)
    y = enc.encode(feats)
    torch.cuda.synchronize()
    return {"audio": audio, "asr_sd": asr_sd, "enc_sd64": _sd64(enc_sd), "dec_sd64": _sd64(dec_sd), "enc": enc, "feats": feats, "y": y,
            "dec": ParaformerDecoder(asr_sd, dev)}


def _bench_decoded(bench):
    if "decoded" not in bench:
        bench["decoded"] = bench["dec"].decode(bench["y"])
    return bench["decoded"]


# ---- 2. encoder path matrix (3 layers) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", ENC_SHAPES)
def test_encoder_paths_vs_oracle(enc3, B, T):
    from oracle import paraformer_oracle as po
    enc, sd64 = enc3
    x = torch.randn(B, T, 560, generator=torch.Generator().manual_seed(1000 * B + T))
    out = enc.encode(x.to(dev))
    assert out.shape == (B, T, 512)
    utt, row = enc_errors(out, po.sanm_encoder_forward(x.double(), sd64))
    print(f"\nencoder 3 layers (B={B}, T={T}) {tuple(pf_paths('enc', B, T, T))}: worst utterance {float(utt.max()):.2e}, worst row {float(row.max()):.2e}")
    assert float(utt.max()) < 1e-4, (B, T, utt)
    assert float(row.max()) < 1e-3, (B, T, divmod(int(row.argmax()), T))


# ---- 3. encoder at the benchmark shape, 50 layers -------------------------------------------------------------------------------
def test_encoder_bench_shape_full_depth(bench):
    from oracle import paraformer_oracle as po
    B, T = BENCH_SHAPE
    assert tuple(pf_paths("enc", B, T, T)) == ("direct", "attn_gemm", "sp512", "n/a")
    assert tuple(pf_paths("enc", 1, T, T)) == ("splitk", "attn_small", "n/a", "n/a")
    y, feats, enc = bench["y"], bench["feats"], bench["enc"]
    assert y.shape == (B, T, 512) and bool(torch.isfinite(y).all())
    utt, row = enc_errors(y[SUB], po.sanm_encoder_forward(feats[SUB].double().cpu(), bench["enc_sd64"]))
    print(f"\nencoder 50 layers (B={B}, T={T}) utterances {SUB} vs fp64: per utterance {[f'{e:.2e}' for e in utt.tolist()]}, "
          f"worst row {float(row.max()):.2e}")
    assert float(utt.max()) < 1e-4, utt
    assert float(row.max()) < 1e-3, divmod(int(row.argmax()), T)
    # every utterance of the big launch against the same utterance alone (B = 1: split-K Linears, small attention)
    alone = []
    for b in range(B):
        yb = enc.encode(feats[b:b + 1])[0]
        alone.append(float(((yb - y[b]).norm() / y[b].norm()).item()))
    print(f"encoder 50 layers: utterance of the B={B} launch vs alone (B=1), worst rel-L2 {max(alone):.2e} (utterance {int(np.argmax(alone))})")
    assert max(alone) < 1e-4, [(b, e) for b, e in enumerate(alone) if e >= 1e-4][:8]


# ---- 4. decoder path matrix (2 blocks) through decode_embeds --------------------------------------------------------------------
def _counts(B, L):
    """ragged counts for B >= 2 (the matrix as a whole has 0, 1, L-1 and L); a single utterance is full"""
    pat = [L, L - 1, 1, 0, (2 * L) // 3, L // 2]
    return [pat[b % len(pat)] for b in range(B)] if B > 1 else [L]


def _dec_inputs(B, L, T, counts):
    g = torch.Generator().manual_seed(7 * B + 13 * L + T)
    enc = torch.randn(B, T, 512, generator=g)
    emb = torch.randn(B, L, 512, generator=g)
    for b, n in enumerate(counts):
        emb[b, n:] = 0.0
    return enc, emb


@pytest.mark.parametrize("B,L,T", DEC_SHAPES)
def test_decoder_paths_vs_oracle(dec2, B, L, T):
    from oracle import paraformer_oracle as po
    dec, sd64 = dec2
    counts = _counts(B, L)
    enc, emb = _dec_inputs(B, L, T, counts)
    ids, score = dec.decode_embeds(emb.to(dev), torch.tensor(counts, dtype=torch.int32, device=dev), enc.to(dev), L)
    logits = po.sanm_decoder_forward(emb.double(), counts, enc.double(), sd64, 2)
    agreement, err = check_ids(ids.cpu(), score.cpu(), logits, counts, (B, L, T))
    print(f"\ndecoder 2 blocks (B={B}, L={L}, T={T}) {tuple(pf_paths('dec', B, L, T))} counts {counts}: "
          f"agreement {agreement:.4f}, score error {err:.2e}")


@pytest.mark.parametrize("B,L,T", [(4, 300, 500), (4, 128, 600), (6, 200, 437), (2, 256, 500)])
def test_decoder_masking_invariance(dec2, B, L, T):
    """only the counts of utterances 1 and 3 (mod B) change: every other utterance's ids and scores are bit-identical"""
    dec, _ = dec2
    c1 = _counts(B, L)
    enc, emb = _dec_inputs(B, L, T, c1)
    c2 = list(c1)
    c2[1] = L // 3
    if B > 3:
        c2[3] = L
    e, m = enc.to(dev), emb.to(dev)
    i1, s1 = dec.decode_embeds(m, torch.tensor(c1, dtype=torch.int32, device=dev), e, L)
    i2, s2 = dec.decode_embeds(m, torch.tensor(c2, dtype=torch.int32, device=dev), e, L)
    same = [b for b in range(B) if c1[b] == c2[b]]
    assert same and torch.equal(i1[same], i2[same]) and torch.equal(s1[same], s2[same])
    changed = [b for b in range(B) if c1[b] != c2[b]]
    assert not torch.equal(s1[changed], s2[changed])          # the mask did reach the changed utterances


# ---- 5. CIF + decoder at the benchmark shape, 16 blocks -------------------------------------------------------------------------
def test_cif_decoder_bench_shape_full_depth(bench):
    from oracle import paraformer_oracle as po
    B, T = BENCH_SHAPE
    y, dec, sd64 = bench["y"], bench["dec"], bench["dec_sd64"]
    alphas, emb, counts, peaks = dec.predict(y)
    cnt = counts.cpu().tolist()
    L = max(cnt)
    paths = tuple(pf_paths("dec", B, L, T))
    print(f"\nCIF + decoder 16 blocks: B={B}, T={T}, L={L} (counts {min(cnt)}..{L}) {paths}")
    assert paths == ("direct", "attn_gemm", "rect", "direct")
    ys = y[SUB].double().cpu()
    _, a_ref = po.cif_alphas(ys, sd64)
    aerr = float((alphas[SUB].double().cpu() - a_ref).abs().max())
    assert aerr < 2e-5, aerr
    # integrate-and-fire on the device's alphas: exact decisions, as in test_cif_predictor_vs_oracle
    fired, fires = po.cif(torch.cat((y[SUB].cpu(), torch.zeros(len(SUB), 1, 512)), 1), alphas[SUB].cpu())
    for j, b in enumerate(SUB):
        n = fired[j].shape[0]
        assert peaks[b, :n].cpu().tolist() == torch.nonzero(fires[j] >= 1.0)[:, 0].tolist()
        assert n == T + 1 or int(peaks[b, n]) == -1
        assert cnt[b] == int(torch.floor(alphas[b].cpu().sum()))
        assert float((emb[b, :n].cpu() - fired[j]).norm() / fired[j].norm()) < 1e-5
    # the decoder alone on the device's embeddings and counts
    ids, score = dec.decode_embeds(emb, counts, y, L)
    logits = po.sanm_decoder_forward(emb[SUB, :L].double().cpu(), [cnt[b] for b in SUB], ys, sd64, 16)
    agreement, err = check_ids(ids[SUB].cpu(), score[SUB].cpu(), logits, [cnt[b] for b in SUB], "B=120 decode_embeds")
    print(f"decode_embeds at B={B} vs fp64 on {SUB}: alphas {aerr:.1e}, agreement {agreement:.4f}, score error {err:.2e}")
    # decode() of the whole batch: the same ids as decode_embeds everywhere, the oracle's chain on the subset
    res = _bench_decoded(bench)
    ids_h = ids.cpu().numpy()
    assert all(res[b]["token_ids"] == ids_h[b, :cnt[b]].tolist() for b in range(B))
    ref, logits2 = po.paraformer_decode(ys, sd64, 16)
    lp = torch.log_softmax(logits2, -1)
    worst = [check_decoded(res[b], ref[j][0], ref[j][1], lp[j]) for j, b in enumerate(SUB)]
    print(f"decode() at B={B} vs paraformer_decode: agreement >= {min(a for a, _ in worst):.4f}, score error {max(e for _, e in worst):.2e}")


# ---- 6. the H3 stage as the benchmark drives it ---------------------------------------------------------------------------------
class _Rec:
    """stands in for HotPath.asr / HotPath.dec: records the batch shape of every launch"""

    def __init__(self, inner, shapes):
        self.inner, self.shapes = inner, shapes

    def __call__(self, x):
        self.shapes.append(tuple(x.shape))
        return self.inner(x)

    def decode(self, y):
        self.shapes.append(("dec",) + tuple(y.shape[:2]))
        return self.inner.decode(y)


def test_h3_stage_as_the_benchmark_drives_it(sd2, bench):
    from oracle import frontend_oracle as fo
    from oracle import paraformer_oracle as po
    from targetdiarization_amd.pipeline import HotPath
    B, T = BENCH_SHAPE
    per = B // 2
    hp = HotPath(sd2, None, bench["asr_sd"], asr_rows_per_launch=65536)
    shapes = []
    hp.asr, hp.dec = _Rec(hp.asr, shapes), _Rec(hp.dec, shapes)
    audio = bench["audio"]
    streams = [torch.from_numpy(audio[:per].reshape(-1)).to(dev), torch.from_numpy(audio[per:].reshape(-1)).to(dev)]   # 2 x 1800 s
    enc, dres = hp.encode_device(streams, decode=True)
    assert shapes == [(B, SEG), ("dec", B, T)], shapes                          # 120 segments, ONE launch sequence
    assert [tuple(e.shape) for e in enc] == [(per * T, 512)] * 2 and [len(d) for d in dres] == [per, per]
    # the pipeline's launch is the direct B = 120 launch of the same audio: bit-identical encoder outputs and decoder results
    assert torch.equal(torch.cat(enc).view(B, T, 512), bench["y"])
    base = _bench_decoded(bench)
    for si in range(2):
        for k in range(per):
            r, b0 = dres[si][k], base[si * per + k]
            assert r["token_ids"] == b0["token_ids"] and r["scores"] == b0["scores"]
            assert r["timestamp"] == [[a + 30000.0 * k, e + 30000.0 * k] for a, e in b0["timestamp"]], (si, k)
    # one segment of each stream end to end against the oracle chain: fbank/LFR -> encoder (50) -> CIF + decoder (16)
    for si, k in ((0, 17), (1, per - 1)):
        wav = torch.from_numpy(audio[si * per + k]).double()
        feats = fo.asr_features(wav, torch.zeros(560, dtype=torch.float64), torch.ones(560, dtype=torch.float64))
        ref = po.sanm_encoder_forward(feats[None], bench["enc_sd64"])
        utt, row = enc_errors(enc[si][k * T:(k + 1) * T][None], ref)
        ids_ref, logits = po.paraformer_decode(ref, bench["dec_sd64"], 16)
        a, err = check_decoded(dres[si][k], ids_ref[0][0], ids_ref[0][1], torch.log_softmax(logits[0], -1), off_ms=30000.0 * k)
        print(f"\nH3 stream {si} segment {k} vs the oracle chain: encoder {float(utt[0]):.2e} (worst row {float(row.max()):.2e}), "
              f"{len(ids_ref[0][0])} tokens, agreement {a:.4f}, score error {err:.2e}")
        assert float(utt[0]) < 1e-4 and float(row.max()) < 1e-3

    # ragged tails: 3.3 s (its own launch) and 250 samples (< 400: dropped); the 30 s segments keep their bucket and launch
    tail = torch.from_numpy(_tail_audio(52800)).to(dev)
    streams2 = [torch.cat((streams[0], tail)), torch.cat((streams[1], tail[:250]))]
    shapes.clear()
    enc2, dres2 = hp.encode_device(streams2, decode=True)
    assert shapes == [(B, SEG), ("dec", B, T), (1, 52800), ("dec", 1, 55)], shapes
    assert [len(d) for d in dres2] == [per + 1, per] and [e.shape[0] for e in enc2] == [per * T + 55, per * T]
    assert torch.equal(enc2[0][: per * T], enc[0]) and torch.equal(enc2[1], enc[1])
    assert dres2[0][:per] == dres[0] and dres2[1] == dres[1]
    t_alone = bench["enc"](tail[None])
    assert torch.equal(enc2[0][per * T:], t_alone[0])
    t_dec = bench["dec"].decode(t_alone)[0]
    assert dres2[0][per]["token_ids"] == t_dec["token_ids"]
    assert dres2[0][per]["timestamp"] == [[a + 30000.0 * per, e + 30000.0 * per] for a, e in t_dec["timestamp"]]

    # the HotPath default (32768 rows per launch: chunks of 65 + 55 segments) against the benchmark's single launch
    hp.asr_rows_per_launch = 32768
    shapes.clear()
    enc3, dres3 = hp.encode_device(streams, decode=True)
    assert shapes == [(65, SEG), ("dec", 65, T), (55, SEG), ("dec", 55, T)], shapes
    worst = 0.0
    for si in range(2):
        assert [r["token_ids"] for r in dres3[si]] == [r["token_ids"] for r in dres[si]]
        a, b = enc3[si].view(per, T, 512).double(), enc[si].view(per, T, 512).double()
        worst = max(worst, float(((a - b).flatten(1).norm(dim=1) / b.flatten(1).norm(dim=1)).max()))
    print(f"H3 asr_rows_per_launch 32768 (65 + 55) vs 65536 (120): token ids equal, encoder worst segment rel-L2 {worst:.1e}")
    assert worst < 1e-5


def _tail_audio(n):
    from test_gpu_configs import _synth
    return _synth(1, 12)[0, :n]
