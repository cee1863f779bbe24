"""-m gpu: Paraformer's upsampling timestamp predictor (csrc/pf_timestamps.hip behind ParaformerDecoder.upsampled / decode) against
tests/pf_timestamps_oracle.py in fp64 (third-party architecture, recipe weights: parity with funasr unpinned).  Continuous outputs
at the project's bar, rel-L2 < 1e-4; the peak scan bit for bit against the host scan of the device's own alphas."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pf_timestamps_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
BLOCKS, VOCAB = 2, 512
E2E_CASES = [(3, 50, 21), (2, 120, 22)]          # (B, T, seed)


def rel_l2(a, b):
    a = a.detach().double().cpu().reshape(-1); b = torch.as_tensor(b).double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def make_enc(B, T, seed=0):
    return torch.randn(B, T, 512, generator=torch.Generator().manual_seed(seed + 1000 * B + T))


@pytest.fixture(scope="module")
def sd():
    from targetdiarization_amd import weights as W
    out = dict(W.recipe_paraformer_decoder_state_dict(0, BLOCKS, vocab=VOCAB))
    out.update(W.recipe_paraformer_timestamp_state_dict(0))
    return out


@pytest.fixture(scope="module")
def sd64(sd):
    return orc.cast(sd, torch.float64)


@pytest.fixture(scope="module")
def dec(sd):
    from targetdiarization_amd.paraformer import ParaformerDecoder
    d = ParaformerDecoder(sd, device="cuda:0")
    yield d
    d.close()


@pytest.fixture(scope="module")
def dec_plain(sd):
    from targetdiarization_amd.paraformer import ParaformerDecoder
    d = ParaformerDecoder({k: v for k, v in sd.items() if not k.startswith(("predictor.upsample_cnn", "predictor.blstm", "predictor.cif_output2"))}, device="cuda:0")
    yield d
    d.close()


# B in {1, 3, 5}: the recurrence works on tiles of 4 clips (one partial tile, one full + a remainder); T = 1: a 3-step sequence
@pytest.mark.parametrize("B,T", [(b, t) for t in (1, 2, 7, 50) for b in (1, 3, 5)] + [(2, 167)])
def test_head_vs_fp64_oracle(dec, sd64, B, T):
    """BLSTM output, alphas before and after the re-normalisation against the fp64 oracle; (2, 167): 501 steps, drift over a long
    recurrence.  The counts are an input of the head: any positive numbers do."""
    from targetdiarization_amd.pf_timestamps import cif_wo_hidden
    enc = make_enc(B, T)
    counts = torch.arange(B, dtype=torch.int32) + T // 4 + 1
    alphas, peaks, tap, raw = dec.upsampled(enc.cuda(), counts.cuda(), tap=True, raw=True)
    assert alphas.shape == (B, 3 * T) and peaks.shape == (B, 3 * T) and tap.shape == (B, 3 * T, 1024)
    ref = orc.upsampled_head(enc.double(), counts, sd64)
    errs = {k: rel_l2(v, ref[k]) for k, v in (("tap", tap), ("raw", raw), ("alphas", alphas))}
    print(f"B={B} T={T} rel-L2 {errs}")
    assert all(e < 1e-4 for e in errs.values()), errs
    # without the tap the BLSTM output goes through the workspace: the same numbers
    a2, p2 = dec.upsampled(enc.cuda(), counts.cuda())
    assert torch.equal(bits(a2), bits(alphas)) and torch.equal(bits(p2), bits(peaks))
    # the discrete part: the device scan IS the host's fp32 loop on the device's alphas
    a_h, p_h = alphas.cpu().numpy(), peaks.cpu().numpy()
    for b in range(B):
        assert np.array_equal(cif_wo_hidden(a_h[b]).view(np.uint32), p_h[b].view(np.uint32)), b


def test_directions_do_not_leak(dec):
    """the reverse direction at step u sees steps >= u only, the forward direction steps <= u: altering the first (second) half of a
    clip leaves the reverse (forward) columns of the other half bit-equal"""
    T, cut = 8, 4
    enc = make_enc(1, T, seed=5)
    counts = torch.tensor([3], dtype=torch.int32).cuda()
    base = dec.upsampled(enc.cuda(), counts, tap=True)[2]
    e1 = enc.clone(); e1[:, :cut] += 1.0
    e2 = enc.clone(); e2[:, cut:] += 1.0
    t1 = dec.upsampled(e1.cuda(), counts, tap=True)[2]
    t2 = dec.upsampled(e2.cuda(), counts, tap=True)[2]
    assert torch.equal(bits(t1[:, 3 * cut:, 512:]), bits(base[:, 3 * cut:, 512:]))
    assert torch.equal(bits(t2[:, :3 * cut, :512]), bits(base[:, :3 * cut, :512]))
    assert not torch.equal(bits(t1[:, 3 * cut:, :512]), bits(base[:, 3 * cut:, :512]))       # the forward half does depend on it
    assert not torch.equal(bits(t2[:, :3 * cut, 512:]), bits(base[:, :3 * cut, 512:]))


def test_batch_independence(dec):
    B, T = 5, 50
    enc = make_enc(B, T, seed=3).cuda()
    counts = (torch.arange(B, dtype=torch.int32) + 9).cuda()
    tap = dec.upsampled(enc, counts, tap=True)[2]
    for k in range(B):
        lone = dec.upsampled(enc[k:k + 1], counts[k:k + 1], tap=True)[2]
        assert rel_l2(tap[k], lone[0]) < 1e-5, k


def test_zero_sum_clip_is_left_unscaled(sd):
    """smooth_factor2 = 0 makes every alpha relu(-0.01) = 0: counts / 0 must not reach the output"""
    from targetdiarization_amd.paraformer import ParaformerDecoder
    d = ParaformerDecoder(sd, device="cuda:0", smooth_factor2=0.0)
    a, p = d.upsampled(make_enc(2, 7).cuda(), torch.tensor([2, 3], dtype=torch.int32).cuda())
    assert float(a.abs().max()) == 0.0 and float(p.abs().max()) == 0.0
    d.close()


@pytest.mark.parametrize("B,T,seed", E2E_CASES)
def test_decode_timestamps_vs_fp64_oracle(dec, sd64, B, T, seed):
    """decode() with the head against the fp64 oracle: the same token count, every boundary within one upsampled frame (20 ms), at
    most 5 % of the boundaries different at all.  The seeds are such that the oracle in fp32 against itself in fp64 stays inside
    these bounds on the CPU (checked when the test was written: 0 of 70 and 0 of 114 boundaries differ)."""
    enc = make_enc(B, T, seed)
    res = dec.decode(enc.cuda())
    ref, _, _ = orc.decode_timestamps(enc.double(), sd64, BLOCKS)
    nb = nd = 0
    for b in range(B):
        n, ts = ref[b]
        assert n > 0 and len(res[b]["token_ids"]) == n and len(res[b]["timestamp"]) == n, (b, n, len(res[b]["timestamp"]))
        d = np.abs(np.array(res[b]["timestamp"]) - np.array(ts))
        assert d.max() <= 20, (b, d.max())
        nb += d.size; nd += int((d > 0).sum())
    print(f"B={B} T={T}: {nd} of {nb} boundaries differ")
    assert nd <= 0.05 * nb, (nd, nb)


def test_decoder_without_the_head_is_unchanged(dec_plain):
    """no head: has_timestamps False, decode() gives the 60 ms definition (recomputed here from predict()'s peaks), and the C entry
    point answers with an error code"""
    from targetdiarization_amd import _lib
    assert dec_plain.has_timestamps is False and dec_plain.cif_residual is True
    enc = make_enc(2, 50, seed=4).cuda()
    res = dec_plain.decode(enc)
    _, _, counts, peaks = dec_plain.predict(enc)
    for b in range(2):
        n, prev, ts = int(counts[b]), -1, []
        for k in range(n):
            pk = int(peaks[b, k])
            pk = prev if pk < 0 else pk
            ts.append([int(round((prev + 1) * 60.0)), int(round((pk + 1) * 60.0))])
            prev = pk
        assert n > 0 and res[b]["timestamp"] == ts and len(res[b]["token_ids"]) == n
    l = _lib.lib()
    assert l.tdx_pfdec_timestamps_workspace_bytes(dec_plain._h, 2, 50) == 0
    out = torch.empty(2, 150, device="cuda:0"); ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
    rc = l.tdx_pfdec_timestamps(dec_plain._h, enc.data_ptr(), 2, 50, counts.data_ptr(), out.data_ptr(), out.data_ptr(), None, ws.data_ptr(), ws.numel(), None)
    assert rc != 0 and b"no timestamp head" in l.tdx_last_error()
    with pytest.raises(_lib.TdxError):
        dec_plain.upsampled(enc, counts)


@pytest.mark.parametrize("missing", ["predictor.upsample_cnn.bias", "predictor.blstm.weight_hh_l0_reverse", "predictor.cif_output2.weight"])
def test_partial_head_fails_at_create(sd, missing):
    from targetdiarization_amd import _lib
    from targetdiarization_amd.weights import pack_blob
    blob = pack_blob({k: v for k, v in sd.items() if k != missing})
    h = C.c_void_p()
    l = _lib.lib()
    rc = l.tdx_pfdec_create(BLOCKS, VOCAB, (C.c_char * len(blob)).from_buffer_copy(blob), len(blob), 0, C.byref(h))
    assert rc == 2 and missing.encode() in l.tdx_last_error()


def test_cif_residual_switch(sd, sd64, dec, dec_plain):
    """with the head the main branch is CifPredictorV3's relu(conv + bias), without it V2's relu(conv + bias + x); an explicit value wins"""
    from targetdiarization_amd.paraformer import ParaformerDecoder
    assert dec.has_timestamps is True and dec.cif_residual is False
    enc = make_enc(2, 50, seed=6)
    for d, residual in ((dec, False), (dec_plain, True)):
        a = d.predict(enc.cuda())[0]
        assert float((a.double().cpu() - orc.cif_alphas(enc.double(), sd64, residual)).abs().max()) < 2e-5
    forced = ParaformerDecoder(sd, device="cuda:0", cif_residual=True)
    assert forced.has_timestamps and forced.cif_residual is True
    assert torch.equal(bits(forced.predict(enc.cuda())[0]), bits(dec_plain.predict(enc.cuda())[0]))
    forced.close()


def test_asr_detection_with_the_head():
    """ASRProcessor.asr_detection end to end with the head's weights: one timestamp per token, in seconds, non-decreasing, inside the clip"""
    from targetdiarization_amd import weights as W
    from targetdiarization_amd.asr_processor import ASRProcessor
    sd = dict(W.recipe_paraformer_state_dict(0, 2)); sd.update(W.recipe_paraformer_decoder_state_dict(0, 2)); sd.update(W.recipe_paraformer_timestamp_state_dict(0))
    asr = ASRProcessor(is_asr=True, asr_state_dict=sd, cuda_device=0, verbose_log=False, token_list=[f"t{i}" for i in range(8404)])
    assert asr.nar_decoder.has_timestamps
    wav = W.recipe_wave("asr", 1, 48000)[0]
    r = asr.asr_detection(wav, asr_engine="paraformer")[0]
    toks = r["text"].split(" ")
    assert len(toks) > 3 and len(r["timestamp"]) == len(toks) and [t for t, _ in r["timestamp"]] == toks
    flat = [x for _, (s, e) in r["timestamp"] for x in (s, e)]
    assert all(a <= b for a, b in zip(flat, flat[1:])) and 0.0 <= flat[0] and flat[-1] <= 3.0
