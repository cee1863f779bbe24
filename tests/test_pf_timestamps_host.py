"""CPU tests of Paraformer's upsampling timestamps: the host rules (targetdiarization_amd/pf_timestamps.py) on hand-made peaks —
the expected values are worked out by hand from the rules (a fire at frame f counts as f - 1.5; one frame = 20 ms; times are
int(seconds * 1000)) —, the host scan against the oracle's, and the recipe weights of the head."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pf_timestamps_oracle as orc  # noqa: E402
from targetdiarization_amd.pf_timestamps import cif_wo_hidden, ts_prediction_lfr6  # noqa: E402


def peaks_at(U, fires):
    p = np.full(U, 0.5, np.float32)
    p[list(fires)] = 1.0
    return p


FLAT = lambda U, v=0.1: np.full(U, v, np.float32)  # noqa: E731


def test_exact_fire_count_and_far_tail():
    # fires 4, 14, 24 -> 2.5, 12.5, 22.5; no leading <sil> (2.5 <= 5); tail 40 - 22.5 > 5: b ends at (40 + 22.5) / 2 = 31.25
    text, ts = ts_prediction_lfr6(FLAT(40), peaks_at(40, [4, 14, 24]), ["a", "b"])
    assert ts == [[50, 250], [250, 625]]
    assert text == "a 0.050 0.250;b 0.250 0.625;<sil> 0.625 0.800;"
    # a trailing </s> has no timestamp; the VAD offset is added in ms
    assert ts_prediction_lfr6(FLAT(40), peaks_at(40, [4, 14, 24]), ["a", "b", "</s>"], vad_offset_ms=1000)[1] == [[1050, 1250], [1250, 1625]]


def test_leading_silence_both_sides_of_the_threshold():
    t_no, ts_no = ts_prediction_lfr6(FLAT(40), peaks_at(40, [6, 14, 24]), ["a", "b"])      # 4.5 <= 5
    t_yes, ts_yes = ts_prediction_lfr6(FLAT(40), peaks_at(40, [7, 14, 24]), ["a", "b"])    # 5.5 > 5
    assert ts_no == [[90, 250], [250, 625]] and t_no.startswith("a 0.090")
    assert ts_yes == [[110, 250], [250, 625]] and t_yes.startswith("<sil> 0.000 0.110;a 0.110")


def test_token_cap_13_frames_split_12_not():
    # 13 frames (2.5 -> 15.5): a = [2.5, 14.5] + <sil> [14.5, 15.5]; b starts at 15.5, ends at (40 + 25.5) / 2 = 32.75
    text, ts = ts_prediction_lfr6(FLAT(40), peaks_at(40, [4, 17, 27]), ["a", "b"])
    assert ts == [[50, 290], [310, 655]] and "a 0.050 0.290;<sil> 0.290 0.310;b" in text
    # 12 frames (2.5 -> 14.5): not split; b = [14.5, (40 + 24.5) / 2 = 32.25]
    text, ts = ts_prediction_lfr6(FLAT(40), peaks_at(40, [4, 16, 26]), ["a", "b"])
    assert ts == [[50, 290], [290, 645]] and text.count("<sil>") == 1


def test_both_tail_rules():
    # last fire 25.5: 30 - 25.5 = 4.5 <= 5 -> the last token runs to the end of the clip, no closing <sil>
    text, ts = ts_prediction_lfr6(FLAT(30), peaks_at(30, [4, 16, 27]), ["a", "b"])
    assert ts == [[50, 290], [290, 600]] and "<sil>" not in text
    # last fire 24.5: 5.5 > 5 -> midpoint (30 + 24.5) / 2 = 27.25 and a closing <sil>
    text, ts = ts_prediction_lfr6(FLAT(30), peaks_at(30, [4, 16, 26]), ["a", "b"])
    assert ts == [[50, 290], [290, 545]] and text.endswith("<sil> 0.545 0.600;")


def test_renormalising_branch_too_few_fires():
    # 3 characters need 4 fires, the peaks hold 1: alphas (30 x 0.05) are rescaled to sum 4 = 30 x 0.13333 and scanned with
    # threshold 0.9999: 8 frames -> 1.0667 fires at frame 7 (rest 0.0668), 7 more -> 1.0001 at 14 (0.0002), 8 more -> 1.0669 at 22
    # (0.0670), 7 more -> 1.0003 at 29: fires 5.5, 12.5, 20.5, 27.5; leading <sil>; tail 2.5 <= 5: c runs to frame 30
    text, ts = ts_prediction_lfr6(FLAT(30, 0.05), peaks_at(30, [10]), ["a", "b", "c"])
    assert ts == [[110, 250], [250, 410], [410, 600]] and text.startswith("<sil> 0.000 0.110;")


def test_renormalising_branch_too_many_fires():
    # 1 character needs 2 fires, the peaks hold 5: alphas (30 x 0.1) rescaled to sum 2 = 30 x 0.066667: 15 frames -> 1.0000 fires
    # at frame 14 (rest 0.0001), 15 more -> 1.0001 at 29: fires 12.5, 27.5 = 15 frames > 12: a = [12.5, 24.5] + <sil>
    text, ts = ts_prediction_lfr6(FLAT(30), peaks_at(30, [3, 9, 15, 21, 27]), ["a"])
    assert ts == [[250, 490]] and text == "<sil> 0.000 0.250;a 0.250 0.490;<sil> 0.490 0.600;"


def test_empty_character_list_and_no_fire():
    assert ts_prediction_lfr6(FLAT(30), peaks_at(30, [4, 14, 27]), []) == ("", [])
    assert ts_prediction_lfr6(FLAT(30), peaks_at(30, [4, 14, 27]), ["</s>"]) == ("", [])
    assert ts_prediction_lfr6(np.zeros(30, np.float32), peaks_at(30, []), ["a"]) == ("", [])       # nothing to rescale, no fire


def test_host_scan_equals_oracle_scan_bit_for_bit():
    g = torch.Generator().manual_seed(7)
    for U in (1, 3, 150, 1500):
        a = torch.rand(4, U, generator=g) * 0.3
        ref = orc.cif_wo_hidden(a).numpy()
        for b in range(4):
            got = cif_wo_hidden(a[b].numpy())
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref[b].view(np.uint32))
    assert (orc.cif_wo_hidden(torch.rand(1, 1500, generator=g) * 0.3) >= orc.THRESHOLD).sum() > 100       # the reset branch is exercised


def test_oracle_timestamps_equal_host_rules():
    """the two restatements of the rules (numpy in the product, torch in the oracle) agree on random alphas, count off or not"""
    g = torch.Generator().manual_seed(11)
    for n in (0, 1, 5, 9, 14, 30):
        a = torch.rand(150, generator=g) * 0.13
        p = orc.cif_wo_hidden(a[None])[0]
        assert orc.timestamps(a, p, n) == ts_prediction_lfr6(a.numpy(), p.numpy(), [f"t{i}" for i in range(n)])[1], n


def test_recipe_head_shapes_and_sums():
    """12 tensors; the decoder recipe is unchanged by them; gates unsaturated; the sum of the alphas before re-normalisation
    is within a factor 2 of the token count"""
    from targetdiarization_amd import weights as W
    ts = W.recipe_paraformer_timestamp_state_dict(0)
    assert list(ts) == list(W.paraformer_timestamp_param_shapes()) and len(ts) == 12
    assert all(tuple(v.shape) == W.paraformer_timestamp_param_shapes()[k] for k, v in ts.items())
    dec = W.recipe_paraformer_decoder_state_dict(0, 1, vocab=64)
    assert not set(ts) & set(dec)
    sd = dict(dec); sd.update(ts)
    enc = torch.randn(2, 50, 512, generator=torch.Generator().manual_seed(1))
    counts = torch.floor(orc.cif_alphas(enc, sd, residual=False).sum(-1))
    h = orc.upsampled_head(enc, counts, sd)
    assert float(h["tap"].abs().max()) < 0.99 and 0.1 < float(h["tap"].std()) < 0.4
    ratio = h["raw"].sum(-1) / counts
    assert float(ratio.min()) > 0.5 and float(ratio.max()) < 2.0, ratio
    assert torch.allclose(h["alphas"].sum(-1), counts, rtol=1e-5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_oracle_runs_in_both_precisions(dtype):
    from targetdiarization_amd import weights as W
    sd = orc.cast(W.recipe_paraformer_timestamp_state_dict(0), dtype)
    enc = torch.randn(1, 7, 512, generator=torch.Generator().manual_seed(2)).to(dtype)
    h = orc.upsampled_head(enc, torch.tensor([2]), sd)
    assert h["tap"].shape == (1, 21, 1024) and h["tap"].dtype == dtype and h["peaks"].dtype == dtype
    # ConvTranspose1d with kernel = stride: frame 3t + j is tap j of encoder frame t
    y = torch.einsum("btc,cdj->btjd", enc, sd["predictor.upsample_cnn.weight"]).reshape(1, 21, 512) + sd["predictor.upsample_cnn.bias"]
    ref = torch.nn.functional.conv_transpose1d(enc.transpose(1, 2), sd["predictor.upsample_cnn.weight"], sd["predictor.upsample_cnn.bias"], stride=3)
    assert torch.allclose(y, ref.transpose(1, 2), atol=1e-5)
