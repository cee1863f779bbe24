"""Apollo restorer on the device (csrc/apollo.hip, apollo.ApolloRestorer) against the reference's outputs (tests/golden, minted
from the reference's own apollo.py) and the float64 restatement (tests/apollo_oracle.py); restore_audio's contract; the restorer
inside hot loop B of TargetDiarization."""
import os

import numpy as np
import pytest
import torch

import apollo_oracle as orc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def oracle(xs, sd, num_layers):
    sd64 = orc.cast_state_dict(sd, torch.float64)
    return [orc.apollo_forward(x.double().cpu().unsqueeze(0), sd64, num_layers)[0] for x in xs]


@pytest.fixture(scope="module")
def sd6():
    from targetdiarization_amd.weights import recipe_apollo_state_dict
    return recipe_apollo_state_dict(seed=0)


@pytest.fixture(scope="module")
def sd2():
    from targetdiarization_amd.weights import recipe_apollo_state_dict
    return recipe_apollo_state_dict(seed=5, num_layers=2)


@pytest.fixture(scope="module")
def rest6(sd6):
    from targetdiarization_amd.apollo import ApolloRestorer
    return ApolloRestorer(sd6, DEV)


def test_reference_goldens_6_layers(rest6):
    g = np.load(os.path.join(GOLD, "apollo_ref_6l.npz"))
    xs = [torch.from_numpy(g["x44137"]).to(DEV), torch.from_numpy(g["x1324"]).to(DEV)]
    ys = rest6(xs)
    torch.cuda.synchronize()
    errs = [rel(ys[0], g["y44137"]), rel(ys[1], g["y1324"])]
    print("apollo 6 layers vs reference goldens rel-L2:", errs)
    assert ys[0].shape == (44137,) and ys[1].shape == (1324,)
    assert max(errs) < 1e-4
    assert rest6.flops([44100]) > 2.4e11


def test_ragged_batch_2_layers(sd2):
    from targetdiarization_amd.apollo import ApolloRestorer
    from targetdiarization_amd.weights import recipe_wave
    r = ApolloRestorer(sd2, DEV, num_layers=2)
    lens = [442, 44137, 3 * 44100 + 200]
    xs = [torch.from_numpy(recipe_wave(f"apollo-ragged{n}", 1, n)[0]).to(DEV) for n in lens]
    ys = r(xs)
    alone = [r([x])[0] for x in xs]
    torch.cuda.synchronize()
    refs = oracle(xs, sd2, 2)
    errs = [rel(y, o) for y, o in zip(ys, refs)]
    same = [rel(y, a) for y, a in zip(ys, alone)]
    print("apollo 2 layers ragged vs fp64 oracle:", errs, "batched vs alone:", same)
    assert max(errs) < 1e-4
    assert max(same) <= 1e-6
    with pytest.raises(Exception):
        r([torch.zeros(441, device=DEV)])


def test_two_10s_clips_6_layers(rest6, sd6):
    from targetdiarization_amd.weights import recipe_wave
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    xs = [torch.from_numpy(recipe_wave(f"apollo-10s{i}", 1, 441000 + 37 * i, amp=0.3)[0]).to(DEV) for i in range(2)]
    ys = rest6(xs)
    torch.cuda.synchronize()
    errs = [rel(y, o) for y, o in zip(ys, oracle(xs, sd6, 6))]
    print("apollo 6 layers 2 x 10 s vs fp64 oracle:", errs)
    assert max(errs) < 1e-4


def test_long_clip_cut_into_windows(sd2):
    """a clip longer than the row budget is cut into frame windows with the 54-frame halo: equal to the unsplit run"""
    from targetdiarization_amd.apollo import ApolloRestorer
    from targetdiarization_amd.weights import recipe_wave
    small = ApolloRestorer(sd2, DEV, num_layers=2, rows_per_launch=80 * 160)
    big = ApolloRestorer(sd2, DEV, num_layers=2)
    n = 500 * 441 + 123
    x = torch.from_numpy(recipe_wave("apollo-long", 1, n)[0]).to(DEV)
    assert len(small.plan([n])) > 3 and len(big.plan([n])) == 1
    y_small, y_big = small([x, x[:5000]]), big([x, x[:5000]])
    torch.cuda.synchronize()
    split = rel(y_small[0], y_big[0])
    err = rel(y_small[0], oracle([x], sd2, 2)[0])
    print("apollo windowed vs unsplit:", split, "vs fp64 oracle:", err)
    assert split <= 1e-6 and rel(y_small[1], y_big[1]) <= 1e-6
    assert err < 1e-4


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("audio_only", [False, True])
def test_restore_audio_contract(sd2, keep, audio_only, capsys):
    from targetdiarization_amd import ops
    from targetdiarization_amd.audio_processor import AudioProcessor
    from targetdiarization_amd.weights import recipe_wave
    ap = AudioProcessor(is_restore_audio=True, restorer_state_dict=sd2, cuda_device=0, verbose_log=True)
    assert ap.is_restore_audio
    x = recipe_wave("apollo-16k", 1, 12345, amp=0.3)[0]
    res = ap.restore_audio(x, 16000, keep_sampling_rate=keep, output_audio_only=audio_only)
    assert "Running module: restore_audio" in capsys.readouterr().out
    out, sr = (res, None) if audio_only else res
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.ndim == 1
    up = ops.resample_poly(torch.from_numpy(x).to(DEV), 16000, 44100)
    ref = oracle([up], sd2, 2)[0].float().to(DEV)
    if keep:
        ref = ops.resample_poly(ref, 44100, 16000)
    assert out.shape == ref.shape                 # 44.1 kHz length, or the resampled-back length (ceil rule both ways)
    if not audio_only:
        assert sr == (16000 if keep else 44100)
    err = rel(out, ref)
    print(f"restore_audio keep={keep} audio_only={audio_only} vs oracle:", err)
    assert err < 1e-4
    # device tensors in -> device tensors out; [n, C] -> C clips, returned [C, n]
    xt = torch.from_numpy(np.stack([x, 0.5 * x], 1)).to(DEV)
    y2 = ap.restore_audio(xt, 16000, keep_sampling_rate=keep, output_audio_only=True)
    assert isinstance(y2, torch.Tensor) and y2.is_cuda and y2.shape == (2, ref.shape[0])
    assert rel(y2[0], out) <= 1e-6


def test_restore_audio_skips_on_bad_weights(sd2, capsys):
    from targetdiarization_amd.audio_processor import AudioProcessor
    bad = dict(sd2)
    del bad["net.1.band_net.output.weight"]
    ap = AudioProcessor(is_restore_audio=True, restorer_state_dict=bad, cuda_device=0)
    assert not ap.is_restore_audio
    assert "Failed to init restorer model" in capsys.readouterr().out
    x = np.ones(2000, dtype=np.float32)
    assert ap.restore_audio(x, 16000) is x
    assert "Skip module: restore_audio" in capsys.readouterr().out
    ap = AudioProcessor(is_restore_audio=False, restorer_state_dict=sd2, cuda_device=0)
    assert not ap.is_restore_audio and ap.restore_audio(x, 16000, output_audio_only=True) is x


def test_separate_overlaps_hands_restored_streams_to_vad():
    """TargetASR.py:626-634: the chosen target and noise streams are restored before VAD; all segments in one batched call"""
    from targetdiarization_amd import ops
    from targetdiarization_amd.target_diarization import TargetDiarization
    from targetdiarization_amd.weights import recipe_apollo_state_dict, recipe_eres2netv2_state_dict, recipe_state_dict, recipe_wave
    sep, spk = recipe_state_dict(seed=1, num_blocks=2), recipe_eres2netv2_state_dict(0)
    rsd = recipe_apollo_state_dict(seed=2, num_layers=1)
    seen0, seen1 = [], []

    def vad_of(seen):
        def vad(a):
            seen.append(np.array(a, dtype=np.float32, copy=True))
            return [[0.0, round(a.shape[0] / 16000.0, 3)]]
        return vad
    td0 = TargetDiarization(cuda_device=0, sep_state_dict=sep, spk_state_dict=spk, vad=vad_of(seen0))
    td1 = TargetDiarization(cuda_device=0, sep_state_dict=sep, spk_state_dict=spk, vad=vad_of(seen1), restorer_state_dict=rsd)
    assert not td0.hp.ap.is_restore_audio and td1.hp.ap.is_restore_audio
    audio = recipe_wave("apollo-td", 1, 32000, amp=0.3)[0]
    target = td0.hp.spk.get_speaker_embeddings([audio[:16000]])[0]
    ranges = [(0.1, 0.9), (1.0, 1.95)]
    r0 = td0._separate_overlaps(audio, ranges, target)
    r1 = td1._separate_overlaps(audio, ranges, target)
    # the first len(ranges) calls see the segments, then target, noise of each segment
    assert len(seen0) == len(seen1) == 3 * len(ranges)
    for a, b in zip(seen0[:2], seen1[:2]):
        assert np.array_equal(a, b)
    for k in range(2, 6):
        raw, got = seen0[k], seen1[k]
        up = ops.resample_poly(torch.from_numpy(raw).to(DEV), 16000, 44100)
        ref = ops.resample_poly(oracle([up], rsd, 1)[0].float().to(DEV), 44100, 16000)
        assert got.shape == ref.shape
        assert rel(got, ref) < 1e-4
        assert rel(got, raw) > 1e-3                       # it did change
    assert [len(x) for x in r0] == [len(x) for x in r1] == [2, 2]
    assert np.array_equal(r1[0][0][1], seen1[2]) and np.array_equal(r1[1][1][1], seen1[5])
