"""CPU tests of the silero-VAD host side (targetdiarization_amd/silero.py, weights.py) and of the oracle the GPU tests compare
against (tests/silero_vad_oracle.py): the get_speech_timestamps state machine on hand-written probability tracks, the window
construction against an independent slice-and-mirror, state-dict normalisation, the strict blob, the file loader, and the
conditions on the test clips that tests/test_gpu_silero_vad.py leans on."""
import ctypes as C

import numpy as np
import pytest
import torch

import silero_vad_oracle as orc
from targetdiarization_amd import silero as S

W = 512


def track(*runs):
    return np.concatenate([np.full(n, p) for p, n in runs])


# ---- the state machine: threshold 0.5, neg 0.35, min_speech 250 ms = 4000, min_silence 100 ms = 1600, pad 30 ms = 480 samples ----
def test_hysteresis_band_and_short_dips():
    p = track((0.1, 4), (0.9, 10), (0.4, 1), (0.9, 5), (0.1, 10))
    # 0.4 is under the threshold but not under neg = 0.35: no pending end; the segment closes at the first silent chunk (20)
    assert S.speech_timestamps(p, 30 * W) == [[4 * W - 480, 20 * W + 480]]
    p[14] = 0.3                                                  # under neg: a pending end, cleared by the next speech chunk
    assert S.speech_timestamps(p, 30 * W) == [[4 * W - 480, 20 * W + 480]]
    assert S.speech_timestamps(p, 30 * W, neg_threshold=0.45) == [[4 * W - 480, 20 * W + 480]]
    assert S.speech_timestamps(p, 30 * W, return_seconds=True) == [[0.1, 0.7]]          # 1568 / 16000 = 0.098, 10720 / 16000 = 0.67


def test_silence_shorter_than_and_equal_to_min_silence():
    p = track((0.9, 10), (0.1, 3), (0.9, 10), (0.1, 6))
    n = 29 * W
    # three silent chunks: at the third, 512 i - temp_end = 1024 samples
    assert S.speech_timestamps(p, n, min_silence_duration_ms=64) == [[0, 5120 + 480], [6656 - 480, 11776 + 480]]      # 1024 >= 1024: closes
    assert S.speech_timestamps(p, n, min_silence_duration_ms=65) == [[0, 11776 + 480]]                                 # 1024 < 1040: goes on
    assert S.speech_timestamps(p, n) == [[0, 11776 + 480]]                                                               # default 1600
    assert S.speech_timestamps(p, n, min_silence_duration_ms=64, return_seconds=True) == [[0.0, round(0.35, 1)], [0.4, 0.8]]


def test_min_speech_exactly_and_just_over():
    p = track((0.1, 2), (0.9, 8), (0.1, 8))                      # a segment of 8 chunks = 4096 samples = 256 ms
    assert S.speech_timestamps(p, 18 * W, min_speech_duration_ms=256) == []                     # not LONGER than min_speech
    assert S.speech_timestamps(p, 18 * W, min_speech_duration_ms=255) == [[1024 - 480, 5120 + 480]]
    assert S.speech_timestamps(p, 18 * W) == [[1024 - 480, 5120 + 480]]                         # default 4000
    assert S.speech_timestamps(track((0.1, 2), (0.9, 7), (0.1, 8)), 17 * W) == []              # 3584 samples


def test_padding_between_neighbours():
    p = track((0.9, 10), (0.1, 1), (0.9, 10), (0.1, 3))
    # min_silence 0: one silent chunk splits; the gap of 512 < 2 * 480 is shared, half each
    assert S.speech_timestamps(p, 24 * W, min_silence_duration_ms=0) == [[0, 5120 + 256], [5632 - 256, 10752 + 480]]
    # a gap of 1536 >= 960: 480 on each side (test_silence_shorter_than_and_equal_to_min_silence has the same case)
    p = track((0.9, 10), (0.1, 3), (0.9, 10), (0.1, 3))
    assert S.speech_timestamps(p, 26 * W, min_silence_duration_ms=0) == [[0, 5600], [6176, 11776 + 480]]
    assert S.speech_timestamps(p, 26 * W, min_silence_duration_ms=0, speech_pad_ms=0) == [[0, 5120], [6656, 11776]]


def test_clip_ending_in_speech_and_empty_input():
    n = 13 * W - 100
    assert S.speech_timestamps(track((0.1, 3), (0.9, 10)), n) == [[1536 - 480, n]]              # closes at n_samples, the pad is capped there
    assert S.speech_timestamps(track((0.1, 3), (0.9, 7)), 10 * W - 100) == []                   # 3484 samples: too short
    assert S.speech_timestamps(track((0.1, 3), (0.9, 10), (0.2, 2)), 15 * W) == [[1536 - 480, 15 * W]]      # pending end, never confirmed
    assert S.speech_timestamps([], 0) == [] and S.speech_timestamps(np.zeros(0), 0, return_seconds=True) == []
    assert S.speech_timestamps(track((0.1, 20)), 20 * W) == []
    assert S.speech_timestamps(track((0.5, 20)), 20 * W) == [[0, 20 * W]]                       # p >= threshold counts as speech


# ---- the oracle ---------------------------------------------------------------------------------------------
def test_oracle_windows_against_slice_and_mirror():
    rng = np.random.default_rng(7)
    for n in (1, 511, 512, 513, 1537, 5 * W):
        x = rng.standard_normal(n)
        got = orc.windows(torch.from_numpy(x)).numpy()
        N = (n + W - 1) // W
        xp = np.concatenate([x, np.zeros(N * W - n)])
        assert got.shape == (N, 640)
        for i in range(N):
            chunk = xp[i * W:(i + 1) * W]
            ctx = xp[i * W - 64:i * W] if i else np.zeros(64)
            mirror = chunk[-2:-66:-1]                            # the chunk's own tail without the edge sample, reversed
            assert mirror.shape == (64,) and mirror[0] == chunk[510] and mirror[63] == chunk[447]
            assert np.array_equal(got[i], np.concatenate([ctx, chunk, mirror])), (n, i)


def test_oracle_state_is_carried_and_causal():
    sd = orc.calibrated_state_dict()
    a, b = orc.causal_pair(5)
    pa, pb = orc.forward(sd, a)[0], orc.forward(sd, b)[0]
    assert torch.equal(pa[:6], pb[:6]) and not torch.equal(pa[6:], pb[6:])
    # (h, c) carried: the second half of a clip differs from the same samples run as a clip of their own
    half = orc.forward(sd, a[6 * W:])[0]
    assert float((half - pa[6:]).abs().max()) > 1e-4


def test_normalize_state_dict_and_blob():
    from targetdiarization_amd.weights import pack_blob, pack_silero_vad_blob, recipe_silero_vad_state_dict, silero_vad_param_shapes
    sd = recipe_silero_vad_state_dict(0)
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(silero_vad_param_shapes()) and len(sd) == 15
    assert all(v.dtype == torch.float32 for v in sd.values())
    again = recipe_silero_vad_state_dict(0)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    # the basis is the windowed DFT: row k real, row 129 + k imaginary
    basis = sd["stft.forward_basis_buffer"][:, 0].double()
    n = torch.arange(256, dtype=torch.float64)
    hann = 0.5 - 0.5 * torch.cos(2 * np.pi * n / 256)
    assert float((basis[3] - torch.cos(2 * np.pi * 3 * n / 256) * hann).abs().max()) < 1e-6
    assert float((basis[129 + 3] + torch.sin(2 * np.pi * 3 * n / 256) * hann).abs().max()) < 1e-6
    raw = {}
    for k, v in sd.items():
        raw["_model." + k] = v
        raw["_model_8k." + k] = torch.zeros(1)
    norm = S.normalize_state_dict(raw)
    assert list(norm) == list(sd) and all(norm[k] is sd[k] for k in sd)
    assert list(S.normalize_state_dict(sd)) == list(sd)
    assert pack_silero_vad_blob(raw) == pack_blob(sd) == pack_silero_vad_blob(sd)


def test_blob_is_strict_both_ways():
    """names and shapes are checked before any device work, so this needs no GPU"""
    from targetdiarization_amd import _lib
    from targetdiarization_amd.build import build_lib
    from targetdiarization_amd.weights import pack_silero_vad_blob, recipe_silero_vad_state_dict
    build_lib()
    lib = _lib.lib()

    def create(sd):
        blob = pack_silero_vad_blob(sd)
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        h = C.c_void_p()
        return lib.tdx_silero_create(buf, len(blob), 0, C.byref(h)), lib.tdx_last_error()
    sd = recipe_silero_vad_state_dict(0)
    for name in ("stft.forward_basis_buffer", "encoder.2.reparam_conv.bias", "decoder.rnn.weight_hh", "decoder.decoder.2.weight"):
        miss = dict(sd); miss.pop(name)
        rc, err = create(miss)
        assert rc == 2 and name.encode() in err
    extra = dict(sd); extra["decoder.rnn.weight_hr"] = torch.zeros(4)
    rc, err = create(extra)
    assert rc == 2 and b"unexpected tensor: decoder.rnn.weight_hr" in err
    turned = dict(sd); turned["decoder.rnn.weight_ih"] = sd["decoder.rnn.weight_ih"].t().contiguous()          # [128,512]: same numel
    rc, err = create(turned)
    assert rc == 2 and b"decoder.rnn.weight_ih" in err
    flat = dict(sd); flat["decoder.decoder.2.weight"] = sd["decoder.decoder.2.weight"].reshape(1, 128)
    rc, err = create(flat)
    assert rc == 2 and b"decoder.decoder.2.weight" in err
    assert lib.tdx_silero_create(None, 0, 0, None) == 1
    assert lib.tdx_silero_workspace_bytes(None, 1, 10) == 0 and lib.tdx_silero_flops(None, 10) == 0.0
    assert lib.tdx_silero_forward(None, None, None, 1, 1, None, None, None, None, 0, None) == 1


def test_file_loader(tmp_path):
    from safetensors.torch import save_file
    from targetdiarization_amd.weights import recipe_silero_vad_state_dict
    sd = recipe_silero_vad_state_dict(0)
    raw = {"_model." + k: v for k, v in sd.items()}
    raw["_model_8k.decoder.rnn.bias_ih"] = torch.zeros(512)
    p = str(tmp_path / "silero_vad.safetensors")
    save_file(raw, p)
    got = S.load_model_file(p)
    assert set(got) == set(raw)
    norm = S.normalize_state_dict(got)
    assert set(norm) == set(sd) and all(torch.equal(norm[k], sd[k]) for k in sd)
    q = str(tmp_path / "silero_vad.pt")                          # not a TorchScript archive: the torch.load fallback
    torch.save(dict(sd), q)
    got = S.load_model_file(q)
    assert set(got) == set(sd) and torch.equal(got["decoder.rnn.bias_hh"], sd["decoder.rnn.bias_hh"])
    junk = str(tmp_path / "junk.jit")
    open(junk, "wb").write(b"not a model")
    assert S.load_model_file(junk) is None and S.load_model_file(str(tmp_path / "absent.safetensors")) is None
    assert S.load_model_file(None) is None and S.load_model_file(str(tmp_path)) is None
    assert S.build_silero() is None and S.build_silero(None, None) is None
    with pytest.raises(ValueError):
        S.build_silero(model_file=junk)


def test_server_env_forwards_the_model_file():
    from targetdiarization_amd.server import env_to_kwargs
    assert env_to_kwargs({"SILERO_VAD_MODEL": "/models/silero_vad.safetensors"})["silero_model_file"] == "/models/silero_vad.safetensors"
    assert "silero_model_file" not in env_to_kwargs({})


# ---- the conditions tests/test_gpu_silero_vad.py leans on --------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_probs():
    sd = orc.calibrated_state_dict()
    clips = orc.prob_clips() + orc.e2e_clips()
    return clips, [orc.forward(sd, c)[0].numpy() for c in clips]


def test_gpu_test_inputs_stay_clear_of_the_thresholds(oracle_probs):
    """Conditions on the inputs, not tolerances: the end-to-end test demands timestamps EQUAL to the oracle's, which holds only
    if no chunk's p is near 0.5 or 0.35, and both sides must hold at least 20 % of every clip of >= 8 chunks."""
    clips, probs = oracle_probs
    cal = orc.calibration()
    clear = max(0.02, 20 * cal["p_device_bound"])
    assert [len(c) for c in clips[:8]] == list(orc.PROB_SAMPLES) and [len(p) for p in probs[:8]] == [1, 1, 1, 2, 2, 4, 33, 313]
    for c, p in zip(clips, probs):
        d = float(np.minimum(np.abs(p - 0.5), np.abs(p - 0.35)).min())
        assert d >= clear, (len(c), d, clear)
        if len(p) >= 8:
            share = float((p >= 0.5).mean())
            assert 0.2 <= share <= 0.8, (len(c), share)
        assert 0.01 < p.min() and p.max() < 0.99                 # the logit is recovered from p: keep it where fp32 has the digits


def test_e2e_clips_exercise_the_state_machine(oracle_probs):
    """three bursts per clip, the one under 250 ms never becomes a segment; the second clip ends in speech"""
    clips, probs = oracle_probs
    for c, p, lab in zip(clips[8:], probs[8:], orc.e2e_labels()):
        assert 4.0 * 16000 <= len(c) <= 6.0 * 16000
        assert np.array_equal(p >= 0.5, lab > 0)
        assert len(S.speech_timestamps(p, len(c), min_silence_duration_ms=100)) == 2             # the short burst is dropped
        assert len(S.speech_timestamps(p, len(c), min_silence_duration_ms=100, min_speech_duration_ms=100)) == 3
    b = S.speech_timestamps(probs[9], len(clips[9]))
    assert b[-1][1] == len(clips[9])


def test_calibration_file_carries_the_measured_bound():
    cal = orc.calibration()
    assert cal["calibration_voiced_min_p"] > 0.5 and cal["calibration_silent_max_p"] < 0.35
    assert 0 < cal["p_fp32_vs_fp64_max_abs"] < 1e-4 and cal["p_device_bound"] == 10.0 * cal["p_fp32_vs_fp64_max_abs"]
    assert len(cal["head_weight"]) == 128 and cal["check_min_distance_from_thresholds"] >= 0.02
