"""CPU tests of the FSMN-VAD stage: the host segmenter (targetdiarization_amd/vad.py) against the worked examples of its
specification, ASRProcessor.vad_detection's post-processing through a stub model, the oracle's LFR, the conditions the GPU
test's inputs have to meet (checked with the fp64 oracle alone), the weight catalogue and the strict blob loader."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import fsmn_vad_oracle as orc
from targetdiarization_amd import vad as V


def pat(T, *ranges, step=1):
    s = [0] * T
    for a, b in ranges:
        for t in range(a, b, step):
            s[t] = 1
    return s


TABLE = [
    (pat(600, (100, 300)), 6025, 800, [[740, 3000]]),
    (pat(600, (100, 300)), 6025, 500, [[740, 3000]]),
    (pat(600, (100, 300)), 6025, 0, [[740, 3050]]),
    (pat(600, (100, 300), (330, 420)), 6025, 500, [[740, 3000], [3140, 4200]]),
    (pat(600, (100, 300), (330, 420)), 6025, 0, [[740, 3050], [3050, 4250]]),
    (pat(600, (10, 24), (450, 600)), 6025, 800, [[4240, 6025]]),        # 14 speech frames never trigger; the clip ends in speech
    (pat(600, (100, 114)), 6025, 800, []),
    (pat(600, (100, 115)), 6025, 800, [[740, 1150]]),
    (pat(600, (100, 300), step=2), 6025, 800, []),                     # every second frame: the window never reaches 150 ms
    (pat(7000, (50, 6900)), 70025, 800, [[240, 60240], [60240, 69000]]),
]


@pytest.mark.parametrize("case", range(len(TABLE)))
def test_segmenter_worked_examples(case):
    speech, dur, sil, want = TABLE[case]
    assert V.speech_segments(speech, dur, sil) == want


def test_segments_never_overlap_and_stay_inside_the_clip():
    rng = np.random.default_rng(5)
    for trial in range(60):
        T = int(rng.integers(1, 900))
        s = np.zeros(T, dtype=int)
        for _ in range(int(rng.integers(0, 8))):                        # bursts of any length, some with holes
            a = int(rng.integers(0, T)); b = min(T, a + int(rng.integers(1, 200)))
            s[a:b] = rng.random(b - a) < rng.choice([1.0, 0.8, 0.5])
        dur = (400 + 160 * (T - 1)) // 16
        for sil in (0, 300, 500, 800):
            out = V.speech_segments(s.tolist(), dur, sil)
            prev = 0
            for a, b in out:
                assert prev <= a < b <= max(dur, T * 10), (trial, sil, out)
                prev = b


def test_segments_from_posteriors_uses_the_speech_noise_threshold():
    p0 = np.ones(600); p0[100:300] = 0.2                                # 1 - 0.2 >= 0.2 + 0.6 holds with equality
    assert V.segments(p0, 6025 * 16, 800) == [[740, 3000]]
    p0[100:300] = 0.21
    assert V.segments(p0, 6025 * 16, 800) == []
    assert V.segments(np.zeros(0), 100) == []


# ------------------------------------------------------------------------------------------------------------
# ASRProcessor.vad_detection: post-processing through a stub model
# ------------------------------------------------------------------------------------------------------------
class StubVad:
    def __init__(self, value):
        self.value, self.calls = value, []

    def detect_batch_ms(self, clips, max_end_silence_ms=800):
        self.calls.append((len(clips), int(clips[0].shape[0]), max_end_silence_ms))
        return [[list(v) for v in self.value] for _ in clips]


def _asrp(value):
    from targetdiarization_amd.asr_processor import ASRProcessor
    a = ASRProcessor(verbose_log=False)
    a.vad, a.is_vad = StubVad(value), True
    return a


def test_vad_detection_without_a_model_prints_and_returns_empty(capsys):
    from targetdiarization_amd.asr_processor import ASRProcessor
    a = ASRProcessor(verbose_log=False)
    assert a.is_vad is False and a.vad_detection(np.zeros(16000, np.float32)) == []
    assert "FunASR VAD model hasn't been loaded" in capsys.readouterr().out
    b = ASRProcessor(is_vad=True, vad_model_dir="/nonexistent/dir", verbose_log=False)      # a failed load switches the feature off
    assert b.is_vad is False and "Failed to load FunASR VAD model" in capsys.readouterr().out
    assert b.vad_detection(np.zeros(16000, np.float32)) == []


def test_vad_detection_postprocessing():
    audio = np.zeros(16000 * 12, np.float32)
    a = _asrp([[500, 1200], [1500, 1900], [2500, 6500], [7000, 7300]])
    assert a.vad_detection(audio) == [[0.5, 1.2], [1.5, 1.9], [2.5, 6.5], [7.0, 7.3]]
    assert a.vad.calls[-1] == (1, 16000 * 12, 500)                                           # int(0.5 * 1000)
    a.vad_detection(audio, min_silence_sec=0.8); assert a.vad.calls[-1][2] == 800
    assert a.vad_detection(audio, format_to_sec=False) == [[500, 1200], [1500, 1900], [2500, 6500], [7000, 7300]]
    # merge: a range shorter than min_clip_sec takes its successor in; the short tail goes to its predecessor
    assert a.vad_detection(audio, min_clip_sec=1.0) == [[0.5, 1.9], [2.5, 7.3]]
    assert a.vad_detection(audio, min_clip_sec=100.0) == [[0.5, 7.3]]
    # split: duration 4.0 > 1.5 -> int(4.0 // 1.5) = 2 cuts -> 3 equal parts
    got = a.vad_detection(audio, max_clip_sec=1.5)
    assert got[:2] == [[0.5, 1.2], [1.5, 1.9]] and got[-1] == [7.0, 7.3] and len(got) == 6
    np.testing.assert_allclose(got[2:5], [[2.5, 2.5 + 4 / 3], [2.5 + 4 / 3, 2.5 + 8 / 3], [2.5 + 8 / 3, 6.5]], rtol=0, atol=1e-12)
    # format_to_sec=False returns the detector's own ranges, untouched by merge / split (ASRProcessor.py:814-817)
    assert a.vad_detection(audio, min_clip_sec=1.0, format_to_sec=False) == [[500, 1200], [1500, 1900], [2500, 6500], [7000, 7300]]
    # the one deviation: nothing detected and min_clip_sec > 0 -> [] (the reference raises IndexError)
    assert _asrp([]).vad_detection(audio, min_clip_sec=1.0) == []
    with pytest.raises(ValueError):
        a.vad_detection("clip.wav")
    with pytest.raises(ValueError):
        a.vad_detection(b"\0\0")


def test_vad_detection_output_folder_goes_through_ap(tmp_path, capsys):
    audio = np.arange(16000 * 3, dtype=np.float32)
    a = _asrp([[500, 1000], [1500, 2500]])
    a.vad_detection(audio, output_folder=str(tmp_path / "out"))
    assert "nothing written" in capsys.readouterr().out and not (tmp_path / "out").exists()

    class Ap:
        written = []

        @staticmethod
        def split_audio_by_time(audio_data, sampling_rate, start_time, end_time):
            return audio_data[int(start_time * sampling_rate):int(end_time * sampling_rate)]

        def write_to_file(self, output_path, audio_data, sampling_rate):
            self.written.append((output_path, len(audio_data), sampling_rate))
    a.ap = Ap()
    a.vad_detection(audio, output_folder=str(tmp_path / "out"), output_name="seg")
    assert Ap.written == [(f"{tmp_path}/out/seg_0.wav", 8000, 16000), (f"{tmp_path}/out/seg_1.wav", 16000, 16000)]


def test_vad_detection_reads_paths_through_ap_like_the_reference(tmp_path):
    """:750-756, :801-804: a file at 16 kHz is cut from the MONO audio; a file at another rate is resampled (keyword arguments) for the
    detector and cut from the audio as read, at its own rate"""
    class Ap:
        def __init__(self, rate):
            self.rate, self.written, self.resampled = rate, [], None

        def read_audio(self, path):
            return np.ones((self.rate * 3, 2), np.float32), self.rate

        def audio_resample(self, target_sr, orig_sr, audio_data):            # another parameter order than the reference's
            self.resampled = (orig_sr, target_sr)
            return np.ones((3 * target_sr, 2), np.float32), target_sr

        @staticmethod
        def audio_to_mono(audio):
            return audio.mean(axis=1)

        @staticmethod
        def split_audio_by_time(audio_data, sampling_rate, start_time, end_time):
            return audio_data[int(start_time * sampling_rate):int(end_time * sampling_rate)]

        def write_to_file(self, output_path, audio_data, sampling_rate):
            self.written.append((output_path, audio_data.shape, sampling_rate))
    a = _asrp([[500, 1000]])
    a.ap = Ap(16000)
    assert a.vad_detection("dir/talk.wav", output_folder=str(tmp_path)) == [[0.5, 1.0]]
    assert a.vad.calls[-1][1] == 48000 and a.ap.resampled is None
    assert a.ap.written == [(f"{tmp_path}/talk_0.wav", (8000,), 16000)]
    a.ap = Ap(8000)
    a.vad_detection("dir/talk.wav", output_folder=str(tmp_path))
    assert a.ap.resampled == (8000, 16000) and a.vad.calls[-1][1] == 48000
    assert a.ap.written == [(f"{tmp_path}/talk_0.wav", (4000, 2), 8000)]


# ------------------------------------------------------------------------------------------------------------
# the oracle and the inputs of the GPU test
# ------------------------------------------------------------------------------------------------------------
def test_oracle_lfr_hand_written():
    from oracle import frontend_oracle as fo
    f = torch.arange(5, dtype=torch.float64)[:, None] * 10 + torch.arange(2, dtype=torch.float64)[None]     # frame t = [10t, 10t+1]
    got = fo.apply_lfr(f, 5, 1)
    idx = [[0, 0, 0, 1, 2], [0, 0, 1, 2, 3], [0, 1, 2, 3, 4], [1, 2, 3, 4, 4], [2, 3, 4, 4, 4]]
    want = torch.stack([torch.cat([f[i] for i in row]) for row in idx])
    assert torch.equal(got, want)
    one = fo.apply_lfr(f[:1], 5, 1)
    assert torch.equal(one, f[:1].repeat(1, 5))


def test_oracle_memory_has_zero_history_and_no_right_context():
    sd, _ = orc.calibrated_state_dict()
    sdd = {k: v.double() for k, v in sd.items()}
    g = torch.Generator().manual_seed(3)
    x = torch.randn(50, 400, generator=g, dtype=torch.float64)
    full = orc.encoder(sdd, x)
    assert torch.allclose(orc.encoder(sdd, x[:30]), full[:30], rtol=0, atol=1e-12)      # causal: a frame ignores what follows
    tail = orc.encoder(sdd, x[10:])
    assert torch.allclose(tail[4 * 19:], full[10 + 4 * 19:], rtol=0, atol=1e-12)        # 4 x 19 frames of history, no more
    assert not torch.allclose(tail[:19], full[10:29], rtol=0, atol=1e-6)


@pytest.fixture(scope="module")
def cal_model():
    return orc.calibrated_state_dict()


def _p0(cal_model, clip):
    sd, cmvn = cal_model
    return orc.forward(sd, cmvn, clip)[0].numpy()


def test_gpu_test_inputs_stay_clear_of_the_threshold(cal_model):
    """Conditions on the inputs, not tolerances: the end-to-end test demands ranges EQUAL to the oracle's, which holds only
    if no frame's p0 is near the decision point (every clip), and both sides of 0.2 must hold at least 20 % of each clip's
    frames.  Exempt from the second condition, by construction: the 1-frame clip (one frame is on one side), the 5-frame clip
    (five LFR-overlapping frames cannot hold a voiced and a silent stretch: it is the all-silence clip, the single frame the
    speech one) and the leak pair (the test needs one clip wholly loud and one wholly silent)."""
    for i, (T, c) in enumerate(zip(orc.POSTERIOR_FRAMES, orc.posterior_clips())):
        p = _p0(cal_model, c)
        assert len(p) == T and int((np.abs(p - 0.2) < 0.02).sum()) == 0, T
        if T >= 19:
            assert (p <= 0.2).mean() >= 0.2 and (p > 0.2).mean() >= 0.2, (T, float((p <= 0.2).mean()))
    assert (_p0(cal_model, orc.posterior_clips()[0]) <= 0.2).all() and (_p0(cal_model, orc.posterior_clips()[1]) > 0.2).all()
    for i, c in enumerate(orc.e2e_clips()):
        p = _p0(cal_model, c)
        assert int((np.abs(p - 0.2) < 0.02).sum()) == 0, i
        assert (p <= 0.2).mean() >= 0.2 and (p > 0.2).mean() >= 0.2, (i, float((p <= 0.2).mean()))
    loud, silent = (_p0(cal_model, c) for c in orc.leak_pair())
    assert int((np.abs(loud - 0.2) < 0.02).sum()) == 0 and int((np.abs(silent - 0.2) < 0.02).sum()) == 0
    assert (loud <= 0.2).mean() > 0.8 and (silent > 0.2).all()


def test_e2e_clips_exercise_the_segmenter(cal_model):
    """three bursts per clip, the one under 150 ms never becomes a segment; the second clip ends in speech"""
    a, b = orc.e2e_clips()
    assert 4.0 * 16000 <= len(a) <= 6.0 * 16000 and 4.0 * 16000 <= len(b) <= 6.0 * 16000
    sa = V.segments(_p0(cal_model, a), len(a), 500)
    sb = V.segments(_p0(cal_model, b), len(b), 500)
    assert len(sa) == 2 and len(sb) == 2 and sb[-1][1] == len(b) // 16
    assert V.segments(_p0(cal_model, a), len(a), 0) != V.segments(_p0(cal_model, a), len(a), 800)


def test_calibration_file_carries_the_measured_bound():
    cal = orc.calibration()
    assert cal["check_frames_near_threshold"] == 0 and 0.2 <= cal["check_speech_share"] <= 0.8 and cal["check_label_agreement"] > 0.9
    assert 0 < cal["p0_fp32_vs_fp64_max_abs"] < 1e-3
    assert cal["p0_device_bound"] == pytest.approx(10 * cal["p0_fp32_vs_fp64_max_abs"], rel=1e-12)
    assert len(cal["cmvn_shift"]) == len(cal["cmvn_scale"]) == 400 and len(cal["row0_weight"]) == 140


# ------------------------------------------------------------------------------------------------------------
# weights
# ------------------------------------------------------------------------------------------------------------
def test_recipe_shapes_and_am_mvn(tmp_path):
    from targetdiarization_amd.weights import fsmn_vad_param_shapes, parse_kaldi_cmvn, recipe_fsmn_vad_state_dict
    shapes = fsmn_vad_param_shapes()
    sd = recipe_fsmn_vad_state_dict(0)
    assert list(sd) == list(shapes) and all(tuple(sd[k].shape) == shapes[k] for k in shapes)
    assert shapes["encoder.fsmn.3.fsmn_block.conv_left.weight"] == (128, 1, 20, 1) and "encoder.fsmn.0.linear.linear.bias" not in shapes
    assert torch.equal(recipe_fsmn_vad_state_dict(0)["encoder.in_linear1.linear.weight"], sd["encoder.in_linear1.linear.weight"])
    assert not torch.equal(recipe_fsmn_vad_state_dict(1)["encoder.in_linear1.linear.weight"], sd["encoder.in_linear1.linear.weight"])
    shift, scale = np.arange(400) * -0.5, 1.0 / (1.0 + np.arange(400))
    (tmp_path / "am.mvn").write_text("<Nnet>\n<Splice> 400 400\n[ 0 ]\n<AddShift> 400 400\n<LearnRateCoef> 0 [ " + " ".join(map(repr, shift.tolist())) +
                                     " ]\n<Rescale> 400 400\n<LearnRateCoef> 0 [ " + " ".join(map(repr, scale.tolist())) + " ]\n</Nnet>\n")
    a, b = parse_kaldi_cmvn(str(tmp_path / "am.mvn"))
    np.testing.assert_array_equal(a, shift.astype(np.float32)); np.testing.assert_array_equal(b, scale.astype(np.float32))
    assert V.load_model_dir(str(tmp_path)) is None                          # no model.pt beside it
    torch.save({k[len("encoder."):]: v for k, v in sd.items()}, tmp_path / "model.pt")
    got, cmvn = V.load_model_dir(str(tmp_path))
    assert set(got) == {k[len("encoder."):] for k in sd} and np.array_equal(cmvn[0], a)
    assert V.build_vad(None, None, "iic/speech_fsmn_vad_zh-cn-16k-common-pytorch") is None


def test_blob_is_strict_both_ways():
    """names and sizes are checked before any device work, so this needs no GPU"""
    from targetdiarization_amd import _lib
    from targetdiarization_amd.build import build_lib
    from targetdiarization_amd.weights import pack_fsmn_vad_blob, recipe_fsmn_vad_state_dict
    build_lib()
    lib = _lib.lib()

    def create(sd, cmvn=None):
        blob = pack_fsmn_vad_blob(sd, cmvn)
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        h = C.c_void_p()
        return lib.tdx_fsmnvad_create(buf, len(blob), 0, C.byref(h)), lib.tdx_last_error()
    sd = recipe_fsmn_vad_state_dict(0)
    for name in ("encoder.fsmn.2.fsmn_block.conv_left.weight", "encoder.out_linear2.linear.bias", "encoder.in_linear1.linear.weight"):
        miss = dict(sd); miss.pop(name)
        rc, err = create(miss)
        assert rc == 2 and name.encode() in err
    extra = dict(sd); extra["encoder.fsmn.0.linear.linear.bias"] = torch.zeros(128)
    rc, err = create(extra)
    assert rc == 2 and b"unexpected tensor: encoder.fsmn.0.linear.linear.bias" in err
    wrong = dict(sd); wrong["encoder.fsmn.1.affine.linear.weight"] = torch.zeros(250, 127)
    rc, err = create(wrong)
    assert rc == 2 and b"encoder.fsmn.1.affine.linear.weight" in err
    turned = dict(sd); turned["encoder.in_linear1.linear.weight"] = sd["encoder.in_linear1.linear.weight"].t().contiguous()   # [400,140]: same numel
    rc, err = create(turned)
    assert rc == 2 and b"encoder.in_linear1.linear.weight" in err
    flat = dict(sd); flat["encoder.fsmn.0.fsmn_block.conv_left.weight"] = sd["encoder.fsmn.0.fsmn_block.conv_left.weight"].reshape(128, 20)
    rc, err = create(flat)
    assert rc == 2 and b"encoder.fsmn.0.fsmn_block.conv_left.weight" in err
    rc, err = create(sd, (np.zeros(399, np.float32), np.ones(399, np.float32)))
    assert rc == 2 and b"cmvn.shift" in err
    assert lib.tdx_fsmnvad_create(None, 0, 0, None) == 1
    assert lib.tdx_fsmnvad_workspace_bytes(None, 10) == 0 and lib.tdx_fsmnvad_flops(None, 10) == 0.0
