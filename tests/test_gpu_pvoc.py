"""Phase-vocoder time stretch, pitch shift, EQ match and the windowed-sinc resampler on the device (effects.PhaseVocoder,
csrc/pvoc.hip) against the float64 oracle of tests/pvoc_oracle.py.  A phase vocoder's output depends on every bin's whole phase
history, so every stage is checked against the oracle applied to the device's own input to that stage, and the end-to-end
comparison is made on the inputs test_pvoc_host.py shows to be well-conditioned."""
import math

import numpy as np
import pytest

import pvoc_cases as cases
import pvoc_oracle as orc
from targetdiarization_amd import effects

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
_RUNS, _PITCH = {}, {}


@pytest.fixture(scope="module")
def pv():
    p = effects.PhaseVocoder("cuda:0")
    yield p
    p.close()


def run(pv, name, rate):
    """one device call per (input, rate) per process -> (y, taps)"""
    if (name, rate) not in _RUNS:
        taps = {}
        _RUNS[name, rate] = (pv.time_stretch(cases.signal(name), rate, taps=taps), taps)
    return _RUNS[name, rate]


def run_pitch(pv, name, n_steps):
    if (name, n_steps) not in _PITCH:
        taps = {}
        _PITCH[name, n_steps] = (pv.pitch_shift(cases.signal(name), cases.SR, n_steps, taps=taps), taps)
    return _PITCH[name, n_steps]


def rel(a, b, den=None):
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b if den is None else den))


# ---- 1. analysis
@pytest.mark.parametrize("name", cases.ALL)
def test_analysis_tap(pv, name):
    D = run(pv, name, 0.8)[1]["spec"]
    ref = cases.spectrum(name)
    assert D.shape == ref.shape and D.dtype == np.complex64
    err, f32 = cases.analysis_error(D, ref), cases.f32_analysis_figure(name)
    print(name, "analysis: device", err, "float32 mode", f32)
    assert err <= 8 * f32 and err < 1e-5


# ---- 2. the phase vocoder alone
def check_vocoder(D, got, rate, what):
    ref = orc.phase_vocoder(D, rate)
    assert got.shape == ref.shape, what
    bound = 16 * EPS * orc.neighbour_mag(D, rate)
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.max() > 0 else 0.0
    print(what, "rate", rate, "worst error / bound", worst)
    assert np.all(err <= bound), what


@pytest.mark.parametrize("rate", cases.RATES)
@pytest.mark.parametrize("name", cases.ALL)
def test_phase_vocoder_stage(pv, name, rate):
    taps = run(pv, name, rate)[1]
    check_vocoder(taps["spec"], taps["stretched"], rate, name)


def random_spectrum(T, seed):
    r = np.random.default_rng(seed)
    return ((r.standard_normal((1025, T)) + 1j * r.standard_normal((1025, T))) * r.uniform(0.01, 10.0, (1025, 1))).astype(np.complex64)


@pytest.mark.parametrize("T", [effects.SEG - 3, effects.SEG + 5, effects.SWEEP + 7])
@pytest.mark.parametrize("rate", [0.8, 1.25, 0.5])
def test_phase_vocoder_of_a_given_spectrum(pv, T, rate):
    D = random_spectrum(T, T)
    check_vocoder(D, pv.phase_vocoder(D, rate), rate, f"random T {T}")


def test_phase_vocoder_device_tensor_and_columns_beyond_the_end(pv):
    import torch
    D = random_spectrum(40, 9)
    D[:, -2:] *= 1000.0                     # loud last columns: the two columns after them are exact zeros, whatever lies in memory
    out = pv.phase_vocoder(torch.from_numpy(D).to("cuda:0"), 0.8)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.complex64
    got = out.cpu().numpy()
    check_vocoder(D, got, 0.8, "loud tail")
    assert np.array_equal(got, pv.phase_vocoder(D, 0.8))
    steps = np.arange(0, 40, 0.8)
    last = steps.astype(int) == 39          # output frames whose second column lies beyond the end
    assert last.sum() >= 1
    want = (1.0 - np.mod(steps, 1.0)[last]) * np.abs(D[:, 39:40].astype(np.complex128))
    assert np.all(np.abs(np.abs(got[:, last].astype(np.complex128)) - want) <= 16 * EPS * np.abs(D[:, 39:40]))


# ---- 3. synthesis alone
@pytest.mark.parametrize("name,rate", [(n, r) for n in cases.ALL for r in (0.8, 1.25)] + [("tiny", 0.5), ("tiny", 0.1), ("odd", 0.5), ("long", 0.5)])
def test_synthesis_stage(pv, name, rate):
    y, taps = run(pv, name, rate)
    n = cases.signal(name).shape[0]
    assert y.shape == (int(round(n / rate)),) and y.dtype == np.float32
    ref = orc.istft(taps["stretched"], length=y.shape[0])
    e = rel(y, ref)
    print(name, rate, "synthesis", e)
    assert e < 1e-5


def test_istft_with_a_length_that_cuts_frames(pv):
    D = run(pv, "noise_chirp", 0.8)[1]["stretched"]
    for length in (3000, None, D.shape[1] * 512 + 999):
        y = pv.istft(D, length=length)
        ref = orc.istft(D, length=length)
        assert y.shape == ref.shape
        assert rel(y, ref) < 1e-5
    assert math.ceil((3000 + 2048) / 512) < D.shape[1]
    assert np.all(pv.istft(D, length=D.shape[1] * 512 + 999)[-400:] == 0)          # beyond the covered range


# ---- 4. the resampler alone
@pytest.mark.parametrize("ratio", [2.0 ** (-3 / 12), 2.0 ** (4 / 12), 2.0 ** (-0.5 / 12), 1.0])
@pytest.mark.parametrize("name", ["noise_chirp", "odd"])
def test_resampler(pv, name, ratio):
    x = cases.signal(name)
    y = pv.resample(x, ratio)
    ref = orc.resample_sinc(x, ratio)
    assert y.shape == ref.shape == (math.ceil(x.shape[0] * ratio),) and y.dtype == np.float32
    e = rel(y, ref, den=x.astype(np.float64))
    print(name, ratio, "resample", e)
    assert e < 1e-5


def test_resampler_positions_are_fp64(pv):
    n, ratio = (1 << 25) + 1000, 2.0 ** (-0.5 / 12)
    j = np.arange(n, dtype=np.float64)
    x = (j / n + 0.5 * np.sin(2 * np.pi * j / 100.0)).astype(np.float32)
    y = pv.resample(x, ratio)
    n_out = math.ceil(n * ratio)
    assert y.shape == (n_out,)
    idx = np.arange(n_out - 3000, n_out - 2000)
    ref = orc.resample_sinc(x, ratio, idx=idx)
    e = rel(y[idx], ref)
    # the same outputs at positions rounded to float32: off by up to two samples of a sine of period 100
    p32 = (idx.astype(np.float32) / np.float32(ratio)).astype(np.float64)
    e32 = rel(orc.resample_sinc(x, ratio, idx=idx, pos=p32), ref)
    print("resample near sample 2^25: fp64 positions", e, "float32 positions", e32)
    assert e < 1e-5 and e32 > 1e-3


# ---- 5. end to end
@pytest.mark.parametrize("rate", cases.RATES)
@pytest.mark.parametrize("name", cases.END_TO_END)
def test_time_stretch_end_to_end(pv, name, rate):
    y = run(pv, name, rate)[0]
    ref = cases.stretched(name, rate)
    assert y.shape == ref.shape == (int(round(cases.signal(name).shape[0] / rate)),)
    e, f32 = rel(y, ref), cases.f32_figure(name, rate)
    print(name, rate, "time_stretch: device", e, "float32 mode", f32)
    assert e <= 8 * f32 and e < 1e-4


@pytest.mark.parametrize("n_steps", cases.STEPS)
@pytest.mark.parametrize("name", cases.END_TO_END)
def test_pitch_shift_end_to_end(pv, name, n_steps):
    y = run_pitch(pv, name, n_steps)[0]
    ref = cases.shifted(name, n_steps)
    assert y.shape == ref.shape == cases.signal(name).shape and y.dtype == np.float32
    e, f32 = rel(y, ref), cases.f32_figure_pitch(name, n_steps)
    print(name, n_steps, "pitch_shift: device", e, "float32 mode", f32)
    assert e <= 8 * f32 and e < 1e-4


def test_pitch_shift_stages(pv):
    y, taps = run_pitch(pv, "noise_chirp", 3)
    rate = 2.0 ** (-3 / 12)
    check_vocoder(taps["spec"], taps["stretched"], rate, "pitch +3")
    ref = orc.fix_length(orc.resample_sinc(taps["synth"], rate), y.shape[0])
    assert rel(y, ref) < 1e-5


# ---- 6. identity
@pytest.mark.parametrize("name", cases.ALL)
def test_rate_one_is_the_identity(pv, name):
    x = cases.signal(name)
    y = run(pv, name, 1.0)[0]
    assert y.shape == x.shape
    e = rel(y, x)
    print(name, "time_stretch(x, 1) vs x", e)
    assert e < 1e-5


# ---- 7. shapes and determinism
def test_channels_are_bit_identical_to_single_calls(pv):
    names = ["noise_chirp", "harmonic", "gapped"]
    x = np.stack([cases.signal(n) for n in names])
    y = pv.time_stretch(x, 0.8)
    z = pv.pitch_shift(x, cases.SR, 3)
    assert y.shape == (3, 30000) and z.shape == x.shape
    for c, n in enumerate(names):
        assert np.array_equal(y[c], run(pv, n, 0.8)[0]), n
        assert np.array_equal(z[c], run_pitch(pv, n, 3)[0]), n


def test_a_grown_workspace_changes_nothing(pv):
    run(pv, "long", 0.5)                                  # the fixture's workspace has grown
    fresh = effects.PhaseVocoder("cuda:0")
    try:
        for name in ("odd", "tiny"):
            assert np.array_equal(pv.time_stretch(cases.signal(name), 0.8), fresh.time_stretch(cases.signal(name), 0.8))
            assert np.array_equal(pv.pitch_shift(cases.signal(name), cases.SR, -4), fresh.pitch_shift(cases.signal(name), cases.SR, -4))
    finally:
        fresh.close()


def test_close_and_budget():
    from targetdiarization_amd._lib import TdxError
    p = effects.PhaseVocoder("cuda:0", workspace_budget_bytes=1 << 20)
    with pytest.raises(TdxError, match=r"workspace of \d+ bytes; the budget is 1048576"):
        p.time_stretch(cases.signal("noise_chirp"), 0.8)
    assert p.resample(cases.signal("tiny"), 1.0).shape == (100,)
    p.close()
    p.close()
    for call in (lambda: p.time_stretch(cases.signal("tiny"), 0.8), lambda: p.pitch_shift(cases.signal("tiny"), cases.SR, 1),
                 lambda: p.resample(cases.signal("tiny"), 0.9), lambda: p.eq_match(cases.signal("odd"), cases.signal("odd")),
                 lambda: p.phase_vocoder(random_spectrum(4, 0), 0.8)):
        with pytest.raises(TdxError):
            call()


def test_bad_arguments(pv):
    from targetdiarization_amd._lib import TdxError
    with pytest.raises(ValueError):
        pv.time_stretch(cases.signal("tiny"), -1.0)
    with pytest.raises(ValueError):
        pv.time_stretch(np.zeros((2, 2, 2), np.float32), 1.0)
    with pytest.raises(TdxError, match="n_fft must be a multiple of 128"):
        pv.eq_match(cases.signal("odd"), cases.signal("odd"), n_fft=1000, hop_length=250)
    with pytest.raises(TdxError, match="hop_length a multiple of 4"):
        pv.eq_match(cases.signal("odd"), cases.signal("odd"), n_fft=1024, hop_length=250)
    with pytest.raises(TdxError, match="ratio must lie in"):
        pv.resample(cases.signal("tiny"), 1000.0)


# ---- 8. eq_match
def check_gain(taps, target_stft):
    ms, mt = np.abs(taps["spec"].astype(np.complex128)).mean(axis=1), np.abs(np.asarray(target_stft).astype(np.complex128)).mean(axis=1)
    assert np.abs(taps["mean_source"] - ms).max() <= 4 * EPS * ms.max()      # fp64 sums of float32 hypots
    assert np.abs(taps["mean_target"] - mt).max() <= 4 * EPS * mt.max()
    g = taps["gain"]
    assert g.min() >= np.float32(0.1) and g.max() <= 10
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = mt / ms
    away = (np.abs(ratio - 0.1) > 1e-4) & (np.abs(ratio - 10) > 1e-4) & (ms > 0)
    ref = np.clip(ratio, 0.1, 10)
    assert away.sum() > 0.9 * g.shape[0]
    assert np.all(g[~away & (ratio < 1)] < 0.1001) and np.all(g[~away & (ratio > 1)] > 9.999)
    assert (np.abs(g[away] - ref[away]) / ref[away]).max() < 1e-5
    return g


@pytest.mark.parametrize("n_fft,hop", [(2048, 512), (512, 128), (1024, 256), (4096, 1024), (1024, 512), (384, 96)])
def test_eq_match(pv, n_fft, hop):
    src, tgt = cases.signal("noise_chirp"), cases.signal("harmonic")
    St = orc.stft(tgt, n_fft, hop).astype(np.complex64)
    taps = {}
    y = pv.eq_match(src, target_stft=St, n_fft=n_fft, hop_length=hop, taps=taps)
    assert y.shape == (hop * (src.shape[0] // hop),) and y.dtype == np.float32
    assert cases.analysis_error(taps["spec"], orc.stft(src, n_fft, hop)) < 1e-5
    g = check_gain(taps, St)
    ref = orc.istft(taps["spec"].astype(np.complex128) * g[:, None].astype(np.float64), hop)
    e = rel(y, ref, den=src.astype(np.float64))
    print(n_fft, hop, "eq_match stage", e)
    assert e < 1e-4
    # the target as samples, against the oracle end to end
    y2 = pv.eq_match(src, target=tgt, n_fft=n_fft, hop_length=hop)
    e2 = rel(y2, orc.eq_match(src, tgt, n_fft=n_fft, hop=hop)[0], den=src.astype(np.float64))
    print(n_fft, hop, "eq_match end to end", e2)
    assert e2 < 1e-4


def test_eq_match_to_itself_is_the_round_trip(pv):
    src = cases.signal("noise_chirp")
    taps = {}
    y = pv.eq_match(src, target=src, taps=taps)
    assert np.array_equal(taps["gain"], np.ones(1025, np.float32))
    assert rel(y, src[:y.shape[0]]) < 1e-5
    assert np.array_equal(y, pv.istft(taps["spec"]))


def test_eq_match_zero_means_stay_finite(pv):
    tgt = cases.signal("harmonic")
    taps = {}
    y = pv.eq_match(np.zeros(5000, np.float32), target=tgt, taps=taps)          # every source mean is exactly 0: gain 10, output 0
    assert np.all(taps["mean_source"] == 0) and np.all(taps["gain"] == 10) and np.all(y == 0)
    St = orc.stft(tgt).astype(np.complex64)
    St[100:200] = 0                                                              # a band of exact zeros in the target: gain 0.1
    y = pv.eq_match(cases.signal("noise_chirp"), target_stft=St, taps=taps)
    assert np.all(taps["mean_target"][100:200] == 0) and np.all(taps["gain"][100:200] == np.float32(0.1)) and np.isfinite(y).all()


# ---- 9. the reference's surface
@pytest.fixture(scope="module")
def ap():
    from targetdiarization_amd.audio_processor import AudioProcessor
    return AudioProcessor(cuda_device=0, verbose_log=True)


def test_audio_processor_stretch_and_pitch(pv, ap, capsys):
    x = cases.signal("noise_chirp")
    y = ap.audio_stretch(x, cases.SR, 0.8)
    out = capsys.readouterr().out
    assert "Running module: audio_stretch" in out and "Speed factor: 0.8" in out
    assert np.array_equal(y, run(pv, "noise_chirp", 0.8)[0])
    z = ap.audio_pitch(x, cases.SR, 3)
    assert "Running module: audio_pitch" in capsys.readouterr().out
    assert np.array_equal(z, run_pitch(pv, "noise_chirp", 3)[0])
    st = np.stack([x, cases.signal("harmonic")], axis=1)                         # [n, 2]
    y2, z2 = ap.audio_stretch(st, cases.SR, 0.8), ap.audio_pitch(st, cases.SR, 3)
    assert y2.shape == (30000, 2) and z2.shape == st.shape and y2.dtype == z2.dtype == np.float32
    for c, name in enumerate(("noise_chirp", "harmonic")):
        assert rel(y2[:, c], cases.stretched(name, 0.8)) <= 8 * cases.f32_figure(name, 0.8)
        assert rel(z2[:, c], cases.shifted(name, 3)) <= 8 * cases.f32_figure_pitch(name, 3)


def test_audio_processor_skip_paths(ap, capsys):
    from targetdiarization_amd.audio_processor import AudioProcessor
    x = cases.signal("odd")
    assert ap.audio_stretch(x, cases.SR, 0.0) is x and "Speed factor is zero. Skip." in capsys.readouterr().out
    assert ap.audio_pitch(x, cases.SR, 0.0) is x and "Pitch semitone is zero. Skip." in capsys.readouterr().out
    assert ap.audio_stretch(x, cases.SR, -1.5) is x and "not positive" in capsys.readouterr().out
    assert ap.eq_match(x, "target.wav") is x and "file name" in capsys.readouterr().out
    assert ap.eq_match(x, "target.pkl") is x and "file name" in capsys.readouterr().out
    st = np.stack([x, x], axis=1)
    assert ap.eq_match(st, x) is st and "mono" in capsys.readouterr().out
    cpu = AudioProcessor(cuda_device=-1, verbose_log=False)
    for got in (cpu.audio_stretch(x, cases.SR, 0.8), cpu.audio_pitch(x, cases.SR, 3), cpu.eq_match(x, x)):
        assert got is x
    assert capsys.readouterr().out.count("no device") == 3
    for name in ("audio_stretch", "audio_pitch", "eq_match"):                     # run_modules dispatches by name (:284-292)
        assert callable(getattr(ap, name))


def test_audio_processor_eq_match(ap, capsys):
    src, tgt = cases.signal("noise_chirp"), cases.signal("harmonic")
    ref = orc.eq_match(src, tgt)[0]
    y = ap.eq_match(src, tgt)
    out = capsys.readouterr().out
    assert "Running module: eq_match" in out and "FFT window size: 2048" in out and "Hop length: 512" in out
    assert rel(y, ref, den=src.astype(np.float64)) < 1e-4
    St = orc.stft(tgt, 1024, 256).astype(np.complex64)
    y = ap.eq_match(src, dict(stft=St, sampling_rate=16000, n_fft=1024, hop_length=256))
    assert rel(y, orc.eq_match(src, target_stft=St, n_fft=1024, hop=256)[0], den=src.astype(np.float64)) < 1e-4
    y = ap.eq_match(src, dict(array=tgt, n_fft=1024, hop_length=4096))            # hop_length > n_fft -> n_fft / 4 (:519-520)
    assert "Hop length: 256" in capsys.readouterr().out
    assert rel(y, orc.eq_match(src, tgt, n_fft=1024, hop=256)[0], den=src.astype(np.float64)) < 1e-4
    # the three sampling-rate branches (:525-545)
    for target_sr, target in ((8000, dict(stft=St, sampling_rate=8000, n_fft=1024, hop_length=256)), (8000, tgt), (32000, tgt),
                              (32000, dict(stft=St, sampling_rate=32000, n_fft=1024, hop_length=256))):
        y = ap.eq_match(src, target, source_sampling_rate=16000, target_sampling_rate=target_sr)
        assert "Failed" not in capsys.readouterr().out
        assert y is not src and y.ndim == 1 and np.isfinite(y).all() and abs(y.shape[0] - src.shape[0]) <= 2048
