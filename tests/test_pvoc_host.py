"""CPU tests of the phase-vocoder oracle (tests/pvoc_oracle.py) and the host plans (effects.stretch_plan / pitch_plan): the oracle's
STFT / iSTFT are pinned to torch's in float64, its identities hold, and the inputs of the GPU end-to-end checks are shown to be
well-conditioned (and `tone` to be not) for the oracle alone."""
import math
import os
import re

import numpy as np
import pytest
import torch

import pvoc_cases as cases
import pvoc_oracle as orc
from targetdiarization_amd import effects

N_FFT, HOP = 2048, 512


def t_stft(x):
    w = torch.hann_window(N_FFT, periodic=True, dtype=torch.float64)
    return torch.stft(torch.from_numpy(np.asarray(x, dtype=np.float64)), N_FFT, HOP, window=w, center=True, pad_mode="constant", return_complex=True)


@pytest.mark.parametrize("name", ["noise_chirp", "odd", "tiny"])
def test_stft_is_torch_stft(name):
    x = cases.signal(name)
    ref = t_stft(x).numpy()
    got = orc.stft(x)
    assert got.shape == ref.shape == (1025, 1 + x.shape[0] // HOP)
    err = np.abs(got - ref).max()
    print(name, "stft vs torch", err)
    assert err < 1e-9


@pytest.mark.parametrize("name,length", [("noise_chirp", None), ("noise_chirp", 23000), ("odd", 5003), ("odd", None)])
def test_istft_is_torch_istft(name, length):
    D = t_stft(cases.signal(name))
    w = torch.hann_window(N_FFT, periodic=True, dtype=torch.float64)
    ref = torch.istft(D, N_FFT, HOP, window=w, center=True, length=length).numpy()
    got = orc.istft(D.numpy(), length=length)
    assert got.shape == ref.shape
    err = np.abs(got - ref).max()
    print(name, length, "istft vs torch", err)
    assert err < 1e-12


def test_istft_with_a_length_that_cuts_frames():
    D = orc.stft(cases.signal("noise_chirp"))
    full = orc.istft(D)
    cut = orc.istft(D, length=3000)          # ceil((3000 + 2048) / 512) = 10 of 47 frames
    assert cut.shape == (3000,)
    assert np.abs(cut[:2500] - full[:2500]).max() < 1e-12      # samples whose frames are all among the 10


def test_round_trip_identity():
    x = cases.signal("noise_chirp").astype(np.float64)
    y = orc.istft(orc.stft(x))
    assert y.shape[0] == HOP * (x.shape[0] // HOP)
    assert np.abs(y - x[:y.shape[0]]).max() < 1e-12


@pytest.mark.parametrize("name", cases.ALL)
def test_rate_one_is_the_identity(name):
    x = cases.signal(name).astype(np.float64)
    y = cases.stretched(name, 1.0)
    assert y.shape == x.shape
    err = np.linalg.norm(y - x)
    print(name, "time_stretch(x, 1) - x", err / np.linalg.norm(x))
    assert err <= 1e-9 * np.linalg.norm(x)


def test_resample_at_ratio_one_is_the_identity():
    x = cases.signal("odd").astype(np.float64)
    assert np.abs(orc.resample_sinc(x, 1.0) - x).max() < 1e-12


@pytest.mark.parametrize("n_steps", cases.STEPS)
def test_pitch_shift_moves_a_tone(n_steps):
    x = cases.signal("tone")
    y = cases.shifted("tone", n_steps)
    assert y.shape == x.shape
    spec = np.abs(np.fft.rfft(y * np.hanning(y.shape[0])))
    peak = np.argmax(spec) * cases.SR / y.shape[0]
    want = 440.0 * 2.0 ** (n_steps / 12)
    print(n_steps, "peak", peak, "want", want)
    assert abs(peak - want) <= cases.SR / N_FFT          # one bin of the 2048-point transform


@pytest.mark.parametrize("n", [100, 5003, 24000, cases.LONG_N])
@pytest.mark.parametrize("rate", cases.RATES)
def test_stretch_plan(n, rate):
    p = effects.stretch_plan(n, rate)
    T = 1 + n // HOP
    steps = np.arange(0, T, rate)
    assert p["T"] == T and p["T_out"] == steps.shape[0] == math.ceil(T / rate)
    assert np.array_equal(p["idx"], [int(s) for s in steps]) and p["idx"].dtype == np.int32
    assert np.array_equal(p["alpha"], np.mod(steps, 1.0)) and p["alpha"].dtype == np.float64
    assert p["length"] == int(round(n / rate))
    assert p["idx"].max() < T


@pytest.mark.parametrize("n", [100, 5003, 24000])
@pytest.mark.parametrize("n_steps", cases.STEPS)
def test_pitch_plan(n, n_steps):
    p = effects.pitch_plan(n, n_steps)
    rate = 2.0 ** (-n_steps / 12)
    s = effects.stretch_plan(n, rate)
    assert p["rate"] == rate == p["ratio"] and p["length"] == s["length"] and np.array_equal(p["idx"], s["idx"])
    assert p["n_out"] == math.ceil(s["length"] * rate) and p["n_final"] == n
    assert orc.resample_sinc(np.zeros(s["length"]) + 1.0, rate).shape[0] == p["n_out"]


def test_plans_reject_bad_arguments():
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            effects.stretch_plan(1000, bad)
    with pytest.raises(ValueError):
        effects.stretch_plan(0, 1.0)
    with pytest.raises(ValueError):
        effects.pitch_plan(1000, 3, bins_per_octave=0)


def test_scan_constants_match_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "tdx.h")).read()
    assert int(re.search(r"#define TDX_PVOC_SEG (\d+)", txt).group(1)) == effects.SEG
    assert int(re.search(r"#define TDX_PVOC_SLOTS (\d+)", txt).group(1)) == effects.SLOTS
    T = 1 + cases.LONG_N // HOP
    assert T > effects.SWEEP and T % effects.SEG and (2 * T) % effects.SEG


@pytest.mark.parametrize("name", cases.END_TO_END)
def test_end_to_end_inputs_are_well_conditioned(name):
    """the float32-mode oracle within 1.25e-5 rel-L2 of the float64 one, so that 8x stays under the 1e-4 cap of test_gpu_pvoc.py"""
    for rate in cases.RATES:
        f = cases.f32_figure(name, rate)
        print(name, "rate", rate, "float32 mode vs float64", f)
        assert f <= 1.25e-5
    for n_steps in cases.STEPS:
        f = cases.f32_figure_pitch(name, n_steps)
        print(name, "steps", n_steps, "float32 mode vs float64", f)
        assert f <= 1.25e-5


def test_tone_is_not_well_conditioned():
    """bins at the float32 noise floor carry an arbitrary phase: the documented sensitivity, and why `tone` is left out end to end"""
    f = cases.f32_figure("tone", 0.8)
    print("tone float32 mode vs float64", f)
    assert f > 1e-4


def test_eq_match_oracle():
    src, tgt = cases.signal("noise_chirp"), cases.signal("harmonic")
    y, ms, mt, g = orc.eq_match(src, tgt)
    assert g.min() >= 0.1 and g.max() <= 10 and (g == 0.1).any() and ((g > 0.1) & (g < 10)).any()
    same, _, _, g1 = orc.eq_match(src, src)
    assert np.array_equal(g1, np.ones_like(g1))
    assert np.abs(same - orc.istft(orc.stft(src))).max() < 1e-12
    # a source whose band is exactly zero: the guarded gain is 10 and the result finite; upstream's formula is NaN there
    S = orc.stft(src).copy()
    S[100:200] = 0
    yz, msz, _, gz = orc.eq_match(target=tgt, source_stft=S)
    assert np.all(msz[100:200] == 0) and np.all(gz[100:200] == 10) and np.isfinite(yz).all()
    yn, _, _, gn = orc.eq_match(target_stft=np.where(np.arange(1025)[:, None] < 150, 0, orc.stft(tgt)), source_stft=S, guard=False)
    assert np.isnan(gn[100:150]).all() and np.isnan(yn).any()


def test_c_abi_rejects_bad_arguments_without_a_device():
    from targetdiarization_amd import _lib
    l = _lib.lib()
    for n, r in ((100, 0.5), (24000, 2.0 ** (-3 / 12)), (30000, 2.0 ** (4 / 12)), (5003, 1.0)):
        assert l.tdx_resample_sinc_length(n, r) == math.ceil(n * r)
    assert l.tdx_resample_sinc_length(0, 1.0) == 0 and l.tdx_resample_sinc_length(10, -1.0) == 0
    assert l.tdx_pvoc_workspace_bytes(None, 2048, 512, 1, 1000, 10) == 0
    assert l.tdx_resample_sinc(None, 1, 10, 1.0, None, 10, None) != 0 and b"null argument" in l.tdx_last_error()
    assert l.tdx_pvoc_prepare(None, 2048) != 0 and b"null argument" in l.tdx_last_error()
    assert l.tdx_pvoc_stretch(None, None, 1, 10, None, None, None, 1, 10, None, None, None, None, 0, None) != 0
    assert l.tdx_pvoc_vocode(None, None, 1025, 4, 512, None, None, None, 5, None, None) != 0
    assert l.tdx_pvoc_istft(None, None, 4, 2048, 512, -1, None, None, 0, None) != 0
    assert l.tdx_pvoc_eq_match(None, None, 10, None, 10, None, 0, 2048, 512, None, None, None, None, None, None, 0, None) != 0
