"""The inputs of the phase-vocoder tests, shared by test_pvoc_host.py (CPU) and test_gpu_pvoc.py, and the float64 / float32-mode
oracle results they compare against (computed once per process).

Two recipes differ from the first draft of the table, because the draft failed the conditioning check of test_pvoc_host.py (the
oracle's float32 mode must stay within 1.25e-5 rel-L2 of its float64 mode at every rate; an input that does not is replaced):
  * `noise_chirp` (and `gapped`, cut from it): the chirp's amplitude is 0.1, not 0.5.  At 0.5 the rounding of the loud chirp in a
    float32 analysis moved the phase of the noise bins next to it: 1.3e-5 to 1.6e-5 at the rates 0.8 and 1.25; at 0.1: 3e-6.
  * `long`: five steady partials (150 h Hz, 0.3 / h) over 1e-2 N(0, 1), not the recipe of `noise_chirp`.  The float32 analysis
    error enters every frame's phase increment and the running sum carries it on, so the figure grows with the number of
    frames: at this length `noise_chirp`'s recipe gives 1.05e-5 and `harmonic`'s 1.4e-5 at rate 0.8, this one 4.3e-6."""
import functools

import numpy as np

import pvoc_oracle as orc
from targetdiarization_amd import effects

SR = 16000
RATES = [0.8, 1.25, 2.0 ** (3 / 12), 0.5, 1.0]
STEPS = [3, -4, 0.5]
END_TO_END = ["noise_chirp", "harmonic", "gapped", "long"]      # well-conditioned (test_pvoc_host.py shows it); `tone` is not
ALL = END_TO_END + ["tone", "tiny", "odd"]
# T and T' (rate 0.5: 2 T) both beyond one sweep of the scan's segment slots and no multiple of the segment length
LONG_N = 512 * (effects.SWEEP + 4) + 137
assert (1 + LONG_N // 512) > effects.SWEEP and (1 + LONG_N // 512) % effects.SEG and (2 * (1 + LONG_N // 512)) % effects.SEG


def _noise_chirp(n, seed):
    t = np.arange(n) / SR
    return 0.1 * np.random.default_rng(seed).standard_normal(n) + 0.1 * np.sin(2 * np.pi * (200 * t + 300 * t * t))


def _harmonic(n, seed, partials=20, noise=1e-3):
    t = np.arange(n) / SR
    return sum(0.3 / h * np.sin(2 * np.pi * 150 * h * t) for h in range(1, partials)) + noise * np.random.default_rng(seed).standard_normal(n)


@functools.lru_cache(maxsize=None)
def signal(name):
    n = 24000
    t = np.arange(n) / SR
    if name == "noise_chirp":
        x = _noise_chirp(n, 1)
    elif name == "harmonic":
        x = _harmonic(n, 2)
    elif name == "gapped":
        x = _noise_chirp(n, 1).copy()
        x[8000:14000] = 0.0
    elif name == "tone":
        x = 0.5 * np.sin(2 * np.pi * 440 * t)
    elif name == "long":
        x = _harmonic(LONG_N, 3, partials=6, noise=1e-2)
    elif name == "tiny":
        x = 0.1 * np.random.default_rng(4).standard_normal(100)
    elif name == "odd":
        x = 0.1 * np.random.default_rng(5).standard_normal(5003)
    else:
        raise KeyError(name)
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def spectrum(name, f32=False):
    return orc.stft(signal(name), dtype=np.float32 if f32 else np.float64)


@functools.lru_cache(maxsize=None)
def stretched(name, rate, f32=False):
    """the oracle's time_stretch of `name` (float64 result; f32: from the float32-mode analysis)"""
    return orc.time_stretch(signal(name), rate, D=spectrum(name, f32))


@functools.lru_cache(maxsize=None)
def shifted(name, n_steps, f32=False):
    return orc.pitch_shift(signal(name), n_steps, D=spectrum(name, f32))


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def f32_figure(name, rate):
    """rel-L2 between the oracle's float32 mode and its float64 mode on time_stretch(name, rate)"""
    return rel(stretched(name, rate, True), stretched(name, rate))


@functools.lru_cache(maxsize=None)
def f32_figure_pitch(name, n_steps):
    return rel(shifted(name, n_steps, True), shifted(name, n_steps))


@functools.lru_cache(maxsize=None)
def f32_analysis_figure(name):
    """the largest error of the float32-mode analysis over a frame, relative to the frame's largest |value|"""
    return analysis_error(spectrum(name, True), spectrum(name))


def analysis_error(D, D64):
    """largest |D - D64| over a frame relative to the frame's largest |D64|, at its worst frame; an all-zero frame must be exact"""
    err, top = np.abs(D - D64).max(axis=0), np.abs(D64).max(axis=0)
    assert np.all(err[top == 0] == 0)
    return float((err[top > 0] / top[top > 0]).max())
