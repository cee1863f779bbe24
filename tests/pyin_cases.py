"""The inputs the pyin tests share: every signal and observation matrix the device tests (test_gpu_pyin.py) name is listed here, and
the CPU tests (test_pyin_host.py) assert the input conditions on exactly this list, so that a device test cannot hide a failure
behind a frame it does not compare.  Oracle results are computed once per process and never modified."""
import functools

import numpy as np

import pyin_oracle as orc

DEFAULT = dict(sr=16000, fmin=50.0, fmax=300.0)
GEOMETRY_N = [1, 511, 512, 513, 2048, 16000, 3 * 16000 + 123]

# name -> (oracle parameters, samples, seed).  No seed had to be replaced to meet the conditions of test_pyin_host.py.
SIGNALS = {f"n{n}": (DEFAULT, n, n) for n in GEOMETRY_N}
SIGNALS.update({
    "sr8000": (dict(sr=8000, fmin=50.0, fmax=300.0), 6000, 1),                       # width 281 of 311 bins
    "sr22050_wide": (dict(sr=22050, fmin=65.4, fmax=2093.0), 8000, 2),               # 601 bins, min_period 10
    "sr44100_4096": (dict(sr=44100, fmin=50.0, fmax=300.0, frame_length=4096), 8000, 3),
    "no_center": (dict(DEFAULT, center=False), 8000, 4),
    "fill_none": (DEFAULT, 7000, 5),
    "long20s": (DEFAULT, 20 * 16000, 1),
})
# One sample alone in its frame: d[tau] is that sample squared for every lag, yin is 1 everywhere, and which rows come out as troughs
# is decided by the last bit of the arithmetic — in upstream, in the oracle and on the device alike.  The frame is not robust by
# construction; what holds for it is yin = 1 (compared), voiced_prob <= no_trough_prob and an unvoiced path.
DEGENERATE = {"n1", "batch2"}

for _k in range(5):                                                                   # the batch test's clips
    SIGNALS[f"batch{_k}"] = (DEFAULT, [700, 5000, 1, 12345, 2049][_k], 10 + _k)


@functools.lru_cache(maxsize=None)
def plan(name):
    return orc.params(**SIGNALS[name][0])


@functools.lru_cache(maxsize=None)
def signal(name):
    kw, n, seed = SIGNALS[name]
    y = orc.voiced_signal(n, kw["sr"], seed=seed)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 oracle, flush=False (what the device is compared with): dict of yin, shifts, obs, vp, states, f0, voiced, robust"""
    P, y = plan(name), signal(name)
    yin, sh = orc.yin_shifts(y, P, flush=False)
    obs, vp = orc.observation(yin, sh, P)
    states = orc.viterbi_dense(obs, P)
    f0 = P.freqs[states % P.npb]
    r = dict(yin=yin, shifts=sh, obs=obs, vp=vp, states=states, f0=f0, voiced=states < P.npb,
             robust=orc.robust_frames(y, P, seed=0, yin_sh=(yin, sh)))
    for v in r.values():
        v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def fp32_mode(name):
    """the oracle's float32 direct-difference mode -> (yin, shifts, obs)"""
    P, y = plan(name), signal(name)
    yin, sh = orc.yin_shifts(y, P, dtype=np.float32, direct=True)
    return yin, sh, orc.observation(yin, sh, P)[0]


def frame_rel_err(a, ref):
    """largest |a - ref| of each frame relative to the frame's largest |ref| (1 where the frame is all zero): [n_lags, T] -> [T]"""
    mx = np.max(np.abs(ref), axis=0)
    return np.max(np.abs(np.asarray(a, np.float64) - ref), axis=0) / np.where(mx == 0, 1.0, mx)


# ---- observation matrices for the decoding stage alone (16 kHz defaults: 622 states, width 141)
VITERBI_T = [1, 2, 3, 300]


@functools.lru_cache(maxsize=None)
def random_obs(T, seed=None, density=0.03):
    """sparse random voiced rows (a few candidates per frame, total probability <= 1) with pyin's uniform unvoiced rows -> [S, T]"""
    P = orc.params(**DEFAULT)
    r = np.random.default_rng(T if seed is None else seed)
    o = np.zeros((2 * P.npb, T))
    m = r.uniform(size=(P.npb, T)) < density
    o[:P.npb][m] = r.uniform(size=int(m.sum()))
    tot = o[:P.npb].sum(0)
    o[:P.npb] *= np.where(tot > 1, r.uniform(0.5, 1, size=T) / np.maximum(tot, 1e-30), 1.0)
    o[P.npb:] = (1 - np.clip(o[:P.npb].sum(0), 0, 1)) / P.npb
    o = o.astype(np.float32).astype(np.float64)                # what the device is given, exactly
    o.setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def jump_obs(T):
    """voiced_prob exactly 1 (the unvoiced rows are 0): one candidate at bin 0 in even frames, at the top bin in odd ones, so every
    step is a jump of 310 bins past a band of 70"""
    P = orc.params(**DEFAULT)
    o = np.zeros((2 * P.npb, T))
    for t in range(T):
        o[0 if t % 2 == 0 else P.npb - 1, t] = 1.0
    o.setflags(write=False)
    return o
