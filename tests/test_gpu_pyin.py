"""pYIN on the device (pitch.Pyin, csrc/pyin.hip) against the float64 restatement (tests/pyin_oracle.py, flush=False).  Every input is
listed in tests/pyin_cases.py, where the CPU tests assert the conditions these comparisons rest on (test_pyin_host.py).

yin taps: the largest error of a frame, relative to the frame's largest value, is at most 8 x what the oracle's float32 mode shows on
the same input (the factor covers another summation order over the 1024 terms) and below 2.5e-6; per value it is below 1e-5, the
perturbation that defines a robust frame (bound: 8 partial sums of 128 non-negative terms, a pairwise combine, a chunked running
sum and two divisions are under 160 roundings of 2^-24 = 9.5e-6).  shift taps: -b / a is ill-conditioned wherever the curvature a
is small, so no float32 yin reproduces the float64 shifts there to 2.5e-6; asserted instead: the device's shifts are bit for bit
the float32 parabola of the device's own yin, and on the rows whose |a| and whose distance from the |b| < |a| edge are at least 1e-2
of the frame's largest yin value they are within 8 x the float32 mode's error on those rows (plus 1e-6 absolute).
Paths: an unvoiced stretch has many equally likely paths (test_pyin_host.py, "Ties"), so what is compared is what can be seen — the
voiced flag of every frame, the state of every voiced frame — and the float64 score of the device's path."""
import numpy as np
import pytest

import pyin_cases as cases
import pyin_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pyin():
    from targetdiarization_amd.pitch import Pyin
    p = Pyin("cuda:0")
    yield p
    p.close()


_runs = {}


def run(pyin, name, **extra):
    """one device call per input and process: (f0, voiced, vp, taps)"""
    key = (name, tuple(sorted(extra.items())))
    if key not in _runs:
        kw = dict(cases.SIGNALS[name][0])
        taps = {}
        f0, v, vp = pyin.pyin(cases.signal(name), taps=taps, **kw, **extra)
        _runs[key] = (f0, v, vp, taps)
    return _runs[key]


def parabola32(x):
    """the float32 parabolic shifts of x [T, n_lags], operation by operation as the kernel"""
    x = np.asarray(x, np.float32)
    sh = np.zeros_like(x)
    xm, x0, xp = x[:, :-2], x[:, 1:-1], x[:, 2:]
    a = (xm + xp) - np.float32(2) * x0
    b = (xp - xm) * np.float32(0.5)
    ok = np.abs(b) < np.abs(a)
    with np.errstate(divide="ignore", invalid="ignore"):
        sh[:, 1:-1] = np.where(ok, -b / np.where(ok, a, np.float32(1)), np.float32(0))
    return sh


def check_taps(name, taps):
    P, ref = cases.plan(name), cases.reference(name)
    yin32, sh32, _ = cases.fp32_mode(name)
    yin, sh = taps["yin"].T, taps["shifts"].T
    assert yin.shape == ref["yin"].shape and yin.dtype == np.float32
    e_dev = float(np.max(cases.frame_rel_err(yin, ref["yin"])))
    e_32 = float(np.max(cases.frame_rel_err(yin32, ref["yin"])))
    nz = ref["yin"] != 0
    e_val = float(np.max(np.abs(yin.astype(np.float64) - ref["yin"])[nz] / ref["yin"][nz])) if nz.any() else 0.0
    print(f"{name}: yin err / frame max: device {e_dev:.3e}, float32 mode {e_32:.3e}, ratio {e_dev / max(e_32, 1e-30):.3f}; per value {e_val:.3e}")
    assert e_dev <= 8 * e_32 and e_dev < 2.5e-6
    assert e_val < 1e-5 and np.all(yin[~nz] == 0)
    assert np.array_equal(sh, parabola32(yin.T).T)
    x = ref["yin"]
    a = np.zeros_like(x)
    a[1:-1] = np.abs((x[:-2] + x[2:]) - 2 * x[1:-1])
    b = np.zeros_like(x)
    b[1:-1] = np.abs(x[2:] - x[:-2]) / 2
    mx = np.max(np.abs(x), axis=0, keepdims=True)
    well = (a >= 1e-2 * mx) & (np.abs(a - b) >= 1e-2 * mx)        # (|b| < |a| decides between -b / a and 0: not near that edge either)
    well[[0, -1]] = False
    if well.any():
        s_dev = float(np.max(np.abs(sh - ref["shifts"])[well]))
        s_32 = float(np.max(np.abs(sh32 - ref["shifts"])[well]))
        print(f"{name}: shift err on {int(well.sum())} well-conditioned rows: device {s_dev:.3e}, float32 mode {s_32:.3e}")
        assert s_dev <= 8 * s_32 + 1e-6


def check_obs(name, taps, vp):
    ref = cases.reference(name)
    rb = ref["robust"]
    obs = taps["obs"].T.astype(np.float64)
    err = np.max(np.abs(obs - ref["obs"]), axis=0)
    print(f"{name}: obs err on {int(rb.sum())} robust frames of {len(rb)}: {err[rb].max() if rb.any() else 0.0:.3e}; "
          f"columns that differ among the others: {int((err[~rb] > 1e-6).sum())}")
    assert np.all(err[rb] <= 1e-6)
    assert np.all(np.abs(vp - ref["vp"])[rb] <= 1e-6)
    return rb


def check_path(name, f0, voiced, vp, taps, fill_nan=True):
    """the device's path against the oracle's; where a frame is not robust the device decodes its own column, so then the reference
    path is the oracle's decoding of the device's observation taps"""
    P, ref = cases.plan(name), cases.reference(name)
    obs_dev = taps["obs"].T.astype(np.float64)
    want = ref["states"] if ref["robust"].all() else orc.viterbi_dense(obs_dev, P)
    wv = want < P.npb
    st = taps["states"]
    assert np.array_equal(voiced, wv) and np.array_equal(st[wv], want[wv])
    wf0 = P.freqs[want % P.npb]
    if fill_nan:
        assert np.all(np.isnan(f0[~wv])) and np.array_equal(f0[wv], wf0[wv])
    a, b = orc.score(st, obs_dev, P), orc.score(want, obs_dev, P)
    print(f"{name}: score of the device's path {a:.12g}, optimum {b:.12g}")
    assert abs(a - b) <= 1e-9 * abs(b)


# ---------------------------------------------------------------- geometry
@pytest.mark.parametrize("n", cases.GEOMETRY_N)
def test_geometry(pyin, n):
    name = f"n{n}"
    f0, voiced, vp, taps = run(pyin, name)
    T = 1 + n // 512
    assert f0.shape == voiced.shape == vp.shape == (T,)
    assert f0.dtype == np.float64 and voiced.dtype == bool and vp.dtype == np.float64
    check_taps(name, taps)
    if name in cases.DEGENERATE:
        assert vp[0] <= 0.01 + 1e-6 and not voiced[0] and np.isnan(f0[0])
        return
    check_obs(name, taps, vp)
    check_path(name, f0, voiced, vp, taps)


# ---------------------------------------------------------------- parameters
@pytest.mark.parametrize("name", ["sr8000", "sr22050_wide", "sr44100_4096", "no_center"])
def test_parameters(pyin, name):
    f0, voiced, vp, taps = run(pyin, name)
    assert f0.shape == (cases.reference(name)["yin"].shape[1],)
    check_taps(name, taps)
    check_obs(name, taps, vp)
    check_path(name, f0, voiced, vp, taps)


def test_fill_na_none(pyin):
    """fill_na=None keeps the frequency of the unvoiced state: equal to the oracle's wherever the frame is voiced, a bin frequency
    everywhere (the unvoiced states of a tied stretch are not comparable)"""
    name = "fill_none"
    P = cases.plan(name)
    f0, voiced, vp, taps = run(pyin, name, fill_na=None)
    assert not np.isnan(f0).any() and np.all(np.isin(f0, P.freqs))
    assert np.array_equal(f0, P.freqs[taps["states"] % P.npb])
    check_obs(name, taps, vp)
    check_path(name, f0, voiced, vp, taps, fill_nan=False)
    g0 = run(pyin, name)[0]
    assert np.array_equal(np.isnan(g0), ~voiced) and np.array_equal(g0[voiced], f0[voiced])


# ---------------------------------------------------------------- the decoding stage alone
def viterbi_case(pyin, o, identical):
    from targetdiarization_amd.pitch import pyin_plan
    P = orc.params(**cases.DEFAULT)
    st = pyin.viterbi(o.T, pyin_plan(**cases.DEFAULT))
    want = orc.viterbi_banded(o, P)
    a, b = orc.score(st, o, P), orc.score(want, o, P)
    print(f"T={o.shape[1]}: score {a:.15g}, optimum {b:.15g}, states equal {bool(np.array_equal(st, want))}")
    assert st.shape == want.shape and st.min() >= 0 and st.max() < 2 * P.npb
    assert abs(a - b) <= 1e-9 * abs(b)
    if identical:
        assert np.array_equal(st, want)


@pytest.mark.parametrize("T", cases.VITERBI_T)
def test_viterbi_random(pyin, T):
    viterbi_case(pyin, cases.random_obs(T), identical=T >= 3)        # (T = 1, 2: all unvoiced, every state ties)


@pytest.mark.parametrize("T", cases.VITERBI_T)
def test_viterbi_out_of_band_jumps(pyin, T):
    viterbi_case(pyin, cases.jump_obs(T), identical=T >= 2)


def test_viterbi_drift_5000_frames(pyin):
    viterbi_case(pyin, cases.random_obs(5000), identical=False)


def test_viterbi_wide_state_space(pyin):
    """1037 bins, more than the 1024 threads of the workgroup: some threads own two bins of each half; a band of 27"""
    from targetdiarization_amd.pitch import pyin_plan
    kw = dict(sr=22050, fmin=30.0, fmax=3000.0, max_transition_rate=8.0, resolution=0.08)
    pl = pyin_plan(**kw)
    P = orc.params(**kw)
    assert pl.n_pitch_bins == P.npb > 1024 and pl.width == P.width
    r = np.random.default_rng(7)
    T = 40
    o = np.zeros((2 * P.npb, T))
    for t in range(T):
        o[r.integers(0, P.npb, size=3), t] = r.uniform(0.05, 0.3, size=3)
    o[P.npb:] = (1 - o[:P.npb].sum(0)) / P.npb
    o = o.astype(np.float32).astype(np.float64)
    st = pyin.viterbi(o.T, pl)
    want = orc.viterbi_dense(o, P)
    a, b = orc.score(st, o, P), orc.score(want, o, P)
    assert abs(a - b) <= 1e-9 * abs(b)
    v = want < P.npb
    assert np.array_equal(st < P.npb, v) and np.array_equal(st[v], want[v])


# ---------------------------------------------------------------- end to end
def test_end_to_end_20_s(pyin):
    name = "long20s"
    f0, voiced, vp, taps = run(pyin, name)
    check_taps(name, taps)
    rb = check_obs(name, taps, vp)
    check_path(name, f0, voiced, vp, taps)
    ref = cases.reference(name)
    assert np.all(np.abs(vp - ref["vp"])[rb] <= 1e-6)
    assert voiced.sum() > 200


def test_all_frames_robust_equals_the_oracle(pyin):
    """on inputs whose frames are all robust, f0 (NaN-aware), voiced_flag and voiced_prob are the oracle's"""
    seen = 0
    for name in ("n2048", "n16000", "n48123", "sr8000", "no_center"):
        ref = cases.reference(name)
        if not ref["robust"].all():
            continue
        seen += 1
        f0, voiced, vp, _ = run(pyin, name)
        assert np.array_equal(voiced, ref["voiced"]) and np.max(np.abs(vp - ref["vp"])) <= 1e-6
        assert np.array_equal(f0[voiced], ref["f0"][voiced]) and np.all(np.isnan(f0[~voiced]))
    assert seen >= 3


def test_silence(pyin):
    f0, voiced, vp = pyin.pyin(np.zeros(5000, np.float32), **cases.DEFAULT)
    assert f0.shape == (10,) and np.all(np.isnan(f0)) and not voiced.any() and np.all(vp == 0)


# ---------------------------------------------------------------- batches, channels, the wrapper
def test_batch_is_bit_identical_to_single_calls(pyin):
    clips = [cases.signal(f"batch{k}") for k in range(5)]
    together = pyin.pyin_batch(clips, **cases.DEFAULT)
    for c, (f0, v, vp) in zip(clips, together):
        g0, gv, gvp = pyin.pyin(c, **cases.DEFAULT)
        assert np.array_equal(f0, g0, equal_nan=True) and np.array_equal(v, gv) and np.array_equal(vp, gvp)


def test_two_channels_equal_their_channels_alone(pyin):
    a, b = cases.signal("batch1"), cases.signal("fill_none")[:5000]
    f0, v, vp = pyin.pyin(np.stack([a, b]), **cases.DEFAULT)
    assert f0.shape == v.shape == vp.shape == (2, 10)
    for k, c in enumerate((a, b)):
        g0, gv, gvp = pyin.pyin(c, **cases.DEFAULT)
        assert np.array_equal(f0[k], g0, equal_nan=True) and np.array_equal(v[k], gv) and np.array_equal(vp[k], gvp)


def test_wrapper_and_close():
    from targetdiarization_amd import _lib
    from targetdiarization_amd.asr_processor import ASRProcessor
    from targetdiarization_amd.pitch import Pyin
    y = cases.signal("fill_none")
    proc = ASRProcessor(cuda_device=0, verbose_log=False)
    f0 = proc.f0_compute(y)
    p = Pyin("cuda:0")
    want = p.pyin(y, **cases.DEFAULT)[0]
    assert f0.shape == want.shape == (1 + len(y) // 512,) and np.array_equal(f0, want, equal_nan=True)
    assert np.array_equal(proc.f0_compute(y, 16000, 80.0, 400.0), p.pyin(y, fmin=80.0, fmax=400.0, sr=16000)[0], equal_nan=True)
    assert proc.f0_compute(y, fmin=7000.0, fmax=7900.0).size == 0               # rejected parameters: printed, empty result
    p.close()
    with pytest.raises(_lib.TdxError):
        p.pyin(y, **cases.DEFAULT)
    proc.pitch.close()
