"""CPU tests of the pyin restatement (tests/pyin_oracle.py), of the host plan (pitch.pyin_plan), of the f0_compute wrapper without a
device — and of the INPUT CONDITIONS of the device tests (test_gpu_pyin.py), asserted here for every input those tests name
(tests/pyin_cases.py): few non-robust frames, float32 alone changes few observation columns, and no ties that could be seen.

Ties.  The unvoiced rows of an observation column are all equal, and the triangular transition makes many unvoiced paths between
two voiced stretches exactly as likely as each other (the same bin steps in another order), so first-maximum and last-maximum
decoding differ on unvoiced frames of every gated signal: measured on the 20 s signal, 84 of 626 states, none of them voiced.
What can be seen of a path — the voiced flag of every frame and the state of every voiced frame — is what must not depend on the
tie rule, and that is what is asserted (and what the device tests compare)."""
import numpy as np
import pytest

import pyin_cases as cases
import pyin_oracle as orc

from targetdiarization_amd import _lib
from targetdiarization_amd.pitch import pyin_plan


# ---------------------------------------------------------------- the decoding stage: banded == dense
@pytest.mark.parametrize("T", cases.VITERBI_T)
def test_banded_viterbi_equals_dense_on_random_matrices(T):
    P = orc.params(**cases.DEFAULT)
    o = cases.random_obs(T)
    for last in (False, True):
        assert np.array_equal(orc.viterbi_banded(o, P, last=last), orc.viterbi_dense(o, P, last=last))


@pytest.mark.parametrize("T", cases.VITERBI_T)
def test_banded_viterbi_equals_dense_on_out_of_band_jumps(T):
    P = orc.params(**cases.DEFAULT)
    o = cases.jump_obs(T)
    assert np.all(o[P.npb:] == 0) and np.all(o[:P.npb].sum(0) == 1)
    dense = orc.viterbi_dense(o, P)
    assert np.array_equal(orc.viterbi_banded(o, P), dense)
    if T >= 3:                                                   # the path does jump past the band (310 bins, half width 70)
        assert np.max(np.abs(np.diff(dense[1:] % P.npb))) > P.width // 2 or len(set(dense[1:] % P.npb)) == 1


def test_tie_free_viterbi_inputs():
    """the matrices on which the device tests also demand identical states: first and last maximum give the same path there"""
    P = orc.params(**cases.DEFAULT)
    for T in (3, 300):
        o = cases.random_obs(T)
        assert np.array_equal(orc.viterbi_dense(o, P), orc.viterbi_dense(o, P, last=True)), T
    for T in cases.VITERBI_T:
        o = cases.jump_obs(T)
        if T >= 2:
            assert np.array_equal(orc.viterbi_dense(o, P), orc.viterbi_dense(o, P, last=True)), T


def test_score_is_what_viterbi_maximises():
    P = orc.params(**cases.DEFAULT)
    o = cases.random_obs(300)
    best = orc.viterbi_dense(o, P)
    s = orc.score(best, o, P)
    rng = np.random.default_rng(0)
    for _ in range(20):
        other = best.copy()
        other[rng.integers(0, 300)] = rng.integers(0, 2 * P.npb)
        assert orc.score(other, o, P) <= s


# ---------------------------------------------------------------- the whole restatement
@pytest.mark.parametrize("f", [100.0, 220.5])
def test_pure_tone_comes_out_at_the_nearest_bin(f):
    P = orc.params(**cases.DEFAULT)
    y = np.sin(2 * np.pi * f * np.arange(16000) / 16000)
    f0, voiced, vp, _, _ = orc.pyin(y, P)
    want = P.freqs[np.argmin(np.abs(P.freqs - f))]
    assert voiced[3:-3].all() and np.all(f0[3:-3] == want)


@pytest.mark.parametrize("n", cases.GEOMETRY_N + [1023, 1024, 1025])
def test_frame_counts(n):
    P = orc.params(**cases.DEFAULT)
    assert orc.frames(np.zeros(n), P).shape == (2048, 1 + n // 512)
    assert pyin_plan(16000, 50.0, 300.0).frames(n) == 1 + n // 512


def test_frame_counts_without_centering():
    pl = pyin_plan(16000, 50.0, 300.0, center=False)
    assert pl.frames(2048) == 1 and pl.frames(8000) == 12
    assert orc.frames(np.zeros(8000), orc.params(**dict(cases.DEFAULT, center=False))).shape[1] == 12
    with pytest.raises(_lib.TdxError):
        pl.frames(2047)


def test_flush_matters_only_near_silence():
    """upstream's 1e-6 flush against none, on a copy of the 20 s signal whose tone peaks at -60 dBFS: f0, flag and probability are
    the same in every frame louder than -80 dBFS, and every frame in which they differ is quieter than -85 dBFS.  (The copy's
    noise floor between the tone bursts lies at -89 dBFS: 45 of its frames differ, which is the deviation itself and why the
    comparison is by level.)  The device sums the differences directly and has nothing to flush — this is what confines that
    deviation to frames near -90 dBFS."""
    P = cases.plan("long20s")
    y = cases.signal("long20s").astype(np.float64) * 1e-3 / 0.3
    a = orc.pyin(y, P, flush=True)
    b = orc.pyin(y, P, flush=False)
    rms = np.sqrt(np.mean(orc.frames(y, P)[1:P.win_length + 1] ** 2, axis=0))
    db = 20 * np.log10(np.maximum(rms, 1e-12))
    differ = (a[1] != b[1]) | ~((a[0] == b[0]) | (np.isnan(a[0]) & np.isnan(b[0]))) | (np.abs(a[2] - b[2]) > 1e-6)
    print(f"frames that differ: {int(differ.sum())}, the loudest at {db[differ].max() if differ.any() else float('nan'):.1f} dBFS; louder than -80 dBFS: {int((db > -80).sum())}")
    assert (db > -80).sum() > 250
    assert not np.any(differ & (db > -80))
    assert np.all(db[differ] < -85)


# ---------------------------------------------------------------- the host plan
def test_plan_agrees_with_the_oracle():
    pl = pyin_plan(16000, 50.0, 300.0)
    P = orc.params(**cases.DEFAULT)
    assert (pl.min_period, pl.max_period, pl.n_pitch_bins, pl.width) == (53, 320, 311, 141)
    assert (P.min_period, P.max_period, P.npb, P.width) == (53, 320, 311, 141)
    assert np.array_equal(pl.beta_probs, P.beta_probs) and np.array_equal(pl.freqs, P.freqs)
    lt = np.log(orc.transition(P) + orc.TINY)
    hw = P.width // 2
    for i in (0, 1, 69, 70, 71, 155, 240, 309, 310):
        for j in range(max(0, i - hw), min(P.npb, i + hw + 1)):
            assert abs(lt[i, j] - (pl.log_band[i, j - i + hw] + pl.params.log_stay)) < 1e-13
            assert abs(lt[P.npb + i, j] - (pl.log_band[i, j - i + hw] + pl.params.log_switch)) < 1e-13
    for name in ("sr8000", "sr22050_wide", "sr44100_4096"):
        kw = cases.SIGNALS[name][0]
        pl, P = pyin_plan(**kw), cases.plan(name)
        assert (pl.min_period, pl.max_period, pl.n_pitch_bins, pl.width) == (P.min_period, P.max_period, P.npb, P.width)
    assert (cases.plan("sr8000").npb, cases.plan("sr8000").width) == (311, 281)
    assert (cases.plan("sr22050_wide").npb, cases.plan("sr22050_wide").min_period) == (601, 10)


def test_plan_raises_where_upstream_raises():
    with pytest.raises(_lib.TdxError, match="width"):
        pyin_plan(8000, 100.0, 200.0)                            # 121 bins < width 281
    with pytest.raises(_lib.TdxError, match="at least"):
        pyin_plan(16000, 7000.0, 7900.0)                         # periods 2 .. 3
    with pytest.raises(_lib.TdxError, match="pad_mode"):
        pyin_plan(16000, 50.0, 300.0, pad_mode="reflect")
    with pytest.raises(_lib.TdxError, match="frame_length"):
        pyin_plan(16000, 50.0, 300.0, frame_length=16384)
    with pytest.raises(_lib.TdxError, match="states"):
        pyin_plan(22050, 20.0, 8000.0, frame_length=8192, resolution=0.03)


def test_c_abi_rejects_bad_parameters_without_a_device():
    import ctypes as C
    from targetdiarization_amd.build import build_lib
    build_lib()
    l = _lib.lib()
    assert l.tdx_pyin_create(0, None) == 1
    pl = pyin_plan(16000, 50.0, 300.0)
    one = C.c_void_p(1)                                          # never dereferenced: every check below fails first

    def viterbi(**kw):
        p = _lib.PyinParams.from_buffer_copy(pl.params)
        for k, v in kw.items():
            setattr(p, k, v)
        return l.tdx_pyin_viterbi(one, one, 10, C.byref(p), one, pl.tables.size, one, one, 1 << 30, None)

    assert viterbi(n_pitch_bins=2049) == 1 and b"4096" in l.tdx_last_error()
    assert viterbi(n_pitch_bins=140) == 1 and b"width" in l.tdx_last_error()
    assert viterbi(max_period=54) == 1 and b"max_period - min_period" in l.tdx_last_error()
    p = _lib.PyinParams.from_buffer_copy(pl.params)
    p.frame_length = 16384
    tab = (C.c_int64 * 4)(0, 100, 0, 1)
    assert l.tdx_pyin_forward(one, one, 100, tab, one, 1, C.byref(p), one, pl.tables.size, one, one, None, None, None, one, 1 << 30, None) == 1
    assert b"frame_length" in l.tdx_last_error()
    assert l.tdx_pyin_workspace_bytes(None, C.byref(pl.params), 10) == 0


# ---------------------------------------------------------------- the wrapper without a device
def test_f0_compute_without_a_device(capsys):
    from targetdiarization_amd.asr_processor import ASRProcessor
    p = ASRProcessor(cuda_device=-1, verbose_log=False)
    out = p.f0_compute(np.zeros(1000, np.float32))
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.size == 0
    assert "f0_compute" in capsys.readouterr().out
    with pytest.raises(ValueError):
        p.f0_compute("clip.wav")


# ---------------------------------------------------------------- input conditions of the device tests
@pytest.mark.parametrize("name", sorted(cases.SIGNALS))
def test_input_conditions(name):
    P, y, ref = cases.plan(name), cases.signal(name), cases.reference(name)
    T = ref["yin"].shape[1]
    bad = int((~ref["robust"]).sum())
    yin32, sh32, obs32 = cases.fp32_mode(name)
    diff = int((np.max(np.abs(obs32 - ref["obs"]), axis=0) > 1e-6).sum())
    e32 = float(np.max(cases.frame_rel_err(yin32, ref["yin"])))
    last = orc.viterbi_dense(ref["obs"], P, last=True)
    print(f"{name}: T={T} non-robust {bad} fp32 columns differ {diff} fp32 yin err {e32:.2e} states differ under the tie rule {int((last != ref['states']).sum())}")
    if name in cases.DEGENERATE:                                  # (pyin_cases.DEGENERATE: one sample, yin = 1 in every row)
        assert T == 1 and np.max(np.abs(ref["yin"] - 1)) < 1e-9 and np.max(np.abs(yin32 - 1)) < 320 * 2.0 ** -24   # (a float32 running sum of 320 equal terms)
        assert ref["vp"][0] <= P.no_trough_prob + 1e-12 and not ref["voiced"][0]
        return
    assert bad <= 0.02 * T
    assert diff <= 0.005 * T
    silent = not np.any(y)
    if not silent:
        v = ref["voiced"]
        assert np.array_equal(last < P.npb, v) and np.array_equal(last[v], ref["states"][v])


def test_prototype_figures_on_the_20_s_signal():
    """float32 direct difference against the float64 FFT form: yin within 4e-6 of the frame maximum (the axis-0 numpy sum adds its
    1024 terms one after the other: 2.8e-6 measured), at most one column in 626 differs, the same visible path, the same score"""
    P, ref = cases.plan("long20s"), cases.reference("long20s")
    yin32, sh32, obs32 = cases.fp32_mode("long20s")
    assert np.max(cases.frame_rel_err(yin32, ref["yin"])) < 4e-6
    assert (np.max(np.abs(obs32 - ref["obs"]), axis=0) > 1e-6).sum() <= 1
    s32 = orc.viterbi_dense(obs32, P)
    v = ref["voiced"]
    assert np.array_equal(s32 < P.npb, v) and np.array_equal(s32[v], ref["states"][v])
    a, b = orc.score(s32, ref["obs"], P), orc.score(ref["states"], ref["obs"], P)
    assert abs(a - b) <= 1e-9 * abs(b)
