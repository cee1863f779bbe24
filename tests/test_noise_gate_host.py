"""CPU tests of the spectral gate's host side: the oracle pins itself (scipy's four calls against a plain numpy restatement),
noise_gate.chunk_plan / gate_params against the oracle's own arithmetic, the C-ABI's argument checks without a device, and the
wiring with the flag off."""
import ctypes as C

import numpy as np
import pytest

import noise_gate_oracle as orc
from targetdiarization_amd import noise_gate as ng


@pytest.mark.parametrize("n,kw", [(1, {}), (255, {}), (256, {}), (3000, {}), (2 * 4096 + 500, dict(chunk_size=4096, padding=1024))])
def test_oracle_agrees_with_plain_numpy(n, kw):
    """the filtfilt seeding (each pass starts from the steady state of its first sample) and the frame grid of
    stft(boundary="zeros", padded=False) / istft, restated with explicit loops: 1e-12 relative"""
    x = orc.burst_signal(n, seed=n)
    a, b = orc.reduce_noise(x, 16000, **kw), orc.reduce_noise_plain(x, 16000, **kw)
    assert a.shape == b.shape == x.shape
    assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()


def test_zero_state_filter_is_not_the_oracle():
    """the zero-state reading of the time smoothing is wrong by more than 10 %"""
    import scipy.signal as ss
    A = np.abs(np.random.RandomState(0).randn(200, 3)) + 1.0
    b = orc.params(16000)[0]
    ref = ss.filtfilt([b], [1, b - 1], A, axis=0, padtype=None)
    y = ss.lfilter([b], [1, b - 1], A, axis=0)
    z = ss.lfilter([b], [1, b - 1], y[::-1], axis=0)[::-1]
    assert np.abs(z - ref).max() > 0.1 * np.abs(ref).max()


def test_chunk_plan():
    assert ng.chunk_plan(600000) == [(-30000, 630000, 0, 600000)]
    two = ng.chunk_plan(600001)
    assert two == [(-30000, 630000, 0, 600000), (570000, 1230000, 600000, 600001)]
    for n, cs, pad in [(1, 4096, 1024), (4096, 4096, 1024), (4097, 4096, 1024), (3 * 4096 + 777, 4096, 1024), (600001, 600000, 30000)]:
        p = ng.chunk_plan(n, cs, pad)
        assert p == orc.plan(n, cs, pad)
        assert p[0][2] == 0 and p[-1][3] == n and all(a[3] == b[2] for a, b in zip(p, p[1:]))        # the kept ranges tile [0, n)
        assert all(lo <= k0 - pad and k1 + pad <= hi for lo, hi, k0, k1 in p)
    with pytest.raises(ValueError, match="padding must be >= 1024"):
        ng.chunk_plan(100, 4096, 1023)
    with pytest.raises(ValueError, match="empty"):
        ng.chunk_plan(0)


def test_gate_params():
    for sr, want in [(16000, (16, 3)), (44100, (5, 8)), (8000, (32, 1))]:
        b, nf, nt, (tf, tt) = ng.gate_params(sr)
        assert (nf, nt) == want == orc.params(sr)[1:]
        filt = orc.smoothing_filter(nf, nt)
        assert tf.shape == (2 * nf + 1,) and tt.shape == (2 * nt + 1,)
        assert np.allclose(tf, filt.sum(axis=1), rtol=0, atol=1e-15) and np.allclose(tt, filt.sum(axis=0), rtol=0, atol=1e-15)
        assert np.allclose(np.outer(tf, tt), filt, rtol=0, atol=1e-15)
        # the device evaluates the taps as (k + 1 - |j - k|) / (k + 1)^2
        for k, t in ((nf, tf), (nt, tt)):
            assert np.allclose(t, (k + 1 - np.abs(np.arange(2 * k + 1) - k)) / float((k + 1) ** 2), rtol=0, atol=1e-15)
    assert abs(ng.gate_params(16000)[0] - 0.0079680640) < 1e-9
    b, nf, nt, (tf, tt) = ng.gate_params(16000, time_mask_smooth_ms=0)
    assert nt == 0 and tt.tolist() == [1.0] and nf == 16
    with pytest.raises(ValueError):
        ng.gate_params(16000, freq_mask_smooth_hz=8000)


def test_table_follows_the_plan():
    g = ng.SpectralGate.__new__(ng.SpectralGate)
    g.rows_per_launch = 60
    tab, max_rows = g.table([(2, 4097), (1, 10)], 4096, 1024)
    # 2 channels x 2 buffers of 6144 samples (28 rows each), then one buffer of 2058 samples (12 rows): rounds of 56, 56, 12 rows
    assert tab.shape == (5, 8) and tab[:, 7].tolist() == [0, 28, 0, 28, 0] and max_rows == 56
    assert tab[0].tolist() == [-1024, 1024, 5121, 1024, 5120, 0, 6144, 0]
    assert tab[1].tolist() == [4096 - 1024, 0, 1025, 1024, 1025, 4096, 6144, 28]
    assert tab[2, 0] == 4097 - 1024 and tab[2, 5] == 4097
    assert tab[4].tolist() == [2 * 4097 - 1024, 1024, 1034, 1024, 1034, 2 * 4097, 2058, 0]


@pytest.fixture(scope="module")
def lib():
    from targetdiarization_amd import _lib
    from targetdiarization_amd.build import build_lib
    build_lib()
    return _lib.lib()


def test_abi_validates_without_a_device(lib):
    assert lib.tdx_ngate_create(0, None) == 1 and b"null" in lib.tdx_last_error()
    h = C.c_void_p()
    assert lib.tdx_ngate_create(-1, C.byref(h)) == 1
    assert lib.tdx_ngate_rows(6144) == 28 and lib.tdx_ngate_rows(0) == 0
    assert lib.tdx_ngate_workspace_bytes(None, 100) == 0
    fake = C.c_void_p(64)                      # never dereferenced: every check below comes before the handle is used
    assert lib.tdx_ngate_workspace_bytes(fake, 3) == 0 and lib.tdx_ngate_workspace_bytes(fake, 28) >= 28 * 3424 * 4
    good = [-1024, 1024, 2024, 1024, 2024, 0, 3048, 0]

    def call(tab, n_total=1000, rows=16384, b=0.008, nf=16, nt=3, prop=1.0, nbuf=1):
        t = (C.c_int64 * len(tab))(*tab)
        return lib.tdx_ngate_forward(fake, fake, n_total, t, fake, nbuf, rows, b, nf, nt, 2.0, 10.0, prop, fake, None, None, None, None, fake, 1 << 40, None)

    def bad(i, v):
        t = list(good)
        t[i] = v
        return t
    assert lib.tdx_ngate_forward(None, None, 0, None, None, 0, 0, 0.0, 0, 0, 0.0, 0.0, 0.0, None, None, None, None, None, None, 0, None) == 1
    for kw, msg in [(dict(n_total=0), b"n_total"), (dict(nbuf=0), b"nbuf"), (dict(b=0.0), b"coefficient"), (dict(nf=129), b"nf, nt"),
                    (dict(nt=-1), b"nf, nt"), (dict(prop=1.5), b"prop_decrease"), (dict(rows=3), b"rows_per_launch"), (dict(rows=14), b"more than rows_per_launch")]:
        assert call(good, **kw) == 1 and msg in lib.tdx_last_error(), (kw, lib.tdx_last_error())
    for tab, msg in [(bad(6, 0), b"frames"), (bad(6, 256 * 32768), b"frames"), (bad(1, -1), b"valid range outside the buffer"),
                     (bad(2, 3049), b"valid range outside the buffer"), (bad(0, -1025), b"valid range outside the input"),
                     (bad(0, -23), b"valid range outside the input"), (bad(4, 3049), b"keep range outside the buffer"),
                     (bad(3, 255), b"four frames"), (bad(4, 2561), b"four frames"), (bad(5, 1), b"keep range outside the output"),
                     (bad(5, -1), b"keep range outside the output"), (bad(7, 1), b"row0")]:
        assert call(tab) == 1 and msg in lib.tdx_last_error(), (tab, lib.tdx_last_error())
    # a table that passes every check stops at the workspace size, still before the device
    t = (C.c_int64 * 8)(*good)
    assert lib.tdx_ngate_forward(fake, fake, 1000, t, fake, 1, 16384, 0.008, 16, 3, 2.0, 10.0, 1.0, fake, None, None, None, None, fake, 16, None) == 4


def test_flag_off_changes_nothing(capsys):
    from targetdiarization_amd.audio_processor import AudioProcessor
    from targetdiarization_amd.server import env_to_kwargs
    from targetdiarization_amd.target_diarization import TargetDiarization
    ap = AudioProcessor(cuda_device=-1, verbose_log=False)
    assert ap.noise_reduce is False and ap.noise_gate is None
    x = orc.burst_signal(16000)
    assert ap.denoise_vocal(x, 16000) is x and ap.denoise_vocal(x, 16000, fast_mode=True) is x
    assert "audio returned unchanged" in capsys.readouterr().out
    assert AudioProcessor(cuda_device=-1, noise_reduce=True).noise_reduce is False            # no device: the flag stays off

    class HP:
        pass
    td = TargetDiarization.__new__(TargetDiarization)
    td.hp = HP()
    td.hp.ap = ap
    y = td.audio_preprocess(x)
    assert np.array_equal(y, td.audio_loudness_control(x))                                    # ends after the first loudness pass
    a, b = td.audio_preprocess_batch([(x, 16000), (x[:8000], 16000)])
    assert np.array_equal(a, y) and np.array_equal(b, td.audio_loudness_control(x[:8000]))
    assert "noise_reduce" not in env_to_kwargs({}) and "noise_reduce" not in env_to_kwargs({"NOISE_REDUCE": "0"})
    assert env_to_kwargs({"NOISE_REDUCE": "1"})["noise_reduce"] is True
