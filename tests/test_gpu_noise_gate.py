"""noisereduce's spectral gate on the device (noise_gate.SpectralGate, csrc/noise_gate.hip) against the float64 scipy
restatement of the same steps (tests/noise_gate_oracle.py).  The output tolerance is the project's denoise tolerance
(tests/test_gpu_denoise.py): ||y - ref|| / ||x|| < 1e-5 per clip; a float32 run of the plain restatement measures 1.6e-7."""
import numpy as np
import pytest

import noise_gate_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
SMALL = dict(chunk_size=4096, padding=1024)


@pytest.fixture(scope="module")
def gate():
    from targetdiarization_amd.noise_gate import SpectralGate
    g = SpectralGate("cuda:0")
    yield g
    g.close()


def rel(y, ref, x):
    return float(np.linalg.norm(np.asarray(y, np.float64) - ref) / np.linalg.norm(np.asarray(x, np.float64)))


def check(gate, x, sr=16000, **kw):
    y = gate.reduce_noise(x, sr, **kw)
    ref = orc.reduce_noise(x, sr, **kw)
    assert y.dtype == np.float32 and y.shape == np.asarray(x).shape
    e = rel(y, ref, x)
    print(f"n={np.asarray(x).shape} sr={sr} {kw}: rel err {e:.3e}")
    assert np.isfinite(y).all() and e < TOL
    return y


@pytest.mark.parametrize("n", [1, 255, 256, 1000, 4096, 4097, 3 * 4096 + 777])
def test_small_geometry(gate, n):
    """one buffer up to n = 4096, then two and four chunks"""
    check(gate, orc.burst_signal(n, seed=n), **SMALL)


def test_real_geometry_two_buffers(gate):
    """noisereduce's own chunk_size = 600000, padding = 30000: n = 600001 gives two buffers of 2579 frames"""
    check(gate, orc.burst_signal(600001, seed=1))


@pytest.mark.parametrize("frames", [63, 64, 65])
def test_frames_around_the_scan_segment(gate, frames):
    """the scan's segment is 64 frames: one segment short of full, full, and a second segment of one frame"""
    n = (frames - 1) * 256 - 2048
    assert 1 + (n + 2048) // 256 == frames
    check(gate, orc.burst_signal(n, seed=frames), chunk_size=16384, padding=1024)


def test_more_segments_than_slots(gate):
    """more than 64 x 64 frames in one buffer: every slot of the scan workgroup takes a second segment"""
    n = 4100 * 256
    check(gate, orc.burst_signal(n, seed=2), chunk_size=1 << 21, padding=1024)


@pytest.mark.parametrize("sr,kw", [(8000, {}), (16000, {}), (44100, {}), (16000, dict(time_mask_smooth_ms=0)), (16000, dict(prop_decrease=0.5))])
def test_rates_and_parameters(gate, sr, kw):
    """(nf, nt) = (32, 1), (16, 3), (5, 8); nt = 0; prop_decrease = 0.5"""
    check(gate, orc.burst_signal(5000, sr=sr, seed=sr), sr=sr, **SMALL, **kw)


def test_two_channels(gate):
    x = np.stack([orc.burst_signal(5000, seed=3), orc.burst_signal(5000, seed=4)])
    y = check(gate, x, **SMALL)
    for c in range(2):
        assert np.array_equal(y[c], gate.reduce_noise(x[c], 16000, **SMALL))


def test_silence(gate):
    """digital silence: exact zeros, no NaN (noisereduce returns NaN); zeros around a signal: finite and equal to the oracle
    under the same s == 0 rule"""
    y = gate.reduce_noise(np.zeros(5000, np.float32), 16000, **SMALL)
    assert np.array_equal(y, np.zeros(5000, np.float32))
    x = orc.burst_signal(9000, seed=5)
    x[:3000] = 0
    x[6000:] = 0
    check(gate, x, **SMALL)
    # (the filtfilt reaches every frame of a buffer that holds signal, so s == 0 needs a wholly silent buffer)
    x = orc.burst_signal(5 * 4096, seed=6)
    x[:2 * 4096] = 0
    x[3 * 4096:] = 0
    assert not np.isfinite(orc.reduce_noise(x, 16000, zero_rule=False, **SMALL)).all()
    check(gate, x, **SMALL)


def test_taps(gate):
    """the intermediate planes of one buffer (196 frames) against the oracle's.  Bound per quantity: 16 x the error of a float32
    numpy run of the plain restatement against the float64 oracle (the device sums its DFT in another order than numpy's FFT).
    Measured on the CPU for this clip, float32 numpy vs float64 oracle, absolute: |S| 7.8e-6 (of 77), smoothed |S| 1.5e-5
    (of 33), mask 1.3e-5, smoothed mask 7.8e-7.  Measured on the device (MI355X) against the same oracle: |S| 1.08e-4 (bound
    1.24e-4: a 1024-term DFT summed in a fixed order against numpy's log-depth FFT), smoothed |S| 5.6e-6, mask 1.37e-5,
    smoothed mask 4.5e-7.  Both sets are in DESIGN 8.19; the test prints the figures of its run."""
    x = orc.burst_signal(48000, seed=0)
    kw = dict(chunk_size=1 << 16, padding=1024)
    ref, f32, dev = {}, {}, {}
    orc.reduce_noise(x, 16000, taps=ref, **kw)
    orc.reduce_noise_plain(x, 16000, dtype=np.float32, taps=f32, **kw)
    gate.reduce_noise(x, 16000, taps=dev, **kw)
    for k in ("mag", "smooth", "mask", "mask_smooth"):
        assert dev[k].shape == ref[k].shape == (196, 513)
        bound = 16 * float(np.abs(f32[k].astype(np.float64) - ref[k]).max())
        err = float(np.abs(dev[k].astype(np.float64) - ref[k]).max())
        print(f"tap {k}: device {err:.3e}, float32 numpy {bound / 16:.3e}, bound {bound:.3e}")
        assert err < bound


def test_independence():
    """a clip's bits do not depend on its batch, on the round split or on the call"""
    from targetdiarization_amd.noise_gate import SpectralGate
    one, three = SpectralGate("cuda:0"), SpectralGate("cuda:0", rows_per_launch=30)
    try:
        clips = [orc.burst_signal(n, seed=10 + i) for i, n in enumerate([3 * 4096, 1, 5000, 257, 4096])]
        alone = [one.reduce_noise(c, 16000, **SMALL) for c in clips]
        batch = one.reduce_noise_batch(clips, 16000, **SMALL)
        for a, b in zip(alone, batch):
            assert np.array_equal(a, b)
        # buffers of 6144 samples take 28 rows: rows_per_launch = 30 puts the three buffers of clip 0 into three rounds
        tab, max_rows = three.table([(1, 3 * 4096)], 4096, 1024)
        assert tab[:, 7].tolist() == [0, 0, 0] and max_rows == 28 and one.table([(1, 3 * 4096)], 4096, 1024)[0][:, 7].tolist() == [0, 28, 56]
        assert np.array_equal(three.reduce_noise(clips[0], 16000, **SMALL), alone[0])
        assert np.array_equal(one.reduce_noise(clips[0], 16000, **SMALL), alone[0])
    finally:
        one.close()
        three.close()


def test_handle_lifetime():
    from targetdiarization_amd import _lib
    from targetdiarization_amd.noise_gate import SpectralGate
    g = SpectralGate("cuda:0")
    g.reduce_noise(orc.burst_signal(1000), 16000, **SMALL)
    g.close()
    g.close()
    with pytest.raises(_lib.TdxError):
        g.reduce_noise(orc.burst_signal(1000), 16000, **SMALL)


def test_audio_processor_flag(capsys):
    from targetdiarization_amd.audio_processor import AudioProcessor
    ap = AudioProcessor(noise_reduce=True, cuda_device=0, verbose_log=True)
    assert ap.noise_reduce and not ap.is_denoise_vocal
    x = orc.burst_signal(16000, seed=7)
    ref = orc.reduce_noise(x, 16000)
    for kw in ({}, dict(fast_mode=True)):
        y = ap.denoise_vocal(x, 16000, **kw)
        assert rel(y, ref, x) < TOL
    assert "Using method: noisereduce" in capsys.readouterr().out
    assert AudioProcessor(noise_reduce=True, cuda_device=-1).noise_reduce is False


def test_target_diarization_preprocess(sd2):
    """the reference's full chain (TargetDiarization.py:171-176): loudness control, gate, loudness control — the host loudness
    function stands on both sides; infer()'s batch of input and target clip gives the same bits as one clip at a time"""
    from targetdiarization_amd.target_diarization import TargetDiarization
    td = TargetDiarization(cuda_device=0, sep_state_dict=sd2, noise_reduce=True)
    assert td.hp.ap.noise_reduce
    x, t = orc.burst_signal(24000, seed=8), orc.burst_signal(9000, seed=9)
    y = td.audio_preprocess(x)
    head = td.audio_loudness_control(x)
    ref = td.audio_loudness_control(orc.reduce_noise(head, 16000).astype(np.float32))
    assert y.shape == x.shape and rel(y, ref, head) < TOL
    a, b = td.audio_preprocess_batch([(x, 16000), (t, 16000)])
    assert np.array_equal(a, y) and np.array_equal(b, td.audio_preprocess(t))
