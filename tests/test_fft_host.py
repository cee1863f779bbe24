"""CPU tests of the FFT's host side: the float64 oracle against the goldens minted from the reference
(tools/make_goldens_band_mix.py), fft.band_mix_plan against the boolean masks of the full rfftfreq expression, the four host-only
AudioProcessor methods against the goldens, and the argument rules of every tdx_fft_* entry point (no device is touched)."""
import ast
import ctypes as C
import os

import numpy as np
import pytest

import fft_oracle as orc
from targetdiarization_amd import _lib
from targetdiarization_amd import fft as tfft


@pytest.fixture(scope="module")
def G(gold):
    return np.load(os.path.join(gold, "band_mix.npz"))


@pytest.fixture(scope="module")
def cases(G):
    return [ast.literal_eval(str(c)) for c in G["mixf_cases"]]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---- 1. the oracle against the goldens
def test_oracle_reproduces_mix_audio_by_freq(G, cases):
    assert len(cases) >= 16
    seen_odd = seen_same = False
    for name, n, n_aux, sr, mr, ar, align in cases:
        a, b = G[f"mixf_{name}_main"].astype(np.float64), G[f"mixf_{name}_aux"].astype(np.float64)
        assert a.shape == (n,) and b.shape == (n_aux,)
        y = orc.mix_audio_by_freq(a, b, sr, mr, ar, align)
        if bool(G[f"mixf_{name}_same"]):
            assert y is a, name                                       # the unchanged return on a length mismatch
            seen_same = True
            continue
        ref = G[f"mixf_{name}_out"]
        assert ref.dtype == np.float64 and y.dtype == np.float64
        assert y.shape == ref.shape == (2 * (n // 2),), name          # an odd clip comes back one sample shorter
        seen_odd |= n % 2 == 1
        assert rel(y, ref) <= 1e-12, (name, rel(y, ref))
    assert seen_odd and seen_same


def test_oracle_smallest_input(G):
    """n = 1: the reference raises (irfft of 0 points); the build returns audio_main"""
    assert bool(G["mixf_n1_raises"])
    a = np.array([0.5])
    assert orc.mix_audio_by_freq(a, np.array([0.25])) is a
    m2 = np.zeros((4, 2))
    assert orc.mix_audio_by_freq(m2, m2) is m2


def _host_checks(impl, G):
    """the four host-only methods of `impl` (the oracle module or an AudioProcessor) against the goldens: values, dtype, shape"""
    x = G["host_x"]
    for tag, db, clip in (("p6", 6.0, False), ("p20clip", 20.0, True), ("m3", -3.0, False), ("zero", 0.0, True)):
        y, ref = impl.audio_gain(x, db, clip), G[f"gain_{tag}"]
        assert y.dtype == ref.dtype and y.shape == ref.shape and rel(y, ref) <= 1e-12, tag
    assert bool(G["gain_zero_same"]) and impl.audio_gain(x, 0.0) is x
    for key, args in (("norm_default", ()), ("norm_m6", (-6.0,))):
        y, ref = impl.audio_normalize(x, *args), G[key]
        assert y.dtype == ref.dtype and y.shape == ref.shape and rel(y, ref) <= 1e-12, key
    z = np.zeros(16, dtype=np.float32)
    assert bool(G["norm_zero_same"]) and impl.audio_normalize(z) is z
    clips = [G[f"mix_clip{k}"] for k in range(3)]
    for key, kw in (("mix_sum_norm", {}), ("mix_sum_raw", dict(normalize=False)), ("mix_stack_norm", dict(combine_channels=False))):
        y, ref = impl.mix_audio(list(clips), **kw), G[key]
        assert y.dtype == ref.dtype and y.shape == ref.shape and rel(y, ref) <= 1e-12, key
    assert bool(G["mix_single_same"]) and impl.mix_audio([x]) is x
    for k, (kind, db) in enumerate((("brown", 0.0), ("pink", 0.0), ("pink", -6.0), ("silence", 0.0), ("white", 3.0))):
        np.random.seed(k)
        y, ref = impl.generate_noise(8000, 0.05, db, kind), G[f"noise_{k}_{kind}"]
        assert y.dtype == ref.dtype and y.shape == ref.shape == (400,), kind
        assert rel(y, ref) <= 1e-12, (kind, rel(y, ref))


def test_oracle_reproduces_host_methods(G):
    _host_checks(orc, G)


# ---- 2. band_mix_plan against the boolean masks
RANGES = [([0, 4000], [0, 8000]), (None, None), ([0, 0], [0, 8000]), ([3000, 100], [0, 8000]), ([0, 1000], [3000, 5000]),
          ([500, 2500], [500, 2500]), ([0, 4000], [2000, 99999]), ([-10, 4000], [4000, 8000]), ([0, 2000], [2000, 2000])]


def _run_of(mask):
    idx = np.flatnonzero(mask)
    if idx.size == 0:
        return None
    assert idx[-1] - idx[0] + 1 == idx.size               # one contiguous run
    return [int(idx[0]), int(idx[-1]) + 1]


@pytest.mark.parametrize("sr", [8000, 16000, 44100])
@pytest.mark.parametrize("n", [2, 3, 5, 16, 1000, 1009, 16000, 160000, 160001, 999983])
def test_band_mix_plan_equals_masks(n, sr):
    for mr, ar in RANGES:
        plan = tfft.band_mix_plan(n, sr, mr, ar)
        masks = orc.band_sets(n, sr, mr, ar)
        assert plan["main_freq_range"] == masks[3] and plan["aux_freq_range"] == masks[4]
        for key, mask in zip(("main", "aux", "overlap"), masks[:3]):
            lo, hi = plan[key]
            assert 0 <= lo <= hi <= n // 2 + 1
            run = _run_of(mask)
            assert (hi - lo == 0) if run is None else ([lo, hi] == run), (n, sr, mr, ar, key, plan[key], run)
        assert plan["count"] == int(masks[2].sum())
        assert plan["ranges"] == plan["main"] + plan["aux"] + plan["overlap"] and plan["n"] == n


def test_band_mix_plan_limit_on_a_bin():
    """n a multiple of 16000 at 16 kHz: 4000 Hz is a bin, where main's `<` and aux's / the overlap's `<=` differ"""
    for n in (16000, 160000):
        k = 4000 * n // 16000
        assert np.fft.rfftfreq(n, 1 / 16000)[k] == 4000.0
        p = tfft.band_mix_plan(n, 16000, [0, 4000], [0, 8000])
        assert p["main"] == [0, k] and p["aux"] == [0, n // 2 + 1] and p["overlap"] == [0, k + 1] and p["count"] == k + 1
        p = tfft.band_mix_plan(n, 16000, [0, 4000], [4000, 8000])
        assert p["overlap"] == [k, k + 1] and p["count"] == 1
    d = [0, 4000]
    tfft.band_mix_plan(1000, 16000, d, None)
    assert d == [0, 4000]                                   # the caller's list is left alone


# ---- 3. the host-only AudioProcessor methods
def test_audio_processor_host_methods(G):
    from targetdiarization_amd.audio_processor import AudioProcessor
    ap = AudioProcessor(verbose_log=False, cuda_device=-1)
    _host_checks(ap, G)


def test_mix_audio_by_freq_degrades_without_device(G, capsys):
    """the paths that never reach the device, and the never-raise rule on a CPU-only processor"""
    from targetdiarization_amd.audio_processor import AudioProcessor
    ap = AudioProcessor(verbose_log=False, cuda_device=-1)
    a, b = np.ones(8, dtype=np.float32), np.ones(6, dtype=np.float32)
    assert ap.mix_audio_by_freq(a, b) is a                  # lengths differ, no force_align
    one = np.ones(1, dtype=np.float32)
    assert ap.mix_audio_by_freq(one, one) is one
    m2 = np.ones((8, 2), dtype=np.float32)
    assert ap.mix_audio_by_freq(m2, m2) is m2
    assert ap.mix_audio_by_freq(a, a) is a                  # no device: the reason is printed, the input returned
    assert "Failed in mix_audio_by_freq" in capsys.readouterr().out
    import inspect
    sig = inspect.signature(AudioProcessor.mix_audio_by_freq).parameters
    assert [k for k in sig] == ["self", "audio_main", "audio_aux", "sampling_rate", "main_freq_range", "aux_freq_range", "force_align"]
    assert sig["sampling_rate"].default == 16000 and sig["main_freq_range"].default == [0, 4000]
    assert sig["aux_freq_range"].default == [0, 8000] and sig["force_align"].default is False


# ---- 4. argument validation without a GPU
@pytest.fixture(scope="module")
def lib():
    from targetdiarization_amd.build import build_lib
    build_lib()
    return _lib.lib()


def test_workspace_functions_outside_the_limits(lib):
    assert lib.tdx_fft_workspace_bytes(0, 1) == 0 and lib.tdx_fft_workspace_bytes((1 << 26) + 1, 1) == 0
    assert lib.tdx_fft_workspace_bytes(16, 0) == 0 and lib.tdx_fft_workspace_bytes(16, 65536) == 0
    assert lib.tdx_fft_workspace_bytes(1, 1) > 0 and lib.tdx_fft_workspace_bytes(1 << 26, 1) > 0 and lib.tdx_fft_workspace_bytes(1009, 65535) > 0
    assert lib.tdx_fft_band_mix_workspace_bytes(1) == 0 and lib.tdx_fft_band_mix_workspace_bytes((1 << 26) + 1) == 0
    assert lib.tdx_fft_band_mix_workspace_bytes(2) > 0 and lib.tdx_fft_band_mix_workspace_bytes(1 << 26) > 0


def test_argument_validation_without_gpu(lib):
    """every limit of include/tdx.h is TDX_E_INVALID with a message of its own, before the device is touched (the pointers are made up)"""
    X, Y, W = 0x10000, 0x20000, 0x30000
    big = 1 << 40
    calls = {
        "tdx_fft_c2c": lambda x=X, n=64, b=1, y=Y, w=W, wb=big: lib.tdx_fft_c2c(x, n, b, 0, y, w, wb, None),
        "tdx_fft_r2c": lambda x=X, n=64, b=1, y=Y, w=W, wb=big: lib.tdx_fft_r2c(x, n, b, y, w, wb, None),
        "tdx_fft_c2r": lambda x=X, n=64, b=1, y=Y, w=W, wb=big: lib.tdx_fft_c2r(x, n, b, y, w, wb, None),
    }
    for name, call in calls.items():
        msgs = []
        for kw in (dict(x=None), dict(y=None), dict(w=None), dict(n=0), dict(n=(1 << 26) + 1), dict(b=0), dict(b=65536), dict(y=X),
                   dict(x=X + 4), dict(wb=lib.tdx_fft_workspace_bytes(64, 1) - 1), dict(n=1009, wb=lib.tdx_fft_workspace_bytes(1009, 1) - 1)):
            assert call(**kw) == 1, (name, kw)
            msg = lib.tdx_last_error().decode()
            assert msg.startswith(name + ":"), msg
            msgs.append(msg)
        # null / n / batch / in-place / alignment / workspace: six different messages
        assert len(set(msgs)) == 6, msgs

    def mix(m=X, a=Y, n=1000, r=(0, 251, 0, 501, 0, 251), y=0x40000, t=(None, None, None), w=W, wb=big):
        return lib.tdx_fft_band_mix(m, a, n, (C.c_long * 6)(*r) if r is not None else None, y, *t, w, wb, None)
    msgs = []
    for kw in (dict(m=None), dict(a=None), dict(r=None), dict(y=None), dict(w=None), dict(n=1), dict(n=(1 << 26) + 1),
               dict(r=(-1, 251, 0, 501, 0, 251)), dict(r=(0, 502, 0, 501, 0, 251)), dict(r=(0, 251, 300, 200, 0, 251)), dict(r=(0, 251, 0, 501, 0, 502)),
               dict(y=X), dict(y=Y), dict(y=0x40004), dict(t=(0x50004, None, None)), dict(wb=lib.tdx_fft_band_mix_workspace_bytes(1000) - 1)):
        assert mix(**kw) == 1, kw
        msg = lib.tdx_last_error().decode()
        assert msg.startswith("tdx_fft_band_mix:"), msg
        msgs.append(msg)
    # null / n / main range / aux range / overlap range / in-place / alignment / workspace
    assert len(set(msgs)) == 8, msgs


def test_device_fft_needs_a_device():
    with pytest.raises(_lib.TdxError):
        tfft.DeviceFFT("cpu")
    assert tfft.DeviceFFT.TILE == tfft.TILE == 4096
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tdx.h")).read()
    assert f"#define TDX_FFT_TILE {tfft.TILE}\n" in hdr
