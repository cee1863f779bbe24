"""CPU test of csrc/dft_basis.hpp, the host helpers that build every "window x DFT" GEMM operand (fbank, MDX, Whisper, Apollo, the
spectral gate, the phase vocoder), through the host-only hooks of libtdx_diag.so.  No device is touched.

The reference is a numpy float64 restatement of the two formulas.  Every entry must lie within one float32 ulp of the largest entry
of its image: half an ulp is the cast, the rest covers the one double ulp by which two libm cos / sin may differ before the cast.
Exact conditions: padding rows and columns are 0.0, the imaginary synthesis columns of DC and Nyquist are 0.0, analysis row 0 is the
window as float32, and column 0 of every analysis row is (win[0], -0 or 0)."""
import ctypes as C
import math

import numpy as np
import pytest

from targetdiarization_amd import _lib


@pytest.fixture(scope="module")
def diag():
    from targetdiarization_amd.build import build_lib
    build_lib()
    return _lib.diag()


def hann(N):      # libm, as the helper computes it
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * i / N) for i in range(N)], dtype=np.float64)


def trig(N, nbin):
    """cos, sin of 2 pi ((k n) mod N) / N as [nbin][N]"""
    idx = (np.arange(nbin, dtype=np.int64)[:, None] * np.arange(N, dtype=np.int64)[None, :]) % N
    ang = 2.0 * np.pi * idx / N
    return np.cos(ang), np.sin(ang)


def stft_geo(n_fft):
    nbin, BP, NPAIR = n_fft // 2 + 1, n_fft // 2 + 16, n_fft // 2 + 64
    return nbin, BP, NPAIR, 2 * BP


def run_analysis(diag, N, nbin, im_row0, ld, rows, use_hann):
    out = np.zeros((rows, ld), dtype=np.float32)
    assert diag.tdx_diag_dft_analysis(N, nbin, im_row0, ld, rows, int(use_hann), out.ctypes.data_as(C.c_void_p)) == 0, diag.tdx_diag_last_error()
    return out


def run_synthesis(diag, N, nbin, im_off, ld, gain_kind):
    out = np.zeros((N, ld), dtype=np.float32)
    assert diag.tdx_diag_dft_synthesis(N, nbin, im_off, ld, gain_kind, out.ctypes.data_as(C.c_void_p)) == 0, diag.tdx_diag_last_error()
    return out


def close_to(got, ref):
    tol = float(np.spacing(np.float32(np.abs(ref).max())))
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"max |got - ref| = {err:.3e}, one float32 ulp of the largest entry = {tol:.3e}")
    return err <= tol


ANALYSIS = {      # N, nbin, im_row0, ld, rows, hann
    "fbank": (512, 257, 320, 512, 640, False),
    "whisper": (400, 201, 256, 416, 512, True),
    "apollo": (882, 442, 442, 896, 896, True),
    "stft128": (128,) + (stft_geo(128)[0], stft_geo(128)[2], 128, 2 * stft_geo(128)[2], True),
    "stft1024": (1024,) + (stft_geo(1024)[0], stft_geo(1024)[2], 1024, 2 * stft_geo(1024)[2], True),
}


@pytest.mark.parametrize("name", list(ANALYSIS))
def test_analysis_basis(diag, name):
    N, nbin, im_row0, ld, rows, use_hann = ANALYSIS[name]
    got = run_analysis(diag, N, nbin, im_row0, ld, rows, use_hann)
    win = hann(N) if use_hann else np.ones(N)
    cs, sn = trig(N, nbin)
    ref = np.zeros((rows, ld))
    ref[:nbin, :N] = win * cs
    ref[im_row0:im_row0 + nbin, :N] = -win * sn
    assert close_to(got, ref)
    written = np.zeros((rows, ld), dtype=bool)
    written[:nbin, :N] = True
    written[im_row0:im_row0 + nbin, :N] = True
    assert not got[~written].any() and not np.signbit(got[~written]).any()      # padding rows and columns: +0.0, never written
    assert np.array_equal(got[0, :N], win.astype(np.float32))                   # bin 0: cos = 1
    assert np.all(got[:nbin, 0] == np.float32(win[0]))                          # n = 0: cos = 1 ...
    assert np.all(got[im_row0:im_row0 + nbin, 0] == 0.0)                        # ... and -win * sin(0) = -0.0 or 0.0


SYNTHESIS = {     # N, nbin, im_off, ld, gain_kind (0: 1 / N, 1: hann / 4, 2: hann / N)
    "gate1024": (1024, stft_geo(1024)[0], stft_geo(1024)[1], stft_geo(1024)[3], 1),
    "pvoc1024": (1024, stft_geo(1024)[0], stft_geo(1024)[1], stft_geo(1024)[3], 2),
    "pvoc128": (128, stft_geo(128)[0], stft_geo(128)[1], stft_geo(128)[3], 2),
    "mdx384": (384, 128, 128, 256, 0),                                          # nbin < N / 2 + 1: no Nyquist column
}


@pytest.mark.parametrize("name", list(SYNTHESIS))
def test_synthesis_basis(diag, name):
    N, nbin, im_off, ld, kind = SYNTHESIS[name]
    got = run_synthesis(diag, N, nbin, im_off, ld, kind)
    gain = np.full(N, 1.0 / N) if kind == 0 else hann(N) * 0.25 if kind == 1 else hann(N) / N
    cs, sn = trig(N, nbin)
    k = np.arange(nbin)
    edge = (k == 0) | (2 * k == N)
    coef = gain[:, None] * np.where(edge, 1.0, 2.0)[None, :]
    ref = np.zeros((N, ld))
    ref[:, :nbin] = coef * cs.T
    ref[:, im_off:im_off + nbin] = np.where(edge[None, :], 0.0, -coef * sn.T)
    assert close_to(got, ref)
    written = np.zeros((N, ld), dtype=bool)
    written[:, :nbin] = True
    written[:, im_off:im_off + nbin] = True
    assert not got[~written].any() and not np.signbit(got[~written]).any()      # padding columns
    assert not got[:, im_off].any()                                             # Im of DC is ignored
    if 2 * (nbin - 1) == N:
        assert not got[:, im_off + nbin - 1].any()                              # Im of Nyquist too
        assert np.array_equal(got[:, nbin - 1], (gain * np.where(np.arange(N) % 2, -1.0, 1.0)).astype(np.float32))   # weight 1, not 2
    assert np.array_equal(got[:, 0], gain.astype(np.float32))                   # DC: weight 1, cos = 1


def test_hooks_refuse_what_would_leave_the_buffer(diag):
    buf = np.zeros(16, dtype=np.float32).ctypes.data_as(C.c_void_p)
    assert diag.tdx_diag_dft_analysis(8, 5, 4, 8, 16, 0, buf) == 1       # im rows overlap the re rows
    assert diag.tdx_diag_dft_analysis(8, 5, 8, 8, 12, 0, buf) == 1       # im rows beyond `rows`
    assert diag.tdx_diag_dft_analysis(8, 5, 8, 4, 16, 0, buf) == 1       # ld < N
    assert diag.tdx_diag_dft_analysis(8, 6, 8, 8, 16, 0, buf) == 1       # nbin > N / 2 + 1
    assert diag.tdx_diag_dft_synthesis(8, 5, 8, 12, 0, buf) == 1         # im columns beyond ld
    assert diag.tdx_diag_dft_synthesis(8, 5, 8, 16, 3, buf) == 1         # unknown gain
