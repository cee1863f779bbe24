"""noisereduce's spectral gate over the C-ABI (tdx_ngate_*): `nr.reduce_noise(y=audio_data, sr=sampling_rate)`, the body of the
reference's `denoise_vocal` when the MDX model is absent or `fast_mode` is set (AudioProcessor.py:645-656).  Non-stationary mode
with noisereduce's defaults; the package is third-party and not available here, so the algorithm — the chunk plan, the
`filtfilt` smoothing, the sigmoid mask, the triangular mask filter — is restated from upstream (parity with the package itself
is unpinned; parity with a float64 scipy restatement of the same steps is what the tests pin).

    gate = SpectralGate("cuda:0")
    y = gate.reduce_noise(x, 16000)                       # [n] or [C, n] -> float32 ndarray of the same shape
    ys = gate.reduce_noise_batch([x0, x1, ...], 16000)    # all clips in one launch sequence

One deviation: where the smoothed magnitude is exactly 0 (digital silence) upstream divides 0 by 0 and returns NaN; the mask is
0 there.  `chunk_plan` and `gate_params` are pure host functions."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

N_FFT, HOP, NBIN = 1024, 256, 513
DEFAULTS = dict(prop_decrease=1.0, time_constant_s=2.0, freq_mask_smooth_hz=500, time_mask_smooth_ms=50,
                thresh_n_mult_nonstationary=2, sigmoid_slope_nonstationary=10, chunk_size=600000, padding=30000)


def chunk_plan(n: int, chunk_size: int = 600000, padding: int = 30000):
    """noisereduce's chunking of one channel of n samples: a list of (lo, hi, keep_lo, keep_hi) in clip coordinates.  A buffer
    covers [lo, hi) (samples outside [0, n) are zero), is gated on its own, and its samples [keep_lo, keep_hi) are kept."""
    n, chunk_size, padding = int(n), int(chunk_size), int(padding)
    if n < 1:
        raise ValueError("chunk_plan: the clip is empty")
    if chunk_size < 1:
        raise ValueError("chunk_plan: chunk_size must be >= 1")
    if padding < N_FFT:
        raise ValueError(f"chunk_plan: padding must be >= {N_FFT} (every kept sample needs its four STFT frames), got {padding}")
    if n <= chunk_size:
        return [(-padding, n + padding, 0, n)]
    return [(s - padding, s + chunk_size + padding, s, min(s + chunk_size, n)) for s in range(0, n, chunk_size)]


def tri(k: int) -> np.ndarray:
    """noisereduce's triangle of 2k + 1 taps: concatenate(linspace(0, 1, k + 1, endpoint=False), linspace(1, 0, k + 2))[1:-1]"""
    return np.concatenate([np.linspace(0, 1, k + 1, endpoint=False), np.linspace(1, 0, k + 2)])[1:-1]


def gate_params(sr, time_constant_s: float = 2.0, freq_mask_smooth_hz=500, time_mask_smooth_ms=50):
    """(b, nf, nt, (freq_taps, time_taps)): the coefficient of the time smoothing filtfilt([b], [1, b - 1]), the half widths of
    the mask filter in bins and frames, and its two normalised marginals (their outer product is noisereduce's filter)."""
    sr = float(sr)
    if not sr > 0:
        raise ValueError("gate_params: sr must be positive")
    t = float(time_constant_s) * sr / HOP
    if not t > 0:
        raise ValueError("gate_params: time_constant_s must be positive")
    b = (np.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t)
    nf = int(freq_mask_smooth_hz / (sr / (N_FFT / 2))) if freq_mask_smooth_hz else 0
    nt = int(time_mask_smooth_ms / ((HOP / sr) * 1000.0)) if time_mask_smooth_ms else 0
    if not (0 <= nf <= 128 and 0 <= nt <= 128):
        raise ValueError(f"gate_params: the mask filter of {nf} bins x {nt} frames is outside the supported 0 .. 128")
    tf, tt = tri(nf), tri(nt)
    return float(b), nf, nt, (tf / tf.sum(), tt / tt.sum())


class SpectralGate:
    def __init__(self, device="cuda:0", rows_per_launch: int = 16384):
        self._l = _lib.lib()
        self.rows_per_launch = int(rows_per_launch)
        if self.rows_per_launch < 4:
            raise _lib.TdxError("SpectralGate: rows_per_launch must be >= 4")
        self._own = _lib.Handle(device, "SpectralGate", self._l.tdx_ngate_create, self._l.tdx_ngate_destroy)
        self.device, self._h, self._guard = self._own.device, self._own.ptr, self._own.guard

    def table(self, shapes, chunk_size: int, padding: int):
        """the buffer table of tdx_ngate_forward (include/tdx.h) for clips of `shapes` = [(channels, n), ...] packed back to
        back, channel after channel -> (int64 [nbuf, 8], rows of the largest round)"""
        rows_of = lambda L: L // HOP + 1 + 3
        tab, off, row, max_rows = [], 0, 0, 0
        for (ch, n) in shapes:
            for _ in range(ch):
                for (lo, hi, k0, k1) in chunk_plan(n, chunk_size, padding):
                    L = hi - lo
                    r = rows_of(L)
                    if r > self.rows_per_launch:
                        raise _lib.TdxError(f"SpectralGate: a buffer of {L} samples needs {r} rows; rows_per_launch is {self.rows_per_launch}")
                    if row and row + r > self.rows_per_launch:
                        row = 0
                    tab.append((off + lo, max(0, -lo), min(L, n - lo), k0 - lo, k1 - lo, off + k0, L, row))
                    row += r
                    max_rows = max(max_rows, row)
                off += n
        return np.asarray(tab, dtype=np.int64).reshape(-1, 8), max_rows

    def reduce_noise_batch(self, clips, sr, prop_decrease: float = 1.0, time_constant_s: float = 2.0, freq_mask_smooth_hz=500,
                           time_mask_smooth_ms=50, thresh_n_mult_nonstationary=2, sigmoid_slope_nonstationary=10,
                           chunk_size: int = 600000, padding: int = 30000, taps=None):
        """clips: arrays [n] or [C, n] (rows are channels, as noisereduce reads them) -> list of float32 ndarrays of the same
        shapes.  `taps`: a dict that receives `mag`, `smooth`, `mask`, `mask_smooth` [F, 513] of the first buffer of the call."""
        arrs = [np.ascontiguousarray(np.asarray(c), dtype=np.float32) for c in clips]
        if not arrs:
            return []
        for a in arrs:
            if a.ndim not in (1, 2) or a.size == 0:
                raise ValueError(f"SpectralGate: a clip must be [n] or [C, n] and not empty, got shape {a.shape}")
        b, nf, nt, _ = gate_params(sr, time_constant_s, freq_mask_smooth_hz, time_mask_smooth_ms)
        shapes = [(1, a.shape[0]) if a.ndim == 1 else a.shape for a in arrs]
        tab, max_rows = self.table(shapes, chunk_size, padding)
        nbuf = tab.shape[0]
        tab_h = (C.c_int64 * tab.size)(*tab.reshape(-1).tolist())
        flat = np.concatenate([a.reshape(-1) for a in arrs]) if len(arrs) > 1 else arrs[0].reshape(-1)
        with torch.cuda.device(self.device), self._guard.call():
            x = torch.from_numpy(flat).to(self.device)
            y = torch.empty_like(x)
            tab_d = torch.from_numpy(tab).to(self.device)
            tp = [None] * 4
            if taps is not None:
                F = int(tab[0, 6]) // HOP + 1
                tp = [torch.empty((F, NBIN), dtype=torch.float32, device=self.device) for _ in range(4)]
            self.launch(x, y, tab_h, tab_d, nbuf, max_rows, b, nf, nt, float(thresh_n_mult_nonstationary), float(sigmoid_slope_nonstationary),
                        float(prop_decrease), tp)
            out = y.cpu().numpy()
            if taps is not None:
                for k, t in zip(("mag", "smooth", "mask", "mask_smooth"), tp):
                    taps[k] = t.cpu().numpy()
        outs, o = [], 0
        for a in arrs:
            outs.append(out[o:o + a.size].reshape(a.shape))
            o += a.size
        return outs

    def launch(self, x, y, tab_h, tab_d, nbuf, max_rows, b, nf, nt, thresh=2.0, slope=10.0, prop=1.0, taps=(None, None, None, None)):
        """enqueue tdx_ngate_forward on the current stream: x, y packed float32 device tensors, the table as a ctypes int64 array
        and as a device tensor (inside `with self._guard.call():`; tools/noise_gate_bench.py times this)"""
        ws = self._guard.workspace(int(self._l.tdx_ngate_workspace_bytes(self._h, max_rows)))
        st = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._l.tdx_ngate_forward(self._h, x.data_ptr(), x.numel(), tab_h, tab_d.data_ptr(), nbuf, self.rows_per_launch, b, nf, nt,
                                             thresh, slope, prop, y.data_ptr(), *[t.data_ptr() if t is not None else None for t in taps],
                                             ws.data_ptr(), ws.numel(), st))

    def reduce_noise(self, y, sr, **params):
        return self.reduce_noise_batch([y], sr, **params)[0]

    def close(self):
        self._own.close()
