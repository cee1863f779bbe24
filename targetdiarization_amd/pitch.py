"""Probabilistic YIN pitch tracking over the C-ABI (tdx_pyin_*): `librosa.pyin(audio, fmin=fmin, fmax=fmax, sr=sampling_rate)`,
the body of the reference's `ASRProcessor.f0_compute` (ASRProcessor.py:1003-1010).  librosa is third-party and not available
here, so the algorithm — the cumulative mean normalised difference, the parabolic shifts, the Boltzmann / beta trough
probabilities, the banded transition matrix, the Viterbi decoding — is restated from upstream's published source (parity with the
package itself is unpinned; parity with a float64 numpy/scipy restatement of the same steps is what the tests pin).

    p = Pyin("cuda:0")
    f0, voiced_flag, voiced_prob = p.pyin(y, fmin=50.0, fmax=300.0, sr=16000)     # y [n] or [C, n]
    results = p.pyin_batch([y0, y1, ...], fmin=50.0, fmax=300.0, sr=16000)        # all clips in one launch sequence

Two deviations: the difference function is summed directly in float32 (upstream: an FFT autocorrelation whose terms below 1e-6
are flushed to 0, which only matters for frames near -90 dBFS), and `pad_mode` must be "constant".  `pyin_plan` is a pure host
function."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from . import _lib

TINY = float(np.finfo(np.float64).tiny)
MAX_FRAME, MAX_PERIOD, MAX_STATES, MAX_THRESH = 8192, 4096, 4096, 254


def triangle(width: int) -> np.ndarray:
    """scipy.signal.get_window("triangle", width, fftbins=False) for odd width: (1 .. h .. 1) / h, h = (width + 1) / 2"""
    h = (width + 1) // 2
    up = np.arange(1, h + 1, dtype=np.float64) * 2.0 / (width + 1)
    return np.concatenate([up, up[-2::-1]])


def pyin_plan(sr, fmin, fmax, frame_length: int = 2048, win_length=None, hop_length=None, n_thresholds: int = 100,
              beta_parameters=(2, 18), boltzmann_parameter=2, resolution: float = 0.1, max_transition_rate: float = 35.92,
              switch_prob: float = 0.01, no_trough_prob: float = 0.01, center: bool = True, pad_mode: str = "constant"):
    """The host side of one pyin configuration: periods, pitch bins, transition width, the threshold and Boltzmann tables and the
    log transition band.  Raises TdxError where upstream raises (and for what the device does not support).  `.frames(n)` is the
    frame count of a clip of n samples."""
    E = _lib.TdxError
    if fmin is None or fmax is None:
        raise E("pyin: both fmin and fmax must be provided")
    sr, fmin, fmax = float(sr), float(fmin), float(fmax)
    frame_length = int(frame_length)
    win_length = frame_length // 2 if win_length is None else int(win_length)
    hop_length = frame_length // 4 if hop_length is None else int(hop_length)
    if pad_mode != "constant":
        raise E(f"pyin: pad_mode {pad_mode!r} is unsupported (only \"constant\")")
    if not (sr > 0 and fmax > fmin > 0):
        raise E(f"pyin: need sr > 0 and 0 < fmin < fmax, got sr={sr}, fmin={fmin}, fmax={fmax}")
    if not 4 <= frame_length <= MAX_FRAME:
        raise E(f"pyin: frame_length={frame_length} is outside the supported 4 .. {MAX_FRAME}")
    if not 1 <= win_length < frame_length:
        raise E(f"pyin: win_length={win_length} cannot exceed given frame_length={frame_length}")
    if hop_length < 1:
        raise E(f"pyin: hop_length={hop_length} must be a positive integer")
    if not 1 <= int(n_thresholds) <= MAX_THRESH:
        raise E(f"pyin: n_thresholds={n_thresholds} is outside the supported 1 .. {MAX_THRESH}")
    if not (0.0 <= switch_prob <= 1.0 and 0.0 <= no_trough_prob <= 1.0):
        raise E("pyin: switch_prob and no_trough_prob must lie in [0, 1]")
    if not 0 < resolution < 1:
        raise E(f"pyin: resolution={resolution} must be in range (0, 1)")
    if not max_transition_rate > 0:
        raise E("pyin: max_transition_rate must be strictly positive")
    min_period = max(int(np.floor(sr / fmax)), 1)
    max_period = min(int(np.ceil(sr / fmin)), frame_length - win_length - 1)
    if max_period - min_period < 2:
        raise E(f"pyin: min(ceil(sr / fmin), frame_length - win_length - 1) = {max_period} must be at least floor(sr / fmax) + 2 = {min_period + 2}")
    if max_period > MAX_PERIOD:
        raise E(f"pyin: max_period={max_period} is above the supported {MAX_PERIOD}")
    n_lags = max_period - min_period + 1
    bps = int(np.ceil(1.0 / resolution))
    n_pitch_bins = int(np.floor(12 * bps * np.log2(fmax / fmin))) + 1
    width = int(round(max_transition_rate * 12 * hop_length / sr)) * bps + 1
    if n_pitch_bins < width:
        raise E(f"pyin: the transition width {width} exceeds the {n_pitch_bins} pitch bins (upstream raises too)")
    if width % 2 == 0:
        raise E(f"pyin: an even transition width ({width}) is unsupported")
    if 2 * n_pitch_bins > MAX_STATES:
        raise E(f"pyin: {2 * n_pitch_bins} states are above the supported {MAX_STATES}")
    from scipy.stats import beta as _beta
    nth = int(n_thresholds)
    thr = np.linspace(0, 1, nth + 1)
    beta_probs = np.diff(_beta.cdf(thr, beta_parameters[0], beta_parameters[1]))
    beta_cum = np.array([np.sum(beta_probs[:m]) for m in range(nth + 1)])
    lam = float(boltzmann_parameter)
    cnt = np.arange(n_lags + 1, dtype=np.float64)
    with np.errstate(divide="ignore"):
        bfact = (1 - np.exp(-lam)) / (1 - np.exp(-lam * cnt))
    bfact[0] = 0.0
    bexp = np.exp(-lam * cnt)
    tri = triangle(width)
    hw = width // 2
    rows = np.empty(n_pitch_bins)
    for i in range(n_pitch_bins):
        rows[i] = np.sum(tri[max(0, hw - i): min(width, hw + n_pitch_bins - i)])
    tables = np.concatenate([thr, beta_probs, beta_cum, bfact, bexp, np.log(tri), -np.log(rows)]).astype(np.float64)
    params = _lib.PyinParams(frame_length=frame_length, win_length=win_length, hop_length=hop_length, center=int(bool(center)),
                             min_period=min_period, max_period=max_period, n_pitch_bins=n_pitch_bins, n_thresholds=nth, width=width,
                             sr=sr, fmin=fmin, bins_per_octave=float(12 * bps), no_trough_prob=float(no_trough_prob),
                             log_stay=float(np.log(1.0 - switch_prob + TINY)), log_switch=float(np.log(switch_prob + TINY)),
                             log_init_unvoiced=float(np.log(1.0 / n_pitch_bins + TINY)))

    def frames(n: int) -> int:
        n = int(n)
        if center:
            return 1 + n // hop_length
        if n < frame_length:
            raise E(f"pyin: input is too short (n={n}) for frame_length={frame_length}")
        return 1 + (n - frame_length) // hop_length

    return SimpleNamespace(sr=sr, fmin=fmin, fmax=fmax, frame_length=frame_length, win_length=win_length, hop_length=hop_length,
                           center=bool(center), min_period=min_period, max_period=max_period, n_lags=n_lags, bins_per_semitone=bps,
                           n_pitch_bins=n_pitch_bins, width=width, thresholds=thr, beta_probs=beta_probs, triangle=tri, row_sums=rows,
                           log_band=np.log(tri)[None, :] - np.log(rows)[:, None], tables=tables, params=params, frames=frames,
                           freqs=fmin * 2.0 ** (np.arange(n_pitch_bins) / (12.0 * bps)))


class Pyin:
    def __init__(self, device="cuda:0"):
        self._l = _lib.lib()
        self._own = _lib.Handle(device, "Pyin", self._l.tdx_pyin_create, self._l.tdx_pyin_destroy)
        self.device, self._h, self._guard = self._own.device, self._own.ptr, self._own.guard

    def _tables(self, plan):
        import torch
        return torch.from_numpy(plan.tables).to(self.device)

    def launch(self, plan, x, tab_h, tab_d, nclips, tables_d, states, vprob, taps=(None, None, None)):
        """enqueue tdx_pyin_forward on the current stream (inside `with self._guard.call():`; tools/pyin_bench.py times this)"""
        import torch
        frames = int(states.numel())
        ws = self._guard.workspace(int(self._l.tdx_pyin_workspace_bytes(self._h, C.byref(plan.params), frames)))
        st = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._l.tdx_pyin_forward(self._h, x.data_ptr(), x.numel(), tab_h, tab_d.data_ptr(), nclips, C.byref(plan.params),
                                            tables_d.data_ptr(), tables_d.numel(), states.data_ptr(), vprob.data_ptr(),
                                            *[t.data_ptr() if t is not None else None for t in taps], ws.data_ptr(), ws.numel(), st))

    def launch_viterbi(self, plan, obs, tables_d, states):
        """enqueue tdx_pyin_viterbi over obs [T, 2 n_pitch_bins] on the current stream (inside `with self._guard.call():`)"""
        import torch
        T = int(obs.shape[0])
        ws = self._guard.workspace(int(self._l.tdx_pyin_workspace_bytes(self._h, C.byref(plan.params), T)))
        st = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._l.tdx_pyin_viterbi(self._h, obs.data_ptr(), T, C.byref(plan.params), tables_d.data_ptr(), tables_d.numel(),
                                            states.data_ptr(), ws.data_ptr(), ws.numel(), st))

    def viterbi(self, obs, plan) -> np.ndarray:
        """the decoding stage alone: obs [T, 2 n_pitch_bins] probabilities (float32) -> int64 states [T]"""
        import torch
        o = np.ascontiguousarray(np.asarray(obs), dtype=np.float32)
        if o.ndim != 2 or o.shape[0] < 1 or o.shape[1] != 2 * plan.n_pitch_bins:
            raise ValueError(f"Pyin.viterbi: obs must be [T >= 1, {2 * plan.n_pitch_bins}], got {o.shape}")
        with torch.cuda.device(self.device), self._guard.call():
            od = torch.from_numpy(o).to(self.device)
            states = torch.empty(o.shape[0], dtype=torch.int32, device=self.device)
            self.launch_viterbi(plan, od, self._tables(plan), states)
            return states.cpu().numpy().astype(np.int64)

    def pyin_batch(self, clips, *, fmin, fmax, sr=22050, frame_length: int = 2048, win_length=None, hop_length=None,
                   n_thresholds: int = 100, beta_parameters=(2, 18), boltzmann_parameter=2, resolution: float = 0.1,
                   max_transition_rate: float = 35.92, switch_prob: float = 0.01, no_trough_prob: float = 0.01, fill_na=np.nan,
                   center: bool = True, pad_mode: str = "constant", taps=None):
        """clips: arrays [n] or [C, n] -> list of (f0, voiced_flag, voiced_prob), float64 / bool / float64 of shape [T] or [C, T].
        `taps`: a dict that receives `yin`, `shifts` [frames, n_lags], `obs` [frames, 2 n_pitch_bins] and `states` [frames] of
        all frames of the call (the channels of the clips in order)."""
        import torch
        plan = pyin_plan(sr, fmin, fmax, frame_length, win_length, hop_length, n_thresholds, beta_parameters, boltzmann_parameter,
                         resolution, max_transition_rate, switch_prob, no_trough_prob, center, pad_mode)
        arrs = [np.ascontiguousarray(np.asarray(c), dtype=np.float32) for c in clips]
        if not arrs:
            return []
        for a in arrs:
            if a.ndim not in (1, 2) or a.size == 0:
                raise ValueError(f"Pyin: a clip must be [n] or [C, n] and not empty, got shape {a.shape}")
            if not np.isfinite(a).all():
                raise _lib.TdxError("Pyin: audio buffer is not finite everywhere")
        tab, off, frame0 = [], 0, 0
        for a in arrs:
            n = a.shape[-1]
            T = plan.frames(n)
            for _ in range(1 if a.ndim == 1 else a.shape[0]):
                tab.append((off, n, frame0, T))
                off += n
                frame0 += T
        tab = np.asarray(tab, dtype=np.int64).reshape(-1, 4)
        if tab.shape[0] > 65535:
            raise _lib.TdxError("Pyin: more than 65535 channels in one call")
        tab_h = (C.c_int64 * tab.size)(*tab.reshape(-1).tolist())
        flat = np.concatenate([a.reshape(-1) for a in arrs])                 # (a copy: the caller's array may be read-only)
        with torch.cuda.device(self.device), self._guard.call():
            x = torch.from_numpy(flat).to(self.device)
            tab_d = torch.from_numpy(tab).to(self.device)
            states = torch.empty(frame0, dtype=torch.int32, device=self.device)
            vprob = torch.empty(frame0, dtype=torch.float32, device=self.device)
            tp = [None] * 3
            if taps is not None:
                tp = [torch.empty((frame0, w), dtype=torch.float32, device=self.device) for w in (plan.n_lags, plan.n_lags, 2 * plan.n_pitch_bins)]
            self.launch(plan, x, tab_h, tab_d, tab.shape[0], self._tables(plan), states, vprob, tp)
            st = states.cpu().numpy().astype(np.int64)
            vp = vprob.cpu().numpy().astype(np.float64)
            if taps is not None:
                for k, t in zip(("yin", "shifts", "obs"), tp):
                    taps[k] = t.cpu().numpy()
                taps["states"] = st
        f0 = plan.freqs[st % plan.n_pitch_bins]
        voiced = st < plan.n_pitch_bins
        if fill_na is not None:
            f0[~voiced] = fill_na
        outs, o = [], 0
        for a in arrs:
            ch = 1 if a.ndim == 1 else a.shape[0]
            T = plan.frames(a.shape[-1])
            shape = (T,) if a.ndim == 1 else (ch, T)
            sl = slice(o, o + ch * T)
            outs.append((f0[sl].reshape(shape), voiced[sl].reshape(shape), vp[sl].reshape(shape)))
            o += ch * T
        return outs

    def pyin(self, y, *, fmin, fmax, sr=22050, **params):
        return self.pyin_batch([y], fmin=fmin, fmax=fmax, sr=sr, **params)[0]

    def close(self):
        self._own.close()
