"""The any-length FFT over the C-ABI (tdx_fft_*, csrc/fft.hpp) and the band mix behind
`AudioProcessor.mix_audio_by_freq` (the reference's AudioProcessor.py:845-882).

    f = DeviceFFT("cuda:0")
    X = f.fft(x)                      # complex [n] or [batch, n] -> complex64 of the same shape (np.fft.fft)
    x = f.ifft(X)                     # np.fft.ifft
    X = f.rfft(x)                     # real [.., n] -> complex64 [.., n // 2 + 1]
    x = f.irfft(X, n)                 # complex [.., n // 2 + 1] -> float32 [.., n]
    y = f.band_mix(main, aux, plan)   # two real clips [n] -> float32 [2 * (n // 2)]

Every call takes numpy arrays or device tensors and returns the same kind.  `band_mix_plan` is a pure host function (numpy only)."""
from __future__ import annotations

import ctypes as C

import numpy as np

TILE = 4096                       # TDX_FFT_TILE of include/tdx.h: the points one workgroup transforms in LDS
MAX_N = 1 << 26


def band_mix_plan(n: int, sampling_rate, main_freq_range=None, aux_freq_range=None) -> dict:
    """The frequency sets of the reference's mix_audio_by_freq (:858-875) as bin ranges [lo, hi) over the n // 2 + 1 bins of a clip of n
    samples: dict with main_freq_range / aux_freq_range (the clamped limits), main, aux, overlap (the bin ranges), count (the overlap's
    bins) and ranges (the six numbers in the order tdx_fft_band_mix takes them).  The bin frequencies are np.fft.rfftfreq's own fp64
    expression k * (1.0 / (n * (1 / sampling_rate))); it is monotone in k, so every set is one run of bins and its ends are found by
    bisection — no array of n // 2 + 1 frequencies is built."""
    n = int(n)
    if n < 1:
        raise ValueError("band_mix_plan: the clip is empty")
    half = int(sampling_rate / 2)
    if not main_freq_range:
        main_freq_range = [0, int(sampling_rate / 4)]
    if not aux_freq_range:
        aux_freq_range = [0, half]
    mr = [max(0, main_freq_range[0]), min(main_freq_range[1], half)]
    ar = [max(0, aux_freq_range[0]), min(aux_freq_range[1], half)]
    val = 1.0 / (n * (1 / sampling_rate))
    nb = n // 2 + 1

    def first(pred):                      # the first bin k in [0, nb] with pred(k * val); pred is monotone in k
        lo, hi = 0, nb
        while lo < hi:
            mid = (lo + hi) // 2
            if pred(np.float64(mid) * val):
                hi = mid
            else:
                lo = mid + 1
        return lo

    def ge(x):
        return first(lambda f: f >= x)

    def gt(x):
        return first(lambda f: f > x)

    def run(lo, hi):
        return [lo, max(lo, hi)]

    main = run(ge(mr[0]), ge(mr[1]))                             # lo <= f < hi
    aux = run(ge(ar[0]), gt(ar[1]))                              # lo <= f <= hi
    over = run(ge(max(mr[0], ar[0])), gt(min(mr[1], ar[1])))
    return dict(n=n, sampling_rate=sampling_rate, main_freq_range=mr, aux_freq_range=ar, main=main, aux=aux, overlap=over,
                count=over[1] - over[0], ranges=main + aux + over)


class DeviceFFT:
    TILE = TILE

    def __init__(self, device="cuda:0", workspace_budget_bytes: int = 16 << 30):
        import torch

        from . import _lib
        self._lib = _lib
        self._l = _lib.lib()
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.TdxError("DeviceFFT needs a HIP device (cuda:N); there is no CPU path")
        self.device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        self.workspace_budget_bytes = int(workspace_budget_bytes)
        self._guard = _lib.HandleGuard(self.device)

    # ---- plumbing
    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _workspace(self, who, need, what):
        need = int(need)
        if need == 0:
            raise self._lib.TdxError(f"DeviceFFT.{who}: {what} is outside what tdx_fft_* accepts (include/tdx.h)")
        if need > self.workspace_budget_bytes:
            raise self._lib.TdxError(f"DeviceFFT.{who}: {what} needs a workspace of {need} bytes; the budget is {self.workspace_budget_bytes}")
        return self._guard.workspace(need)

    def _in(self, x, who, complex_):
        """-> (device tensor [batch, n] of complex64 / float32, contiguous; is_tensor; is_1d)"""
        import torch
        is_t = isinstance(x, torch.Tensor)
        if is_t:
            t = x.to(self.device, torch.complex64 if complex_ else torch.float32)
        else:
            a = np.asarray(x)
            if not complex_ and np.iscomplexobj(a):
                raise ValueError(f"{who}: the input must be real")
            t = torch.from_numpy(np.require(a, dtype=np.complex64 if complex_ else np.float32, requirements=["C", "W"])).to(self.device)
        if t.ndim not in (1, 2) or t.numel() == 0:
            raise ValueError(f"{who}: the input must be [n] or [batch, n] and not empty, got shape {tuple(t.shape)}")
        return t.reshape(-1, t.shape[-1]).contiguous(), is_t, t.ndim == 1

    @staticmethod
    def _out(t, is_t, one):
        t = t[0] if one else t
        return t if is_t else t.cpu().numpy()

    def _c2c(self, x, inverse, who):
        import torch
        t, is_t, one = self._in(x, who, True)
        b, n = t.shape
        with torch.cuda.device(self.device), self._guard.call():
            ws = self._workspace(who, self._l.tdx_fft_workspace_bytes(n, b), f"{b} rows of {n} points")
            y = torch.empty((b, n), dtype=torch.complex64, device=self.device)
            self._lib.check(self._l.tdx_fft_c2c(torch.view_as_real(t).data_ptr(), n, b, int(inverse), torch.view_as_real(y).data_ptr(), ws.data_ptr(),
                                                ws.numel(), self._stream()))
            return self._out(y, is_t, one)

    # ---- the public calls
    def fft(self, x):
        """np.fft.fft(x) along the last axis"""
        return self._c2c(x, False, "fft")

    def ifft(self, X):
        """np.fft.ifft(X) along the last axis"""
        return self._c2c(X, True, "ifft")

    def rfft(self, x):
        """np.fft.rfft(x) along the last axis"""
        import torch
        t, is_t, one = self._in(x, "rfft", False)
        b, n = t.shape
        with torch.cuda.device(self.device), self._guard.call():
            ws = self._workspace("rfft", self._l.tdx_fft_workspace_bytes(n, b), f"{b} rows of {n} points")
            X = torch.empty((b, n // 2 + 1), dtype=torch.complex64, device=self.device)
            self._lib.check(self._l.tdx_fft_r2c(t.data_ptr(), n, b, torch.view_as_real(X).data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
            return self._out(X, is_t, one)

    def irfft(self, X, n: int):
        """np.fft.irfft(X, n) along the last axis; X holds exactly n // 2 + 1 bins"""
        import torch
        n = int(n)
        t, is_t, one = self._in(X, "irfft", True)
        b = t.shape[0]
        if n < 1 or t.shape[1] != n // 2 + 1:
            raise ValueError(f"irfft: {t.shape[1]} bins do not belong to n = {n} (need n // 2 + 1)")
        with torch.cuda.device(self.device), self._guard.call():
            ws = self._workspace("irfft", self._l.tdx_fft_workspace_bytes(n, b), f"{b} rows of {n} points")
            y = torch.empty((b, n), dtype=torch.float32, device=self.device)
            self._lib.check(self._l.tdx_fft_c2r(torch.view_as_real(t).data_ptr(), n, b, y.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
            return self._out(y, is_t, one)

    def band_mix(self, main, aux, plan, taps=None):
        """The spectra of two real clips [n] blended by frequency band and transformed back: float32 [2 * (n // 2)] (include/tdx.h).
        `plan`: band_mix_plan(n, ...).  `taps`: a dict that receives `main`, `aux` (the two spectra) and `mix` (the blended one), each
        complex64 [n // 2 + 1]."""
        import torch
        m, is_t, one = self._in(main, "band_mix", False)
        a, _, one_a = self._in(aux, "band_mix", False)
        if not (one and one_a) or m.shape != a.shape:
            raise ValueError(f"band_mix: the two clips must be [n] with the same n, got {tuple(m.shape[1:])} and {tuple(a.shape[1:])}")
        n = int(m.shape[1])
        if int(plan["n"]) != n:
            raise ValueError(f"band_mix: the plan is for n = {plan['n']}, the clips have {n} samples")
        ranges = (C.c_long * 6)(*[int(v) for v in plan["ranges"]])
        nb = n // 2 + 1
        with torch.cuda.device(self.device), self._guard.call():
            ws = self._workspace("band_mix", self._l.tdx_fft_band_mix_workspace_bytes(n), f"a clip of {n} samples")
            y = torch.empty(2 * (n // 2), dtype=torch.float32, device=self.device)
            tp = [None] * 3
            if taps is not None:
                tp = [torch.empty(nb, dtype=torch.complex64, device=self.device) for _ in range(3)]
            self._lib.check(self._l.tdx_fft_band_mix(m.data_ptr(), a.data_ptr(), n, ranges, y.data_ptr(),
                                                     *[torch.view_as_real(q).data_ptr() if q is not None else None for q in tp],
                                                     ws.data_ptr(), ws.numel(), self._stream()))
            if taps is not None:
                for key, q in zip(("main", "aux", "mix"), tp):
                    taps[key] = q if is_t else q.cpu().numpy()
            return y if is_t else y.cpu().numpy()
