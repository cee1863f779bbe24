"""Phase-vocoder time stretch, pitch shift and EQ match over the C-ABI (tdx_pvoc_*, tdx_resample_sinc): the bodies of the
reference's `audio_stretch` (AudioProcessor.py:468-499, its `librosa.effects.time_stretch` branch), `audio_pitch` (:452-465,
`librosa.effects.pitch_shift`) and `eq_match` (:502-546).  librosa is third-party and not available here, so the algorithms —
stft / phase_vocoder / istft with librosa 0.10's defaults — are restated from upstream; parity with the package itself is
unpinned, parity with a float64 numpy restatement of the same steps is what the tests pin.  The resampler behind
the pitch shift is the project's own windowed sinc (upstream: soxr_hq, which cannot be matched).

    pv = PhaseVocoder("cuda:0")
    y = pv.time_stretch(x, 0.8)                # [n] or [C, n] -> float32 [round(n / 0.8)] or [C, ...]
    y = pv.pitch_shift(x, 16000, 3)            # same shape as x
    y = pv.eq_match(source, target)            # [n] -> [hop * (n // hop)]
    D2 = pv.phase_vocoder(D, 0.8)              # complex64 [bins, T] -> [bins, T']
    y = pv.resample(x, 2 ** (-3 / 12))         # [ceil(n * ratio)]

`stretch_plan` and `pitch_plan` are pure host functions (numpy only)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

N_FFT, HOP = 2048, 512
SEG, SLOTS = 16, 32              # TDX_PVOC_SEG, TDX_PVOC_SLOTS of include/tdx.h: frames per scan segment, segments per sweep
SWEEP = SEG * SLOTS              # output frames one sweep of the phase scan covers


def stretch_plan(n: int, rate: float, n_fft: int = N_FFT, hop: int = HOP):
    """librosa.effects.time_stretch(y[n], rate) as a plan: dict with T (analysis frames), T_out (= len(arange(0, T, rate))),
    idx (int32 [T_out], the first of the two columns of output frame t), alpha (float64 [T_out], the weight of the second) and
    length (= int(round(n / rate)), the samples the iSTFT is asked for)."""
    n, rate = int(n), float(rate)
    if n < 1:
        raise ValueError("stretch_plan: the clip is empty")
    if not (rate > 0 and math.isfinite(rate)):
        raise ValueError(f"stretch_plan: rate must be a positive number, got {rate}")
    T = 1 + n // int(hop)
    steps = np.arange(0, T, rate, dtype=np.float64)
    length = int(round(n / rate))
    if length < 1:
        raise ValueError(f"stretch_plan: {n} samples at rate {rate} leave no output")
    return dict(n=n, rate=rate, n_fft=int(n_fft), hop=int(hop), T=T, T_out=int(steps.shape[0]), idx=steps.astype(np.int64).astype(np.int32),
                alpha=np.mod(steps, 1.0), length=length)


def pitch_plan(n: int, n_steps: float, bins_per_octave: int = 12, n_fft: int = N_FFT, hop: int = HOP):
    """librosa.effects.pitch_shift(y[n], n_steps=...) as a plan: the stretch plan at rate = 2 ** (-n_steps / bins_per_octave),
    plus ratio (= rate: the stretched clip is resampled from sr / rate to sr), n_out (= ceil(length * ratio), what the
    resampler yields) and n_final (= n: fix_length crops or zero-pads to the input's length)."""
    if int(bins_per_octave) != bins_per_octave or bins_per_octave < 1:
        raise ValueError("pitch_plan: bins_per_octave must be a positive integer")
    rate = 2.0 ** (-float(n_steps) / int(bins_per_octave))
    p = stretch_plan(n, rate, n_fft, hop)
    p.update(ratio=rate, n_out=int(math.ceil(p["length"] * rate)), n_final=int(n))
    return p


def _rows(y, who):
    a = np.require(np.asarray(y), dtype=np.float32, requirements=["C", "W"])      # (a read-only array is copied: torch wants it writable)
    if a.ndim not in (1, 2) or a.size == 0:
        raise ValueError(f"{who}: the audio must be [n] or [C, n] and not empty, got shape {a.shape}")
    return a.reshape(-1, a.shape[-1]), a.ndim == 1


class PhaseVocoder:
    def __init__(self, device="cuda:0", workspace_budget_bytes: int = 8 << 30):
        from . import _lib
        self._lib = _lib
        self._l = _lib.lib()
        self.workspace_budget_bytes = int(workspace_budget_bytes)
        self._own = _lib.Handle(device, "PhaseVocoder", self._l.tdx_pvoc_create, self._l.tdx_pvoc_destroy)
        self.device, self._h, self._guard = self._own.device, self._own.ptr, self._own.guard
        self.launches = 0                    # kernel launches of the last call (tools/pvoc_bench.py reports them)

    # ---- plumbing
    def _open(self, who):
        if not self._h:
            raise self._lib.TdxError(f"PhaseVocoder.{who}: the object is closed")

    def _workspace(self, who, n_fft, hop, ch, n, t_out):
        need = int(self._l.tdx_pvoc_workspace_bytes(self._h, n_fft, hop, ch, n, t_out))
        if need == 0:
            raise self._lib.TdxError(f"PhaseVocoder.{who}: n_fft {n_fft}, hop {hop}, {ch} channels of {n} samples, {t_out} output frames are "
                                     "outside what tdx_pvoc_* accepts (include/tdx.h)")
        if need > self.workspace_budget_bytes:
            raise self._lib.TdxError(f"PhaseVocoder.{who}: {ch} channels of {n} samples need a workspace of {need} bytes; the budget is "
                                     f"{self.workspace_budget_bytes}")
        return self._guard.workspace(need)

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _plan_dev(self, plan):
        import torch
        idx = np.ascontiguousarray(plan["idx"], dtype=np.int32)
        idx_h = idx.ctypes.data_as(C.c_void_p)
        return idx, idx_h, torch.from_numpy(idx).to(self.device), torch.from_numpy(np.ascontiguousarray(plan["alpha"])).to(self.device)

    @staticmethod
    def _ptr(t):
        return t.data_ptr() if t is not None else None

    def _stretch_dev(self, x, plan, taps):
        """x: device float32 [C, n] -> device [C, length]; inside `with self._guard.call():`"""
        import torch
        ch, n = x.shape
        nb = plan["n_fft"] // 2 + 1
        ws = self._workspace("time_stretch", plan["n_fft"], plan["hop"], ch, n, plan["T_out"])
        idx, idx_h, idx_d, alpha_d = self._plan_dev(plan)
        y = torch.empty((ch, plan["length"]), dtype=torch.float32, device=self.device)
        t_spec = t_str = None
        if taps is not None:
            t_spec = torch.empty((ch, plan["T"], nb, 2), dtype=torch.float32, device=self.device)
            t_str = torch.empty((ch, plan["T_out"], nb, 2), dtype=torch.float32, device=self.device)
        self._lib.check(self._l.tdx_pvoc_stretch(self._h, x.data_ptr(), ch, n, idx_h, idx_d.data_ptr(), alpha_d.data_ptr(), plan["T_out"],
                                                 plan["length"], y.data_ptr(), self._ptr(t_spec), self._ptr(t_str), ws.data_ptr(), ws.numel(),
                                                 self._stream()))
        self.launches = 5 + (2 if taps is not None else 0)
        return y, t_spec, t_str

    @staticmethod
    def _cplx(t, mono):
        """device float [C, T, bins, 2] -> complex64 ndarray [C, bins, T] ([bins, T] for mono)"""
        a = np.ascontiguousarray(t.cpu().numpy()).view(np.complex64)[..., 0].transpose(0, 2, 1)
        return a[0] if mono else a

    # ---- the public calls
    def time_stretch(self, y, rate, taps=None):
        """librosa.effects.time_stretch(y, rate=rate).  `taps`: a dict that receives `spec` (the analysis spectrum, complex64
        [bins, T] or [C, bins, T]), `stretched` ([.., bins, T']) and `synth` (= the result)."""
        import torch
        self._open("time_stretch")
        a, mono = _rows(y, "time_stretch")
        plan = stretch_plan(a.shape[1], rate)
        with torch.cuda.device(self.device), self._guard.call():
            out, t_spec, t_str = self._stretch_dev(torch.from_numpy(a).to(self.device), plan, taps)
            res = out.cpu().numpy()
            if taps is not None:
                taps["spec"], taps["stretched"] = self._cplx(t_spec, mono), self._cplx(t_str, mono)
                taps["synth"] = res[0] if mono else res
        return res[0] if mono else res

    def pitch_shift(self, y, sr, n_steps, bins_per_octave: int = 12, taps=None):
        """librosa.effects.pitch_shift(y, sr=sr, n_steps=n_steps, bins_per_octave=bins_per_octave) with the project's own
        resampler in soxr_hq's place; `sr` cancels out of the ratio.  `taps` as in time_stretch: `synth` is the stretched clip
        before it is resampled."""
        import torch
        self._open("pitch_shift")
        if not float(sr) > 0:
            raise ValueError("pitch_shift: sr must be positive")
        a, mono = _rows(y, "pitch_shift")
        plan = pitch_plan(a.shape[1], n_steps, bins_per_octave)
        with torch.cuda.device(self.device), self._guard.call():
            mid, t_spec, t_str = self._stretch_dev(torch.from_numpy(a).to(self.device), plan, taps)
            out = torch.empty((a.shape[0], plan["n_final"]), dtype=torch.float32, device=self.device)
            self._lib.check(self._l.tdx_resample_sinc(mid.data_ptr(), a.shape[0], plan["length"], plan["ratio"], out.data_ptr(), plan["n_final"],
                                                      self._stream()))
            self.launches += 1
            res = out.cpu().numpy()
            if taps is not None:
                taps["spec"], taps["stretched"] = self._cplx(t_spec, mono), self._cplx(t_str, mono)
                s = mid.cpu().numpy()
                taps["synth"] = s[0] if mono else s
        return res[0] if mono else res

    def resample(self, y, ratio):
        """[n] or [C, n] -> [.., ceil(n * ratio)]: the windowed-sinc resampler of include/tdx.h at ratio = target / orig"""
        import torch
        self._open("resample")
        a, mono = _rows(y, "resample")
        ratio = float(ratio)
        n_out = int(self._l.tdx_resample_sinc_length(a.shape[1], ratio))
        if n_out < 1:
            raise ValueError(f"resample: ratio {ratio} leaves no output")
        with torch.cuda.device(self.device), self._guard.call():
            x = torch.from_numpy(a).to(self.device)
            out = torch.empty((a.shape[0], n_out), dtype=torch.float32, device=self.device)
            self._lib.check(self._l.tdx_resample_sinc(x.data_ptr(), a.shape[0], a.shape[1], ratio, out.data_ptr(), n_out, self._stream()))
            res = out.cpu().numpy()
        return res[0] if mono else res

    def phase_vocoder(self, D, rate, hop_length=None):
        """librosa.phase_vocoder(D, rate=rate, hop_length=hop_length): complex64 [bins, T] (ndarray or device tensor) ->
        [bins, T'] of the same kind; hop_length defaults to n_fft // 4 with n_fft = 2 * (bins - 1)."""
        import torch
        self._open("phase_vocoder")
        is_t = isinstance(D, torch.Tensor)
        d = D if is_t else torch.from_numpy(np.ascontiguousarray(np.asarray(D), dtype=np.complex64))
        if d.ndim != 2 or d.shape[0] < 2 or d.shape[1] < 1 or d.dtype != torch.complex64:
            raise ValueError(f"phase_vocoder: D must be complex64 [bins >= 2, T >= 1], got {tuple(d.shape)} {d.dtype}")
        nb, T = int(d.shape[0]), int(d.shape[1])
        n_fft = 2 * (nb - 1)
        hop = int(hop_length) if hop_length is not None else n_fft // 4
        rate = float(rate)
        if not (rate > 0 and math.isfinite(rate)):
            raise ValueError(f"phase_vocoder: rate must be a positive number, got {rate}")
        steps = np.arange(0, T, rate, dtype=np.float64)
        plan = dict(idx=steps.astype(np.int64).astype(np.int32), alpha=np.mod(steps, 1.0))
        t_out = int(steps.shape[0])
        with torch.cuda.device(self.device), self._guard.call():
            src = torch.view_as_real(d.to(self.device).t().contiguous())             # [T, bins, 2]
            idx, idx_h, idx_d, alpha_d = self._plan_dev(plan)
            out = torch.empty((t_out, nb, 2), dtype=torch.float32, device=self.device)
            self._lib.check(self._l.tdx_pvoc_vocode(self._h, src.data_ptr(), nb, T, hop, idx_h, idx_d.data_ptr(), alpha_d.data_ptr(), t_out,
                                                    out.data_ptr(), self._stream()))
            res = torch.view_as_complex(out).t()
            return res.contiguous() if is_t else res.cpu().numpy()

    def prepare(self, n_fft):
        self._open("prepare")
        self._lib.check(self._l.tdx_pvoc_prepare(self._h, int(n_fft)))

    def istft(self, D, n_fft=None, hop_length=None, length=None):
        """librosa.istft(D, hop_length=hop_length, length=length) of a complex64 [bins, T] ndarray -> float32 [length]"""
        import torch
        self._open("istft")
        d = np.ascontiguousarray(np.asarray(D).T, dtype=np.complex64)                # [T, bins]
        if d.ndim != 2 or d.shape[0] < 1 or d.shape[1] < 2:
            raise ValueError(f"istft: D must be [bins >= 2, T >= 1], got {np.asarray(D).shape}")
        T, nb = d.shape
        n_fft = 2 * (nb - 1) if n_fft is None else int(n_fft)
        if n_fft // 2 + 1 != nb:
            raise ValueError(f"istft: {nb} bins do not belong to n_fft {n_fft}")
        hop = n_fft // 4 if hop_length is None else int(hop_length)
        n = hop * (T - 1) if length is None else int(length)
        if n < 1:
            raise ValueError("istft: the result would be empty")
        self.prepare(n_fft)
        with torch.cuda.device(self.device), self._guard.call():
            ws = self._workspace("istft", n_fft, hop, 1, 0, T)
            src = torch.from_numpy(d.view(np.float32)).to(self.device)
            y = torch.empty(n, dtype=torch.float32, device=self.device)
            self._lib.check(self._l.tdx_pvoc_istft(self._h, src.data_ptr(), T, n_fft, hop, -1 if length is None else n, y.data_ptr(), ws.data_ptr(),
                                                   ws.numel(), self._stream()))
            return y.cpu().numpy()

    def eq_match(self, source, target=None, target_stft=None, n_fft: int = 2048, hop_length: int = 512, taps=None):
        """The reference's eq_match (:532-543) for a mono source [n] and a target given as samples [m] or as its spectrum
        (complex [n_fft / 2 + 1, T]) -> float32 [hop * (n // hop)].  A bin whose source mean is exactly 0 gets gain 10 (upstream:
        NaN through the whole clip).  `taps`: a dict that receives `spec` (source spectrum [bins, T]), `mean_source`,
        `mean_target` (float64 [bins]) and `gain` (float32 [bins])."""
        import torch
        self._open("eq_match")
        n_fft, hop = int(n_fft), int(hop_length)
        s = np.require(np.asarray(source), dtype=np.float32, requirements=["C", "W"])
        if s.ndim != 1 or s.size < hop or s.size == 0:
            raise ValueError(f"eq_match: the source must be mono [n] with n >= hop_length, got shape {s.shape}")
        if (target is None) == (target_stft is None):
            raise ValueError("eq_match: give the target as samples or as a spectrum, one of the two")
        nb = n_fft // 2 + 1
        if target is not None:
            t = np.require(np.asarray(target), dtype=np.float32, requirements=["C", "W"])
            if t.ndim != 1 or t.size == 0:
                raise ValueError(f"eq_match: the target must be mono [m] and not empty, got shape {t.shape}")
            n_t, t_t = t.size, 0
        else:
            t = np.ascontiguousarray(np.asarray(target_stft).T, dtype=np.complex64)
            if t.ndim != 2 or t.shape[1] != nb or t.shape[0] < 1:
                raise ValueError(f"eq_match: the target spectrum must be [{nb}, T >= 1] for n_fft {n_fft}, got {np.asarray(target_stft).shape}")
            n_t, t_t = 0, t.shape[0]
            t = t.view(np.float32)
        if int(self._l.tdx_pvoc_workspace_bytes(self._h, n_fft, hop, 1, max(s.size, n_t), 0)) == 0:
            raise self._lib.TdxError(f"PhaseVocoder.eq_match: n_fft {n_fft} / hop_length {hop} not supported: n_fft must be a multiple of 128 in "
                                     "[128, 4096], hop_length a multiple of 4 in [n_fft / 16, n_fft]")
        self.prepare(n_fft)
        T = 1 + s.size // hop
        with torch.cuda.device(self.device), self._guard.call():
            ws = self._workspace("eq_match", n_fft, hop, 1, max(s.size, n_t), 0)
            xs, xt = torch.from_numpy(s).to(self.device), torch.from_numpy(t).to(self.device)
            y = torch.empty(hop * (T - 1), dtype=torch.float32, device=self.device)
            tp = [None] * 4
            if taps is not None:
                tp = [torch.empty((1, T, nb, 2), dtype=torch.float32, device=self.device), torch.empty(nb, dtype=torch.float64, device=self.device),
                      torch.empty(nb, dtype=torch.float64, device=self.device), torch.empty(nb, dtype=torch.float32, device=self.device)]
            self._lib.check(self._l.tdx_pvoc_eq_match(self._h, xs.data_ptr(), s.size, xt.data_ptr() if target is not None else None, n_t,
                                                      xt.data_ptr() if target is None else None, t_t, n_fft, hop, y.data_ptr(),
                                                      *[self._ptr(q) for q in tp], ws.data_ptr(), ws.numel(), self._stream()))
            res = y.cpu().numpy()
            if taps is not None:
                taps["spec"] = self._cplx(tp[0], True)
                taps["mean_source"], taps["mean_target"], taps["gain"] = (q.cpu().numpy() for q in tp[1:])
        return res

    def close(self):
        self._own.close()
