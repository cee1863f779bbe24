"""float64 restatement of noisereduce's non-stationary spectral gate (`nr.reduce_noise(y, sr)` with its defaults), written
independently of targetdiarization_amd/noise_gate.py and importing nothing from it.

`reduce_noise` is the oracle: per buffer it makes exactly the four scipy calls noisereduce makes — `scipy.signal.stft`,
`filtfilt`, `fftconvolve`, `istft` — around noisereduce's chunk plan.  `reduce_noise_plain` is a second restatement in plain
numpy (explicit frame loops, the two seeded recurrences, a direct separable convolution, an explicit overlap-add); the two must
agree to 1e-12, which pins scipy's filtfilt seeding and frame grid.  `dtype=np.float32` runs the plain restatement in float32:
the measure of what single precision costs each intermediate quantity.

`zero_rule=True` applies the project's one deviation: mask = 0 where the smoothed magnitude is exactly 0 (noisereduce: NaN)."""
import numpy as np
import scipy.signal as ss

N_FFT, HOP = 1024, 256


def burst_signal(n, sr=16000, seed=0):
    """gated tone bursts (220 Hz at 0.3, on and off at 1.5 Hz) plus white noise at 0.02"""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(sr)
    gate = (np.sin(2 * np.pi * 1.5 * t) > 0).astype(np.float64)
    return (0.3 * np.sin(2 * np.pi * 220.0 * t) * gate + 0.02 * rng.randn(n)).astype(np.float32)


def plan(n, chunk_size, padding):
    if n <= chunk_size:
        return [(-padding, n + padding, 0, n)]
    return [(s - padding, s + chunk_size + padding, s, min(s + chunk_size, n)) for s in range(0, n, chunk_size)]


def tri(k):
    return np.concatenate([np.linspace(0, 1, k + 1, endpoint=False), np.linspace(1, 0, k + 2)])[1:-1]


def params(sr, time_constant_s=2.0, freq_mask_smooth_hz=500, time_mask_smooth_ms=50):
    t = time_constant_s * sr / HOP
    b = (np.sqrt(1 + 4 * t ** 2) - 1) / (2 * t ** 2)
    nf = int(freq_mask_smooth_hz / (sr / (N_FFT / 2))) if freq_mask_smooth_hz else 0
    nt = int(time_mask_smooth_ms / ((HOP / sr) * 1000)) if time_mask_smooth_ms else 0
    return b, nf, nt


def smoothing_filter(nf, nt):
    f = np.outer(tri(nf), tri(nt))
    return f / f.sum()


def _buffer(x, lo, hi):
    buf = np.zeros(hi - lo, dtype=np.float64)
    a, b = max(lo, 0), min(hi, x.shape[0])
    buf[a - lo:b - lo] = x[a:b]
    return buf


def _mask(A, s, thresh, slope, zero_rule):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = 1.0 / (1.0 + np.exp(-(((A - s) / s) - thresh) * slope))
    if zero_rule:
        m = np.where(s == 0, 0.0, m)
    return m


def gate_scipy(buf, b, nf, nt, thresh, slope, prop, zero_rule, taps=None):
    _, _, S = ss.stft(buf, nfft=N_FFT, nperseg=N_FFT, noverlap=N_FFT - HOP, window="hann", boundary="zeros", padded=False)
    A = np.abs(S)
    s = ss.filtfilt([b], [1, b - 1], A, axis=-1, padtype=None)
    m = _mask(A, s, thresh, slope, zero_rule)
    ms = ss.fftconvolve(m, smoothing_filter(nf, nt), mode="same")
    if taps is not None:
        w = 512.0                                    # scipy scales the spectrum by 1 / sum(hann); the taps are unscaled
        taps.update(mag=(A * w).T, smooth=(s * w).T, mask=m.T, mask_smooth=ms.T)
    ms = ms * prop + (1.0 - prop)
    _, y = ss.istft(S * ms, nfft=N_FFT, nperseg=N_FFT, noverlap=N_FFT - HOP, window="hann", boundary=True)
    return y


def gate_plain(buf, b, nf, nt, thresh, slope, prop, zero_rule, dtype=np.float64, taps=None):
    dt = np.dtype(dtype)
    L = buf.shape[0]
    F = 1 + L // HOP
    win = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N_FFT) / N_FFT)).astype(dt)
    padded = np.zeros(HOP * (F - 1) + N_FFT + HOP, dtype=dt)
    padded[N_FFT // 2:N_FFT // 2 + L] = buf
    S = np.empty((F, N_FFT // 2 + 1), dtype=np.complex64 if dt == np.float32 else np.complex128)
    for f in range(F):
        S[f] = np.fft.rfft((win * padded[HOP * f:HOP * f + N_FFT]).astype(dt)).astype(S.dtype)
    A = np.abs(S).astype(dt)
    b_, a_ = dt.type(b), dt.type(1.0 - b)
    y = np.empty_like(A)
    y[0] = A[0]
    for f in range(1, F):
        y[f] = b_ * A[f] + a_ * y[f - 1]
    s = np.empty_like(A)
    s[F - 1] = y[F - 1]
    for f in range(F - 2, -1, -1):
        s[f] = b_ * y[f] + a_ * s[f + 1]
    m = _mask(A, s, dt.type(thresh), dt.type(slope), zero_rule).astype(dt)
    tf, tt = tri(nf), tri(nt)
    tf, tt = (tf / tf.sum()).astype(dt), (tt / tt.sum()).astype(dt)
    K = m.shape[1]
    mp = np.zeros((F, K + 2 * nf), dtype=dt)
    mp[:, nf:nf + K] = m
    mf = np.zeros_like(m)
    for j in range(2 * nf + 1):
        mf += tf[j] * mp[:, j:j + K]
    mp = np.zeros((F + 2 * nt, K), dtype=dt)
    mp[nt:nt + F] = mf
    ms = np.zeros_like(m)
    for j in range(2 * nt + 1):
        ms += tt[j] * mp[j:j + F]
    if taps is not None:
        taps.update(mag=A, smooth=s, mask=m, mask_smooth=ms)
    ms = ms * dt.type(prop) + dt.type(1.0 - prop)
    out = np.zeros(padded.shape[0], dtype=dt)
    for f in range(F):
        out[HOP * f:HOP * f + N_FFT] += win * np.fft.irfft(S[f] * ms[f], n=N_FFT).astype(dt)
    # four hann^2 at hop 256 sum to 1.5 = 384 / 256: sum(hann^2) = 384 over one window, spread over the hop
    return (out * dt.type(HOP) / dt.type(384.0))[N_FFT // 2:N_FFT // 2 + L]


def _reduce(gate, y, sr, prop_decrease=1.0, time_constant_s=2.0, freq_mask_smooth_hz=500, time_mask_smooth_ms=50,
            thresh_n_mult_nonstationary=2, sigmoid_slope_nonstationary=10, chunk_size=600000, padding=30000, zero_rule=True,
            taps=None, **kw):
    x = np.asarray(y, dtype=np.float64)
    chans = x[None] if x.ndim == 1 else x
    b, nf, nt = params(sr, time_constant_s, freq_mask_smooth_hz, time_mask_smooth_ms)
    out = np.zeros_like(chans)
    first = True
    for c in range(chans.shape[0]):
        for (lo, hi, k0, k1) in plan(chans.shape[1], chunk_size, padding):
            g = gate(_buffer(chans[c], lo, hi), b, nf, nt, float(thresh_n_mult_nonstationary), float(sigmoid_slope_nonstationary),
                     float(prop_decrease), zero_rule, taps=taps if first else None, **kw)
            first = False
            out[c, k0:k1] = g[k0 - lo:k1 - lo]
    return out[0] if x.ndim == 1 else out


def reduce_noise(y, sr, **kw):
    """the oracle (float64, the four scipy calls)"""
    return _reduce(gate_scipy, y, sr, **kw)


def reduce_noise_plain(y, sr, dtype=np.float64, **kw):
    """the second restatement (plain numpy); dtype=np.float32 for the single-precision error measure"""
    return _reduce(gate_plain, y, sr, dtype=dtype, **kw)
