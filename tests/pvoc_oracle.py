"""Float64 numpy restatement of librosa 0.10's stft / phase_vocoder / istft / effects.time_stretch / effects.pitch_shift with
their defaults (n_fft 2048, hop n_fft // 4, periodic Hann, center=True with zero padding), of the reference's eq_match
(AudioProcessor.py:532-543) and of the project's windowed-sinc resampler (include/tdx.h, tdx_resample_sinc).  librosa is not
installed: test_pvoc_host.py pins stft / istft to torch.stft / torch.istft in float64 instead.

`dtype=np.float32` rounds the analysis — frames, basis and products — to float32 (a DFT as a float32 matrix product); the phase
vocoder and the synthesis stay float64 in both modes."""
import numpy as np

TINY32 = float(np.finfo(np.float32).tiny)


def hann(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def frames_of(x, n_fft, hop):
    xp = np.concatenate([np.zeros(n_fft // 2), np.asarray(x, dtype=np.float64), np.zeros(n_fft // 2)])
    T = 1 + (xp.shape[0] - n_fft) // hop
    return np.lib.stride_tricks.as_strided(xp, shape=(T, n_fft), strides=(xp.strides[0] * hop, xp.strides[0]), writeable=False)


def stft(x, n_fft=2048, hop=None, dtype=np.float64):
    """-> complex [1 + n_fft // 2, 1 + n // hop]"""
    hop = n_fft // 4 if hop is None else hop
    fr = frames_of(x, n_fft, hop)
    if dtype == np.float64:
        return np.fft.rfft(fr * hann(n_fft), axis=1).T
    k = np.arange(n_fft // 2 + 1)[:, None] * np.arange(n_fft)[None, :] % n_fft
    ang = 2.0 * np.pi * k / n_fft
    w = hann(n_fft)
    f32 = np.ascontiguousarray(fr, dtype=np.float32)
    re = f32 @ (w * np.cos(ang)).astype(np.float32).T
    im = f32 @ (-w * np.sin(ang)).astype(np.float32).T
    return (re + 1j * im).astype(np.complex64).T


def phase_vocoder(D, rate, hop=None, block=None):
    """librosa.phase_vocoder in float64: D [bins, T] -> [bins, len(arange(0, T, rate))].  `block` = (k0, n_fft): D holds only the
    bins k0 .. k0 + len(D) of an n_fft-point transform (a long clip is vocoded in blocks of bins to bound the memory)"""
    D = np.asarray(D).astype(np.complex128)
    nb, T = D.shape
    k0, n_fft = (0, 2 * (nb - 1)) if block is None else block
    hop = n_fft // 4 if hop is None else hop
    steps = np.arange(0, T, rate, dtype=np.float64)
    phi = 2.0 * np.pi * np.arange(k0, k0 + nb) * hop / n_fft
    Dp = np.pad(D, [(0, 0), (0, 2)], mode="constant")
    i = steps.astype(np.int64)
    alpha = np.mod(steps, 1.0)
    c0, c1 = Dp[:, i], Dp[:, i + 1]
    mag = (1.0 - alpha) * np.abs(c0) + alpha * np.abs(c1)
    dphase = np.angle(c1) - np.angle(c0) - phi[:, None]
    dphase = dphase - 2.0 * np.pi * np.round(dphase / (2.0 * np.pi))
    inc = phi[:, None] + dphase
    acc = np.angle(D[:, 0])[:, None] + np.concatenate([np.zeros((nb, 1)), np.cumsum(inc, axis=1)[:, :-1]], axis=1)
    return mag * (np.cos(acc) + 1j * np.sin(acc))


def neighbour_mag(D, rate):
    """[bins, T']: the larger of the two magnitudes every output element is interpolated from"""
    D = np.asarray(D).astype(np.complex128)
    steps = np.arange(0, D.shape[1], rate, dtype=np.float64)
    a = np.abs(np.pad(D, [(0, 0), (0, 2)], mode="constant"))
    i = steps.astype(np.int64)
    return np.maximum(a[:, i], a[:, i + 1])


def istft(D, hop=None, length=None):
    """librosa.istft (center=True) in float64"""
    D = np.asarray(D).astype(np.complex128)
    nb, T = D.shape
    n_fft = 2 * (nb - 1)
    hop = n_fft // 4 if hop is None else hop
    nF = T if length is None else min(T, int(np.ceil((length + n_fft) / hop)))
    w = hann(n_fft)
    fr = np.fft.irfft(D[:, :nF], n=n_fft, axis=0).T * w
    total = n_fft + hop * (nF - 1)
    y, wss = np.zeros(total), np.zeros(total)
    w2 = w * w
    for f in range(nF):
        y[f * hop:f * hop + n_fft] += fr[f]
        wss[f * hop:f * hop + n_fft] += w2
    nz = wss > TINY32
    y[nz] /= wss[nz]
    if length is None:
        return y[n_fft // 2:total - n_fft // 2]
    y = y[n_fft // 2:n_fft // 2 + length]
    return np.concatenate([y, np.zeros(length - y.shape[0])])


def time_stretch(x, rate, dtype=np.float64, D=None):
    n = np.asarray(x).shape[0]
    D = stft(x, dtype=dtype) if D is None else D
    return istft(phase_vocoder(D, rate), length=int(round(n / rate)))


def resample_sinc(x, rho, idx=None, pos=None):
    """the resampler of include/tdx.h; `idx`: only these output indices (default: all ceil(n rho)); `pos`: their input
    positions, in place of idx / rho"""
    x = np.asarray(x)
    n = x.shape[0]
    n_out = int(np.ceil(n * rho))
    m = np.arange(n_out) if idx is None else np.asarray(idx)
    p = m / rho if pos is None else np.asarray(pos, dtype=np.float64)
    c = min(1.0, rho)
    H = 10.0 / c
    j = np.ceil(p - H).astype(np.int64)[:, None] + np.arange(int(2 * np.ceil(H)) + 2)[None, :]
    d = j - p[:, None]
    inside = np.abs(d) <= H
    h = np.where(inside, c * np.sinc(c * d) * np.i0(5.0 * np.sqrt(np.clip(1.0 - (d / H) ** 2, 0.0, None))) / np.i0(5.0), 0.0)
    xv = np.where((j >= 0) & (j < n), x[np.clip(j, 0, n - 1)].astype(np.float64), 0.0)
    return (h * xv).sum(axis=1) / h.sum(axis=1)


def fix_length(y, n):
    return y[:n] if y.shape[0] >= n else np.concatenate([y, np.zeros(n - y.shape[0])])


def pitch_shift(x, n_steps, bins_per_octave=12, dtype=np.float64, D=None):
    rate = 2.0 ** (-float(n_steps) / bins_per_octave)
    return fix_length(resample_sinc(time_stretch(x, rate, dtype=dtype, D=D), rate), np.asarray(x).shape[0])


def eq_gain(mean_s, mean_t, guard=True):
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.clip(mean_t / mean_s, 0.1, 10)
    return np.where(mean_s == 0, 10.0, g) if guard else g


def eq_match(source=None, target=None, target_stft=None, n_fft=2048, hop=512, guard=True, source_stft=None):
    """-> (y, mean_source, mean_target, gain); guard=False is the upstream formula (a bin with a zero source mean is NaN)"""
    S = stft(source, n_fft, hop) if source_stft is None else np.asarray(source_stft).astype(np.complex128)
    St = stft(target, n_fft, hop) if target_stft is None else np.asarray(target_stft).astype(np.complex128)
    ms, mt = np.abs(S).mean(axis=1), np.abs(St).mean(axis=1)
    g = eq_gain(ms, mt, guard)
    return istft(S * g[:, None], hop), ms, mt, g
