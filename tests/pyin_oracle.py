"""float64 NumPy / scipy restatement of librosa 0.10's `pyin` (librosa is not available here: restated from its published source;
parity with the package itself is unpinned).  The product's pitch.Pyin / csrc/pyin.hip is tested against this file.

    params(sr, fmin, fmax, ...)            every derived number of one configuration, computed here and not taken from the product
    frames(y, P)                            [frame_length, T] centred frames, zero padding
    yin_shifts(y, P, dtype, flush, direct)  stages 2-4: float64 FFT form as upstream (flush = the 1e-6 rule), or the direct difference
                                            in `dtype` — what float32 alone costs, independent of the device
    observation(yin, shifts, P)             stages 5-6 -> obs [2 n_pitch_bins, T], voiced_prob [T]
    transition(P), p_init(P)                stage 7, dense
    viterbi_dense / viterbi_banded          stage 8: librosa.sequence.viterbi, and the banded recursion with the global fallback
    score(states, obs, P)                   a path's log-likelihood in float64
    pyin(y, P, ...)                         (f0, voiced_flag, voiced_prob, states, obs)
    robust_frames, voiced_signal            the input conditions of the device tests"""
import numpy as np
import scipy.signal
import scipy.stats
from types import SimpleNamespace

TINY = np.finfo(np.float64).tiny


def params(sr, fmin, fmax, frame_length=2048, win_length=None, hop_length=None, n_thresholds=100, beta_parameters=(2, 18),
           boltzmann_parameter=2, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01, center=True):
    win_length = frame_length // 2 if win_length is None else win_length
    hop_length = frame_length // 4 if hop_length is None else hop_length
    min_period = max(int(np.floor(sr / fmax)), 1)
    max_period = min(int(np.ceil(sr / fmin)), frame_length - win_length - 1)
    if max_period - min_period < 2:
        raise ValueError("max_period - min_period < 2")
    thr = np.linspace(0, 1, n_thresholds + 1)
    beta_probs = np.diff(scipy.stats.beta.cdf(thr, beta_parameters[0], beta_parameters[1]))
    bps = int(np.ceil(1.0 / resolution))
    npb = int(np.floor(12 * bps * np.log2(fmax / fmin))) + 1
    width = round(max_transition_rate * 12 * hop_length / sr) * bps + 1
    if npb < width:
        raise ValueError("n_pitch_bins < width")
    return SimpleNamespace(sr=sr, fmin=fmin, fmax=fmax, frame_length=frame_length, win_length=win_length, hop_length=hop_length,
                           min_period=min_period, max_period=max_period, n_lags=max_period - min_period + 1, thr=thr, beta_probs=beta_probs,
                           lam=boltzmann_parameter, bps=bps, npb=npb, width=width, switch_prob=switch_prob, no_trough_prob=no_trough_prob,
                           center=center, freqs=fmin * 2.0 ** (np.arange(npb) / (12 * bps)))


def frames(y, P):
    y = np.asarray(y)
    if P.center:
        y = np.pad(y, (P.frame_length // 2, P.frame_length // 2), mode="constant")
    T = 1 + (len(y) - P.frame_length) // P.hop_length
    idx = np.arange(P.frame_length)[:, None] + P.hop_length * np.arange(T)[None, :]
    return y[idx]


def parabolic(x):
    """x [n_lags, T] -> shifts (computed in x's dtype)"""
    sh = np.zeros_like(x)
    a = (x[:-2] + x[2:]) - 2 * x[1:-1]
    b = (x[2:] - x[:-2]) / 2
    ok = np.abs(b) < np.abs(a)
    with np.errstate(divide="ignore", invalid="ignore"):
        sh[1:-1] = np.where(ok, -b / np.where(ok, a, 1), 0)
    return sh


def yin_shifts(y, P, dtype=np.float64, flush=True, direct=False):
    """-> yin [n_lags, T], shifts [n_lags, T].  direct=False: upstream's e[0] + e[tau] - 2 acf[tau] through an rFFT (float64 only);
    direct=True: sum_j (y[j] - y[j+tau])^2 in `dtype` (no flush: there is nothing to flush)."""
    W, N = P.win_length, P.frame_length
    if not direct:
        assert dtype == np.float64
        yf = frames(np.asarray(y, np.float64), P)
        a = np.fft.rfft(yf, N, axis=0)
        b = np.fft.rfft(yf[W:0:-1], N, axis=0)
        acf = np.fft.irfft(a * b, N, axis=0)[W:]
        e = np.cumsum(yf ** 2, axis=0)
        e = e[W:] - e[:-W]
        if flush:
            acf[np.abs(acf) < 1e-6] = 0
            e[np.abs(e) < 1e-6] = 0
        d = e[:1] + e - 2 * acf
    else:
        yf = frames(np.asarray(y, np.float32).astype(dtype), P)
        d = np.zeros((P.max_period + 1, yf.shape[1]), dtype=dtype)
        for tau in range(1, P.max_period + 1):
            diff = yf[1:W + 1] - yf[1 + tau:W + 1 + tau]
            d[tau] = np.sum(diff * diff, axis=0, dtype=dtype)
    tau = np.arange(1, P.max_period + 1).astype(d.dtype)[:, None]
    cm = np.cumsum(d[1:P.max_period + 1], axis=0, dtype=d.dtype) / tau
    den = cm[P.min_period - 1:P.max_period]
    yin = d[P.min_period:P.max_period + 1] / (den + np.finfo(d.dtype).tiny)
    return yin, parabolic(yin)


def boltzmann_pmf(k, lam, n):
    with np.errstate(divide="ignore", invalid="ignore"):
        fact = (1 - np.exp(-lam)) / (1 - np.exp(-lam * n))
        return fact * np.exp(-lam * k)


def observation_column(x, sh, P):
    """one frame: yin values x [n_lags], shifts sh [n_lags] (any float dtype) -> (voiced rows [npb], voiced_prob)"""
    n = len(x)
    x = np.asarray(x, np.float64)
    tr = np.zeros(n, bool)
    tr[1:-1] = (x[1:-1] < x[:-2]) & (x[1:-1] <= x[2:])
    tr[-1] = x[-1] < x[-2]
    tr[0] = x[0] < x[1]
    col = np.zeros(P.npb + 1)
    idx = np.nonzero(tr)[0]
    if len(idx):
        h = x[idx]
        below = np.less.outer(h, P.thr[1:])
        pos = np.cumsum(below, axis=0) - 1
        cnt = np.count_nonzero(below, axis=0)
        prior = boltzmann_pmf(pos, P.lam, cnt)
        prior[~below] = 0
        probs = prior.dot(P.beta_probs)
        g = int(np.argmin(h))
        probs[g] += P.no_trough_prob * np.sum(P.beta_probs[:np.count_nonzero(~below[g])])
        keep = probs != 0
        period = P.min_period + idx[keep] + np.asarray(sh, np.float64)[idx[keep]]
        f0 = P.sr / period
        b = np.clip(np.round(12 * P.bps * np.log2(f0 / P.fmin)), 0, P.npb).astype(int)
        col[b] = probs[keep]                       # assigned in order of increasing period: the longest period wins a bin
    v = col[:P.npb]
    return v, float(np.clip(np.sum(v), 0, 1))


def observation(yin, shifts, P):
    T = yin.shape[1]
    obs = np.zeros((2 * P.npb, T))
    vp = np.zeros(T)
    for t in range(T):
        obs[:P.npb, t], vp[t] = observation_column(yin[:, t], shifts[:, t], P)
    obs[P.npb:] = (1 - vp) / P.npb
    return obs, vp


def local_transition(P):
    tri = scipy.signal.get_window("triangle", P.width, fftbins=False)
    hw = P.width // 2
    loc = np.zeros((P.npb, P.npb))
    for i in range(P.npb):
        for j in range(max(0, i - hw), min(P.npb, i + hw + 1)):
            loc[i, j] = tri[j - i + hw]
    return loc / loc.sum(axis=1, keepdims=True)


def transition(P):
    s = P.switch_prob
    return np.kron(np.array([[1 - s, s], [s, 1 - s]]), local_transition(P))


def p_init(P):
    p = np.zeros(2 * P.npb)
    p[P.npb:] = 1 / P.npb
    return p


def _argmax(v, last, axis=0):
    if not last:
        return np.argmax(v, axis=axis)
    n = v.shape[axis]
    return n - 1 - np.argmax(np.flip(v, axis=axis), axis=axis)


def viterbi_dense(obs, P, last=False, trans=None):
    """librosa.sequence.viterbi over obs [S, T]; last=True takes the LAST maximum instead of the first -> states [T]"""
    S, T = obs.shape
    lt = np.log((transition(P) if trans is None else trans) + TINY)
    lo = np.log(obs.T + TINY)
    value = np.zeros((T, S))
    ptr = np.zeros((T, S), dtype=int)
    value[0] = lo[0] + np.log(p_init(P) + TINY)
    for t in range(1, T):
        tr = value[t - 1][:, None] + lt
        ptr[t] = _argmax(tr, last, axis=0)
        value[t] = lo[t] + np.take_along_axis(tr, ptr[t][None, :], axis=0)[0]
    states = np.zeros(T, dtype=int)
    states[-1] = _argmax(value[-1], last)
    for t in range(T - 2, -1, -1):
        states[t] = ptr[t + 1, states[t + 1]]
    return states


def viterbi_banded(obs, P, last=False):
    """the same path from the band alone: every destination scans the sources within width // 2 bins in both halves, plus the one
    candidate max_k value[k] + log(tiny) whose pointer is that global argmax (considered where that state lies outside the band)"""
    S, T = obs.shape
    npb, hw = P.npb, P.width // 2
    lt = np.log(transition(P) + TINY)          # the band is read from the dense matrix, so the arithmetic is the dense one's
    ltiny = np.log(TINY)
    lo = np.log(obs.T + TINY)
    bins = np.arange(S) % npb
    src = bins[None, :] - hw + np.arange(P.width)[:, None]                     # [width, S] source bin of band row d
    valid = (src >= 0) & (src < npb)
    srcc = np.clip(src, 0, npb - 1)
    ks = np.concatenate([srcc, npb + srcc])                                    # [2 width, S] ascending source state
    ltb = np.where(np.concatenate([valid, valid]), lt[ks, np.arange(S)[None, :]], -np.inf)
    value = np.zeros((T, S))
    ptr = np.zeros((T, S), dtype=int)
    value[0] = lo[0] + np.log(p_init(P) + TINY)
    cols = np.arange(S)
    for t in range(1, T):
        prev = value[t - 1]
        c = prev[ks] + ltb
        m = _argmax(c, last, axis=0)
        bv, bk = c[m, cols], ks[m, cols]
        g = int(_argmax(prev, last))
        fv = prev[g] + ltiny
        out = np.abs(bins - g % npb) > hw
        use = out & ((fv > bv) | ((fv == bv) & ((g > bk) if last else (g < bk))))
        ptr[t] = np.where(use, g, bk)
        value[t] = lo[t] + np.where(use, fv, bv)
    states = np.zeros(T, dtype=int)
    states[-1] = _argmax(value[-1], last)
    for t in range(T - 2, -1, -1):
        states[t] = ptr[t + 1, states[t + 1]]
    return states


def score(states, obs, P, trans=None):
    """log-likelihood of a path under obs [S, T] in float64 (the quantity the Viterbi maximises)"""
    lt = np.log((transition(P) if trans is None else trans) + TINY)
    lo = np.log(np.asarray(obs, np.float64).T + TINY)
    states = np.asarray(states)
    s = lo[0, states[0]] + np.log(p_init(P) + TINY)[states[0]]
    if len(states) > 1:
        s += np.sum(lo[np.arange(1, len(states)), states[1:]]) + np.sum(lt[states[:-1], states[1:]])
    return float(s)


def pyin(y, P, fill_na=np.nan, flush=True, dtype=np.float64, direct=False, last=False):
    yin, sh = yin_shifts(y, P, dtype=dtype, flush=flush, direct=direct)
    obs, vp = observation(yin, sh, P)
    states = viterbi_dense(obs, P, last=last)
    f0 = P.freqs[states % P.npb]
    voiced = states < P.npb
    if fill_na is not None:
        f0[~voiced] = fill_na
    return f0, voiced, vp, states, obs


def robust_frames(y, P, rel=1e-5, draws=16, seed=0, yin_sh=None):
    """-> bool [T]: the frame's observation column is unchanged (1e-9: see below) when every yin value x of the frame is replaced
    `draws` times by x (1 + rel * uniform(-1, 1)).  Relative per value is the error model of the direct difference: d[tau] and its
    cumulative mean are sums of non-negative terms, so float32 loses a relative 1e-7 .. 1e-6 of each value and an exact zero stays
    zero.  The column is a discrete function of yin (comparisons and a rounded bin) times smooth weights: a changed comparison
    near the top thresholds moves it by the beta weight there (< 1e-12), anything that matters moves it by far more than the 1e-9
    allowed here."""
    yin, sh = yin_shifts(y, P, flush=False) if yin_sh is None else yin_sh
    rng = np.random.default_rng(seed)
    T = yin.shape[1]
    ok = np.ones(T, bool)
    for t in range(T):
        x = yin[:, t]
        base, bvp = observation_column(x, sh[:, t], P)
        if not np.any(x):
            continue
        for _ in range(draws):
            xp = x * (1 + rel * rng.uniform(-1, 1, size=x.shape))
            col, vp = observation_column(xp, parabolic(xp[:, None])[:, 0], P)
            if np.max(np.abs(col - base)) > 1e-9:
                ok[t] = False
                break
    return ok


def voiced_signal(n, sr, seed=0, noise=0.01):
    """float32 [n]: a five-harmonic tone gliding 110 -> 220 Hz, gated on and off every 0.4 s with 20 ms ramps, over white noise of
    amplitude `noise`; the stretch from 45 % to 55 % of the clip is exact zeros"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    f = 110.0 * 2.0 ** (t / max(t[-1], 1e-9)) if n > 1 else np.full(n, 110.0)
    ph = 2 * np.pi * np.cumsum(f) / sr
    tone = sum(np.sin(k * ph) / k for k in range(1, 6))
    gate = np.clip((0.2 - np.abs((t % 0.8) - 0.3)) / 0.02, 0, 1)
    y = 0.3 * tone * gate + noise * rng.standard_normal(n)
    y[int(0.45 * n):int(0.55 * n)] = 0.0
    return y.astype(np.float32)
