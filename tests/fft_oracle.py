"""Float64 numpy restatements of the reference's "mix" family (AudioProcessor.py:386-414, 786-882), written from their description
(DESIGN 8.27), for the tests of targetdiarization_amd.fft and of the AudioProcessor methods on top of it.  Checker only.

Everything is computed in float64 whatever the input's dtype: the reference pins numpy < 2, where np.fft transforms float32 input in
double precision.  Two places follow the build, not the reference: with force_align a shorter aux clip is padded with silence (the
reference pads main, then fails), and fewer than 2 samples or input that is not 1-D give audio_main back (the reference raises)."""
import numpy as np


def band_sets(n, sampling_rate, main_freq_range=None, aux_freq_range=None):
    """the three boolean masks over np.fft.rfftfreq(n, 1 / sampling_rate) and the clamped limits"""
    half = int(sampling_rate / 2)
    mr = list(main_freq_range) if main_freq_range else [0, int(sampling_rate / 4)]
    ar = list(aux_freq_range) if aux_freq_range else [0, half]
    mr = [max(0, mr[0]), min(mr[1], half)]
    ar = [max(0, ar[0]), min(ar[1], half)]
    f = np.fft.rfftfreq(n, 1 / sampling_rate)
    return (f >= mr[0]) & (f < mr[1]), (f >= ar[0]) & (f <= ar[1]), (f >= max(mr[0], ar[0])) & (f <= min(mr[1], ar[1])), mr, ar


def mix_audio_by_freq(audio_main, audio_aux, sampling_rate=16000, main_freq_range=(0, 4000), aux_freq_range=(0, 8000), force_align=False,
                      spectra=None, ffts=None):
    """-> float64 [2 * (n // 2)], or audio_main itself where nothing is mixed.  `spectra`: a dict that receives the two spectra (`main`,
    `aux`) and the blended one (`mix`), complex128 [n // 2 + 1].  `ffts`: the two spectra, where a caller has them already (several
    range settings over one pair of clips)."""
    a, b = np.asarray(audio_main), np.asarray(audio_aux)
    if a.ndim != 1 or b.ndim != 1:
        return audio_main
    if a.shape[0] != b.shape[0]:
        if not force_align:
            return audio_main
        b = b[: a.shape[0]] if a.shape[0] < b.shape[0] else np.concatenate((b, np.zeros(a.shape[0] - b.shape[0])))
    n = a.shape[0]
    if n < 2:
        return audio_main
    fa, fb = ffts if ffts is not None else (np.fft.rfft(a.astype(np.float64)), np.fft.rfft(b.astype(np.float64)))
    in_main, in_aux, in_both, _, _ = band_sets(n, sampling_rate, main_freq_range, aux_freq_range)
    mix = np.zeros_like(fa)
    mix[in_main] = fa[in_main]
    mix[in_aux] = fb[in_aux]
    count = int(in_both.sum())
    if count:
        w = np.linspace(1, 0, count)
        mix[in_both] = fa[in_both] * w + fb[in_both] * (1 - w)
    if spectra is not None:
        spectra.update(main=fa, aux=fb, mix=mix)
    return np.fft.irfft(mix)                         # no length: 2 * (n // 2) samples


def audio_gain(audio, gain_db, clip_limit=False):
    if gain_db == 0.0:
        return audio
    out = audio * 10 ** (gain_db / 20.0)
    return np.clip(out, -1, 1) if clip_limit else out


def audio_normalize(audio, target_peak_db=-0.1):
    peak = np.max(np.abs(audio))
    if peak == 0.0:
        return audio
    return np.clip(audio * 10 ** ((target_peak_db - 20 * np.log10(peak)) / 20), -1.0, 1.0)


def mix_audio(clips, combine_channels=True, normalize=True):
    """1-D clips only (the goldens hold no multi-channel entry)"""
    if isinstance(clips, np.ndarray):
        return clips
    if len(clips) == 1:
        return clips[0]
    length = max(c.shape[0] for c in clips)
    padded = [np.concatenate((c, np.zeros(length - c.shape[0], dtype=np.float32))) if c.shape[0] < length else c for c in clips]
    if combine_channels:
        out = np.zeros(length, dtype=np.float32)
        for c in padded:
            out = out + c
    else:
        out = np.stack(padded, axis=1)
    out = out.astype(np.float32)
    return audio_normalize(out) if normalize else out


def generate_noise(sampling_rate=16000, duration_sec=1.0, gain_db=0.0, noise_type="brown"):
    """draws from numpy's global stream, like the reference: seed it with np.random.seed"""
    n = int(duration_sec * sampling_rate)
    noise = np.random.normal(0, 1, n)
    if noise_type == "pink":
        f = np.fft.rfftfreq(n, d=1.0 / sampling_rate)
        shaped = np.fft.irfft(np.fft.rfft(noise) * np.concatenate(([1], 1 / np.sqrt(f[1:]))), n=n)
        noise = shaped / np.max(np.abs(shaped))
    elif noise_type == "brown":
        walk = np.cumsum(noise)
        noise = walk / np.max(np.abs(walk))
    elif noise_type == "silence":
        noise = np.zeros(n)
    noise = noise.astype(np.float32)
    return audio_gain(noise, gain_db) if gain_db != 0.0 else noise
