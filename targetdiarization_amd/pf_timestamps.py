"""Token timestamps from Paraformer's upsampled alphas: a numpy restatement of funasr's `ts_prediction_lfr6_standard`
(third-party, written from the published code: parity unpinned).  The device (csrc/pf_timestamps.hip) supplies `us_alphas` and
`us_peaks` on the 20 ms grid (three upsampled frames per 60 ms encoder frame); everything here is host bookkeeping on a few
hundred numbers per clip.

A "fire" is a frame whose running integral reaches 1 - 1e-4.  n characters need n + 1 fires: character i spans fire i to fire
i + 1, all shifted by `force_time_shift` frames.  When the count is off, the alphas are rescaled to sum n + 1 and scanned again
on the host with the device's loop."""
from __future__ import annotations

import numpy as np

START_END_THRESHOLD = 5        # frames of silence before the first / after the last fire that make a <sil> entry
MAX_TOKEN_DURATION = 12        # frames; a longer token is cut into token + <sil>
FIRE_THRESHOLD = np.float32(1.0 - 1e-4)


def cif_wo_hidden(alphas, threshold=FIRE_THRESHOLD) -> np.ndarray:
    """funasr cif_wo_hidden for one clip, in fp32 and in the sequential order of the device kernel: integ += a; peak = integ;
    if integ >= threshold: integ -= threshold.  alphas [U] -> peaks [U] float32."""
    a = np.ascontiguousarray(alphas, dtype=np.float32)
    thr = np.float32(threshold)
    peaks = np.empty(a.shape[0], dtype=np.float32)
    integ = np.float32(0.0)
    for i in range(a.shape[0]):
        integ = np.float32(integ + a[i])
        peaks[i] = integ
        if integ >= thr:
            integ = np.float32(integ - thr)
    return peaks


def ts_prediction_lfr6(us_alphas, us_peaks, chars, vad_offset_ms: float = 0.0, force_time_shift: float = -1.5, upsample_rate: int = 3):
    """us_alphas, us_peaks [U] of one clip, chars: its tokens (a trailing "</s>" is dropped) ->
    (text_with_times "tok start end;...", [[start_ms, end_ms], ...] with one entry per token, <sil> entries left out).
    No characters, or no fire at all: ("", []).  If the fire count still differs from len(chars) + 1 after the rescan, the first
    min(len(chars), fires - 1) characters get an entry."""
    chars = list(chars)
    if chars and chars[-1] == "</s>":
        chars = chars[:-1]
    if not chars:
        return "", []
    time_rate = 0.06 / upsample_rate
    alphas = np.asarray(us_alphas, dtype=np.float32).reshape(-1)
    peaks = np.asarray(us_peaks, dtype=np.float32).reshape(-1)
    fire = np.nonzero(peaks >= FIRE_THRESHOLD)[0] + force_time_shift
    if len(fire) != len(chars) + 1:
        total = np.float32(alphas.sum(dtype=np.float32))
        if total > 0:
            alphas = alphas / np.float32(total / np.float32(len(chars) + 1))
            peaks = cif_wo_hidden(alphas)
            fire = np.nonzero(peaks >= FIRE_THRESHOLD)[0] + force_time_shift
    if len(fire) == 0:
        return "", []
    num_frames = peaks.shape[0]
    names, spans = [], []
    if fire[0] > START_END_THRESHOLD:
        names.append("<sil>")
        spans.append([0.0, fire[0] * time_rate])
    for i in range(min(len(fire) - 1, len(chars))):
        names.append(chars[i])
        if fire[i + 1] - fire[i] <= MAX_TOKEN_DURATION:
            spans.append([fire[i] * time_rate, fire[i + 1] * time_rate])
        else:
            split = fire[i] + MAX_TOKEN_DURATION
            spans.append([fire[i] * time_rate, split * time_rate])
            spans.append([split * time_rate, fire[i + 1] * time_rate])
            names.append("<sil>")
    if num_frames - fire[-1] > START_END_THRESHOLD:
        end = (num_frames + fire[-1]) * 0.5
        if spans:
            spans[-1][1] = end * time_rate
        spans.append([end * time_rate, num_frames * time_rate])
        names.append("<sil>")
    elif spans:
        spans[-1][1] = num_frames * time_rate
    off_ms = int(round(vad_offset_ms))
    text, out = "", []
    for name, (s, e) in zip(names, spans):
        text += "{} {} {};".format(name, str(s + off_ms / 1000.0 + 0.0005)[:5], str(e + off_ms / 1000.0 + 0.0005)[:5])
        if name != "<sil>":
            out.append([int(s * 1000) + off_ms, int(e * 1000) + off_ms])
    return text, out
