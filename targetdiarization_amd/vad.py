"""FSMN-VAD: the device network over the C-ABI (tdx_fsmnvad_*, csrc/fsmn_vad.hip) and the host segmenter — the stage behind
ASRProcessor.vad_detection (ASRProcessor.py:742-817) and the `vad` plug-in of TargetDiarization / TargetASR / the stream class.

Third-party model (funasr fsmn_vad_streaming), restated from the published code [upstream-recall]; parity with the
published checkpoint is unpinned (none is at hand).  The device returns p0[t], the posterior of the one silence class, per
10 ms frame; `segments` turns it into [start_ms, end_ms] ranges with E2EVadModel's sliding-window detector as the reference
drives it: one whole clip, detect_mode 1, is_final.  Its decibel / SNR gates are left out: at the published -100 dB
thresholds, with the 1e-6 floor in the frame energy, they cannot fire for audio in [-1, 1]."""
from __future__ import annotations

import os
from typing import Sequence

import numpy as np
import torch

from . import _lib
from .frontend import Fbank
from .weights import pack_fsmn_vad_blob, parse_kaldi_cmvn

SPEECH_NOISE_THRES = 0.6
FRAME_MS = 10
NUM_CLASSES = 248


def speech_frames(p0) -> np.ndarray:
    """speech[t] = (1 - p0 >= p0 + speech_noise_thres): class 0 is the only silence class"""
    p = np.asarray(p0, dtype=np.float64).reshape(-1)
    return (1.0 - p >= p + SPEECH_NOISE_THRES).astype(np.int64)


def speech_segments(speech: Sequence[int], dur_ms: int, max_end_sil: int = 800, max_seg_ms: int = 60000):
    """speech[t] in {0,1} per 10 ms frame -> [[start_ms, end_ms], ...].  A 200 ms window of frame decisions switches to speech at
    >= 150 ms of speech and back at <= 150 ms; a segment starts window + 200 ms before the switch (never before the previous end)
    and ends after max_end_sil of silence (100 ms of look-ahead kept), at the 60 s cap, or with the clip.  The detector
    is reset after every end point."""
    T = len(speech); W = 20; UP = 15; DOWN = 15; LOOKBACK = 40
    win = [0] * W; pos = 0; wsum = 0; pre = 0; run = 0; start = None; floor = 0; out = []
    for t in range(T):
        cur = int(speech[t]); wsum += cur - win[pos]; win[pos] = cur; pos = (pos + 1) % W
        if pre == 0 and wsum >= UP:
            pre = 1; ch = "up"
        elif pre == 1 and wsum <= DOWN:
            pre = 0; ch = "down"
        else:
            ch = "speech" if pre else "sil"
        end = None
        if ch == "up":
            run = 0
            if start is None:
                start = max(floor, t - LOOKBACK)
        elif ch in ("down", "speech"):
            run = 0
        else:
            run += 1
            if start is not None and run * FRAME_MS >= max_end_sil - 150:
                end = (t - max(0, max_end_sil // FRAME_MS - 10 - 1)) * FRAME_MS     # look-ahead 100 ms kept, one frame
        if start is not None and end is None:
            if t - start + 1 > max_seg_ms // FRAME_MS:
                end = t * FRAME_MS                                                  # 60 s cap
            elif t == T - 1:
                end = dur_ms                                                        # clip ends inside speech
        if end is not None:
            out.append([start * FRAME_MS, end]); floor = T if end == dur_ms else end // FRAME_MS; start = None
            win = [0] * W; pos = 0; wsum = 0; pre = 0; run = 0                      # detector reset after every end point
    return out


def segments(p0, n_samples: int, max_end_silence_ms: int = 800):
    """frame posteriors of the silence class -> [[start_ms, end_ms], ...] of one clip of n_samples at 16 kHz"""
    return speech_segments(speech_frames(p0), int(n_samples) // 16, max_end_silence_ms)


def clip_ranges(value_sec, min_clip_sec: float = 0.0, max_clip_sec: float = 0.0):
    """ASRProcessor.py:768-798: ranges shorter than min_clip_sec are merged into their successor (the last one into its
    predecessor), ranges longer than max_clip_sec are cut into equal parts.  An empty list stays empty (the reference indexes
    value_sec[0] and raises)."""
    if min_clip_sec > 0 and value_sec:
        merged = []
        current_start, current_end = value_sec[0]
        for next_start, next_end in value_sec[1:]:
            if current_end - current_start < min_clip_sec:
                current_end = next_end
            else:
                merged.append([current_start, current_end])
                current_start, current_end = next_start, next_end
        if current_end - current_start >= min_clip_sec or not merged:
            merged.append([current_start, current_end])
        else:
            merged[-1][1] = current_end
        value_sec = merged
    if max_clip_sec > 0:
        merged = []
        for current_start, current_end in value_sec:
            duration = current_end - current_start
            if duration > max_clip_sec:
                num_clips = int(duration // max_clip_sec)
                clip_duration = duration / (num_clips + 1)
                for i in range(num_clips):
                    merged.append([current_start + i * clip_duration, current_start + (i + 1) * clip_duration])
                merged.append([current_start + num_clips * clip_duration, current_end])
            else:
                merged.append([current_start, current_end])
        value_sec = merged
    return value_sec


def load_model_dir(path):
    """funasr's model directory: model.pt (the state dict, bare or under "state_dict") + am.mvn -> (state_dict, (shift, scale));
    None when `path` is not such a directory"""
    if not isinstance(path, str) or not os.path.isdir(path):
        return None
    pt, mvn = os.path.join(path, "model.pt"), os.path.join(path, "am.mvn")
    if not (os.path.isfile(pt) and os.path.isfile(mvn)):
        return None
    sd = torch.load(pt, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and "state_dict" in sd:
        sd = sd["state_dict"]
    return sd, parse_kaldi_cmvn(mvn)


class FsmnVad:
    """`vad(audio) -> [[start_s, end_s], ...]` on the device.  state_dict: funasr's names (with or without the `encoder.`
    prefix); cmvn = (shift[400], scale[400]) of am.mvn, None = identity."""

    def __init__(self, state_dict, cmvn=None, device="cuda:0"):
        self._l = _lib.lib()
        self._own = _lib.Handle(device, "FsmnVad", self._l.tdx_fsmnvad_create, self._l.tdx_fsmnvad_destroy, blob=pack_fsmn_vad_blob(state_dict, cmvn))
        self.device, self._h, self._guard = self._own.device, self._own.ptr, self._own.guard
        self.fbank = Fbank("asr", self.device)

    def flops(self, rows: int) -> float:
        return float(self._l.tdx_fsmnvad_flops(self._h, rows))

    def workspace_bytes(self, rows: int) -> int:
        return int(self._l.tdx_fsmnvad_workspace_bytes(self._h, rows))

    def forward_into(self, feat, starts, p0, post=None, ws=None):
        """the bare C call on the current stream: feat [rows,80], starts int32 [nclips+1] (device), p0 [rows], post None or
        [rows,248]; ws: a uint8 device tensor of workspace_bytes(rows) (None: the object's grow-only workspace; hold
        `self._guard.call()` around it then).  No allocation when ws is given: this is what a graph capture records."""
        rows, nclips = int(feat.shape[0]), int(starts.shape[0]) - 1
        if ws is None:
            ws = self._guard.workspace(self.workspace_bytes(rows))
        st = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._l.tdx_fsmnvad_forward(self._h, feat.data_ptr(), starts.data_ptr(), nclips, rows, p0.data_ptr(),
                                               post.data_ptr() if post is not None else None, ws.data_ptr(), ws.numel(), st))

    def features(self, clips):
        """list of 1-D clips -> (packed fbank frames [rows,80] on the device, frames per clip); clips of equal length share one
        tdx_fbank launch; a clip below 400 samples has no frames"""
        frames = [max(self.fbank.frames(int(c.shape[0])), 0) for c in clips]
        by_len, parts = {}, [None] * len(clips)
        for i, c in enumerate(clips):
            if frames[i] > 0:
                by_len.setdefault(int(c.shape[0]), []).append(i)
        for idxs in by_len.values():
            x = torch.stack([torch.as_tensor(np.ascontiguousarray(clips[i], dtype=np.float32)) if not isinstance(clips[i], torch.Tensor)
                             else clips[i].to(torch.float32) for i in idxs]).to(self.device)
            f = self.fbank(x)
            for j, i in enumerate(idxs):
                parts[i] = f[j]
        parts = [p for p in parts if p is not None]
        feat = torch.cat(parts).contiguous() if parts else torch.empty(0, 80, device=self.device)
        return feat, frames

    def posteriors(self, clips, with_post: bool = False):
        """list of clips -> list of p0 arrays [T_c] (float32), or of (p0, post [T_c,248]) pairs: ONE packed forward"""
        clips = [c.reshape(-1) for c in clips]
        with torch.cuda.device(self.device):
            feat, frames = self.features(clips)
            rows = int(feat.shape[0])
            starts = np.concatenate([[0], np.cumsum(frames)]).astype(np.int32)
            if rows == 0:
                empty = np.zeros(0, np.float32)
                return [(empty, np.zeros((0, NUM_CLASSES), np.float32)) if with_post else empty for _ in clips]
            if self.workspace_bytes(rows) == 0:
                raise _lib.TdxError(f"FsmnVad: {rows} frames in one forward (limit 2^22): split the batch")
            with self._guard.call():
                p0 = torch.empty(rows, device=self.device)
                post = torch.empty(rows, NUM_CLASSES, device=self.device) if with_post else None
                self.forward_into(feat, torch.from_numpy(starts).to(self.device), p0, post)
            p0 = p0.cpu().numpy()
            post = post.cpu().numpy() if with_post else None
        out = []
        for c in range(len(clips)):
            a, b = int(starts[c]), int(starts[c + 1])
            out.append((p0[a:b], post[a:b]) if with_post else p0[a:b])
        return out

    def detect_batch_ms(self, clips, max_end_silence_ms: int = 800):
        clips = [np.asarray(c).reshape(-1) if not isinstance(c, torch.Tensor) else c.reshape(-1) for c in clips]
        return [segments(p, int(c.shape[0]), max_end_silence_ms) for p, c in zip(self.posteriors(clips), clips)]

    def detect_batch(self, clips, min_silence_sec: float = 0.5):
        """list of 16 kHz clips -> per clip [[start_s, end_s], ...] (3 decimals); one packed forward for all of them"""
        return [[[round(p / 1000, 3) for p in seg] for seg in v] for v in self.detect_batch_ms(clips, int(min_silence_sec * 1000))]

    def __call__(self, audio, min_silence_sec: float = 0.5):
        return self.detect_batch([audio], min_silence_sec)[0]

    def close(self):
        self._own.close()
        self.fbank.close()


def build_vad(vad_state_dict=None, vad_cmvn=None, vad_model_dir=None, cuda_device: int = 0):
    """The device detector from weights, or from a funasr model directory; None when there is neither source."""
    if vad_state_dict is None:
        found = load_model_dir(vad_model_dir)
        if found is None:
            return None
        vad_state_dict, vad_cmvn = found
    return FsmnVad(vad_state_dict, vad_cmvn, device=f"cuda:{cuda_device}")
