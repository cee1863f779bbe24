"""silero-VAD: the device network over the C-ABI (tdx_silero_*, csrc/silero_vad.hip) and the host state machine — the model
behind `get_speech_timestamps(audio, self.vad_model)` in TargetDiarizationStream.should_wait_for_next_chunk
(TargetDiarizationStream.py:128-131, the `stream_vad` plug-in) and AudioProcessor.separate_speaker(low_gpu_ram=True)
(AudioProcessor.py:903-905, the `silero_vad` plug-in).

Third-party model (silero-vad v5, the `silero_vad` package's 16 kHz branch), restated from the published code
[upstream-recall]; parity with the published weights is unpinned (none is at hand).  The device returns one speech
probability per 512-sample chunk; `speech_timestamps` turns them into ranges with upstream's get_speech_timestamps state
machine."""
from __future__ import annotations

import os
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .weights import pack_silero_vad_blob

CHUNK = 512
SR = 16000
FEAT = 128


def speech_timestamps(probs, n_samples: int, threshold: float = 0.5, min_speech_duration_ms: int = 250,
                      min_silence_duration_ms: int = 100, speech_pad_ms: int = 30, neg_threshold=None, return_seconds: bool = False):
    """Upstream's get_speech_timestamps over per-chunk probabilities (chunk i covers samples [512 i, 512 i + 512)) of one
    clip of n_samples at 16 kHz -> [[start, end], ...] in samples, or in seconds rounded to 1 decimal (as upstream does).
    A chunk with p >= threshold opens a segment at 512 i and clears a pending end; inside a segment the first chunk with
    p < neg (threshold - 0.15, at least 0.01) marks a possible end, and once 512 i - end >= min_silence the segment closes there,
    kept only if longer than min_speech; a segment still open at the end closes at n_samples under the same rule.  Then the
    padding: speech_pad on the outer sides (clipped to the clip), between neighbours speech_pad each, or half the gap each
    where the gap is under two pads.  The `max_speech_duration_s` branch of upstream is left out: no call site of the
    reference passes it."""
    p = np.asarray(probs, dtype=np.float64).reshape(-1)
    n_samples = int(n_samples)
    min_speech = SR * min_speech_duration_ms / 1000
    min_silence = SR * min_silence_duration_ms / 1000
    pad = int(SR * speech_pad_ms / 1000)
    neg = max(threshold - 0.15, 0.01) if neg_threshold is None else neg_threshold
    speeches, triggered, start, temp_end = [], False, 0, 0
    for i, v in enumerate(p):
        pos = CHUNK * i
        if v >= threshold and temp_end:
            temp_end = 0
        if v >= threshold and not triggered:
            triggered, start = True, pos
            continue
        if v < neg and triggered:
            if not temp_end:
                temp_end = pos
            if pos - temp_end < min_silence:
                continue
            if temp_end - start > min_speech:
                speeches.append([start, temp_end])
            triggered, temp_end = False, 0
    if triggered and n_samples - start > min_speech:
        speeches.append([start, n_samples])
    for i, s in enumerate(speeches):
        if i == 0:
            s[0] = int(max(0, s[0] - pad))
        if i != len(speeches) - 1:
            gap = speeches[i + 1][0] - s[1]
            if gap < 2 * pad:
                s[1] += int(gap // 2)
                speeches[i + 1][0] = int(max(0, speeches[i + 1][0] - gap // 2))
            else:
                s[1] = int(min(n_samples, s[1] + pad))
                speeches[i + 1][0] = int(max(0, speeches[i + 1][0] - pad))
        else:
            s[1] = int(min(n_samples, s[1] + pad))
    if return_seconds:
        return [[round(a / SR, 1), round(b / SR, 1)] for a, b in speeches]
    return [[int(a), int(b)] for a, b in speeches]


def normalize_state_dict(raw):
    """the 16 kHz branch under its bare names: the `_model.` prefix stripped, the 8 kHz branch (`_model_8k.*`) dropped"""
    out = OrderedDict()
    for k, v in raw.items():
        if k.startswith("_model_8k."):
            continue
        out[k[len("_model."):] if k.startswith("_model.") else k] = v
    return out


def load_model_file(path):
    """a silero-VAD weight file -> state dict (as stored; see normalize_state_dict), None when `path` is not a readable one.
    `.safetensors` through safetensors.torch.load_file; `.jit` / `.pt` through torch.jit.load(...).state_dict(), falling back
    to torch.load(weights_only=True)."""
    if not isinstance(path, str) or not os.path.isfile(path):
        return None
    try:
        if path.endswith(".safetensors"):
            from safetensors.torch import load_file
            return load_file(path)
        try:
            return torch.jit.load(path, map_location="cpu").state_dict()
        except Exception:                                   # noqa: BLE001  (not a TorchScript archive)
            sd = torch.load(path, map_location="cpu", weights_only=True)
            if isinstance(sd, dict) and "state_dict" in sd:
                sd = sd["state_dict"]
            return sd if isinstance(sd, dict) else None
    except Exception:                                       # noqa: BLE001
        return None


def _flat(audio) -> np.ndarray:
    if isinstance(audio, torch.Tensor):
        audio = audio.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(audio, dtype=np.float32).reshape(-1))


class SileroVad:
    """`stream_vad(audio) -> [[start_s, end_s], ...]` (and `.frames(audio) -> [[start, end], ...]` in samples, the
    `AudioProcessor.silero_vad` format) on the device.  state_dict: silero-vad v5's names, with or without `_model.`."""

    def __init__(self, state_dict, device="cuda:0"):
        self._l = _lib.lib()
        self._own = _lib.Handle(device, "SileroVad", self._l.tdx_silero_create, self._l.tdx_silero_destroy,
                                blob=pack_silero_vad_blob(normalize_state_dict(state_dict)))
        self.device, self._h, self._guard = self._own.device, self._own.ptr, self._own.guard

    def flops(self, total_chunks: int) -> float:
        return float(self._l.tdx_silero_flops(self._h, total_chunks))

    def workspace_bytes(self, nclips: int, total_chunks: int) -> int:
        return int(self._l.tdx_silero_workspace_bytes(self._h, nclips, total_chunks))

    def forward_into(self, wav, chunk_starts, prob, tap_feat=None, tap_h=None, ws=None):
        """the bare C call on the current stream: wav [total_chunks*512] (clips packed, each zero-padded to whole chunks),
        chunk_starts int32 [nclips+1] (device), prob [total_chunks], tap_feat / tap_h None or [total_chunks,128]; ws: a uint8
        device tensor of workspace_bytes(nclips, total_chunks) (None: the object's grow-only workspace; hold
        `self._guard.call()` around it then).  No allocation when ws is given: this is what a graph capture records."""
        total, nclips = int(prob.shape[0]), int(chunk_starts.shape[0]) - 1
        if ws is None:
            ws = self._guard.workspace(self.workspace_bytes(nclips, total))
        st = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._l.tdx_silero_forward(self._h, wav.data_ptr(), chunk_starts.data_ptr(), nclips, total, prob.data_ptr(),
                                              tap_feat.data_ptr() if tap_feat is not None else None,
                                              tap_h.data_ptr() if tap_h is not None else None, ws.data_ptr(), ws.numel(), st))

    def probabilities(self, clips, taps: bool = False):
        """list of 1-D 16 kHz clips -> list of p arrays [ceil(n/512)] (float32), or of (p, feat [N,128], h [N,128]) triples:
        ONE packed forward; an empty clip gives empty arrays and takes no part in it"""
        clips = [_flat(c) for c in clips]
        chunks = [(int(c.shape[0]) + CHUNK - 1) // CHUNK for c in clips]
        live = [i for i, n in enumerate(chunks) if n > 0]
        total = int(sum(chunks))
        empty = np.zeros(0, np.float32)
        none = (empty, np.zeros((0, FEAT), np.float32), np.zeros((0, FEAT), np.float32)) if taps else empty
        if total == 0:
            return [none for _ in clips]
        if self.workspace_bytes(len(live), total) == 0:
            raise _lib.TdxError(f"SileroVad: {len(live)} clips / {total} chunks in one forward (limits 1024 / 2^20): split the batch")
        packed = np.zeros(total * CHUNK, np.float32)
        starts = np.zeros(len(live) + 1, np.int32)
        for j, i in enumerate(live):
            packed[starts[j] * CHUNK: starts[j] * CHUNK + clips[i].shape[0]] = clips[i]
            starts[j + 1] = starts[j] + chunks[i]
        with torch.cuda.device(self.device):
            with self._guard.call():
                wav = torch.from_numpy(packed).to(self.device)
                prob = torch.empty(total, device=self.device)
                feat = torch.empty(total, FEAT, device=self.device) if taps else None
                hh = torch.empty(total, FEAT, device=self.device) if taps else None
                self.forward_into(wav, torch.from_numpy(starts).to(self.device), prob, feat, hh)
            prob = prob.cpu().numpy()
            feat, hh = (feat.cpu().numpy(), hh.cpu().numpy()) if taps else (None, None)
        out = [none for _ in clips]
        for j, i in enumerate(live):
            a, b = int(starts[j]), int(starts[j + 1])
            out[i] = (prob[a:b], feat[a:b], hh[a:b]) if taps else prob[a:b]
        return out

    def timestamps_batch(self, clips, **kw):
        """list of clips -> per clip speech_timestamps(p, n_samples, **kw); one packed forward for all of them"""
        clips = [_flat(c) for c in clips]
        return [speech_timestamps(p, int(c.shape[0]), **kw) for p, c in zip(self.probabilities(clips), clips)]

    def frames(self, audio):
        """[[start, end], ...] in samples: get_speech_timestamps(audio, model, threshold=0.5, min_silence_duration_ms=100)"""
        return self.timestamps_batch([audio], threshold=0.5, min_silence_duration_ms=100)[0]

    def __call__(self, audio):
        """[[start_s, end_s], ...]: the same with return_seconds=True (1 decimal)"""
        return self.timestamps_batch([audio], threshold=0.5, min_silence_duration_ms=100, return_seconds=True)[0]

    def close(self):
        self._own.close()


def build_silero(state_dict=None, model_file=None, cuda_device: int = 0):
    """The device detector from weights, or from a weight file; None when there is neither source."""
    if state_dict is None:
        state_dict = load_model_file(model_file)
        if state_dict is None:
            if model_file is not None:
                raise ValueError(f"{model_file}: not a readable silero-VAD weight file")
            return None
    return SileroVad(state_dict, device=f"cuda:{cuda_device}")
