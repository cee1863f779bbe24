"""CAM++ speaker diarization: the stage behind `TargetDiarization.sd_pipeline` (TargetDiarization.py:73, :126).

Restates modelscope's segmentation-clustering pipeline `iic/speech_campplus_speaker-diarization_common`
[upstream-recall: the package is third-party and absent; DESIGN §8.10 is the governing description]:
    speech ranges (the `vad` plug-in) -> 1.5 s windows at a 0.75 s shift -> CAM++ embeddings (csrc/campplus.hip, ONE bucketed
    launch sequence for all windows) -> spectral clustering (clustering.spectral_labels, or spectral_labels_device) -> time post-processing.
The host logic is plain functions over an `embed(list_of_windows) -> [n,192]` callable, so that it runs on the CPU against
an oracle embedder; `CamppDiarizer` binds it to `SpeakerEmbedder.embed_device`.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from .clustering import spectral_labels

SR = 16000
WINDOW = 24000      # 1.5 s
SHIFT = 12000       # 0.75 s


def plan_windows(ranges, n_samples: int, window: int = WINDOW, shift: int = SHIFT):
    """speech ranges [[start_s, end_s], ...] -> windows [(st, ed)] in samples, ed - st == window except for a range
    shorter than one window (one window [a, b), zero-padded by cut_windows)."""
    out = []
    for s, e in ranges:
        a, b = max(0, int(round(s * SR))), min(n_samples, int(round(e * SR)))
        n = b - a
        if n <= 0:
            continue
        last_ed = 0
        for st in range(0, n, shift):
            ed = min(st + window, n)
            if ed <= last_ed:
                break
            out.append((a + max(0, ed - window), a + ed))
            last_ed = ed
    return out


def cut_windows(audio: np.ndarray, windows, window: int = WINDOW):
    """the windows' samples, each zero-padded to `window`"""
    out = []
    for st, ed in windows:
        w = np.asarray(audio[st:ed], dtype=np.float32)
        if w.shape[0] < window:
            w = np.concatenate([w, np.zeros(window - w.shape[0], dtype=np.float32)])
        out.append(w)
    return out


def _merge_same(segs):
    out = []
    for s, e, l in segs:
        if out and out[-1][2] == l and s <= out[-1][1] + 1e-4:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e, l])
    return out


def postprocess(windows, labels, min_dur: float = 1.0):
    """windows [(st, ed)] in samples (chronological) and their labels -> [[start_s, end_s, label], ...]: relabel by first
    appearance, merge adjacent windows of one label, cut overlapping neighbours at the midpoint, hand segments shorter than
    min_dur to the nearer neighbour in time, merge again, renumber the surviving labels by first appearance, round to
    3 decimals."""
    remap = {}
    segs = []
    for (st, ed), l in zip(windows, labels):
        l = remap.setdefault(int(l), len(remap))
        segs.append([st / SR, ed / SR, l])
    segs = _merge_same(segs)
    for i in range(1, len(segs)):
        if segs[i - 1][1] - segs[i][0] > 1e-4:
            mid = 0.5 * (segs[i - 1][1] + segs[i][0])
            segs[i - 1][1] = mid
            segs[i][0] = mid
    if len(segs) > 1:
        for i, sg in enumerate(segs):
            if sg[1] - sg[0] >= min_dur:
                continue
            prev_gap = sg[0] - segs[i - 1][1] if i > 0 else np.inf
            next_gap = segs[i + 1][0] - sg[1] if i + 1 < len(segs) else np.inf
            if prev_gap <= next_gap:            # (ties: the earlier neighbour; it has been settled already)
                sg[2] = segs[i - 1][2]
            else:
                sg[2] = segs[i + 1][2]
        segs = _merge_same(segs)
    dense = {}                                  # labels that lost all their segments leave no gaps in the numbering
    return [[round(s, 3), round(e, 3), dense.setdefault(int(l), len(dense))] for s, e, l in segs]


def diarize(audio: np.ndarray, embed: Callable, vad: Optional[Callable] = None, oracle_num: Optional[int] = None,
            return_windows: bool = False, cluster: Callable = spectral_labels, **cluster_kw):
    """audio: 16 kHz mono float waveform -> {"text": [[start_s, end_s, label], ...]} (intervals.sd_result_parser's input).
    `cluster(embeddings, oracle_num=..., **cluster_kw) -> labels` receives the embeddings as a float64 array, or, where `embed`
    returns a torch tensor, that tensor as it is (clustering.spectral_labels_device takes it on the device)."""
    audio = np.asarray(audio, dtype=np.float32).reshape(-1)
    n = audio.shape[0]
    ranges = vad(audio) if vad is not None else ([[0.0, n / SR]] if n else [])
    windows = plan_windows(ranges, n)
    if not windows:
        res = {"text": []}
        return (res, [], np.zeros(0, dtype=np.int64)) if return_windows else res
    emb = embed(cut_windows(audio, windows))
    if not hasattr(emb, "data_ptr"):            # a device tensor goes to `cluster` as it is
        emb = np.asarray(emb, dtype=np.float64)
    labels = np.asarray(cluster(emb, oracle_num=oracle_num, **cluster_kw))
    res = {"text": postprocess(windows, labels)}
    return (res, windows, labels) if return_windows else res


class CamppDiarizer:
    """`sd_pipeline` on the device: window embeddings from SpeakerEmbedder(arch="campplus").embed_device.  cluster="host" (the default):
    the embeddings come to the host and clustering.spectral_labels runs there.  cluster="device": they stay on the device, the affinity,
    the Laplacian and its eigenvectors are computed there (clustering.spectral_labels_device, csrc/spectral.hip) and only the [n,16]
    eigenvectors and the embeddings come back for the shared k-means / merge tail."""

    def __init__(self, state_dict, cuda_device: int = 0, vad: Optional[Callable] = None, max_batch_frames: int = 40000,
                 cluster: str = "host", **cluster_kw):
        from .speaker import SpeakerEmbedder
        if cluster not in ("host", "device"):
            raise ValueError(f"CamppDiarizer: cluster must be \"host\" or \"device\", not {cluster!r}")
        self.cluster = cluster
        self.embedder = SpeakerEmbedder(state_dict, cuda_device=cuda_device, max_batch_frames=max_batch_frames, arch="campplus")
        self.vad = vad
        self.cluster_kw = cluster_kw

    def embed(self, windows):
        """list of equal-length float32 arrays -> [n,192] array: ONE upload, one bucketed launch sequence"""
        if not windows:
            return np.zeros((0, 192), dtype=np.float32)
        return self.embed_device(windows).cpu().numpy()

    def embed_device(self, windows):
        """the same, the [n,192] float32 result left on the device (n >= 1)"""
        import torch
        x = torch.from_numpy(np.stack(windows)).to(self.embedder.device)
        return self.embedder.embed_device(list(x))

    def __call__(self, audio_16k, oracle_num: Optional[int] = None, return_windows: bool = False):
        if self.cluster == "device":
            from .clustering import spectral_labels_device
            return diarize(audio_16k, self.embed_device, vad=self.vad, oracle_num=oracle_num, return_windows=return_windows,
                           cluster=spectral_labels_device, **self.cluster_kw)
        return diarize(audio_16k, self.embed, vad=self.vad, oracle_num=oracle_num, return_windows=return_windows, **self.cluster_kw)
