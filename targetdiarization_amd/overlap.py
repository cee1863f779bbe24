"""Overlap-aware diarization after pyannote speaker-diarization-3.1 — the stage behind `self.od_pipeline`
(TargetDiarization.py:84,132,143; TargetDiarizationStream.py:175).  Third-party pipeline restated from upstream
[upstream-recall]; DESIGN §8.12 governs.

Plain functions over two callables, so the whole pipeline runs on the CPU against an oracle:
    segment(chunks [n,160000] float32) -> log-probabilities [n,589,7] of the powerset classes (segmentation.PyanNet)
    embed(list of 1-D clips)           -> [n,D] speaker embeddings (speaker.SpeakerEmbedder.get_speaker_embeddings)
`PyannoteDiarizer` binds them to the device models.

A third, optional callable makes step (4) pyannote's own:
    embed_masked(chunks [n,160000], masks [n,3,589]) -> [n,3,D]: every chunk embedded under the frame mask of each local
    speaker (speaker.WeSpeakerResNet34: one trunk pass per chunk, pooled under the three masks); a non-finite row is a
    missing embedding.  With WeSpeaker weights the published clustering threshold applies (parity with the published
    checkpoint is unpinned: no weights can be fetched).

Deviations from pyannote: without `embed_masked` the embedder is the project's own (ERes2NetV2 on the samples of a
speaker's frames, instead of wespeaker ResNet34 with a frame mask in its pooling), and the published clustering threshold
is uncalibrated for it; a (chunk, speaker) without an embedding joins the cluster that the other chunks hear on its active
frames (pyannote's distance to a NaN vector falls to cluster 0)."""
from __future__ import annotations

import numpy as np

SR = 16000
CHUNK = 160000                 # 10 s
STEP = 16000                   # 1 s
FRAME_STEP = 270               # samples per frame of the segmentation network
FRAME_FIELD = 991              # its receptive field
FRAMES = 589                   # frames of one chunk
POWERSET = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1]], dtype=np.int8)
DEFAULT_THRESHOLD = 0.7045654963945799      # speaker-diarization-3.1's published clustering threshold
MIN_CLUSTER_SIZE = 12
MIN_NUM_FRAMES = 2             # ceil(589 * 400 / 160000): 400 samples is the shortest clip that yields one fbank frame [upstream-recall]


def chunk_plan(n: int):
    """-> (chunk start samples, frames of the global grid).  A clip of at most 10 s is one (zero-padded) chunk; a longer one
    has chunks at k * 1 s while they fit, plus one zero-padded chunk at the next step when samples are left over."""
    if n <= CHUNK:
        starts = [0]
    else:
        starts = list(range(0, n - CHUNK + 1, STEP))
        if (n - CHUNK) % STEP > 0:
            starts.append(starts[-1] + STEP)
    return starts, frame_offset(starts[-1]) + FRAMES


def frame_offset(start: int) -> int:
    """global frame of a chunk's first frame"""
    return int(round(start / FRAME_STEP))


def cut_chunks(wave: np.ndarray, starts) -> np.ndarray:
    x = np.zeros((len(starts), CHUNK), dtype=np.float32)
    for i, a in enumerate(starts):
        seg = wave[a:a + CHUNK]
        x[i, :len(seg)] = seg
    return x


def powerset_to_speakers(logp: np.ndarray) -> np.ndarray:
    """[n,F,7] -> binary [n,F,3]: the hard argmax through the powerset table"""
    return POWERSET[np.argmax(logp, axis=-1)]


def speaker_count(seg: np.ndarray, starts, total: int) -> np.ndarray:
    """per global frame: rint of the mean, over the chunks that cover it, of the chunk's number of active speakers; 0 where
    no chunk covers the frame"""
    s, c = np.zeros(total), np.zeros(total)
    for k, a in enumerate(starts):
        o = frame_offset(a)
        s[o:o + seg.shape[1]] += seg[k].sum(axis=-1)
        c[o:o + seg.shape[1]] += 1
    return np.rint(np.divide(s, c, out=np.zeros(total), where=c > 0)).astype(np.int64)


def _runs(mask: np.ndarray):
    """[(first, last), ...] of the runs of True"""
    d = np.diff(np.concatenate([[0], mask.astype(np.int8), [0]]))
    return list(zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1))


def gather_clips(chunks: np.ndarray, seg: np.ndarray, min_embed_sec: float = 0.4):
    """One clip per (chunk, local speaker): the samples of the frames where it speaks alone, or, when those are fewer than
    min_embed_sec, of all its active frames; runs of frames are concatenated.  -> (clips, [(chunk, speaker), ...]); a pair
    with less than min_embed_sec either way is left out: its embedding is missing."""
    need = min_embed_sec * SR / FRAME_STEP
    clips, owner = [], []
    for k in range(seg.shape[0]):
        alone = seg[k].sum(axis=-1) == 1
        for j in range(seg.shape[2]):
            act = seg[k, :, j] > 0
            use = act & alone
            if use.sum() < need:
                use = act
            if use.sum() < need or not use.any():
                continue
            parts = [chunks[k, a * FRAME_STEP: min((b + 1) * FRAME_STEP, CHUNK)] for a, b in _runs(use)]
            clips.append(np.concatenate(parts))
            owner.append((k, j))
    return clips, owner


def pooling_masks(seg: np.ndarray, min_num_frames: int = MIN_NUM_FRAMES) -> np.ndarray:
    """[n,F,S] binary -> [n,S,F] float32 pooling masks: a speaker's frames without overlap (`clean`) when there are more than
    min_num_frames of them, else all its active frames"""
    clean = seg * (seg.sum(axis=-1, keepdims=True) < 2)
    few = clean.sum(axis=1, keepdims=True) <= min_num_frames
    return np.ascontiguousarray(np.where(few, seg, clean).transpose(0, 2, 1), dtype=np.float32)


def masked_embeddings(chunks: np.ndarray, seg: np.ndarray, embed_masked, min_num_frames: int = MIN_NUM_FRAMES):
    """pyannote's step (4): -> (emb [m,D], [(chunk, speaker), ...]) of the speakers that are active somewhere in their chunk
    and whose embedding came back finite; the others have none"""
    E = np.asarray(embed_masked(chunks, pooling_masks(seg, min_num_frames)), dtype=np.float64)
    active = seg.sum(axis=1) > 0
    owner = [(k, j) for k in range(seg.shape[0]) for j in range(seg.shape[2]) if active[k, j] and np.isfinite(E[k, j]).all()]
    emb = np.stack([E[k, j] for k, j in owner]) if owner else np.zeros((0, 1))
    return emb, owner


def _unit(x):
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-12)


def cluster_embeddings(X: np.ndarray, threshold: float = DEFAULT_THRESHOLD, min_cluster_size: int = MIN_CLUSTER_SIZE):
    """Centroid-linkage agglomerative clustering of the L2-normalised rows of X, cut at `threshold`; clusters smaller than
    min(min_cluster_size, max(1, round(0.1 n))) join the nearest large one (cosine distance of centroids); no large
    cluster: one cluster.  -> (labels [n] in 0..K-1, centroids [K,D])"""
    n = X.shape[0]
    U = _unit(np.asarray(X, dtype=np.float64))
    if n == 1:
        return np.zeros(1, dtype=np.int64), U.copy()
    from scipy.cluster.hierarchy import fcluster, linkage
    labels = fcluster(linkage(U, method="centroid", metric="euclidean"), threshold, criterion="distance") - 1
    msz = min(min_cluster_size, max(1, int(round(0.1 * n))))
    ids, sizes = np.unique(labels, return_counts=True)
    large = ids[sizes >= msz]
    if len(large) == 0:
        labels = np.zeros(n, dtype=np.int64)
    else:
        cen = {c: U[labels == c].mean(axis=0) for c in ids}
        L = _unit(np.stack([cen[c] for c in large]))
        for c in ids[sizes < msz]:
            labels[labels == c] = large[int(np.argmin(1.0 - L @ _unit(cen[c])))]
    _, labels = np.unique(labels, return_inverse=True)
    return labels.astype(np.int64), np.stack([U[labels == c].mean(axis=0) for c in range(labels.max() + 1)])


def assign_speakers(seg, starts, total, emb, owner, threshold=DEFAULT_THRESHOLD, min_cluster_size=MIN_CLUSTER_SIZE, min_active_ratio=0.2):
    """-> [n,3] cluster of every (chunk, local speaker), -1 for a speaker that is never active.  Trained on the embeddings
    whose speaker is active in at least 20 % of its chunk's frames (none is: one cluster); every present embedding then goes
    to the nearest centroid (cosine); the missing ones, which have no vector to measure from, are assigned afterwards (module
    docstring)."""
    n, F, S = seg.shape
    out = np.full((n, S), -1, dtype=np.int64)
    active = seg.sum(axis=1) > 0
    train = np.array([seg[k, :, j].mean() >= min_active_ratio for k, j in owner], dtype=bool)
    if not train.any():
        out[active] = 0
        return out
    emb = np.asarray(emb, dtype=np.float64)
    _, cen = cluster_embeddings(emb[train], threshold, min_cluster_size)
    near = np.argmin(1.0 - _unit(emb) @ _unit(cen).T, axis=1)
    for (k, j), c in zip(owner, near):
        out[k, j] = c
    missing = [(k, j) for k in range(n) for j in range(S) if active[k, j] and out[k, j] < 0]
    if missing:
        heard = np.zeros((total, cen.shape[0]))
        for (k, j), c in zip(owner, near):
            o = frame_offset(starts[k])
            heard[o:o + F, c] += seg[k, :, j]
        for k, j in missing:
            o = frame_offset(starts[k])
            out[k, j] = int(np.argmax((heard[o:o + F] * seg[k, :, j:j + 1]).sum(axis=0)))
    return out


def reconstruct(seg, starts, total, clusters, count):
    """per chunk and cluster the max over the local speakers assigned to it, summed over the chunks on the global grid; per
    frame the count[t] clusters with the largest sums are on.  -> binary [total,K]"""
    K = int(clusters.max()) + 1 if clusters.size and clusters.max() >= 0 else 0
    act = np.zeros((total, max(K, 1)))
    for k, a in enumerate(starts):
        o = frame_offset(a)
        for c in range(K):
            js = np.flatnonzero(clusters[k] == c)
            if len(js):
                act[o:o + seg.shape[1], c] += seg[k][:, js].max(axis=1)
    order = np.argsort(-act, axis=1, kind="stable")
    on = np.zeros_like(act, dtype=bool)
    for r in range(min(act.shape[1], int(count.max()) if count.size else 0)):
        rows = np.flatnonzero(count > r)
        on[rows, order[rows, r]] = True
    return on & (act > 0)


def tracks_of(on: np.ndarray, n_samples: int):
    """runs per cluster -> [(start_s, end_s, "SPEAKER_%02d"), ...] sorted by start; a run goes from the middle of its first
    frame to the middle of its last; clusters are numbered by first appearance; clipped to the clip"""
    mid = lambda t: (t * FRAME_STEP + FRAME_FIELD / 2.0) / SR
    dur = n_samples / SR
    runs = []
    for c in range(on.shape[1]):
        for a, b in _runs(on[:, c]):
            s, e = min(mid(a), dur), min(mid(b), dur)
            if e > s:
                runs.append((s, e, c))
    runs.sort(key=lambda r: (r[0], r[2]))
    names = {}
    for _, _, c in runs:
        names.setdefault(c, "SPEAKER_%02d" % len(names))
    return [(round(float(s), 3), round(float(e), 3), names[c]) for s, e, c in runs]


def diarize(wave, segment, embed, threshold: float = DEFAULT_THRESHOLD, min_embed_sec: float = 0.4, min_cluster_size: int = MIN_CLUSTER_SIZE,
            embed_masked=None):
    """16 kHz mono clip -> [(start_s, end_s, "SPEAKER_xx"), ...] (what od_result_parser reads).  With `embed_masked` the
    embeddings are pooled under frame masks (module docstring) and `embed` / min_embed_sec are not used."""
    wave = np.asarray(wave, dtype=np.float32).reshape(-1)
    if wave.shape[0] == 0:
        return []
    starts, total = chunk_plan(wave.shape[0])
    chunks = cut_chunks(wave, starts)
    seg = powerset_to_speakers(np.asarray(segment(chunks)))
    count = speaker_count(seg, starts, total)
    if not count.any():
        return []
    if embed_masked is not None:
        emb, owner = masked_embeddings(chunks, seg, embed_masked)
    else:
        clips, owner = gather_clips(chunks, seg, min_embed_sec)
        emb = np.asarray(embed(clips)) if clips else np.zeros((0, 1))
    clusters = assign_speakers(seg, starts, total, emb, owner, threshold, min_cluster_size)
    return tracks_of(reconstruct(seg, starts, total, clusters, count), wave.shape[0])


class PyannoteDiarizer:
    """`od_pipeline(audio) -> [(start, end, "SPEAKER_xx"), ...]` on the device: segmentation.PyanNet for the chunks, `embed`
    (HotPath.spk.get_speaker_embeddings, or any callable) for the cross-chunk identity, or `embedder`
    (speaker.WeSpeakerResNet34), which takes its place with masked pooling.  threshold <= 0: the published one."""

    def __init__(self, model, embed, threshold: float = 0.0, min_embed_sec: float = 0.4, min_cluster_size: int = MIN_CLUSTER_SIZE,
                 embedder=None):
        self.model = model
        self.embed = embed
        self.embedder = embedder
        self.threshold = float(threshold) if threshold and threshold > 0 else DEFAULT_THRESHOLD
        self.min_embed_sec = min_embed_sec
        self.min_cluster_size = min_cluster_size

    def segment(self, chunks: np.ndarray) -> np.ndarray:
        import torch
        return self.model.log_probs(torch.from_numpy(np.ascontiguousarray(chunks, dtype=np.float32)).to(self.model.device)).cpu().numpy()

    def embed_masked(self, chunks: np.ndarray, masks: np.ndarray) -> np.ndarray:
        import torch
        dev = self.embedder.device
        return self.embedder(torch.from_numpy(np.ascontiguousarray(chunks, dtype=np.float32)).to(dev),
                             torch.from_numpy(np.ascontiguousarray(masks, dtype=np.float32)).to(dev)).cpu().numpy()

    def __call__(self, audio):
        return diarize(audio, self.segment, self.embed, self.threshold, self.min_embed_sec, self.min_cluster_size,
                       embed_masked=self.embed_masked if self.embedder is not None else None)

    def close(self):
        self.model.close()
        if self.embedder is not None:
            self.embedder.close()


def load_model_dir(path):
    """a pyannote checkpoint (segmentation or embedding) in a directory: pytorch_model.bin (the state dict, bare or under "state_dict");
    None when `path` is not such a directory"""
    import os
    if not isinstance(path, str) or not os.path.isdir(path):
        return None
    ckpt = os.path.join(path, "pytorch_model.bin")
    if not os.path.isfile(ckpt):
        return None
    import torch
    sd = torch.load(ckpt, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and "state_dict" in sd:
        sd = sd["state_dict"]
    return sd


def build_od_pipeline(od_state_dict=None, od_model_dir=None, embed=None, threshold: float = 0.0, cuda_device: int = 0,
                      od_embed_state_dict=None, od_embed_model_dir=None):
    """The device overlap detector from weights, or from a directory holding pytorch_model.bin; None when there is neither
    source.  A directory that fails — an unreadable file, a checkpoint the loader rejects, no embedder to share — is reported
    and leaves None, like the reference's other optional stages; weights handed in directly fail loudly.
    od_embed_state_dict / od_embed_model_dir: WeSpeaker ResNet34 weights for the masked-pooling embedder, which then takes
    the place of `embed`; a directory that fails is reported and leaves the `embed` path."""
    from .segmentation import PyanNet

    def make_embedder():
        from .speaker import WeSpeakerResNet34
        if od_embed_state_dict is not None:
            return WeSpeakerResNet34(od_embed_state_dict, device=f"cuda:{cuda_device}")
        if od_embed_model_dir is None:
            return None
        try:
            sd = load_model_dir(od_embed_model_dir)
            if sd is None:
                raise FileNotFoundError("no pytorch_model.bin")
            return WeSpeakerResNet34(sd, device=f"cuda:{cuda_device}")
        except Exception as e:
            print(f"Failed to load the overlap detector's embedder from {od_embed_model_dir}: {e}")
            return None

    def make(sd):
        if embed is None and od_embed_state_dict is None and od_embed_model_dir is None:
            raise ValueError("the overlap detector needs a speaker embedder: pass spk_state_dict, od_embed or od_embed_state_dict")
        model = PyanNet(sd, device=f"cuda:{cuda_device}")
        try:
            embedder = make_embedder()
            if embedder is None and embed is None:
                raise ValueError("the overlap detector needs a speaker embedder: pass spk_state_dict or od_embed")
        except BaseException:
            model.close()
            raise
        return PyannoteDiarizer(model, embed, threshold, embedder=embedder)

    if od_state_dict is not None:
        return make(od_state_dict)
    try:
        sd = load_model_dir(od_model_dir)
        return make(sd) if sd is not None else None
    except Exception as e:
        print(f"Failed to load the overlap detector from {od_model_dir}: {e}")
        return None
