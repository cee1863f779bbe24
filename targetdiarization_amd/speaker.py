"""ERes2NetV2, CAM++ and WeSpeaker ResNet34 speaker-embedding extractors over the C-ABI (tdx_eres2net_*, tdx_campp_*,
tdx_wespk_*) and the TargetASR-compatible host methods (TargetASR.py:144-163)."""
from __future__ import annotations


import numpy as np
import torch

from . import _lib, ops
from .frontend import Fbank
from .weights import drop_num_batches_tracked, pack_blob


class ERes2NetV2:
    def __init__(self, state_dict, device="cuda:0", graph_frames: int = 4000):
        """graph_frames: forwards with B*F <= graph_frames fbank frames are replayed as HIP graphs (_lib.GraphRunner); 0 disables"""
        self.graph_frames = graph_frames
        self._l = _lib.lib()
        self._own = _lib.Handle(device, "ERes2NetV2", self._l.tdx_eres2net_create, self._l.tdx_eres2net_destroy, blob=pack_blob(state_dict))
        self.device, self._h, self._guard = self._own.device, self._own.ptr, self._own.guard
        self._graphs = _lib.GraphRunner(self.device)
        self.fbank = Fbank("sv", self.device)

    def flops(self, B, F):
        return float(self._l.tdx_eres2net_flops(self._h, B, F))

    def embed_features(self, feat: torch.Tensor) -> torch.Tensor:
        """feat [B,F,80] (mean-normalised fbank) -> [B,192]"""
        feat = feat.to(self.device, torch.float32).contiguous()
        B, F, _ = feat.shape
        nb = int(self._l.tdx_eres2net_workspace_bytes(self._h, B, F))
        if nb == 0:
            raise _lib.TdxError("ERes2NetV2: need at least 9 fbank frames")
        with torch.cuda.device(self.device), self._guard.call():
            if self.graph_frames and B * F <= self.graph_frames:
                def launch(si, so, ws, st):
                    _lib.check(self._l.tdx_eres2net_forward(self._h, si.data_ptr(), B, F, so.data_ptr(), ws.data_ptr(), ws.numel(), st))
                out = self._graphs((B, F), feat, (B, 192), nb, launch)        # None until the shape is seen a second time
                if out is not None:
                    return out
            ws = self._guard.workspace(nb)
            out = torch.empty(B, 192, device=self.device)
            st = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(self._l.tdx_eres2net_forward(self._h, feat.data_ptr(), B, F, out.data_ptr(), ws.data_ptr(), ws.numel(), st))
            return out

    def __call__(self, wav: torch.Tensor) -> torch.Tensor:
        """wav [B,N] in [-1,1] -> [B,192]; all B clips share N (bucket by length)."""
        if wav.ndim == 1:
            wav = wav[None]
        return self.embed_features(self.fbank(wav))

    def close(self):
        self._own.close()
        self.fbank.close()


class CAMPPlus:
    """CAM++ (csrc/campplus.hip): the same front end and surface as ERes2NetV2; state_dict with 3D-Speaker's names."""

    def __init__(self, state_dict, device="cuda:0"):
        self._l = _lib.lib()
        self._own = _lib.Handle(device, "CAMPPlus", self._l.tdx_campp_create, self._l.tdx_campp_destroy,
                                blob=pack_blob(drop_num_batches_tracked(state_dict)))
        self.device, self._h, self._guard = self._own.device, self._own.ptr, self._own.guard
        self.fbank = Fbank("sv", self.device)

    def flops(self, B, F):
        return float(self._l.tdx_campp_flops(self._h, B, F))

    def embed_features(self, feat: torch.Tensor) -> torch.Tensor:
        """feat [B,F,80] (mean-normalised fbank) -> [B,192]"""
        feat = feat.to(self.device, torch.float32).contiguous()
        B, F, _ = feat.shape
        nb = int(self._l.tdx_campp_workspace_bytes(self._h, B, F))
        if nb == 0:
            raise _lib.TdxError("CAMPPlus: need at least 9 fbank frames (and B*F*80 < 2^31 per launch)")
        with torch.cuda.device(self.device), self._guard.call():
            ws = self._guard.workspace(nb)
            out = torch.empty(B, 192, device=self.device)
            st = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(self._l.tdx_campp_forward(self._h, feat.data_ptr(), B, F, out.data_ptr(), ws.data_ptr(), ws.numel(), st))
            return out

    def __call__(self, wav: torch.Tensor) -> torch.Tensor:
        """wav [B,N] in [-1,1] -> [B,192]; all B clips share N (bucket by length)."""
        if wav.ndim == 1:
            wav = wav[None]
        return self.embed_features(self.fbank(wav))

    def close(self):
        self._own.close()
        self.fbank.close()


class WeSpeakerResNet34:
    """WeSpeaker ResNet34 with pyannote's masked statistics pooling (csrc/wespeaker.hip): the embedder of pyannote
    speaker-diarization-3.1; state_dict with upstream's names under `resnet.`.  One trunk pass per chunk, pooled under each of
    the S frame masks.  Batches above max_chunks_per_launch are cut on the host."""

    EMB = 256

    def __init__(self, state_dict, device="cuda:0", max_chunks_per_launch: int = 16):
        self._l = _lib.lib()
        self._own = _lib.Handle(device, "WeSpeakerResNet34", self._l.tdx_wespk_create, self._l.tdx_wespk_destroy,
                                blob=pack_blob(drop_num_batches_tracked(state_dict)))
        self.device, self._h, self._guard = self._own.device, self._own.ptr, self._own.guard
        self.max_chunks_per_launch = max(1, min(int(max_chunks_per_launch), 64))
        self.fbank = Fbank("wespeaker", self.device)

    @staticmethod
    def flops(B, F):
        """multiply-adds x 2 of the trunk and seg_1 for B chunks of F frames (one pooling)"""
        fl, H, W, cin = 2.0 * 80 * F * 9 * 32, 80, F, 32
        for li, nb in enumerate((3, 4, 6, 3)):
            cout = 32 << li
            for i in range(nb):
                stride = 2 if (i == 0 and li > 0) else 1
                H, W = (H - 1) // stride + 1, (W - 1) // stride + 1
                fl += 2.0 * H * W * cout * (9 * cin + 9 * cout + (cin if (stride != 1 or cin != cout) else 0))
                cin = cout
        return float(B) * (fl + 2.0 * 5120 * 256)

    def workspace_bytes(self, B, F, S=1):
        return int(self._l.tdx_wespk_workspace_bytes(self._h, B, F, S))

    def embed_features(self, feat: torch.Tensor, weights: torch.Tensor = None) -> torch.Tensor:
        """feat [B,F,80] (Fbank("wespeaker")), weights None | [B,S,Fw] per-frame masks on any frame grid -> [B,S,256]
        ([B,256] without weights); a row whose mask vanishes on the trunk's frames is NaN"""
        feat = feat.to(self.device, torch.float32).contiguous()
        B, F, _ = feat.shape
        if weights is not None:
            weights = weights.to(self.device, torch.float32).contiguous()
            if weights.ndim != 3 or weights.shape[0] != B:
                raise _lib.TdxError(f"WeSpeakerResNet34: weights must be [B,S,Fw] with B = {B}, got {tuple(weights.shape)}")
        S, Fw = (1, 1) if weights is None else (int(weights.shape[1]), int(weights.shape[2]))
        out = torch.empty(B, S, self.EMB, device=self.device)
        with torch.cuda.device(self.device), self._guard.call():
            st = torch.cuda.current_stream(self.device).cuda_stream
            for b0 in range(0, max(B, 1), self.max_chunks_per_launch):
                nb_ = min(self.max_chunks_per_launch, B - b0)
                nbytes = self.workspace_bytes(nb_, F, S) if self._h else 1
                if nbytes == 0:
                    raise _lib.TdxError("WeSpeakerResNet34: need 1 <= B, F >= 1, 1 <= S <= 8, Fw >= 1 and B*F*2560 < 2^31 per launch")
                ws = self._guard.workspace(nbytes)
                _lib.check(self._l.tdx_wespk_forward(self._h, feat[b0:b0 + nb_].data_ptr(), nb_, F,
                                                     None if weights is None else weights[b0:b0 + nb_].data_ptr(), S, Fw,
                                                     out[b0:b0 + nb_].data_ptr(), ws.data_ptr(), ws.numel(), st))
        return out[:, 0] if weights is None else out

    def __call__(self, wav: torch.Tensor, weights: torch.Tensor = None) -> torch.Tensor:
        """wav [B,N] in [-1,1] -> [B,S,256] ([B,256] without weights); all B clips share N"""
        if wav.ndim == 1:
            wav = wav[None]
        return self.embed_features(self.fbank(wav), weights)

    def close(self):
        self._own.close()
        self.fbank.close()


class SpeakerEmbedder:
    """The two hot-path methods of the reference's TargetASR (TargetASR.py:144-163) plus the
    batched forms the MI355X pipeline uses (hot loops A/C of TargetDiarization.infer issue one
    embedding call per segment; here equal-length segments share a launch)."""

    def __init__(self, state_dict, cuda_device: int = 0, max_batch_frames: int = 40000, arch: str = "eres2netv2"):
        if arch == "eres2netv2":
            self.model = ERes2NetV2(state_dict, device=f"cuda:{cuda_device}")
        elif arch == "campplus":
            self.model = CAMPPlus(state_dict, device=f"cuda:{cuda_device}")
        else:
            raise _lib.TdxError(f"SpeakerEmbedder: unknown arch {arch!r} (eres2netv2 | campplus)")
        self.arch = arch
        self.device = self.model.device
        self.max_batch_frames = max_batch_frames

    @staticmethod
    def _read_wav(path: str) -> np.ndarray:
        """16 kHz mono PCM16 .wav -> float32 in [-1,1] (stdlib `wave`; anything else is outside the hot path:
        the reference decodes through modelscope's loader)."""
        import wave
        with wave.open(path, "rb") as w:
            if w.getframerate() != 16000 or w.getnchannels() != 1 or w.getsampwidth() != 2:
                raise _lib.TdxError(f"get_speaker_embedding: {path}: need 16 kHz mono PCM16 (resampling/decoding is outside the hot path)")
            return np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16).astype(np.float32) / 32768.0

    # TargetASR.py:155-163
    def get_speaker_embedding(self, wav_file, embedding_model="eres2netv2_large"):
        """wav_file: np.ndarray waveform | path of a 16 kHz mono wav | list of either (the reference hands the
        list to the modelscope pipeline, whose 'embs' has one row per item; `.reshape(-1)` concatenates)."""
        if isinstance(wav_file, np.ndarray):
            items = [wav_file.reshape(-1)]
        elif isinstance(wav_file, str):
            items = [wav_file]
        elif isinstance(wav_file, (list, tuple)):
            items = list(wav_file)
        else:
            raise _lib.TdxError(f"get_speaker_embedding: unsupported input type {type(wav_file).__name__}")
        wavs = [self._read_wav(it) if isinstance(it, str) else np.asarray(it, dtype=np.float32).reshape(-1) for it in items]
        return self.get_speaker_embeddings(wavs).reshape(-1)

    def embed_device(self, wavs):
        """list of 1-D DEVICE tensors -> [len(wavs),192] device tensor; clips of equal length are batched.
        Nothing crosses PCIe (hot loops A/C of TargetDiarization.infer on streams that are already resident)."""
        out = torch.zeros(len(wavs), 192, dtype=torch.float32, device=self.device)
        by_len = {}
        for i, w in enumerate(wavs):
            by_len.setdefault(int(w.shape[0]), []).append(i)
        for n, idxs in by_len.items():
            F = 1 + (n - 400) // 160
            step = max(1, self.max_batch_frames // max(F, 1))
            for c in range(0, len(idxs), step):
                chunk = idxs[c:c + step]
                x = torch.stack([wavs[i] for i in chunk]).to(self.device, torch.float32)
                y = self.model(x)
                # (no `out[list] = y`: an index list is uploaded with a pageable H2D copy, which blocks the HOST until the stream
                # has drained — the launches queued behind it then start late and nothing overlaps)
                if chunk == list(range(chunk[0], chunk[0] + len(chunk))):
                    out[chunk[0]:chunk[0] + len(chunk)] = y
                else:
                    for j, i in enumerate(chunk):
                        out[i].copy_(y[j])
        return out

    def get_speaker_embeddings(self, wavs):
        """list of 1-D float32 arrays -> [len(wavs),192] array; clips of equal length are batched."""
        if not wavs:
            return np.zeros((0, 192), dtype=np.float32)
        dev = [torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(self.device) for w in wavs]
        return self.embed_device(dev).cpu().numpy()

    # TargetASR.py:144-152
    @staticmethod
    def cosine_similarity(embedding_a: np.ndarray, embedding_b: np.ndarray):
        if np.all(embedding_a == 0.0) or np.all(embedding_b == 0.0):
            return 1.0
        s = np.dot(embedding_a, embedding_b) / (np.linalg.norm(embedding_a) * np.linalg.norm(embedding_b))
        return float(max(0.0, min(s, 1.0)))

    def cosine_scores(self, embs: np.ndarray, ref: np.ndarray) -> np.ndarray:
        """device form: all N embeddings against one reference in a single launch"""
        e = torch.from_numpy(np.ascontiguousarray(embs, dtype=np.float32)).to(self.device)
        r = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float32)).to(self.device)
        return ops.cosine_scores(e, r).cpu().numpy()
