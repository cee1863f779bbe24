"""Paraformer-large over the C-ABI: SANM encoder (tdx_pfenc_*) plus the ASR feature front-end, and the CIF predictor +
non-autoregressive SANM decoder (tdx_pfdec_*, SURVEY "next" row N2).  Together they replace the neural forward inside
funasr's `AutoModel.generate` (ASRProcessor.py:424); funasr's VAD segmentation, tokenizer files and punctuation stay outside."""
from __future__ import annotations


import torch

from . import _lib
from .frontend import Fbank, lfr_cmvn
from .weights import pack_blob


class ParaformerEncoder:
    def __init__(self, state_dict, device="cuda:0", num_blocks: int | None = None, cmvn_shift=None, cmvn_scale=None, graph_rows: int = 2048):
        """graph_rows: forwards with B*T <= graph_rows LFR frames are replayed as HIP graphs (_lib.GraphRunner); 0 disables"""
        self.graph_rows = graph_rows
        if num_blocks is None:
            num_blocks = 2 + max(int(k.split("encoders.")[1].split(".")[0]) for k in state_dict if ".encoders." in k)
        self.num_blocks = num_blocks
        self._l = _lib.lib()
        self._own = _lib.Handle(device, "ParaformerEncoder", self._l.tdx_pfenc_create, self._l.tdx_pfenc_destroy, num_blocks, blob=pack_blob(state_dict))
        self.device, self._h, self._guard = self._own.device, self._own.ptr, self._own.guard
        self._graphs = _lib.GraphRunner(self.device)
        self.fbank = Fbank("asr", self.device)
        # am.mvn vectors (funasr WavFrontend.apply_cmvn): (x + shift) * scale; identity if absent
        self.cmvn_shift = (cmvn_shift if cmvn_shift is not None else torch.zeros(560)).to(self.device).float()
        self.cmvn_scale = (cmvn_scale if cmvn_scale is not None else torch.ones(560)).to(self.device).float()

    def flops(self, B, T):
        return float(self._l.tdx_pfenc_flops(self._h, B, T))

    def features(self, wav: torch.Tensor) -> torch.Tensor:
        """wav [B,N] in [-1,1] -> LFR+CMVN features [B,ceil(F/6),560]"""
        return lfr_cmvn(self.fbank(wav), self.cmvn_shift, self.cmvn_scale)

    def encode(self, feats: torch.Tensor) -> torch.Tensor:
        feats = feats.to(self.device, torch.float32).contiguous()
        B, T, _ = feats.shape
        nb = int(self._l.tdx_pfenc_workspace_bytes(self._h, B, T))
        with self._guard.call():
            if self.graph_rows and B * T <= self.graph_rows:
                def launch(si, so, ws, st):
                    _lib.check(self._l.tdx_pfenc_forward(self._h, si.data_ptr(), None, B, T, so.data_ptr(), ws.data_ptr(), ws.numel(), st))
                out = self._graphs((B, T), feats, (B, T, 512), nb, launch)    # None until the shape is seen a second time
                if out is not None:
                    return out
            ws = self._guard.workspace(nb)
            out = torch.empty(B, T, 512, device=self.device)
            st = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(self._l.tdx_pfenc_forward(self._h, feats.data_ptr(), None, B, T, out.data_ptr(), ws.data_ptr(), ws.numel(), st))
            return out

    def __call__(self, wav: torch.Tensor) -> torch.Tensor:
        return self.encode(self.features(wav))

    def close(self):
        self._own.close()
        self.fbank.close()


class ParaformerDecoder:
    """CIF predictor + NAR SANM decoder (funasr CifPredictorV2 + ParaformerSANMDecoder, third-party: parity unpinned).
    `decode(enc)` returns, per utterance, {"token_ids", "scores", "timestamp": [[start_ms, end_ms], ...]}.
    Timestamps, WITH the upsampling head's weights in the state dict (`predictor.upsample_cnn.*`, `predictor.blstm.*`,
    `predictor.cif_output2.*`: funasr's CifPredictorV3, what the reference's "-vad-punc" bundle carries): funasr's — the device
    computes the upsampled alphas and peaks on the 20 ms grid (`upsampled`), pf_timestamps.ts_prediction_lfr6 turns them into
    one [start_ms, end_ms] per token; a trailing `</s>` (`eos_id`) gets none and is dropped from the result.
    WITHOUT them (the published Paraformer has no timestamps of its own): token k spans from the encoder frame after the
    previous integrate-and-fire peak to its own peak, in 60 ms LFR frames — an own definition, documented in INTEGRATION.md.
    cif_residual: relu(conv(x) + bias + x) (CifPredictorV2) or without the `+ x` (V3); None = True without the head, False with it."""

    FRAME_MS = 60.0

    def __init__(self, state_dict, device="cuda:0", num_blocks: int | None = None, vocab: int | None = None, cif_residual: bool | None = None,
                 smooth_factor2: float = 0.25, noise_threshold2: float = 0.01, eos_id: int = 2):
        if num_blocks is None:
            num_blocks = 1 + max(int(k.split("decoders.")[1].split(".")[0]) for k in state_dict if "decoder.decoders." in k)
        if vocab is None:
            vocab = int(state_dict["decoder.output_layer.bias"].shape[0])
        self.num_blocks, self.vocab = num_blocks, vocab
        self._l = _lib.lib()
        keep = {k: v for k, v in state_dict.items() if k.startswith(("predictor.cif_", "predictor.upsample_cnn.", "predictor.blstm.", "decoder.decoders",
                                                                     "decoder.after_norm", "decoder.output_layer"))}
        self._own = _lib.Handle(device, "ParaformerDecoder", self._l.tdx_pfdec_create, self._l.tdx_pfdec_destroy, num_blocks, vocab, blob=pack_blob(keep))
        self.device, self._h, self._guard = self._own.device, self._own.ptr, self._own.guard
        self.has_timestamps = bool(self._l.tdx_pfdec_has_timestamps(self._h))
        self.cif_residual = (not self.has_timestamps) if cif_residual is None else bool(cif_residual)
        _lib.check(self._l.tdx_pfdec_set_cif_residual(self._h, int(self.cif_residual)))
        self.eos_id = eos_id
        if self.has_timestamps:
            _lib.check(self._l.tdx_pfdec_set_alpha2(self._h, smooth_factor2, noise_threshold2))

    def predict(self, enc: torch.Tensor):
        """enc [B,T,512] -> (alphas [B,T+1], embeds [B,T+1,512], counts int32 [B], peaks int32 [B,T+1]) on the device"""
        enc = enc.to(self.device, torch.float32).contiguous()
        B, T, _ = enc.shape
        alphas = torch.empty(B, T + 1, device=self.device)
        emb = torch.empty(B, T + 1, 512, device=self.device)
        counts = torch.empty(B, dtype=torch.int32, device=self.device)
        peaks = torch.empty(B, T + 1, dtype=torch.int32, device=self.device)
        nb = int(self._l.tdx_pfdec_predict_workspace_bytes(self._h, B, T))
        with self._guard.call():
            ws = self._guard.workspace(nb)
            st = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(self._l.tdx_pfdec_predict(self._h, enc.data_ptr(), B, T, alphas.data_ptr(), emb.data_ptr(), counts.data_ptr(), peaks.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), st))
        return alphas, emb, counts, peaks

    def upsampled(self, enc: torch.Tensor, counts: torch.Tensor, tap: bool = False, raw: bool = False):
        """the timestamp head: enc [B,T,512], counts int32 [B] (from `predict`) -> (us_alphas [B,3T], us_peaks [B,3T]) on the device;
        tap=True appends the BLSTM output [B,3T,1024], raw=True the alphas before their re-normalisation [B,3T]"""
        enc = enc.to(self.device, torch.float32).contiguous()
        counts = counts.to(self.device, torch.int32).contiguous()
        B, T, _ = enc.shape
        U = 3 * T
        alphas = torch.empty(B, U, device=self.device)
        peaks = torch.empty(B, U, device=self.device)
        y = torch.empty(B, U, 1024, device=self.device) if tap else None
        nb = int(self._l.tdx_pfdec_timestamps_workspace_bytes(self._h, B, T))
        with self._guard.call():
            ws = self._guard.workspace(nb)
            st = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(self._l.tdx_pfdec_timestamps(self._h, enc.data_ptr(), B, T, counts.data_ptr(), alphas.data_ptr(), peaks.data_ptr(),
                                                    y.data_ptr() if tap else None, ws.data_ptr(), ws.numel(), st))
            out = (alphas, peaks) + ((y,) if tap else ())
            if raw:
                out += (ws[: B * U * 4].view(torch.float32).reshape(B, U).clone(),)
        return out

    def decode_embeds(self, emb: torch.Tensor, counts: torch.Tensor, enc: torch.Tensor, L: int):
        """the decoder alone: emb [B,R,512] (first L rows used), counts int32 [B], enc [B,T,512] -> (ids int32 [B,L], scores [B,L])"""
        enc = enc.to(self.device, torch.float32).contiguous()
        emb = emb.to(self.device, torch.float32).contiguous()
        B, T, _ = enc.shape
        ids = torch.empty(B, L, dtype=torch.int32, device=self.device)
        score = torch.empty(B, L, device=self.device)
        nb = int(self._l.tdx_pfdec_decode_workspace_bytes(self._h, B, L, T))
        with self._guard.call():
            ws = self._guard.workspace(nb)
            st = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(self._l.tdx_pfdec_decode(self._h, emb.data_ptr(), emb.shape[1], counts.data_ptr(), enc.data_ptr(), B, L, T, ids.data_ptr(),
                                                score.data_ptr(), ws.data_ptr(), ws.numel(), st))
        return ids, score

    def decode(self, enc: torch.Tensor):
        """enc [B,T,512] (equal-length segments of a batch) -> list of per-utterance results"""
        alphas, emb, counts, peaks = self.predict(enc)
        cnt = counts.cpu().tolist()                        # the one host read: the decoder's row count is data dependent
        L = max(cnt) if cnt else 0
        B = enc.shape[0]
        if L < 1:
            return [{"token_ids": [], "scores": [], "timestamp": []} for _ in range(B)]
        ids, score = self.decode_embeds(emb, counts, enc, L)
        if self.has_timestamps:
            return self._decode_upsampled(enc, counts, cnt, ids, score)
        ids_h, score_h, peaks_h = ids.cpu().numpy(), score.cpu().numpy(), peaks[:, :L].cpu().numpy()
        out = []
        for b in range(B):
            n = cnt[b]
            ts, prev = [], -1
            for k in range(n):
                pk = int(peaks_h[b, k])
                if pk < 0:                                 # fewer fires than floor(sum alphas): the reference pads those frames with zeros
                    pk = prev
                ts.append([int(round((prev + 1) * self.FRAME_MS)), int(round((pk + 1) * self.FRAME_MS))])
                prev = pk
            out.append({"token_ids": [int(t) for t in ids_h[b, :n]], "scores": [float(s) for s in score_h[b, :n]], "timestamp": ts})
        return out

    def _decode_upsampled(self, enc, counts, cnt, ids, score):
        """timestamps from the upsampling head: one device call for the batch, then funasr's rules per clip on the host.  The tokens
        kept are those with a timestamp: the trailing </s> is dropped, as funasr drops it from the character list."""
        from .pf_timestamps import ts_prediction_lfr6
        us_alphas, us_peaks = self.upsampled(enc, counts)
        ids_h, score_h, ua, up = ids.cpu().numpy(), score.cpu().numpy(), us_alphas.cpu().numpy(), us_peaks.cpu().numpy()
        out = []
        for b in range(enc.shape[0]):
            n = cnt[b]
            if n > 0 and int(ids_h[b, n - 1]) == self.eos_id:
                n -= 1
            _, ts = ts_prediction_lfr6(ua[b], up[b], [str(int(t)) for t in ids_h[b, :n]])
            n = min(n, len(ts))
            out.append({"token_ids": [int(t) for t in ids_h[b, :n]], "scores": [float(s) for s in score_h[b, :n]], "timestamp": ts[:n]})
        return out

    def close(self):
        self._own.close()
