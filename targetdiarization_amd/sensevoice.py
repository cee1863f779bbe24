"""SenseVoiceSmall over the C-ABI (tdx_sv_*, include/tdx.h N9): the reference's second local recogniser,
`self.asr['sensevoice'].generate(input=wav, cache={}, language=language, use_itn=True, ...)` (ASRProcessor.py:398-402), and the
only place it gets a per-clip language and emotion tag from.  funasr is third-party and absent: the architecture, the prompt
order and the id tables below are restated from upstream, parity with the published checkpoint is unpinned.

The device does everything up to the token ids: Fbank("asr") -> LFR/CMVN -> four prompt rows + features -> 50 + 20 SANM layers ->
CTC head (argmax id and log-prob per frame, never the logits of a whole call) -> greedy collapse.  The host reads the compacted
ids back once per launch sequence and joins the pieces of `token_list` (sentencepiece is absent: the table supplies the pieces)."""
from __future__ import annotations

import ctypes as C
import json
import os
import re

import numpy as np
import torch

from . import _lib
from .frontend import Fbank, lfr_cmvn
from .weights import pack_blob

LID = {"auto": 0, "zh": 3, "en": 4, "yue": 7, "ja": 11, "ko": 12, "nospeech": 13}
TEXTNORM = {"withitn": 14, "woitn": 15}
PROMPT_ROWS = 4

SEARCH_PATTERN = r"<\|(.+?)\|><\|(.+?)\|><\|(.+?)\|><\|(.+?)\|>(.+)"       # ASRProcessor.py:395-397
DELETE_PATTERN = r"<\|(.+?)\|><\|(.+?)\|><\|(.+?)\|><\|(.+?)\|>"
PUNC_PATTERN = r"[^\w\s]"


def parse_tagged_text(text: str, no_punc: bool = False):
    """ASRProcessor.py:406-414: "<|lang|><|emotion|><|event|><|itn|>text" -> (language, emotion, text), lower-cased tags, `zh`
    texts without spaces, no_punc strips punctuation and lower-cases.  A text that does not match the tag pattern (the reference
    raises on None.groups()) gives ("", "", the whole text)."""
    m = re.match(SEARCH_PATTERN, text)
    if m is None:
        lang, emo, body = "", "", text
    else:
        lang, emo, _event, _itn, body = m.groups()
        body = re.sub(DELETE_PATTERN, "", body)
        if lang.lower() == "zh":
            body = body.replace(" ", "")
    if no_punc:
        body = re.sub(PUNC_PATTERN, "", body).lower()
    return lang.lower(), emo.lower(), body


def join_text_only(result_list) -> str:
    """ASRProcessor.py:515-524: the texts joined, a space after one that ends in , . ? !"""
    texts = ""
    for clip in result_list:
        if not clip["text"]:
            continue
        texts = texts + clip["text"] + (" " if clip["text"][-1] in [",", ".", "?", "!"] else "")
    return texts


def load_token_list(path):
    """the piece table: a JSON list, or one piece per line; None when `path` is not a file"""
    if not isinstance(path, str) or not os.path.isfile(path):
        return None
    text = open(path, encoding="utf-8").read()
    try:
        tl = json.loads(text)
        if isinstance(tl, list):
            return [str(t) for t in tl]
    except ValueError:
        pass
    return text.split("\n")[:-1] if text.endswith("\n") else text.split("\n")


class SenseVoiceSmall:
    def __init__(self, state_dict, device="cuda:0", token_list=None, cmvn_shift=None, cmvn_scale=None, num_blocks: int | None = None,
                 tp_blocks: int | None = None, rows_per_launch: int = 32768):
        def count(prefix):
            idx = [int(k[len(prefix):].split(".")[0]) for k in state_dict if k.startswith(prefix)]
            return 1 + max(idx) if idx else 0
        if num_blocks is None:
            num_blocks = 1 + count("encoder.encoders.")
        if tp_blocks is None:
            tp_blocks = count("encoder.tp_encoders.")
        if "ctc.ctc_lo.bias" not in state_dict:
            raise _lib.TdxError("SenseVoiceSmall: the state dict has no ctc.ctc_lo.bias (the vocabulary size is read from it)")
        self.num_blocks, self.tp_blocks, self.vocab = num_blocks, tp_blocks, int(state_dict["ctc.ctc_lo.bias"].shape[0])
        self.token_list = token_list
        self.rows_per_launch = rows_per_launch
        self._l = _lib.lib()
        keep = {k: v for k, v in state_dict.items() if k.startswith(("embed.", "encoder.", "ctc.ctc_lo."))}
        self._own = _lib.Handle(device, "SenseVoiceSmall", self._l.tdx_sv_create, self._l.tdx_sv_destroy, num_blocks, tp_blocks, self.vocab, blob=pack_blob(keep))
        self.device, self._h, self._guard = self._own.device, self._own.ptr, self._own.guard
        self.fbank = Fbank("asr", self.device)
        self.cmvn_shift = (torch.as_tensor(cmvn_shift) if cmvn_shift is not None else torch.zeros(560)).to(self.device).float()
        self.cmvn_scale = (torch.as_tensor(cmvn_scale) if cmvn_scale is not None else torch.ones(560)).to(self.device).float()

    @staticmethod
    def prompt_ids(language: str = "auto", use_itn: bool = True):
        return [LID.get(str(language).lower(), 0), 1, 2, TEXTNORM["withitn" if use_itn else "woitn"]]

    def flops(self, B, T):
        return float(self._l.tdx_sv_flops(self._h, B, T))

    def workspace_bytes(self, B, T):
        return int(self._l.tdx_sv_workspace_bytes(self._h, B, T))

    def _check_open(self):
        if not self._h:
            raise _lib.TdxError("SenseVoiceSmall: the model is closed")

    def features(self, wav: torch.Tensor) -> torch.Tensor:
        """wav [B,N] in [-1,1] -> LFR+CMVN features [B,ceil(F/6),560]"""
        self._check_open()
        return lfr_cmvn(self.fbank(wav), self.cmvn_shift, self.cmvn_scale)

    def forward(self, feats: torch.Tensor, language: str = "auto", use_itn: bool = True, with_enc: bool = False):
        """feats [B,T,560] -> device tensors over the S = T + 4 rows of every utterance: frame_ids int32 [B,S], frame_scores [B,S],
        token_ids / token_frames int32 [B,S] (compacted), counts int32 [B]; with_enc: enc [B,S,512] (the tp_norm output)"""
        self._check_open()
        feats = feats.to(self.device, torch.float32).contiguous()
        B, T, _ = feats.shape
        S = T + PROMPT_ROWS
        nb = self.workspace_bytes(B, T)
        if nb == 0:
            raise _lib.TdxError(f"SenseVoiceSmall: {B} x {S} rows in one forward (limit 2^22): split the batch")
        i32 = dict(dtype=torch.int32, device=self.device)
        out = {"frame_ids": torch.empty(B, S, **i32), "frame_scores": torch.empty(B, S, device=self.device), "token_ids": torch.empty(B, S, **i32),
               "token_frames": torch.empty(B, S, **i32), "counts": torch.empty(B, **i32)}
        if with_enc:
            out["enc"] = torch.empty(B, S, 512, device=self.device)
        prompt = (C.c_int * 4)(*self.prompt_ids(language, use_itn))
        with self._guard.call():
            ws = self._guard.workspace(nb)
            st = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(self._l.tdx_sv_forward(self._h, feats.data_ptr(), B, T, prompt, out["enc"].data_ptr() if with_enc else None,
                                              out["frame_ids"].data_ptr(), out["frame_scores"].data_ptr(), out["token_ids"].data_ptr(),
                                              out["token_frames"].data_ptr(), out["counts"].data_ptr(), ws.data_ptr(), ws.numel(), st))
        return out

    def text_of(self, ids) -> str:
        tl = self.token_list
        return "".join(tl[i] if tl is not None and i < len(tl) else f"<{i}>" for i in ids).replace("▁", " ").strip()

    def decode_batch(self, wav: torch.Tensor, language: str = "auto", use_itn: bool = True):
        """wav [B,N] (equal-length clips, device or host) -> per clip {"text", "token_ids", "frames", "scores"}; one host read"""
        r = self.forward(self.features(wav.to(self.device, torch.float32)), language, use_itn)
        sc_at = torch.gather(r["frame_scores"], 1, r["token_frames"].clamp(min=0).long())
        ids, frm, sc, cnt = r["token_ids"].cpu().numpy(), r["token_frames"].cpu().numpy(), sc_at.cpu().numpy(), r["counts"].cpu().tolist()
        out = []
        for b, n in enumerate(cnt):
            tok = [int(t) for t in ids[b, :n]]
            out.append({"text": self.text_of(tok), "token_ids": tok, "frames": [int(f) for f in frm[b, :n]], "scores": [float(s) for s in sc[b, :n]]})
        return out

    def generate(self, wavs, language: str = "auto", use_itn: bool = True, keys=None):
        """list of 1-D 16 kHz clips (or one clip) -> per clip {"key", "text", "token_ids", "frames", "scores"}; clips of equal length
        share a launch sequence (<= rows_per_launch LFR frames each).  A clip below one fbank frame (400 samples) has an empty result."""
        if isinstance(wavs, (np.ndarray, torch.Tensor)):
            wavs = [wavs]
        clips = [w.reshape(-1) if isinstance(w, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(-1))) for w in wavs]
        res = [{"text": "", "token_ids": [], "frames": [], "scores": []} for _ in clips]
        by_len = {}
        for i, c in enumerate(clips):
            if c.shape[0] >= 400:
                by_len.setdefault(int(c.shape[0]), []).append(i)
        for n, idxs in by_len.items():
            rows = ((1 + (n - 400) // 160) + 5) // 6 + PROMPT_ROWS
            step = max(1, self.rows_per_launch // rows)
            for c in range(0, len(idxs), step):
                chunk = idxs[c:c + step]
                for i, r in zip(chunk, self.decode_batch(torch.stack([clips[i].to(self.device, torch.float32) for i in chunk]), language, use_itn)):
                    res[i] = r
        for i, r in enumerate(res):
            r["key"] = keys[i] if keys is not None else f"clip_{i}"
        return res

    def close(self):
        self._own.close()
        self.fbank.close()


def build_sensevoice(state_dict=None, token_list=None, cmvn=None, model_dir=None, token_file=None, cuda_device: int = 0):
    """The device recogniser from weights, or from a funasr model directory (model.pt + am.mvn); None when there is neither source.
    token_file: the piece table (JSON list or one piece per line) when `token_list` is not given."""
    if state_dict is None:
        from .vad import load_model_dir
        found = load_model_dir(model_dir)
        if found is None:
            return None
        state_dict, cmvn = found
    if token_list is None:
        token_list = load_token_list(token_file)
    shift, scale = cmvn if cmvn is not None else (None, None)
    return SenseVoiceSmall(state_dict, device=f"cuda:{cuda_device}", token_list=token_list, cmvn_shift=shift, cmvn_scale=scale)
