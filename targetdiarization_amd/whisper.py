"""Whisper over the C-ABI (tdx_whisper_*, include/tdx.h N10): the reference's third local recogniser,
`AutoModelForSpeechSeq2Seq.from_pretrained(dir)` + `WhisperProcessor` (ASRProcessor.py:244-251) and
`generate(input_features, task="transcribe", language="chinese", num_beams=1, prompt_ids=...)` + `batch_decode(skip_special_tokens=True)`
(:489-514).  Upstream is Hugging Face transformers' WhisperForConditionalGeneration; tests/whisper_oracle.py restates it and
tests/test_whisper_host.py pins the restatement, the prefix and the language table to the installed upstream.

The device does everything up to the token ids: log-mel features, the encoder, the cross-attention K / V of every decoder layer and
the greedy decoding loop over a KV cache (one host read per 16 steps).  The host builds the prefix, and turns ids into text through
the byte-level BPE alphabet when a piece table is given.  Deviations from the reference: fp32 (it runs .half()), one prefix per call,
greedy decoding only (no beams, temperature fallback, timestamps or long-form), tokenizer files are read when present, never required."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import torch

from . import _lib
from .weights import pack_blob, whisper_config

MAX_BATCH = 32

# openai/whisper tokenizer.py LANGUAGES, in its order: the id of <|code|> is 50259 + the index
LANGUAGES = (
    ("en", "english"), ("zh", "chinese"), ("de", "german"), ("es", "spanish"), ("ru", "russian"), ("ko", "korean"), ("fr", "french"),
    ("ja", "japanese"), ("pt", "portuguese"), ("tr", "turkish"), ("pl", "polish"), ("ca", "catalan"), ("nl", "dutch"), ("ar", "arabic"),
    ("sv", "swedish"), ("it", "italian"), ("id", "indonesian"), ("hi", "hindi"), ("fi", "finnish"), ("vi", "vietnamese"), ("he", "hebrew"),
    ("uk", "ukrainian"), ("el", "greek"), ("ms", "malay"), ("cs", "czech"), ("ro", "romanian"), ("da", "danish"), ("hu", "hungarian"),
    ("ta", "tamil"), ("no", "norwegian"), ("th", "thai"), ("ur", "urdu"), ("hr", "croatian"), ("bg", "bulgarian"), ("lt", "lithuanian"),
    ("la", "latin"), ("mi", "maori"), ("ml", "malayalam"), ("cy", "welsh"), ("sk", "slovak"), ("te", "telugu"), ("fa", "persian"),
    ("lv", "latvian"), ("bn", "bengali"), ("sr", "serbian"), ("az", "azerbaijani"), ("sl", "slovenian"), ("kn", "kannada"), ("et", "estonian"),
    ("mk", "macedonian"), ("br", "breton"), ("eu", "basque"), ("is", "icelandic"), ("hy", "armenian"), ("ne", "nepali"), ("mn", "mongolian"),
    ("bs", "bosnian"), ("kk", "kazakh"), ("sq", "albanian"), ("sw", "swahili"), ("gl", "galician"), ("mr", "marathi"), ("pa", "punjabi"),
    ("si", "sinhala"), ("km", "khmer"), ("sn", "shona"), ("yo", "yoruba"), ("so", "somali"), ("af", "afrikaans"), ("oc", "occitan"),
    ("ka", "georgian"), ("be", "belarusian"), ("tg", "tajik"), ("sd", "sindhi"), ("gu", "gujarati"), ("am", "amharic"), ("yi", "yiddish"),
    ("lo", "lao"), ("uz", "uzbek"), ("fo", "faroese"), ("ht", "haitian creole"), ("ps", "pashto"), ("tk", "turkmen"), ("nn", "nynorsk"),
    ("mt", "maltese"), ("sa", "sanskrit"), ("lb", "luxembourgish"), ("my", "myanmar"), ("bo", "tibetan"), ("tl", "tagalog"), ("mg", "malagasy"),
    ("as", "assamese"), ("tt", "tatar"), ("haw", "hawaiian"), ("ln", "lingala"), ("ha", "hausa"), ("ba", "bashkir"), ("jw", "javanese"),
    ("su", "sundanese"), ("yue", "cantonese"))
LANGUAGE_ALIASES = {"burmese": "my", "valencian": "ca", "flemish": "nl", "haitian": "ht", "letzeburgesch": "lb", "pushto": "ps", "panjabi": "pa",
                    "moldavian": "ro", "moldovan": "ro", "sinhalese": "si", "castilian": "es", "mandarin": "zh"}

# the non-speech ids of the published multilingual generation configs (openai/whisper-*: generation_config.json) [upstream-recall];
# a model directory's own generation_config.json replaces them
_SUPPRESS_COMMON = [1, 2, 7, 8, 9, 10, 14, 25, 26, 27, 28, 29, 31, 58, 59, 60, 61, 62, 63, 90, 91, 92, 93, 359, 503, 522, 542, 873, 893, 902, 918,
                    922, 931, 1350, 1853, 1982, 2460, 2627, 3246, 3253, 3268, 3536, 3846, 3961, 4183, 4667, 6585, 6647, 7273, 9061, 9383, 10428,
                    10929, 11938, 12033, 12331, 12562, 13793, 14157, 14635, 15265, 15618, 16553, 16604, 18362, 18956, 20075, 21675, 22520, 26130,
                    26161, 26435, 28279, 29464, 31650, 32302, 32470, 36865, 42863, 47425, 49870, 50254, 50258]


def language_code(language: str) -> str:
    """a Whisper language name ("chinese"), alias ("mandarin"), code ("zh") or token ("<|zh|>") -> the code"""
    s = str(language).strip().lower()
    if s.startswith("<|") and s.endswith("|>"):
        s = s[2:-2]
    for code, name in LANGUAGES:
        if s == code or s == name:
            return code
    if s in LANGUAGE_ALIASES:
        return LANGUAGE_ALIASES[s]
    raise ValueError(f"unsupported Whisper language: {language!r}")


def default_generation_config(vocab: int) -> dict:
    """the ids of the two multilingual vocabularies: 51865 (99 languages) and 51866 (large-v3: 100, `yue` added)"""
    if vocab not in (51865, 51866):
        raise ValueError(f"no default generation config for a vocabulary of {vocab}: pass generation_config")
    nlang = 99 if vocab == 51865 else 100
    base = 50259 + nlang                      # <|translate|>
    return {"lang_to_id": {f"<|{code}|>": 50259 + i for i, (code, _) in enumerate(LANGUAGES[:nlang])},
            "task_to_id": {"translate": base, "transcribe": base + 1}, "prev_sot_token_id": base + 3, "no_timestamps_token_id": base + 5,
            "decoder_start_token_id": 50258, "eos_token_id": 50257, "suppress_tokens": _SUPPRESS_COMMON + [base, base + 1, base + 2, base + 3, base + 4],
            "begin_suppress_tokens": [220, 50257], "max_length": 448, "is_multilingual": True}


def _gen_dict(gen_cfg) -> dict:
    if gen_cfg is None:
        raise ValueError("a generation config is needed (lang_to_id, task_to_id, no_timestamps_token_id, ...)")
    return gen_cfg if isinstance(gen_cfg, dict) else gen_cfg.to_dict()


def decode_prefix(language, task, prompt_ids, gen_cfg, n_text_ctx: int = 448):
    """The decoder prefix of `generate(language=, task=, prompt_ids=)` without timestamps:
    [<|startofprev|>, prompt...] + [<|startoftranscript|>, <|lang|>, <|task|>, <|notimestamps|>].  The prompt is what get_prompt_ids
    returns (a leading <|startofprev|> is not doubled).  On the short-form path (<= 30 s, the only one here) transformers 5 feeds the
    prompt whole (the cut to n_text_ctx // 2 - 1 ids belongs to its long-form path).  A prefix that leaves no room in n_text_ctx is
    an error, as it is upstream."""
    g = _gen_dict(gen_cfg)
    tok = f"<|{language_code(language)}|>"
    if tok not in g["lang_to_id"]:
        raise ValueError(f"{tok} is not in the generation config's lang_to_id")
    if task not in g["task_to_id"]:
        raise ValueError(f"task {task!r} is not in the generation config's task_to_id")
    init = [int(g["decoder_start_token_id"]), int(g["lang_to_id"][tok]), int(g["task_to_id"][task]), int(g["no_timestamps_token_id"])]
    if prompt_ids is None:
        return init
    p = [int(t) for t in (prompt_ids.tolist() if hasattr(prompt_ids, "tolist") else prompt_ids)]
    prev = int(g["prev_sot_token_id"])
    if p and p[0] == prev:
        p = p[1:]
    if len(p) + 5 >= n_text_ctx:
        raise ValueError(f"a prompt of {len(p)} ids leaves no room in a context of {n_text_ctx}")
    return [prev] + p + init


def new_token_limit(prefix_len: int, max_new_tokens, gen_cfg, n_text_ctx: int = 448) -> int:
    """what generate would apply: max_new_tokens clipped to the room left, or without one the config's max_length, extended
    by the prefix (at most n_text_ctx // 2 - 1 ids of it) and capped at n_text_ctx, as a total length"""
    g = _gen_dict(gen_cfg)
    if max_new_tokens is None and g.get("max_new_tokens") is not None:
        max_new_tokens = g["max_new_tokens"]
    if max_new_tokens is not None:
        return max(0, min(int(max_new_tokens), n_text_ctx - prefix_len))
    total = min(int(g.get("max_length") or 448) + min(n_text_ctx // 2 - 1, prefix_len), n_text_ctx)
    return max(0, total - prefix_len)


def _byte_decoder():
    """inverse of GPT-2's bytes_to_unicode: the printable stand-in of every byte"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(bs, cs)}


_BYTE_DECODER = _byte_decoder()


def decode_text(ids, token_list, eos: int = 50257) -> str:
    """batch_decode(skip_special_tokens=True) for the byte-level BPE alphabet: ids >= eos (the special tokens) are dropped, the
    pieces joined, mapped back to bytes and decoded as UTF-8 with errors="replace".  token_list None: "<id>" placeholders."""
    ids = [int(i) for i in ids if int(i) < eos]
    if token_list is None:
        return "".join(f"<{i}>" for i in ids)
    text = "".join(token_list[i] if i < len(token_list) else "" for i in ids)
    return bytes(_BYTE_DECODER[ch] for ch in text if ch in _BYTE_DECODER).decode("utf-8", errors="replace")


class WhisperASR:
    def __init__(self, state_dict, config, device="cuda:0", token_list=None, tokenizer=None, generation_config=None):
        self.cfg = c = whisper_config(config)
        self.token_list, self.tokenizer = token_list, tokenizer
        self.gen_cfg = _gen_dict(generation_config) if generation_config is not None else default_generation_config(c["vocab"])
        keep = {k: v for k, v in state_dict.items() if k.startswith(("model.", "proj_out."))}
        emb, po = keep.get("model.decoder.embed_tokens.weight"), keep.get("proj_out.weight")
        if po is not None and emb is not None and po.shape == emb.shape and (po is emb or torch.equal(po, emb)):
            del keep["proj_out.weight"]                     # tied: one copy crosses the C-ABI (a different one is reported by create)
        cc = _lib.WhisperConfig(c["n_mels"], c["n_audio_ctx"], c["d_model"], c["enc_heads"], c["enc_layers"], c["enc_ffn"], c["n_text_ctx"],
                                c["dec_heads"], c["dec_layers"], c["dec_ffn"], c["vocab"], int(c["activation"] == "gelu"))
        self._l = _lib.lib()
        self._own = _lib.Handle(device, "WhisperASR", self._l.tdx_whisper_create, self._l.tdx_whisper_destroy, C.byref(cc), blob=pack_blob(keep))
        self.device, self._h, self._guard = self._own.device, self._own.ptr, self._own.guard
        self.n_samples = 320 * c["n_audio_ctx"]             # 30 s in every published model

    def _check_open(self):
        if not self._h:
            raise _lib.TdxError("WhisperASR: the model is closed")

    def _check_batch(self, B):
        if not 1 <= B <= MAX_BATCH:
            raise _lib.TdxError(f"WhisperASR: {B} clips in one call (1..{MAX_BATCH})")

    def workspace_bytes(self, B):
        return int(self._l.tdx_whisper_workspace_bytes(self._h, B))

    def flops(self, B, steps):
        return float(self._l.tdx_whisper_flops(self._h, B, steps))

    def features(self, wavs, lens=None) -> torch.Tensor:
        """list of 1-D 16 kHz clips, or wav [B,N] (+ lens [B]) -> log-mel features [B, n_mels, 2 n_audio_ctx]; a clip is cut or
        zero-padded to 320 n_audio_ctx samples"""
        self._check_open()
        if isinstance(wavs, (list, tuple)):
            clips = [torch.as_tensor(np.asarray(w, dtype=np.float32) if not isinstance(w, torch.Tensor) else w).reshape(-1)[: self.n_samples] for w in wavs]
            lens = [int(cl.shape[0]) for cl in clips]
            N = max(1, max(lens))
            wav = torch.zeros(len(clips), N, dtype=torch.float32, device=self.device)
            for i, cl in enumerate(clips):
                wav[i, : lens[i]] = cl.to(self.device, torch.float32)
        else:
            wav = torch.as_tensor(wavs).to(self.device, torch.float32)
            wav = wav.reshape(1, -1) if wav.dim() == 1 else wav
            wav = wav.contiguous()
        B, N = wav.shape
        self._check_batch(B)
        lens_dev = torch.as_tensor(lens, dtype=torch.int32).to(self.device) if lens is not None else None
        feat = torch.empty(B, self.cfg["n_mels"], 2 * self.cfg["n_audio_ctx"], device=self.device)
        with self._guard.call():
            ws = self._guard.workspace(self.workspace_bytes(B))
            st = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(self._l.tdx_whisper_logmel(self._h, wav.data_ptr(), lens_dev.data_ptr() if lens_dev is not None else None, B, N,
                                                  feat.data_ptr(), ws.data_ptr(), ws.numel(), st))
        return feat

    def encode(self, feats: torch.Tensor, with_state: bool = False):
        """feats [B, n_mels, 2 n_audio_ctx] -> enc [B, n_audio_ctx, d]; with_state: (enc, state), state [dec_layers, 2, B, n_audio_ctx, d]
        the cross-attention K / V that decode() reads"""
        self._check_open()
        c = self.cfg
        feats = feats.to(self.device, torch.float32).contiguous()
        B = feats.shape[0]
        self._check_batch(B)
        if tuple(feats.shape[1:]) != (c["n_mels"], 2 * c["n_audio_ctx"]):
            raise _lib.TdxError(f"WhisperASR.encode: features of shape {tuple(feats.shape)}, expected [B, {c['n_mels']}, {2 * c['n_audio_ctx']}]")
        enc = torch.empty(B, c["n_audio_ctx"], c["d_model"], device=self.device)
        state = torch.empty(c["dec_layers"], 2, B, c["n_audio_ctx"], c["d_model"], device=self.device) if with_state else None
        with self._guard.call():
            ws = self._guard.workspace(self.workspace_bytes(B))
            st = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(self._l.tdx_whisper_encode(self._h, feats.data_ptr(), B, enc.data_ptr(), state.data_ptr() if with_state else None,
                                                  ws.data_ptr(), ws.numel(), st))
        return (enc, state) if with_state else enc

    def decode(self, state: torch.Tensor, prefix, max_new: int, suppress=(), begin_suppress=(), eos=None):
        """greedy decoding from encode()'s state under one prefix -> device tensors step_ids int32 [B, n_text_ctx], step_scores
        [B, n_text_ctx] (step p at column p; columns no step reached hold -1 / 0) and counts int32 [B]"""
        self._check_open()
        c = self.cfg
        B = int(state.shape[2])
        self._check_batch(B)
        if tuple(state.shape) != (c["dec_layers"], 2, B, c["n_audio_ctx"], c["d_model"]) or not state.is_contiguous():
            raise _lib.TdxError("WhisperASR.decode: state is not encode(..., with_state=True)'s")
        eos = int(self.gen_cfg["eos_token_id"] if eos is None else eos)
        ids = torch.full((B, c["n_text_ctx"]), -1, dtype=torch.int32, device=self.device)
        scores = torch.zeros(B, c["n_text_ctx"], device=self.device)
        counts = torch.zeros(B, dtype=torch.int32, device=self.device)
        arr = lambda v: (C.c_int * max(1, len(v)))(*[int(t) for t in v])
        prefix, suppress, begin_suppress = list(prefix), list(suppress), list(begin_suppress)
        with self._guard.call():
            ws = self._guard.workspace(self.workspace_bytes(B))
            st = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(self._l.tdx_whisper_decode(self._h, state.data_ptr(), B, arr(prefix), len(prefix), arr(suppress), len(suppress),
                                                  arr(begin_suppress), len(begin_suppress), eos, int(max_new), ids.data_ptr(), scores.data_ptr(),
                                                  counts.data_ptr(), ws.data_ptr(), ws.numel(), st))
        return ids, scores, counts

    def text_of(self, ids) -> str:
        return decode_text(ids, self.token_list, int(self.gen_cfg["eos_token_id"]))

    def generate(self, wavs, language: str = "chinese", task: str = "transcribe", prompt_ids=None, max_new_tokens=None, keys=None):
        """list of 1-D 16 kHz clips (or one clip) -> per clip {"key", "text", "token_ids", "scores"}: the generated ids (a final
        end-of-text included) and their log-probabilities.  Clips go through in batches of 32, cut to 30 s."""
        self._check_open()
        if isinstance(wavs, (np.ndarray, torch.Tensor)):
            wavs = [wavs]
        g, T = self.gen_cfg, self.cfg["n_text_ctx"]
        prefix = decode_prefix(language, task, prompt_ids, g, T)
        max_new = new_token_limit(len(prefix), max_new_tokens, g, T)
        out = []
        for c0 in range(0, len(wavs), MAX_BATCH):
            chunk = wavs[c0:c0 + MAX_BATCH]
            _, state = self.encode(self.features(chunk), with_state=True)
            ids, scores, counts = self.decode(state, prefix, max_new, g.get("suppress_tokens") or (), g.get("begin_suppress_tokens") or ())
            ids, scores, counts = ids.cpu().numpy(), scores.cpu().numpy(), counts.cpu().tolist()
            p0 = len(prefix) - 1                            # the step that wrote the first generated token
            for b, n in enumerate(counts):
                tok = [int(t) for t in ids[b, p0:p0 + n]]
                out.append({"key": keys[c0 + b] if keys is not None else f"clip_{c0 + b}", "text": self.text_of(tok), "token_ids": tok,
                            "scores": [float(s) for s in scores[b, p0:p0 + n]]})
        return out

    def close(self):
        self._own.close()


def load_token_list(vocab_json):
    """vocab.json ({piece: id}) -> the pieces by id; None when the file is absent"""
    if not isinstance(vocab_json, str) or not os.path.isfile(vocab_json):
        return None
    with open(vocab_json, encoding="utf-8") as f:
        v = json.load(f)
    tl = [""] * (1 + max(v.values()))
    for piece, i in v.items():
        tl[i] = piece
    return tl


def build_whisper(state_dict=None, config=None, model_dir=None, token_list=None, tokenizer=None, generation_config=None, cuda_device: int = 0):
    """The device recogniser from weights + config, or from a transformers model directory: config.json plus model.safetensors or
    pytorch_model.bin, and when present generation_config.json, vocab.json (the piece table) and the tokenizer files (prompts).
    None when there is neither source.  safetensors / transformers are imported here only, and only when a directory needs them."""
    if state_dict is None:
        if not isinstance(model_dir, str) or not os.path.isfile(os.path.join(model_dir, "config.json")):
            return None
        with open(os.path.join(model_dir, "config.json"), encoding="utf-8") as f:
            config = json.load(f)
        st, pt = os.path.join(model_dir, "model.safetensors"), os.path.join(model_dir, "pytorch_model.bin")
        if os.path.isfile(st):
            from safetensors.torch import load_file
            state_dict = load_file(st)
        elif os.path.isfile(pt):
            state_dict = torch.load(pt, map_location="cpu", weights_only=True)
        else:
            return None
        state_dict = {k: v.float() for k, v in state_dict.items()}
        gj = os.path.join(model_dir, "generation_config.json")
        if generation_config is None and os.path.isfile(gj):
            with open(gj, encoding="utf-8") as f:
                generation_config = json.load(f)
        if token_list is None:
            token_list = load_token_list(os.path.join(model_dir, "vocab.json"))
        if tokenizer is None and os.path.isfile(os.path.join(model_dir, "vocab.json")):
            try:
                from transformers import WhisperTokenizer
                tokenizer = WhisperTokenizer.from_pretrained(model_dir, local_files_only=True)
            except Exception as e:
                print(f"Whisper tokenizer not loaded (prompts will be ignored): {e}")
    return WhisperASR(state_dict, config, device=f"cuda:{cuda_device}", token_list=token_list, tokenizer=tokenizer, generation_config=generation_config)
