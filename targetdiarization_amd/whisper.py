"""Whisper over the C-ABI (tdx_whisper_*, include/tdx.h N10): the reference's third local recogniser,
`AutoModelForSpeechSeq2Seq.from_pretrained(dir)` + `WhisperProcessor` (ASRProcessor.py:244-251) and
`generate(input_features, task="transcribe", language="chinese", num_beams=1, prompt_ids=...)` + `batch_decode(skip_special_tokens=True)`
(:489-514).  Upstream is Hugging Face transformers' WhisperForConditionalGeneration; tests/whisper_oracle.py restates it and
tests/test_whisper_host.py pins the restatement, the prefix and the language table to the installed upstream.

The device does everything up to the token ids: log-mel features, the encoder, the cross-attention K / V of every decoder layer and
the greedy decoding loop over a KV cache (one host read per 16 steps).  The host builds the prefix, and turns ids into text through
the byte-level BPE alphabet when a piece table is given.  Deviations from the reference: fp32 (it runs .half()), one prefix per call,
no beam search, tokenizer files are read when present, never required.  generate() is the one-window path; transcribe() is the
long-form one: features of the whole clip, 30 s windows decoded with timestamp tokens under per-row prefixes
(decode_ts), segments cut at the timestamp pairs, the next window from the last timestamp.  Decoding is greedy unless temperatures
are given: decode_ts(temperature=) draws from softmax(logits / T) inside the vocabulary head, and transcribe(temperature=(...))
restates whisper.transcribe's temperature fallback (decode_with_fallback) over it.

Word timestamps (the reference's whisper_v2 / whisper_v3 engines, ASRProcessor.py:232-243, 443-488): decode_xattn() also
captures the cross-attention rows of the alignment heads, token_align() turns them into one encoder frame per token on the device
(transformers' _extract_token_timestamps: normalise over the tokens, median filter, mean over the heads, dynamic time warping), and the
host groups tokens into words as transformers' _combine_tokens_into_words does.  detect_language() is one decode step over the
language ids; load_openai_checkpoint() reads OpenAI's {"dims", "model_state_dict"} files."""
from __future__ import annotations

import ctypes as C
import json
import os
import zlib

import numpy as np
import torch

from . import _lib
from .weights import pack_blob, whisper_config

MAX_BATCH = 32
TIME_PRECISION = 0.02                                  # seconds per encoder position
MEDIAN_WIDTH = 7                                       # WhisperConfig.median_filter_width, openai/whisper timing.py
MAX_ALIGN_HEADS = 64
MAX_TEMPERATURES = 16                                  # attempts per window: a row's noise stream is 16 x the clip's index + the attempt
FALLBACK_TEMPERATURES = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)  # whisper.transcribe's defaults
FALLBACK_COMPRESSION_RATIO = 2.4
PROMPT_RESET_TEMPERATURE = 0.5                         # a window decoded above it does not condition the next one
XATTN_BUDGET = 1 << 30                                 # bytes of captured attention per decode call on the alignment path
UNSPACED_LANGUAGES = ("zh", "ja", "th", "lo", "my", "yue")
PREPEND_PUNCTUATIONS = "\"'“¡¿([{-"
APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"

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


def default_alignment_heads(cfg) -> list:
    """openai/whisper model.py: every head of the upper half of the decoder layers"""
    c = whisper_config(cfg)
    return [[l, h] for l in range(c["dec_layers"] // 2, c["dec_layers"]) for h in range(c["dec_heads"])]


def _pieces_text(ids, token_list) -> str:
    """tokenizer.decode of ordinary ids: the pieces joined, back to bytes, UTF-8 with errors="replace"; "<id>" without a table"""
    if token_list is None:
        return "".join(f"<{int(i)}>" for i in ids)
    text = "".join(token_list[int(i)] if int(i) < len(token_list) else "" for i in ids)
    return bytes(_BYTE_DECODER[ch] for ch in text if ch in _BYTE_DECODER).decode("utf-8", errors="replace")


def split_tokens_on_unicode(ids, token_list):
    """transformers' _split_tokens_on_unicode: cut wherever the ids so far decode to whole code points -> (words, ids per word,
    indices per word)"""
    full = _pieces_text(ids, token_list)
    words, word_ids, word_idx, cur, cur_idx, offset = [], [], [], [], [], 0
    for k, t in enumerate(ids):
        cur.append(int(t))
        cur_idx.append(k)
        dec = _pieces_text(cur, token_list)
        at = dec.find("\ufffd")
        if at < 0 or offset + at >= len(full) or full[offset + at] == "\ufffd":
            words.append(dec); word_ids.append(cur); word_idx.append(cur_idx)
            cur, cur_idx = [], []
            offset += len(dec)
    return words, word_ids, word_idx


def split_tokens_on_spaces(ids, token_list, eos: int = 50257):
    """transformers' _split_tokens_on_spaces: a new word at a special id, a leading space, a punctuation mark or the start"""
    words, word_ids, word_idx = [], [], []
    for sub, sid, sidx in zip(*split_tokens_on_unicode(ids, token_list)):
        if sid[0] >= eos or sub.startswith(" ") or sub.strip() in "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~" or not words:
            words.append(sub); word_ids.append(sid); word_idx.append(sidx)
        else:
            words[-1] = words[-1] + sub
            word_ids[-1].extend(sid)
            word_idx[-1].extend(sidx)
    return words, word_ids, word_idx


def merge_punctuations(words, word_ids, word_idx, prepended=PREPEND_PUNCTUATIONS, appended=APPEND_PUNCTUATIONS):
    """transformers' _merge_punctuations, in place: opening marks join the word after them, closing marks the word before"""
    i, j = len(words) - 2, len(words) - 1
    while i >= 0:
        if words[i].startswith(" ") and words[i].strip() in prepended:
            words[j] = words[i] + words[j]; word_ids[j] = word_ids[i] + word_ids[j]; word_idx[j] = word_idx[i] + word_idx[j]
            words[i], word_ids[i], word_idx[i] = "", [], []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(words):
        if not words[i].endswith(" ") and words[j] in appended:
            words[i] += words[j]; word_ids[i] += word_ids[j]; word_idx[i] += word_idx[j]
            words[j], word_ids[j], word_idx[j] = "", [], []
        else:
            i = j
        j += 1
    words[:] = [w for w in words if w]
    word_ids[:] = [t for t in word_ids if t]
    word_idx[:] = [t for t in word_idx if t]


def combine_tokens_into_words(ids, token_list, language: str = "en", eos: int = 50257):
    """transformers' _combine_tokens_into_words over token_list's byte-level pieces: the unicode split for the languages written
    without spaces, the split on spaces otherwise, then the punctuation merges -> (words, ids per word, indices per word).
    Without a piece table every id is its own word "<id>"."""
    ids = [int(t) for t in ids]
    if token_list is None:
        return [f"<{t}>" for t in ids], [[t] for t in ids], [[k] for k in range(len(ids))]
    if language_code(language) in UNSPACED_LANGUAGES:
        words, word_ids, word_idx = split_tokens_on_unicode(ids, token_list)
    else:
        words, word_ids, word_idx = split_tokens_on_spaces(ids, token_list, eos)
    merge_punctuations(words, word_ids, word_idx)
    return words, word_ids, word_idx


def word_timestamps(ids, times, token_list, language: str = "en", eos: int = 50257):
    """generated ids + one time per id -> [(word, [start_s, end_s]), ...] over the ordinary ids (< eos): a word starts at its first
    token's time and ends where the next word starts, the last one at the final entry of `times`"""
    keep = [k for k, t in enumerate(ids) if int(t) < eos]
    if not keep:
        return []
    words, _, word_idx = combine_tokens_into_words([ids[k] for k in keep], token_list, language, eos)
    starts = [float(times[keep[idx[0]]]) for idx in word_idx]
    ends = starts[1:] + [float(times[-1])]
    return [(w, [s, e]) for w, s, e in zip(words, starts, ends)]


def token_align(xattn: torch.Tensor, nrows, nframes, median_width: int = MEDIAN_WIDTH, want_matrix: bool = False):
    """tdx_token_align: xattn float32 [B, nh, max_rows, n_audio_ctx] on the device, nrows / nframes per clip -> frames int32
    [B, max_rows] (entry i of clip b: the encoder position at which token row i begins; entries >= nrows[b] hold -1) and, with
    want_matrix, the normalised, filtered, head-averaged matrix [B, max_rows, n_audio_ctx] (zeros where nothing is written)"""
    if xattn.dim() != 4 or xattn.dtype != torch.float32 or not xattn.is_cuda or not xattn.is_contiguous():
        raise _lib.TdxError("token_align: xattn must be a contiguous float32 [B, nh, max_rows, n_audio_ctx] tensor on the device")
    B, nh, R, S = xattn.shape
    dev = xattn.device
    l = _lib.lib()
    nr = torch.as_tensor(nrows, dtype=torch.int32).reshape(-1).to(dev)
    nf = torch.as_tensor(nframes, dtype=torch.int32).reshape(-1).to(dev)
    if nr.numel() != B or nf.numel() != B:
        raise _lib.TdxError(f"token_align: {B} clips, {nr.numel()} nrows, {nf.numel()} nframes")
    frames = torch.full((B, R), -1, dtype=torch.int32, device=dev)
    matrix = torch.zeros(B, R, S, device=dev) if want_matrix else None
    with torch.cuda.device(dev):
        ws = torch.empty(max(1, int(l.tdx_token_align_workspace_bytes(B, nh, R, S))), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(l.tdx_token_align(xattn.data_ptr(), B, nh, R, S, nr.data_ptr(), nf.data_ptr(), int(median_width), frames.data_ptr(),
                                     matrix.data_ptr() if want_matrix else None, ws.data_ptr(), ws.numel(), st))
        torch.cuda.current_stream(dev).synchronize()          # the workspace is this call's own
    return (frames, matrix) if want_matrix else frames


_word_timestamps = word_timestamps                     # transcribe() has a switch of that name


def cut_segments(tokens, timestamp_begin: int, seek: int, seek_num_frames: int):
    """transformers' _retrieve_segment: a window's generated ids (no end-of-text) -> ([{"start", "end", "tokens"}], the seek step in
    feature frames).  Consecutive timestamp pairs close segments; with a single closing timestamp the last segment runs to the
    end of the ids and the whole window is consumed, without one the ids after the last pair are dropped and the next window
    starts at that pair's time; with no pair at all the ids are one segment that ends at the last timestamp (the window's end
    when there is none, or only <|0.00|>) and the whole window is consumed."""
    tb = int(timestamp_begin)
    tokens = [int(t) for t in tokens]
    t0 = seek * TIME_PRECISION / 2
    stamp = [t >= tb for t in tokens]
    single_end = stamp[-2:] == [False, True]
    slices = [i + 1 for i in range(len(tokens) - 1) if stamp[i] and stamp[i + 1]]
    if not slices:
        last = int(seek_num_frames * 0.01 / TIME_PRECISION)
        marks = [t for t in tokens if t >= tb]
        if marks and marks[-1] != tb:
            last = marks[-1] - tb
        return [{"start": t0, "end": t0 + last * TIME_PRECISION, "tokens": tokens}], int(seek_num_frames)
    if single_end:
        slices.append(len(tokens))
    else:
        slices[-1] += 1                                    # the pair's second timestamp stays with the last segment
    segs, lo = [], 0
    for k, hi in enumerate(slices):
        sl = tokens[lo:hi]
        end = sl[-1] if (k < len(slices) - 1 or single_end) else sl[-2]
        segs.append({"start": t0 + (sl[0] - tb) * TIME_PRECISION, "end": t0 + (end - tb) * TIME_PRECISION, "tokens": sl})
        lo = hi
    step = int(seek_num_frames) if single_end else (tokens[lo - 2] - tb) * 2
    return segs, (step if step > 0 else int(seek_num_frames))      # (the rules keep a pair's time above 0; a step of 0 would never end)


def longform_prefix(init, history, condition: bool, first_prompt, timestamp_begin: int, prev_sot: int, n_text_ctx: int):
    """transformers' _prepare_decoder_input_ids for one clip.  init: [sot, lang, task]; history: the token lists of the clip's
    segments so far (with conditioning a prompt is the first of them); conditioning: <|startofprev|> + the last n_text_ctx // 2 - 1
    of those ids, the second timestamp of a closing pair skipped, + init.  first_prompt: the prompt of a first window without
    conditioning."""
    if condition and history:
        ids = []
        for s in history:
            ids += list(s[:-1]) if len(s) > 2 and s[-2] >= timestamp_begin else list(s)
        return [int(prev_sot)] + ids[-(n_text_ctx // 2 - 1):] + list(init)
    if first_prompt is not None:
        return [int(prev_sot)] + list(first_prompt) + list(init)
    return list(init)


def compression_ratio(text: str) -> float:
    """openai/whisper utils.compression_ratio: len(bytes) / len(zlib.compress(bytes)) of the text as UTF-8"""
    b = text.encode("utf-8")
    return len(b) / len(zlib.compress(b))


def needs_fallback(ratio, avg, nosp, thresholds) -> bool:
    """whisper.transcribe's decode_with_fallback decision for one decoded window.  thresholds: (compression_ratio_threshold,
    logprob_threshold, no_speech_threshold), each None to skip its check.  Too repetitive (ratio above its threshold) or too
    unlikely (avg_logprob below its threshold) asks for the next temperature, unless the window counts as silent (no_speech_prob
    above its threshold and avg_logprob below its threshold): that one is skipped, not decoded again."""
    cr, lp, ns = thresholds
    need = (cr is not None and ratio > cr) or (lp is not None and avg < lp)
    if ns is not None and lp is not None and nosp > ns and avg < lp:
        need = False
    return bool(need)


def fallback_options(on: bool) -> dict:
    """transcribe()'s keywords behind the whisper_fallback switches: whisper.transcribe's own defaults when on, nothing when off"""
    return dict(temperature=FALLBACK_TEMPERATURES, compression_ratio_threshold=FALLBACK_COMPRESSION_RATIO) if on else {}


def _temperatures(temperature):
    temps = (float(temperature),) if isinstance(temperature, (int, float)) else tuple(float(t) for t in temperature)
    if not 1 <= len(temps) <= MAX_TEMPERATURES:
        raise ValueError(f"{len(temps)} temperatures: 1..{MAX_TEMPERATURES} (a row's noise stream is {MAX_TEMPERATURES} x the clip's index + the attempt)")
    return temps


def _int_array(v):                                      # (one element for an empty list: never a NULL pointer)
    return (C.c_int * max(1, len(v)))(*[int(t) for t in v])


class WhisperASR:
    def __init__(self, state_dict, config, device="cuda:0", token_list=None, tokenizer=None, generation_config=None, alignment_heads=None):
        self.cfg = c = whisper_config(config)
        self.token_list, self.tokenizer = token_list, tokenizer
        self.gen_cfg = _gen_dict(generation_config) if generation_config is not None else default_generation_config(c["vocab"])
        heads = alignment_heads if alignment_heads is not None else self.gen_cfg.get("alignment_heads")
        self.alignment_heads = [[int(l), int(h)] for l, h in (heads if heads is not None else default_alignment_heads(c))]
        if any(not (0 <= l < c["dec_layers"] and 0 <= h < c["dec_heads"]) for l, h in self.alignment_heads):
            raise ValueError(f"alignment_heads: (layer, head) pairs inside {c['dec_layers']} layers x {c['dec_heads']} heads")
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

    def _check_state(self, who, state) -> int:
        c = self.cfg
        B = int(state.shape[2])
        self._check_batch(B)
        if tuple(state.shape) != (c["dec_layers"], 2, B, c["n_audio_ctx"], c["d_model"]) or not state.is_contiguous():
            raise _lib.TdxError(f"WhisperASR.{who}: state is not encode(..., with_state=True)'s")
        return B

    def _decode_buffers(self, B):                       # step_ids, step_scores, counts
        T = self.cfg["n_text_ctx"]
        return (torch.full((B, T), -1, dtype=torch.int32, device=self.device), torch.zeros(B, T, device=self.device),
                torch.zeros(B, dtype=torch.int32, device=self.device))

    def _alloc_xattn(self, B, nh, max_rows):            # None: a shape the C-ABI call rejects with its own message
        ok = 1 <= nh <= MAX_ALIGN_HEADS and max_rows >= 1
        return torch.zeros(B, nh, max_rows, self.cfg["n_audio_ctx"], device=self.device) if ok else None

    def _call(self, fn, B, *args, ws_bytes=None):
        """fn(handle, *args, workspace, its bytes, the current stream) under the model's guard"""
        with self._guard.call():
            ws = self._guard.workspace(self.workspace_bytes(B) if ws_bytes is None else ws_bytes)
            _lib.check(fn(self._h, *args, ws.data_ptr(), ws.numel(), torch.cuda.current_stream(self.device).cuda_stream))

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
        self._call(self._l.tdx_whisper_logmel, B, wav.data_ptr(), lens_dev.data_ptr() if lens_dev is not None else None, B, N, feat.data_ptr())
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
        self._call(self._l.tdx_whisper_encode, B, feats.data_ptr(), B, enc.data_ptr(), state.data_ptr() if with_state else None)
        return (enc, state) if with_state else enc

    def decode(self, state: torch.Tensor, prefix, max_new: int, suppress=(), begin_suppress=(), eos=None):
        """greedy decoding from encode()'s state under one prefix -> device tensors step_ids int32 [B, n_text_ctx], step_scores
        [B, n_text_ctx] (step p at column p; columns no step reached hold -1 / 0) and counts int32 [B]"""
        self._check_open()
        B = self._check_state("decode", state)
        eos = int(self.gen_cfg["eos_token_id"] if eos is None else eos)
        ids, scores, counts = self._decode_buffers(B)
        prefix, suppress, begin_suppress = list(prefix), list(suppress), list(begin_suppress)
        self._call(self._l.tdx_whisper_decode, B, state.data_ptr(), B, _int_array(prefix), len(prefix), _int_array(suppress), len(suppress),
                   _int_array(begin_suppress), len(begin_suppress), eos, int(max_new), ids.data_ptr(), scores.data_ptr(), counts.data_ptr())
        return ids, scores, counts

    def decode_xattn(self, state: torch.Tensor, prefix, max_new: int, suppress=(), begin_suppress=(), eos=None, first_row=None, max_rows=None,
                     heads=None, xattn=None):
        """decode() through tdx_whisper_decode_xattn: the same ids, scores and counts (bit for bit), plus xattn float32
        [B, nh, max_rows, n_audio_ctx]: row p - first_row of head k holds the cross-attention probabilities of `heads[k]` at the
        step that fed position p.  Defaults: the model's alignment heads, first_row = len(prefix) (the first generated token),
        max_rows = max(1, max_new - 1).  Rows no step reached keep what `xattn` held (zeros when it is allocated here)."""
        self._check_open()
        c = self.cfg
        B = self._check_state("decode_xattn", state)
        eos = int(self.gen_cfg["eos_token_id"] if eos is None else eos)
        prefix, suppress, begin_suppress = list(prefix), list(suppress), list(begin_suppress)
        heads = [[int(l), int(h)] for l, h in (self.alignment_heads if heads is None else heads)]
        first_row = len(prefix) if first_row is None else int(first_row)
        max_rows = max(1, int(max_new) - 1) if max_rows is None else int(max_rows)
        nh = len(heads)
        if xattn is None:
            xattn = self._alloc_xattn(B, nh, max_rows)
        elif (tuple(xattn.shape) != (B, nh, max_rows, c["n_audio_ctx"]) or xattn.dtype != torch.float32 or not xattn.is_contiguous()
              or xattn.device != torch.device(self.device)):
            raise _lib.TdxError(f"WhisperASR.decode_xattn: xattn must be contiguous float32 [{B}, {nh}, {max_rows}, {c['n_audio_ctx']}] on {self.device}")
        ids, scores, counts = self._decode_buffers(B)
        flat = [t for pair in heads for t in pair]
        self._call(self._l.tdx_whisper_decode_xattn, B, state.data_ptr(), B, _int_array(prefix), len(prefix), _int_array(suppress), len(suppress),
                   _int_array(begin_suppress), len(begin_suppress), eos, int(max_new), _int_array(flat), nh, first_row, max_rows,
                   xattn.data_ptr() if xattn is not None else None, ids.data_ptr(), scores.data_ptr(), counts.data_ptr())
        return ids, scores, counts, xattn

    def detect_language(self, state: torch.Tensor) -> list:
        """the language code of every clip of encode()'s state: one decode step after <|startoftranscript|> with every id that is
        not a language token suppressed (openai/whisper decoding.py detect_language; transformers' detect_language)"""
        g = self.gen_cfg
        lang_ids = sorted(int(v) for v in g["lang_to_id"].values())
        allowed = set(lang_ids)
        suppress = [i for i in range(self.cfg["vocab"]) if i not in allowed]
        ids, _, _ = self.decode(state, [int(g["decoder_start_token_id"])], 1, suppress, ())
        by_id = {int(v): k for k, v in g["lang_to_id"].items()}
        return [language_code(by_id[int(t)]) for t in ids[:, 0].cpu().tolist()]

    def num_frames(self, n_samples: int) -> int:
        """encoder positions that a clip of n_samples covers: ceil(n / 320), within [1, n_audio_ctx]"""
        return max(1, min(self.cfg["n_audio_ctx"], -(-int(n_samples) // 320)))

    def text_of(self, ids) -> str:
        return decode_text(ids, self.token_list, int(self.gen_cfg["eos_token_id"]))

    def generate(self, wavs, language: str = "chinese", task: str = "transcribe", prompt_ids=None, max_new_tokens=None, keys=None,
                 return_timestamps: bool = False):
        """list of 1-D 16 kHz clips (or one clip) -> per clip {"key", "text", "token_ids", "scores"}: the generated ids (a final
        end-of-text included) and their log-probabilities.  Clips go through in batches of 32, cut to 30 s.
        language None or "auto": the language of every clip is detected and the clips are decoded grouped by language (one prefix
        per decode call); each result then also carries "language" (the code).
        return_timestamps: each result also carries "token_times" (seconds, one per generated id: 0.02 x the encoder position at
        which the alignment heads' cross-attention path enters the token; the last id repeats the one before it, a lone id gets 0)
        and "words" ([(word, [start_s, end_s]), ...] over the ordinary ids).  The ids and scores are those of the plain call."""
        self._check_open()
        if isinstance(wavs, (np.ndarray, torch.Tensor)):
            wavs = [wavs]
        g, T = self.gen_cfg, self.cfg["n_text_ctx"]
        auto = language is None or str(language).strip().lower() == "auto"
        if return_timestamps and not 1 <= len(self.alignment_heads) <= MAX_ALIGN_HEADS:
            raise ValueError(f"{len(self.alignment_heads)} alignment heads: pass 1..{MAX_ALIGN_HEADS} pairs as alignment_heads= or in the generation config")
        sup, beg, eos = g.get("suppress_tokens") or (), g.get("begin_suppress_tokens") or (), int(g["eos_token_id"])
        out = []
        for c0 in range(0, len(wavs), MAX_BATCH):
            chunk = wavs[c0:c0 + MAX_BATCH]
            nsamp = [min(self.n_samples, int(np.prod(np.shape(w)))) for w in chunk]
            _, state = self.encode(self.features(chunk), with_state=True)
            if auto:
                langs = self.detect_language(state)
                groups = [(lg, [b for b, l in enumerate(langs) if l == lg]) for lg in sorted(set(langs))]
            else:
                langs, groups = None, [(language, list(range(len(chunk))))]
            res = [None] * len(chunk)
            for lg, members in groups:
                prefix = decode_prefix(lg, task, prompt_ids, g, T)
                max_new = new_token_limit(len(prefix), max_new_tokens, g, T)
                p0 = len(prefix) - 1                        # the step that wrote the first generated token
                step = len(members)
                if return_timestamps:                       # smaller groups on the alignment path only: the capture buffer stays bounded
                    row_bytes = 4 * len(self.alignment_heads) * max(1, max_new - 1) * self.cfg["n_audio_ctx"]
                    step = max(1, min(step, XATTN_BUDGET // row_bytes))
                for m0 in range(0, len(members), step):
                    mem = members[m0:m0 + step]
                    st = state if len(mem) == len(chunk) else state[:, :, mem].contiguous()
                    if return_timestamps:
                        ids, scores, counts, xattn = self.decode_xattn(st, prefix, max_new, sup, beg)
                        counts_l = counts.cpu().tolist()
                        nrows = [max(0, n - 1) for n in counts_l]
                        frames = token_align(xattn, nrows, [self.num_frames(nsamp[b]) for b in mem]).cpu().tolist()
                        del xattn
                    else:
                        ids, scores, counts = self.decode(st, prefix, max_new, sup, beg)
                        counts_l = counts.cpu().tolist()
                    ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
                    for k, (b, n) in enumerate(zip(mem, counts_l)):
                        tok = [int(t) for t in ids[k, p0:p0 + n]]
                        r = {"key": keys[c0 + b] if keys is not None else f"clip_{c0 + b}", "text": self.text_of(tok), "token_ids": tok,
                             "scores": [float(v) for v in scores[k, p0:p0 + n]]}
                        if auto:
                            r["language"] = langs[b]
                        if return_timestamps:
                            t = [f * TIME_PRECISION for f in frames[k][:max(0, n - 1)]]
                            r["token_times"] = (t + [t[-1]]) if t else [0.0] * n
                            r["words"] = word_timestamps(tok, r["token_times"], self.token_list, language_code(lg), eos)
                        res[b] = r
            out.extend(res)
        return out

    # ---- long-form transcription with timestamp tokens
    def features_long(self, wav) -> torch.Tensor:
        """one 16 kHz clip of any length N -> log-mel features [n_mels, N // 160], nothing cut or padded, the clamp taken over the
        whole clip (WhisperFeatureExtractor with truncation=False)"""
        self._check_open()
        wav = torch.as_tensor(np.asarray(wav, dtype=np.float32) if not isinstance(wav, torch.Tensor) else wav)
        wav = wav.reshape(-1).to(self.device, torch.float32).contiguous()
        N = int(wav.shape[0])
        if N < 1:
            raise _lib.TdxError("WhisperASR.features_long: an empty clip")
        feat = torch.empty(self.cfg["n_mels"], N // 160, device=self.device)
        with self._guard.call():
            ws = self._guard.workspace(max(1, int(self._l.tdx_whisper_logmel_long_workspace_bytes(self._h, N))))
            st = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(self._l.tdx_whisper_logmel_long(self._h, wav.data_ptr(), N, feat.data_ptr() if feat.numel() else None, ws.data_ptr(),
                                                       ws.numel(), st))
        return feat

    def decode_ts(self, state: torch.Tensor, prefixes, max_new, suppress=(), begin_suppress=(), eos=None, no_timestamps_id=None,
                  max_initial_timestamp_index=None, begin=None, sot_pos=None, no_speech_id=None, heads=None, first_row=None, max_rows=None,
                  temperature=None, streams=None, seed=0):
        """greedy decoding under Whisper's timestamp rules, one prefix per row (tdx_whisper_decode_ts) -> step_ids, step_scores,
        counts as decode(), nospeech float32 [B] (None without sot_pos) and xattn [B, nh, max_rows, n_audio_ctx] (None without
        heads).  prefixes: a list of id lists; max_new: an int or one per row; begin: per row, where the row's history starts
        (default: its prefix length); sot_pos: per row, the position of <|startoftranscript|>; first_row: per row (default: its
        prefix length).
        temperature (a float or one per row; None: the greedy entry point, as ever): tdx_whisper_decode_ts_sample, every row draws
        its ids from softmax(logits / T) over the ids the rules allow, a row at 0 decodes greedily; the scores are the drawn ids'
        untempered log-probabilities.  streams: one 64-bit noise stream per row (default 0), seed: the generator's key; a row's
        result depends on (seed, its stream, its inputs) alone."""
        self._check_open()
        g = self.gen_cfg
        B = self._check_state("decode_ts", state)
        prefixes = [[int(t) for t in p] for p in prefixes]
        if len(prefixes) != B:
            raise _lib.TdxError(f"WhisperASR.decode_ts: {B} rows of state, {len(prefixes)} prefixes")
        per_row = lambda v: [int(v)] * B if isinstance(v, int) else [int(t) for t in v]
        max_new = per_row(max_new)
        eos = int(g["eos_token_id"] if eos is None else eos)
        nots = int(g["no_timestamps_token_id"] if no_timestamps_id is None else no_timestamps_id)
        mi = g.get("max_initial_timestamp_index") if max_initial_timestamp_index is None else max_initial_timestamp_index
        mi = -1 if mi is None else int(mi)
        plen = [len(p) for p in prefixes]
        mp = max(1, max(plen))
        opt = lambda v: _int_array(per_row(v)) if v is not None else None
        flat_prefix = [t for p in prefixes for t in p + [0] * (mp - len(p))]
        for name, v in (("max_new", max_new), ("begin", begin), ("sot_pos", sot_pos), ("first_row", first_row)):
            if v is not None and not isinstance(v, int) and len(v) != B:
                raise _lib.TdxError(f"WhisperASR.decode_ts: {name} has {len(v)} entries for {B} rows")
        suppress, begin_suppress = list(suppress), list(begin_suppress)
        ids, scores, counts = self._decode_buffers(B)
        nospeech = torch.zeros(B, device=self.device) if sot_pos is not None else None
        ns_id = int(nots - 1 if no_speech_id is None else no_speech_id)
        xattn, flat, nh = None, None, 0
        if heads is not None:
            heads = [[int(l), int(h)] for l, h in heads]
            nh = len(heads)
            flat = _int_array([t for pair in heads for t in pair])
            max_rows = max(1, max(max_new) - 1) if max_rows is None else int(max_rows)
            xattn = self._alloc_xattn(B, nh, max_rows)
        args = (state.data_ptr(), B, _int_array(flat_prefix), mp, _int_array(plen), opt(begin), _int_array(suppress),
                len(suppress), _int_array(begin_suppress), len(begin_suppress), eos, nots, mi, _int_array(max_new), ns_id, opt(sot_pos),
                nospeech.data_ptr() if nospeech is not None else None, flat, nh, opt(first_row), int(max_rows or 0),
                xattn.data_ptr() if xattn is not None else None, ids.data_ptr(), scores.data_ptr(), counts.data_ptr())
        if temperature is None:
            self._call(self._l.tdx_whisper_decode_ts, B, *args)
            return ids, scores, counts, nospeech, xattn
        temps = [float(temperature)] * B if isinstance(temperature, (int, float)) else [float(t) for t in temperature]
        streams = [0] * B if streams is None else [int(t) for t in streams]
        for name, v in (("temperature", temps), ("streams", streams)):
            if len(v) != B:
                raise _lib.TdxError(f"WhisperASR.decode_ts: {name} has {len(v)} entries for {B} rows")
        self._call(self._l.tdx_whisper_decode_ts_sample, B, *args, (C.c_float * B)(*temps), (C.c_ulonglong * B)(*[t & (2 ** 64 - 1) for t in streams]),
                   int(seed) & (2 ** 64 - 1), ws_bytes=int(self._l.tdx_whisper_decode_sample_workspace_bytes(self._h, B)))
        return ids, scores, counts, nospeech, xattn

    def transcribe(self, wavs, language=None, task: str = "transcribe", prompt_ids=None, condition_on_prev_tokens: bool = True,
                   no_speech_threshold=0.6, logprob_threshold=-1.0, word_timestamps: bool = True, keys=None, temperature=0.0,
                   compression_ratio_threshold=None, seed=0):
        """whisper.transcribe(model, audio, initial_prompt=, word_timestamps=True, language=), as transformers' long-form generate
        runs it: clips of any length, decoded in 30 s windows with timestamp tokens, cut into segments at the timestamp pairs, the
        next window starting at the last timestamp.  Per clip {"key", "language", "text", "segments": [{"id", "seek", "start",
        "end", "text", "tokens", "avg_logprob", "no_speech_prob", "words"}]}.  All clips still running share one encode and one
        decode_ts call per round of the loop, whatever their languages and prefix lengths.
        temperature: a float (0.0: greedy), or up to 16 of them for upstream's decode_with_fallback: a window whose text compresses
        better than compression_ratio_threshold or whose avg_logprob is below logprob_threshold (needs_fallback) is decoded again
        at the next temperature, all such rows of a round in one decode_ts call on their gathered encoder state; the last attempt
        stands.  A row's noise stream is (16 x the clip's index in the call + the attempt) << 32 | seek, so a clip's text does not
        depend on the other clips.  A window decoded above temperature 0.5 does not condition the next one.  With anything but the
        default 0.0 the segments also carry "temperature" and "compression_ratio" (of the attempt that stands)."""
        self._check_open()
        temps = _temperatures(temperature)
        thresholds = (compression_ratio_threshold, logprob_threshold, no_speech_threshold)
        if isinstance(wavs, (np.ndarray, torch.Tensor)):
            wavs = [wavs]
        g, c = self.gen_cfg, self.cfg
        T, nseg = c["n_text_ctx"], 2 * c["n_audio_ctx"]
        if word_timestamps and not 1 <= len(self.alignment_heads) <= MAX_ALIGN_HEADS:
            raise ValueError(f"{len(self.alignment_heads)} alignment heads: pass 1..{MAX_ALIGN_HEADS} pairs as alignment_heads= or in the generation config")
        sup, beg, eos = g.get("suppress_tokens") or (), g.get("begin_suppress_tokens") or (), int(g["eos_token_id"])
        tb, prev = int(g["no_timestamps_token_id"]) + 1, int(g["prev_sot_token_id"])
        prompt = None
        if prompt_ids is not None:
            prompt = [int(t) for t in (prompt_ids.tolist() if hasattr(prompt_ids, "tolist") else prompt_ids)]
            prompt = prompt[1:] if prompt and prompt[0] == prev else prompt
        auto = language is None or str(language).strip().lower() == "auto"
        out = []
        for c0 in range(0, len(wavs), MAX_BATCH):
            chunk = wavs[c0:c0 + MAX_BATCH]
            feats = [self.features_long(w) for w in chunk]
            n = len(chunk)
            F = [int(f.shape[1]) for f in feats]
            seek, langs, inits = [0] * n, [None if auto else language_code(language)] * n, [None] * n
            history = [[list(prompt)] if prompt is not None and condition_on_prev_tokens else [] for _ in range(n)]
            first_prompt = [prompt if not condition_on_prev_tokens else None for _ in range(n)]
            segs = [[] for _ in range(n)]
            while True:
                live = [i for i in range(n) if seek[i] < F[i]]
                if not live:
                    break
                nfr = [min(F[i] - seek[i], nseg) for i in live]
                win = torch.zeros(len(live), c["n_mels"], nseg, device=self.device)
                for k, i in enumerate(live):
                    win[k, :, :nfr[k]] = feats[i][:, seek[i]:seek[i] + nfr[k]]
                _, state = self.encode(win, with_state=True)
                need = [k for k, i in enumerate(live) if langs[i] is None]
                if need:                                    # the language of a clip comes from its first window
                    found = self.detect_language(state if len(need) == len(live) else state[:, :, need].contiguous())
                    for k, lg in zip(need, found):
                        langs[live[k]] = lg
                prefixes = []
                for i in live:
                    if inits[i] is None:
                        inits[i] = decode_prefix(langs[i], task, None, g, T)[:-1]          # no <|notimestamps|>
                    prefixes.append(longform_prefix(inits[i], history[i], condition_on_prev_tokens, first_prompt[i], tb, prev, T))
                    first_prompt[i] = None
                for p in prefixes:
                    if len(p) >= T:
                        raise ValueError(f"a prefix of {len(p)} ids leaves no room in a context of {T}")
                max_new = [new_token_limit(len(p), None, {"max_length": g.get("max_length")}, T) for p in prefixes]
                heads = self.alignment_heads if word_timestamps else None
                sot = [len(p) - len(inits[i]) for p, i in zip(prefixes, live)]
                # decode_with_fallback: attempt a decodes the rows that attempts 0 .. a - 1 left in need, at temps[a]; the last stands
                rows, done = list(range(len(live))), {}
                for attempt, temp in enumerate(temps):
                    whole = len(rows) == len(live)
                    kw = {}
                    if attempt > 0 or temp != 0.0:
                        kw = dict(temperature=[temp] * len(rows), seed=seed,
                                  streams=[((MAX_TEMPERATURES * (c0 + live[k]) + attempt) << 32) | seek[live[k]] for k in rows])
                    ids, scores, counts, nosp, xattn = self.decode_ts(
                        state if whole else state[:, :, rows].contiguous(), prefixes if whole else [prefixes[k] for k in rows],
                        max_new if whole else [max_new[k] for k in rows], suppress=sup, begin_suppress=beg, eos=eos, no_timestamps_id=tb - 1,
                        sot_pos=sot if whole else [sot[k] for k in rows], heads=heads, **kw)
                    counts_l, nosp_l = counts.cpu().tolist(), nosp.cpu().tolist()
                    ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
                    again = []
                    for j, k in enumerate(rows):
                        p0, m = len(prefixes[k]) - 1, counts_l[j]
                        tok = [int(t) for t in ids[j, p0:p0 + m]]
                        avg = float(np.sum(scores[j, p0:p0 + m], dtype=np.float64)) / m if m else 0.0
                        ratio = compression_ratio(self.text_of(tok).strip())
                        done[k] = {"tok": tok, "m": m, "avg": avg, "ratio": ratio, "nosp": nosp_l[j], "temp": temp}
                        if attempt + 1 < len(temps) and needs_fallback(ratio, avg, nosp_l[j], thresholds):
                            again.append(k)
                    if word_timestamps:                     # the alignment of the rows whose attempt stands (0 rows: nothing is written)
                        fr = token_align(xattn, [0 if k in again else max(0, counts_l[j] - 1) for j, k in enumerate(rows)],
                                         [max(1, nfr[k] // 2) for k in rows]).cpu().tolist()
                        for j, k in enumerate(rows):
                            done[k]["frames"] = fr[j]
                        del xattn
                    if not again:
                        break
                    rows = again
                for k, i in enumerate(live):
                    tok, m, avg, nosp_k = done[k]["tok"], done[k]["m"], done[k]["avg"], done[k]["nosp"]
                    if (no_speech_threshold is not None and logprob_threshold is not None and avg < logprob_threshold
                            and nosp_k > no_speech_threshold):
                        seek[i] += nfr[k]                   # a silent window: skipped whole
                        continue
                    body = tok[:-1] if tok and tok[-1] == eos else tok
                    t0 = seek[i] * TIME_PRECISION / 2
                    times = None
                    if word_timestamps:
                        t = [f * TIME_PRECISION for f in done[k]["frames"][:max(0, m - 1)]]
                        times = (t + [t[-1]]) if t else [0.0] * m
                    cut, step = cut_segments(body, tb, seek[i], nfr[k])
                    at = 0
                    for s in cut:
                        words = []
                        if word_timestamps:
                            tt = times[at:at + len(s["tokens"])]
                            words = [(w, [a + t0, b + t0]) for w, (a, b) in _word_timestamps(s["tokens"], tt, self.token_list, langs[i], eos)]
                        at += len(s["tokens"])
                        segs[i].append({"id": len(segs[i]), "seek": seek[i], "start": s["start"], "end": s["end"], "text": self.text_of(s["tokens"]),
                                        "tokens": s["tokens"], "avg_logprob": avg, "no_speech_prob": float(nosp_k), "words": words})
                        if temps != (0.0,):
                            segs[i][-1].update(temperature=done[k]["temp"], compression_ratio=done[k]["ratio"])
                        history[i].append(s["tokens"])
                    if done[k]["temp"] > PROMPT_RESET_TEMPERATURE:
                        history[i] = []                     # upstream's prompt_reset_since: the next window carries no previous text
                    seek[i] += step
            for i in range(n):
                out.append({"key": keys[c0 + i] if keys is not None else f"clip_{c0 + i}", "language": langs[i],
                            "text": "".join(s["text"] for s in segs[i]), "segments": segs[i]})
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


# openai/whisper model.py names -> transformers' (the pairs of transformers' convert_openai_to_hf.py), applied in this order
OPENAI_NAME_MAP = (("blocks", "layers"), ("mlp.0", "fc1"), ("mlp.2", "fc2"), ("mlp_ln", "final_layer_norm"),
                   (".attn.query", ".self_attn.q_proj"), (".attn.key", ".self_attn.k_proj"), (".attn.value", ".self_attn.v_proj"),
                   (".attn_ln", ".self_attn_layer_norm"), (".attn.out", ".self_attn.out_proj"),
                   (".cross_attn.query", ".encoder_attn.q_proj"), (".cross_attn.key", ".encoder_attn.k_proj"),
                   (".cross_attn.value", ".encoder_attn.v_proj"), (".cross_attn_ln", ".encoder_attn_layer_norm"),
                   (".cross_attn.out", ".encoder_attn.out_proj"), ("decoder.ln.", "decoder.layer_norm."), ("encoder.ln_post.", "encoder.layer_norm."),
                   ("token_embedding", "embed_tokens"), ("encoder.positional_embedding", "encoder.embed_positions.weight"),
                   ("decoder.positional_embedding", "decoder.embed_positions.weight"))


def openai_to_hf_name(name: str) -> str:
    for a, b in OPENAI_NAME_MAP:
        name = name.replace(a, b)
    return "model." + name


def openai_dims_to_config(dims) -> dict:
    """openai/whisper ModelDimensions -> whisper_config's dict"""
    d = dict(dims)
    if d["n_audio_state"] != d["n_text_state"]:
        raise ValueError("OpenAI checkpoint: n_audio_state differs from n_text_state")
    return whisper_config(n_mels=d["n_mels"], n_audio_ctx=d["n_audio_ctx"], d_model=d["n_audio_state"], enc_heads=d["n_audio_head"],
                          enc_layers=d["n_audio_layer"], n_text_ctx=d["n_text_ctx"], dec_heads=d["n_text_head"], dec_layers=d["n_text_layer"],
                          vocab=d["n_vocab"])


def load_openai_checkpoint(path):
    """One OpenAI-format .pt file ({"dims", "model_state_dict"}, what whisper.load_model reads; ASRProcessor.py:232-243) ->
    (state dict in transformers' names, fp32, proj_out.weight tied to the token embedding; whisper_config's dict)"""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(ck, dict) or "dims" not in ck or "model_state_dict" not in ck:
        raise ValueError(f"{path}: not an OpenAI Whisper checkpoint (no dims / model_state_dict)")
    sd = {openai_to_hf_name(k): v.float() for k, v in ck["model_state_dict"].items()}
    sd["proj_out.weight"] = sd["model.decoder.embed_tokens.weight"]
    return sd, openai_dims_to_config(ck["dims"])


def build_whisper(state_dict=None, config=None, model_dir=None, token_list=None, tokenizer=None, generation_config=None, cuda_device: int = 0,
                  alignment_heads=None):
    """The device recogniser from weights + config, from a transformers model directory: config.json plus model.safetensors or
    pytorch_model.bin, and when present generation_config.json, vocab.json (the piece table) and the tokenizer files (prompts),
    or from one OpenAI-format .pt file (a vocab.json next to it is read when present).
    None when there is neither source.  safetensors / transformers are imported here only, and only when a directory needs them."""
    if state_dict is None and isinstance(model_dir, str) and os.path.isfile(model_dir):
        state_dict, config = load_openai_checkpoint(model_dir)
        if token_list is None:
            token_list = load_token_list(os.path.join(os.path.dirname(model_dir), "vocab.json"))
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
    return WhisperASR(state_dict, config, device=f"cuda:{cuda_device}", token_list=token_list, tokenizer=tokenizer, generation_config=generation_config,
                      alignment_heads=alignment_heads)
