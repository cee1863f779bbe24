"""Restatement of Whisper's sampled decoding and temperature fallback for the tests: Philox4x32-10 twice (over Python
ints, and numpy-vectorised), the Gumbel noise of include/tdx.h in fp64, `sample_ts` (whisper_longform_oracle.greedy_ts with a
Gumbel-max draw per step under the same rules) and openai/whisper's decode_with_fallback as a loop over a decoder given as a
callable.  tests/test_whisper_fallback_host.py pins the generator to the Random123 known answers and the draw to softmax(v / T)."""
from __future__ import annotations

import zlib

import numpy as np
import torch

import whisper_longform_oracle as lo
import whisper_oracle as wo

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
MAX_TEMPERATURES = 16


def philox_int(counter, key):
    """Philox4x32-10 over Python ints: counter (4 words), key (2 words) -> 4 words"""
    c0, c1, c2, c3 = (int(c) & MASK32 for c in counter)
    k0, k1 = (int(k) & MASK32 for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [c0, c1, c2, c3]


def philox_np(c0, c1, c2, c3, k0, k1):
    """the same over numpy arrays (any broadcastable shapes) -> uint32 [..., 4]"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(v).astype(np.uint64) & np.uint64(MASK32) for v in (c0, c1, c2, c3, k0, k1)])
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def noise_words(seed, stream, p, ids):
    """the raw word of every id of `ids` at context position p (scalar or an array like ids): key (seed lo, seed hi), counter
    (n >> 2, p, stream lo, stream hi), word n & 3"""
    ids = np.asarray(ids, dtype=np.int64)
    seed, stream = int(seed) & (2 ** 64 - 1), int(stream) & (2 ** 64 - 1)
    w = philox_np(ids >> 2, p, stream & MASK32, stream >> 32, seed & MASK32, seed >> 32)
    return np.take_along_axis(w, (ids & 3)[..., None], -1)[..., 0]


def uniform64(words):
    return ((np.asarray(words, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel64(words):
    return -np.log(-np.log(uniform64(words)))


def gumbel32(words):
    """the device's arithmetic with numpy's float32 logarithm"""
    u = ((np.asarray(words, dtype=np.uint32) >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    return -np.log(-np.log(u))


NOISE_GAP = 6.01e-7             # what noise_gap() returns (6.009e-07), rounded up: tests/test_whisper_fallback_host.py recomputes it


def noise_gap():
    """max |g32 - g64| over all 2^23 values of k: the restatement's own fp32-versus-fp64 gap"""
    gap = 0.0
    for k0 in range(0, 1 << 23, 1 << 20):
        w = (np.arange(k0, k0 + (1 << 20), dtype=np.uint32) << np.uint32(9))
        gap = max(gap, float(np.abs(gumbel32(w).astype(np.float64) - gumbel64(w)).max()))
    return gap


def gumbel_argmax(v, temperature, seed, stream, p):
    """Gumbel-max over every id of the logit vector v (fp64) at position p -> the drawn id"""
    v = np.asarray(v, dtype=np.float64)
    return int(np.argmax(v / temperature + gumbel64(noise_words(seed, stream, p, np.arange(v.shape[0])))))


def sample_step(logits, seq, first_step, tb, eos, max_initial, deny, temperature, seed, stream, p):
    """one decision under the rules -> (id, its untempered log-softmax over the allowed set, draw margin, mass margin, greedy id).
    The mass rule is decided on the raw logits; the draw is the largest z = v / T + g among the ids still allowed (ties: the
    lowest id), its margin the gap to the second-largest z; at temperature 0 the id is the argmax and the margin the top-2 gap of
    the logits."""
    lg = torch.as_tensor(logits).double()
    pre = lo.history_rules(lg.shape[0], seq, first_step, tb, eos, max_initial, deny)
    ok = lo.ts_rules(lg, seq, first_step, tb, eos, max_initial, deny)
    m = lg.masked_fill(~ok, float("-inf"))
    greedy = int(m.argmax())
    z = m if temperature == 0 else m / temperature + torch.from_numpy(gumbel64(noise_words(seed, stream, p, np.arange(lg.shape[0]))))
    top = z.topk(2)
    i = int(top.indices[0])
    return i, float(lg[i] - torch.logsumexp(m, 0)), float(top.values[0] - top.values[1]), lo.mass_margin(lg, pre, tb), greedy


def sample_ts(sd, cfg, enc, prefix, max_new, tb, eos, suppress=(), begin_suppress=(), max_initial=None, begin=None, no_speech_id=None,
              sot_pos=None, temperature=0.0, stream=0, seed=0):
    """lo.greedy_ts with a draw per step: fp64 decoding of ONE clip -> {"tokens", "scores", "draw_margins", "mass_margins", "greedy"
    (the argmax of every step's allowed set), "no_speech_prob"}; p is the context position of the id being chosen"""
    V, T = cfg["vocab"], cfg["n_text_ctx"]
    begin = len(prefix) if begin is None else begin
    d_all, d_begin = wo._deny(V, suppress), wo._deny(V, list(suppress) + list(begin_suppress))
    ids = list(prefix)
    r = {"tokens": [], "scores": [], "draw_margins": [], "mass_margins": [], "greedy": [], "no_speech_prob": None}
    E = sd["model.decoder.embed_tokens.weight"]
    for n in range(max(0, min(max_new, T - len(prefix)))):
        h = wo.decoder_hidden(sd, cfg, enc, torch.tensor([ids]))[0]
        if n == 0 and no_speech_id is not None:
            r["no_speech_prob"] = float(torch.softmax(h[sot_pos] @ E.T, 0)[no_speech_id])
        first = len(ids) == begin
        i, s, dm, mm, gr = sample_step(h[-1] @ E.T, ids[begin:], first, tb, eos, max_initial, d_begin if first else d_all, temperature, seed,
                                       stream, len(ids))
        r["tokens"].append(i); r["scores"].append(s); r["draw_margins"].append(dm); r["mass_margins"].append(mm); r["greedy"].append(gr)
        ids.append(i)
        if i == eos:
            break
    return r


def compression_ratio(text):
    b = text.encode("utf-8")
    return len(b) / len(zlib.compress(b))


def needs_fallback(ratio, avg, nosp, compression_ratio_threshold, logprob_threshold, no_speech_threshold):
    """openai/whisper transcribe.py decode_with_fallback"""
    need = False
    if compression_ratio_threshold is not None and ratio > compression_ratio_threshold:
        need = True
    if logprob_threshold is not None and avg < logprob_threshold:
        need = True
    if no_speech_threshold is not None and nosp > no_speech_threshold and logprob_threshold is not None and avg < logprob_threshold:
        need = False
    return need


def row_stream(clip, attempt, seek):
    return ((MAX_TEMPERATURES * clip + attempt) << 32) | seek


def transcribe_loop_fallback(decode_window, F, nseg, init, tb, eos, prev_sot, T, max_length, temperatures, text_of, clip=0, prompt_ids=None,
                             condition=True, no_speech_threshold=None, logprob_threshold=None, compression_ratio_threshold=None):
    """lo.transcribe_loop with decode_with_fallback per window.  decode_window(seek, nframes, prefix, max_new, temperature, attempt,
    stream) -> {"tokens" (a final eos included), "scores", "no_speech_prob"}; text_of(ids) -> the text whose compression is tested.
    Returns {"segments": [... + "temperature", "compression_ratio"], "windows": [... + "attempts": [{"temperature", "stream",
    "avg_logprob", "compression_ratio", "tokens"}], "reset"]}."""
    temperatures = tuple(temperatures)
    if len(temperatures) > MAX_TEMPERATURES:
        raise ValueError(f"{len(temperatures)} temperatures: at most {MAX_TEMPERATURES}")
    prompt = None
    if prompt_ids is not None:
        prompt = [int(t) for t in prompt_ids]
        prompt = prompt[1:] if prompt and prompt[0] == prev_sot else prompt
    history = [prompt] if prompt is not None and condition else []
    seek, segments, windows = 0, [], []
    while seek < F:
        nfr = min(F - seek, nseg)
        prefix = lo.build_prefix(init, history, condition, prompt if (prompt is not None and not condition and not windows) else None, tb, prev_sot, T)
        max_new = lo.token_budget(len(prefix), max_length, T)
        attempts = []
        for attempt, temp in enumerate(temperatures):
            stream = row_stream(clip, attempt, seek)
            r = decode_window(seek, nfr, prefix, max_new, temp, attempt, stream)
            toks = [int(t) for t in r["tokens"]]
            avg = float(sum(r["scores"])) / len(toks) if toks else 0.0
            ratio = compression_ratio(text_of([t for t in toks if t < eos]).strip())
            attempts.append({"temperature": temp, "stream": stream, "avg_logprob": avg, "compression_ratio": ratio, "tokens": toks,
                             "no_speech_prob": r["no_speech_prob"]})
            if not needs_fallback(ratio, avg, r["no_speech_prob"], compression_ratio_threshold, logprob_threshold, no_speech_threshold):
                break
        a = attempts[-1]
        toks, avg, temp = a["tokens"], a["avg_logprob"], a["temperature"]
        win = {"seek": seek, "prefix": prefix, "max_new": max_new, "tokens": toks, "avg_logprob": avg, "no_speech_prob": a["no_speech_prob"],
               "skip": False, "attempts": attempts, "temperature": temp, "reset": False}
        windows.append(win)
        if (no_speech_threshold is not None and logprob_threshold is not None and avg < logprob_threshold
                and a["no_speech_prob"] > no_speech_threshold):
            win["skip"], win["step"] = True, nfr
            seek += nfr
            continue
        body = toks[:-1] if toks and toks[-1] == eos else toks
        segs, step = lo.cut_segments(body, tb, seek, nfr)
        for s in segs:
            s.update(seek=seek, avg_logprob=avg, no_speech_prob=a["no_speech_prob"], temperature=temp, compression_ratio=a["compression_ratio"])
        segments += segs
        history += [s["tokens"] for s in segs]
        if temp > 0.5:                                   # prompt_reset_since: the next window carries no previous text
            history, win["reset"] = [], True
        win["step"] = step
        seek += step
    return {"segments": segments, "windows": windows}
