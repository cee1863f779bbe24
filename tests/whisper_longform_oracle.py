"""Plain-torch restatement, in fp64, of Whisper's long-form transcription as Hugging Face transformers runs it
(`generate(..., return_timestamps=True)` on more than 30 s: generation_whisper.py steps 4-7, WhisperTimeStampLogitsProcessor,
WhisperNoSpeechDetection, WhisperFeatureExtractor(truncation=False)): the timestamp rules as a function of (logits, history), the
long feature extractor, the cutting of a window's ids into segments, and the whole loop over a model given as a callable.
tests/test_whisper_longform_host.py pins every function here to the installed upstream; the GPU tests use only this file and
whisper_oracle.py.  One clip per call, temperature 0 (no fallback, no compression-ratio test)."""
from __future__ import annotations

import torch

import whisper_oracle as wo

TIME_PRECISION = 0.02           # seconds per encoder position = per timestamp id
INPUT_STRIDE = 2                # feature frames per encoder position


def history_rules(V, seq, first_step, tb, eos, max_initial=None, deny=None):
    """the part of the rules that does not look at the logits -> bool [V] allowed"""
    ok = torch.ones(V, dtype=torch.bool) if deny is None else ~torch.as_tensor(deny).clone()
    ok[tb - 1] = False
    seq = [int(t) for t in seq]
    last = len(seq) >= 1 and seq[-1] >= tb
    pen = len(seq) < 2 or seq[-2] >= tb
    if last:
        if pen:
            ok[tb:] = False
        else:
            ok[:eos] = False
    stamps = [t for t in seq if t >= tb]
    if stamps:
        ok[tb:(stamps[-1] if last and not pen else stamps[-1] + 1)] = False
    if first_step:
        ok[:tb] = False
        if max_initial is not None:
            ok[tb + max_initial + 1:] = False
    return ok


def ts_rules(logits, seq, first_step, tb, eos, max_initial=None, deny=None):
    """logits [V] (any float dtype; computed in fp64), seq: the ids generated so far, first_step: the id to come is the first
    generated one, deny: bool [V] of the static suppress masks (applied before the rules) -> bool [V], the ids still allowed
    after WhisperTimeStampLogitsProcessor"""
    lg = torch.as_tensor(logits).double()
    ok = history_rules(lg.shape[0], seq, first_step, tb, eos, max_initial, deny)
    m = lg.masked_fill(~ok, float("-inf"))
    if float(torch.logsumexp(m[tb:], 0)) > float(m[:tb].max()):
        ok[:tb] = False
    return ok


def mass_margin(logits, ok_before_mass, tb):
    """|log-sum-exp of the allowed timestamp logits - the best allowed text logit|; inf when either class is empty"""
    m = torch.as_tensor(logits).double().masked_fill(~ok_before_mass, float("-inf"))
    a, b = float(torch.logsumexp(m[tb:], 0)), float(m[:tb].max())
    return abs(a - b) if a > float("-inf") and b > float("-inf") else float("inf")


def ts_step(logits, seq, first_step, tb, eos, max_initial=None, deny=None):
    """one decision: (id, its log-softmax over what remains, margin): the margin is the smaller of the top-2 gap of the final
    set and the distance of the mass test from its tipping point"""
    lg = torch.as_tensor(logits).double()
    ok = ts_rules(lg, seq, first_step, tb, eos, max_initial, deny)
    pre = history_rules(lg.shape[0], seq, first_step, tb, eos, max_initial, deny)
    m = lg.masked_fill(~ok, float("-inf"))
    top = m.topk(2)
    gap = float(top.values[0] - top.values[1])
    return int(top.indices[0]), float(top.values[0] - torch.logsumexp(m, 0)), min(gap, mass_margin(lg, pre, tb))


def reflect_index(q, N):
    """numpy's "reflect" about 0 and N - 1, as often as it takes"""
    if N == 1:
        return torch.zeros_like(q)
    period = 2 * (N - 1)
    j = q % period
    return torch.where(j >= N, period - j, j)


def logmel_long(wav, n_mels, dtype=torch.float64):
    """WhisperFeatureExtractor(truncation=False, padding="longest") on one clip -> [n_mels, N // 160]; the clamp is the clip's"""
    x = torch.as_tensor(wav).reshape(-1).to(dtype)
    N = x.shape[0]
    F = N // 160
    if F == 0:
        return torch.zeros(n_mels, 0, dtype=dtype)
    xp = x[reflect_index(torch.arange(-200, N + 200), N)]
    frames = xp.unfold(0, 400, 160)[:F] * torch.hann_window(400, periodic=True, dtype=dtype)
    spec = torch.fft.rfft(frames, dim=1)
    power = (spec.real ** 2 + spec.imag ** 2).T
    lm = torch.log10(torch.clamp(wo.mel_filters(n_mels, dtype) @ power, min=1e-10))
    lm = torch.maximum(lm, lm.max() - 8.0)
    return (lm + 4.0) / 4.0


def window(feat, seek, nseg):
    """_get_input_segment: [n_mels, nseg] from frame `seek`, zero-padded in the feature domain"""
    n = min(feat.shape[1] - seek, nseg)
    out = torch.zeros(feat.shape[0], nseg, dtype=feat.dtype)
    out[:, :n] = feat[:, seek:seek + n]
    return out


def cut_segments(tokens, tb, seek, seek_num_frames):
    """_retrieve_segment on a window's generated ids (no eos) -> ([{"start", "end", "tokens"}], seek step in frames)"""
    tokens = [int(t) for t in tokens]
    t0 = seek * TIME_PRECISION / INPUT_STRIDE
    is_ts = [t >= tb for t in tokens]
    single_end = is_ts[-2:] == [False, True]
    pairs = [i + 1 for i in range(len(tokens) - 1) if is_ts[i] and is_ts[i + 1]]
    if pairs:
        slices = list(pairs)
        if single_end:
            slices.append(len(tokens))
        else:
            slices[-1] += 1
        segs, lo = [], 0
        for k, hi in enumerate(slices):
            sl = tokens[lo:hi]
            end_at = -1 if (k < len(slices) - 1 or single_end) else -2
            segs.append({"start": t0 + (sl[0] - tb) * TIME_PRECISION, "end": t0 + (sl[end_at] - tb) * TIME_PRECISION, "tokens": sl})
            lo = hi
        step = seek_num_frames if single_end else (tokens[lo - 2] - tb) * INPUT_STRIDE
        return segs, step
    stamps = [t for t in tokens if t >= tb]
    last = int(seek_num_frames * 0.01 / TIME_PRECISION)
    if stamps and stamps[-1] != tb:
        last = stamps[-1] - tb
    return [{"start": t0, "end": t0 + last * TIME_PRECISION, "tokens": tokens}], seek_num_frames


def build_prefix(init, segments, condition, prompt_first, tb, prev_sot, T):
    """_prepare_decoder_input_ids for one clip: `segments` the token lists so far (a first-segment prompt, without its
    <|startofprev|>, is the first of them)"""
    if condition and segments:
        ids = []
        for s in segments:
            ids += list(s[:-1]) if len(s) > 2 and s[-2] >= tb else list(s)
        return [prev_sot] + ids[-(T // 2 - 1):] + list(init)
    if prompt_first is not None:
        return [prev_sot] + list(prompt_first) + list(init)
    return list(init)


def token_budget(prefix_len, max_length, T):
    """_set_max_new_tokens_and_length with max_new_tokens unset: the total length allowed, minus the prefix"""
    total = min(max_length + min(T // 2 - 1, prefix_len), T)
    return max(0, total - prefix_len)


def transcribe_loop(decode_window, F, nseg, init, tb, eos, prev_sot, T, max_length, prompt_ids=None, condition=True,
                    no_speech_threshold=None, logprob_threshold=None):
    """generate's step 6 for one clip of F feature frames.  decode_window(seek, nframes, prefix, max_new) -> {"tokens" (a final eos
    included), "scores", "no_speech_prob"}.  A prompt conditions the first window only.  Returns {"segments": [...], "windows": [...]}:
    every window's seek, prefix, budget, skip flag, avg_logprob and seek step."""
    prompt = None
    if prompt_ids is not None:
        prompt = [int(t) for t in prompt_ids]
        prompt = prompt[1:] if prompt and prompt[0] == prev_sot else prompt
    history = [prompt] if prompt is not None and condition else []
    seek, segments, windows = 0, [], []
    while seek < F:
        nfr = min(F - seek, nseg)
        prefix = build_prefix(init, history, condition, prompt if (prompt is not None and not condition and not windows) else None, tb, prev_sot, T)
        max_new = token_budget(len(prefix), max_length, T)
        r = decode_window(seek, nfr, prefix, max_new)
        toks = [int(t) for t in r["tokens"]]
        avg = float(sum(r["scores"])) / len(toks) if toks else 0.0
        win = {"seek": seek, "prefix": prefix, "max_new": max_new, "tokens": toks, "avg_logprob": avg, "no_speech_prob": r["no_speech_prob"], "skip": False}
        windows.append(win)
        if (no_speech_threshold is not None and logprob_threshold is not None and avg < logprob_threshold
                and r["no_speech_prob"] > no_speech_threshold):
            win["skip"], win["step"] = True, nfr
            seek += nfr
            continue
        body = toks[:-1] if toks and toks[-1] == eos else toks
        segs, step = cut_segments(body, tb, seek, nfr)
        for s in segs:
            s.update(seek=seek, avg_logprob=avg, no_speech_prob=r["no_speech_prob"])
        segments += segs
        history += [s["tokens"] for s in segs]
        win["step"] = step
        seek += step
    return {"segments": segments, "windows": windows}


def greedy_ts(sd, cfg, enc, prefix, max_new, tb, eos, suppress=(), begin_suppress=(), max_initial=None, begin=None, no_speech_id=None,
              sot_pos=None):
    """fp64 greedy decoding of ONE clip (enc [1, S, d]) under the timestamp rules: {"tokens", "scores", "margins", "no_speech_prob"}"""
    V, T = cfg["vocab"], cfg["n_text_ctx"]
    begin = len(prefix) if begin is None else begin
    d_all, d_begin = wo._deny(V, suppress), wo._deny(V, list(suppress) + list(begin_suppress))
    ids = list(prefix)
    r = {"tokens": [], "scores": [], "margins": [], "no_speech_prob": None}
    E = sd["model.decoder.embed_tokens.weight"]
    for n in range(max(0, min(max_new, T - len(prefix)))):
        h = wo.decoder_hidden(sd, cfg, enc, torch.tensor([ids]))[0]
        if n == 0 and no_speech_id is not None:
            r["no_speech_prob"] = float(torch.softmax(h[sot_pos] @ E.T, 0)[no_speech_id])
        first = len(ids) == begin
        i, s, m = ts_step(h[-1] @ E.T, ids[begin:], first, tb, eos, max_initial, d_begin if first else d_all)
        r["tokens"].append(i); r["scores"].append(s); r["margins"].append(m)
        ids.append(i)
        if i == eos:
            break
    return r
