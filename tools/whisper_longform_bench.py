"""Whisper long-form transcription at the large-v3 shape (d 1280, 20 heads, 32 + 32 layers, 128 mels, vocabulary 51866, recipe
weights): what the timestamp rules, the per-row prefixes and the no-speech pair add to a decode step (tdx_whisper_decode_ts against
tdx_whisper_decode, measured in the same run, the two alternating) at B = 1, 8 and 32; tdx_whisper_logmel_long on 1800 s; and
WhisperASR.transcribe of one 1800 s clip end to end.

    python tools/whisper_longform_bench.py [--batches 1,8,32] [--layers 32] [--warmup 2] [--iters 7] [--steps 16,80] [--seconds 1800]
                                           [--package DIR] [--plain-only] [--out profiles/whisper_longform_bench.json]

The step time is tools/whisper_bench.py's: the difference of the medians of two calls that differ only in the number of generated
tokens, over that difference, by the host clock between synchronisations; end-of-text is suppressed.  The log-mel is timed with
device events, transcribe by the host clock.  transcribe's figures carry the number of windows, the mean prefix length per window
(the prefix is fed one id per step: mean prefix length x the step time is what a batched prefill could save per window) and the
steps run.

--package DIR imports targetdiarization_amd from another checkout (a build of the parent commit) and --plain-only times
tdx_whisper_decode alone: run that build and this build with --plain-only in one session for a like-for-like pair (the default
run alternates the two decode calls, which by itself moves the plain figure a little at B = 32)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.whisper_bench import shader_clock, stats  # noqa: E402

HEADS = [[7, 0], [10, 17], [12, 18], [13, 12], [16, 1], [17, 14], [19, 11], [21, 4], [24, 1], [25, 6]]      # as tools/whisper_timestamps_bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--steps", default="16,80")
    ap.add_argument("--seconds", type=int, default=1800)
    ap.add_argument("--package", default=None)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.package:
        sys.path.insert(0, os.path.abspath(a.package))

    import torch
    import targetdiarization_amd
    from targetdiarization_amd.whisper import WhisperASR, decode_prefix, default_generation_config
    from targetdiarization_amd.weights import recipe_whisper_state_dict, whisper_config

    assert torch.cuda.is_available(), "the benchmark needs a HIP device"
    cfg = whisper_config(d_model=1280, enc_heads=20, enc_layers=a.layers, dec_layers=a.layers, n_mels=128, vocab=51866)
    heads = [[min(l, a.layers - 1), h] for l, h in HEADS]
    m = WhisperASR(recipe_whisper_state_dict(0, cfg), cfg, "cuda:0", alignment_heads=heads)
    gen = default_generation_config(cfg["vocab"])
    prefix = decode_prefix("chinese", "transcribe", None, gen)
    sup = list(gen["suppress_tokens"]) + [gen["eos_token_id"]]
    beg = gen["begin_suppress_tokens"]
    n1, n2 = (int(x) for x in a.steps.split(","))
    S = cfg["n_audio_ctx"]

    rows = []
    for B in (int(x) for x in a.batches.split(",")):
        g = torch.Generator().manual_seed(B)
        feats = (0.5 * torch.randn(B, cfg["n_mels"], 2 * S, generator=g)).to("cuda:0")
        _, state = m.encode(feats, with_state=True)
        calls = {"plain": lambda n: m.decode(state, prefix, n, sup, beg)}
        if not a.plain_only:                                # the same four-id prefix in every row, <|notimestamps|> included: the step count is the plain call's
            calls["ts"] = lambda n: m.decode_ts(state, [prefix] * B, n, sup, beg, sot_pos=[0] * B)
        td = {(k, n): [] for k in calls for n in (n1, n2)}
        for n in (n1, n2):
            for _ in range(a.warmup):
                for fn in calls.values():
                    fn(n)
        for _ in range(a.iters):
            for n in (n1, n2):                              # alternating, the two calls side by side
                for k, fn in calls.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = fn(n)
                    torch.cuda.synchronize()
                    td[(k, n)].append((time.perf_counter() - t0) * 1e6)
                    assert out[2].cpu().tolist() == [n] * B
        st = {k: stats(v) for k, v in td.items()}
        row = {"B": B}
        for k in calls:
            row[f"step_us_{k}"] = round((st[(k, n2)]["median_us"] - st[(k, n1)]["median_us"]) / (n2 - n1), 1)
            row[f"step_spread_us_{k}"] = round((st[(k, n1)]["iqr_us"] + st[(k, n2)]["iqr_us"]) / (n2 - n1), 2)
            row[f"decode_{n2}_new_{k}"] = st[(k, n2)]
        if "ts" in calls:
            row["ts_adds_us"] = round(row["step_us_ts"] - row["step_us_plain"], 1)
            row["ts_adds_percent"] = round(100.0 * (row["step_us_ts"] / row["step_us_plain"] - 1.0), 2)
        rows.append(row)
        print(f"B = {B}: {row}", file=sys.stderr, flush=True)
        del state
    res = {"workload": f"Whisper large-v3 shape, {a.layers} + {a.layers} layers, recipe weights, fp32; decode step = (median of {n2} new tokens - median of "
                       f"{n1}) / {n2 - n1} by the host clock, tdx_whisper_decode and tdx_whisper_decode_ts alternating in one run",
           "package": os.path.relpath(os.path.dirname(os.path.abspath(targetdiarization_amd.__file__)), ROOT), "warmup": a.warmup, "iters": a.iters, "batches": rows}
    if not a.plain_only:
        wav = 0.1 * torch.randn(16000 * a.seconds, generator=torch.Generator().manual_seed(7))
        wav_dev = wav.to("cuda:0")
        for _ in range(a.warmup):
            m.features_long(wav_dev)
        t = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f = m.features_long(wav_dev); e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3)
        res[f"logmel_long_{a.seconds}_s"] = dict(stats(t), frames=int(f.shape[1]),
                                                 workspace_mbytes=round(int(m._l.tdx_whisper_logmel_long_workspace_bytes(m._h, wav.shape[0])) / 1e6, 2))
        log = []
        real = m.decode_ts

        def counted(state, prefixes, max_new, *args, **kw):
            out = real(state, prefixes, max_new, *args, **kw)
            log.append((len(prefixes[0]), int(out[2][0])))
            return out
        m.decode_ts = counted
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = m.transcribe([wav_dev], language="en")[0]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        del m.decode_ts
        step1 = next((row["step_us_ts"] for row in rows if row["B"] == 1), None)
        mean_prefix = sum(p for p, _ in log) / max(1, len(log))
        res[f"transcribe_{a.seconds}_s"] = {"seconds": round(dt, 2), "windows": len(log), "segments": len(r["segments"]), "mean_prefix_len": round(mean_prefix, 1),
                                            "prefix_steps": sum(p for p, _ in log), "generated_steps": sum(n for _, n in log),
                                            "prefix_feed_ms_per_window_at_the_B1_step": round(mean_prefix * step1 / 1e3, 1) if step1 else "not measured"}
    res["shader_clock_after_the_loops"] = shader_clock()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
