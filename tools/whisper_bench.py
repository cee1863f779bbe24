"""Whisper at the large-v3 shape (d 1280, 20 heads, 32 + 32 layers, 128 mels, vocabulary 51866) with recipe weights: the encoder
(tdx_whisper_encode, the cross K / V of the 32 decoder layers included) and the time of one decode step (tdx_whisper_decode) at
B = 1, 8 and 32.

    python tools/whisper_bench.py [--batches 1,8,32] [--layers 32] [--warmup 2] [--iters 7] [--steps 16,80] [--out profiles/whisper_bench.json]

The encoder is timed with device events.  A decode call waits for the device itself (one pinned word per 16 steps), so it is timed
with the host clock between two synchronisations; the step time is the difference of the medians of two calls that differ only in
the number of generated tokens (--steps), over that difference: the four prefix steps, the uploads and the call's fixed costs drop
out.  End-of-text is suppressed so that every clip runs every step.  Per figure: median, min, max and inter-quartile spread.

The yardstick of a step is its byte count, computed here from the shapes: the decoder's weights, the tied head and the cross K / V
every clip reads, over 6.0 TB/s (the HBM read-sweep rate of the MI355X).  `share_of_hbm_bound` is that time over the measured one.
`step_us_b_over_b1` says what the batch costs: the weights are read once per step whatever B is, the cross K / V once per clip.
The shader clock is read from the driver's pp_dpm_sclk table after the timed loops when the file is there ("not measured" otherwise).

This tool checks counts, never values.  The values at this width (d 1280, FFN 5120, 20 heads: K = 1280 and 5120 in every Linear, the
head and the LayerNorms) are checked against the fp64 oracle by tests/test_gpu_whisper_widths.py."""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_READ = 6.0e12


def stats(t):
    t = np.asarray(t, dtype=np.float64)
    q1, q3 = np.percentile(t, [25, 75])
    return {"median_us": round(float(np.median(t)), 1), "min_us": round(float(t.min()), 1), "max_us": round(float(t.max()), 1), "iqr_us": round(float(q3 - q1), 1)}


def shader_clock():
    for p in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            cur = [l for l in open(p).read().splitlines() if l.strip().endswith("*")]
            if cur:
                return cur[0].split(":")[1].strip().rstrip("*").strip()
        except OSError:
            pass
    return "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--steps", default="16,80")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from targetdiarization_amd.whisper import WhisperASR, decode_prefix, default_generation_config
    from targetdiarization_amd.weights import recipe_whisper_state_dict, whisper_config

    assert torch.cuda.is_available(), "the benchmark needs a HIP device"
    cfg = whisper_config(d_model=1280, enc_heads=20, enc_layers=a.layers, dec_layers=a.layers, n_mels=128, vocab=51866)
    t0 = time.perf_counter()
    m = WhisperASR(recipe_whisper_state_dict(0, cfg), cfg, "cuda:0")
    load_s = time.perf_counter() - t0
    gen = default_generation_config(cfg["vocab"])
    prefix = decode_prefix("chinese", "transcribe", None, gen)
    sup = list(gen["suppress_tokens"]) + [gen["eos_token_id"]]
    n1, n2 = (int(x) for x in a.steps.split(","))
    d, S, L, V, ffn = cfg["d_model"], cfg["n_audio_ctx"], cfg["dec_layers"], cfg["vocab"], cfg["dec_ffn"]
    weight_bytes = 4.0 * (L * (6.0 * d * d + 2.0 * d * ffn) + V * d)
    rows = []
    for B in (int(x) for x in a.batches.split(",")):
        g = torch.Generator().manual_seed(B)
        feats = (0.5 * torch.randn(B, cfg["n_mels"], 2 * S, generator=g)).to("cuda:0")
        for _ in range(a.warmup):
            _, state = m.encode(feats, with_state=True)
        torch.cuda.synchronize()
        te = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); _, state = m.encode(feats, with_state=True); e1.record()
            e1.synchronize()
            te.append(e0.elapsed_time(e1) * 1e3)
        td = {n1: [], n2: []}
        for n in (n1, n2):
            for _ in range(a.warmup):
                m.decode(state, prefix, n, sup, gen["begin_suppress_tokens"])
        for _ in range(a.iters):
            for n in (n1, n2):                              # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, _, cnt = m.decode(state, prefix, n, sup, gen["begin_suppress_tokens"])
                torch.cuda.synchronize()
                td[n].append((time.perf_counter() - t0) * 1e6)
        assert cnt.cpu().tolist() == [n2] * B
        s1, s2 = stats(td[n1]), stats(td[n2])
        step_us = (s2["median_us"] - s1["median_us"]) / (n2 - n1)
        step_bytes = weight_bytes + 4.0 * L * 2.0 * B * S * d
        bound_us = step_bytes / HBM_READ * 1e6
        enc = stats(te)
        enc["tflops"] = round(m.flops(B, 0) / (enc["median_us"] * 1e-6) / 1e12, 2)
        rows.append({"B": B, "encoder": enc, f"decode_{n1}_new": s1, f"decode_{n2}_new": s2, "step_us": round(step_us, 1),
                     "step_spread_us": round((s1["iqr_us"] + s2["iqr_us"]) / (n2 - n1), 2), "step_mbytes": round(step_bytes / 1e6, 1),
                     "weights_mbytes": round(weight_bytes / 1e6, 1), "cross_kv_mbytes": round((step_bytes - weight_bytes) / 1e6, 1),
                     "hbm_bound_us": round(bound_us, 1), "share_of_hbm_bound": round(bound_us / step_us, 4),
                     "launches_per_step": 3 + (10 if B <= 8 else 19) * L})
    for r in rows:
        r["step_us_b_over_b1"] = round(r["step_us"] / rows[0]["step_us"], 3)
    line = json.dumps({"workload": f"Whisper large-v3 shape, {a.layers} + {a.layers} layers, recipe weights, fp32; encoder by device events, decode step "
                                   f"= (median of {n2} new tokens - median of {n1}) / {n2 - n1} by the host clock between synchronisations",
                       "hbm_read_rate_assumed_tbs": HBM_READ / 1e12, "warmup": a.warmup, "iters": a.iters, "create_seconds": round(load_s, 1),
                       "shader_clock_after_the_loops": shader_clock(), "batches": rows})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
