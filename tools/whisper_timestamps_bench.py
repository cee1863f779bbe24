"""Whisper word timestamps at the large-v3 shape (d 1280, 20 heads, 32 + 32 layers, 128 mels, vocabulary 51866, recipe weights) with
10 alignment heads: what the capture of their cross-attention rows adds to a decode step (tdx_whisper_decode_xattn against
tdx_whisper_decode, measured in the same run, the two alternating) and what tdx_token_align costs, at B = 1, 8 and 32.

    python tools/whisper_timestamps_bench.py [--batches 1,8,32] [--layers 32] [--warmup 2] [--iters 7] [--steps 16,80] [--out profiles/whisper_timestamps.json]

The step time is tools/whisper_bench.py's: the difference of the medians of two calls that differ only in the number of generated
tokens, over that difference, by the host clock between synchronisations; end-of-text is suppressed.  tdx_token_align is timed with
device events: on the rows the longer decode captured (next to that decode's total time), and on synthetic attention at
(447 rows, 1500 frames) and (60, 1500).  For contrast transformers' _dynamic_time_warping runs once on the host at (447, 1500).
The capture's byte count per step is B x heads x 1500 x (64 floats of K read + the row written once; the softmax passes stay in
LDS) x 4."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.whisper_bench import shader_clock, stats  # noqa: E402

# ten (layer, head) pairs on ten layers of the upper two thirds, as the published large-v3 configuration has them in number and
# spread; which pairs they are does not change the work
HEADS = [[7, 0], [10, 17], [12, 18], [13, 12], [16, 1], [17, 14], [19, 11], [21, 4], [24, 1], [25, 6]]


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
    from targetdiarization_amd.whisper import WhisperASR, decode_prefix, default_generation_config, token_align
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
    S, nh = cfg["n_audio_ctx"], len(heads)

    def time_align(x, nrows, nframes):
        for _ in range(a.warmup):
            token_align(x, nrows, nframes)
        t = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); token_align(x, nrows, nframes); e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3)
        return stats(t)

    rows = []
    for B in (int(x) for x in a.batches.split(",")):
        g = torch.Generator().manual_seed(B)
        feats = (0.5 * torch.randn(B, cfg["n_mels"], 2 * S, generator=g)).to("cuda:0")
        _, state = m.encode(feats, with_state=True)
        bufs = {n: torch.zeros(B, nh, max(1, n - 1), S, device="cuda:0") for n in (n1, n2)}
        plain = lambda n: m.decode(state, prefix, n, sup, beg)
        capt = lambda n: m.decode_xattn(state, prefix, n, sup, beg, xattn=bufs[n])
        td = {(k, n): [] for k in ("plain", "capture") for n in (n1, n2)}
        for n in (n1, n2):
            for _ in range(a.warmup):
                plain(n); capt(n)
        for _ in range(a.iters):
            for n in (n1, n2):                              # alternating, the parent's call and the capturing one side by side
                for k, fn in (("plain", plain), ("capture", capt)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = fn(n)
                    torch.cuda.synchronize()
                    td[(k, n)].append((time.perf_counter() - t0) * 1e6)
        assert out[2].cpu().tolist() == [n2] * B
        st = {k: stats(v) for k, v in td.items()}
        step = {k: (st[(k, n2)]["median_us"] - st[(k, n1)]["median_us"]) / (n2 - n1) for k in ("plain", "capture")}
        spread = {k: (st[(k, n1)]["iqr_us"] + st[(k, n2)]["iqr_us"]) / (n2 - n1) for k in ("plain", "capture")}
        row = {"B": B, "step_us_plain": round(step["plain"], 1), "step_us_capture": round(step["capture"], 1),
               "step_spread_us_plain": round(spread["plain"], 2), "step_spread_us_capture": round(spread["capture"], 2),
               "capture_adds_us": round(step["capture"] - step["plain"], 1), "capture_adds_percent": round(100.0 * (step["capture"] / step["plain"] - 1.0), 2),
               "capture_mbytes_per_step": round(B * nh * S * (64 + 1) * 4 / 1e6, 1),
               f"decode_{n2}_new_plain": st[("plain", n2)], f"decode_{n2}_new_capture": st[("capture", n2)],
               f"align_of_the_{n2 - 1}_captured_rows": time_align(bufs[n2], [n2 - 1] * B, [S] * B)}
        for nr in (447, 60):
            x = torch.softmax(4.0 * torch.randn(B, nh, nr, S, generator=torch.Generator(device="cuda:0").manual_seed(nr + B), device="cuda:0"), dim=-1)
            row[f"align_{nr}_rows_{S}_frames"] = time_align(x, [nr] * B, [S] * B)
            del x
        rows.append(row)
        del bufs
    host = "not measured"
    try:
        from transformers.models.whisper.generation_whisper import _dynamic_time_warping
        M = np.random.default_rng(0).standard_normal((447, 1500))
        t0 = time.perf_counter()
        _dynamic_time_warping(-M)
        host = round(time.perf_counter() - t0, 3)
    except ImportError:
        pass
    line = json.dumps({"workload": f"Whisper large-v3 shape, {a.layers} + {a.layers} layers, recipe weights, fp32, {nh} alignment heads; decode step = (median of "
                                   f"{n2} new tokens - median of {n1}) / {n2 - n1} by the host clock, plain and capturing calls alternating in one run; "
                                   "tdx_token_align by device events",
                       "warmup": a.warmup, "iters": a.iters, "shader_clock_after_the_loops": shader_clock(),
                       "host_dynamic_time_warping_447x1500_seconds": host, "batches": rows})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
