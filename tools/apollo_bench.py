"""Apollo restorer throughput in hot loop B's form: `restore_audio(keep_sampling_rate=True)` on separated 16 kHz streams —
resample to 44.1 kHz, restore, resample back (AudioProcessor.restore_streams_device: one batched restorer call).

    python tools/apollo_bench.py [--streams 64] [--min-s 1] [--max-s 10] [--seed 0] [--warmup 2] [--iters 5]
                                 [--layers 6] [--rows-per-launch 524288]

Default workload: 64 mono streams resident on the device, lengths uniform in [1, 10] s from a seeded generator (~350 s of audio),
recipe weights.  Prints one JSON line: ms per call (device events), x real time, end-to-end TFLOP/s from the model FLOPs
(ApolloRestorer.flops of the 44.1 kHz lengths), the restorer alone (already resampled streams), and the peak device memory."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from targetdiarization_amd.audio_processor import AudioProcessor          # noqa: E402
from targetdiarization_amd.weights import recipe_apollo_state_dict, recipe_wave   # noqa: E402


def timed(fn, warmup: int, iters: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--streams", type=int, default=64)
    ap_.add_argument("--min-s", type=float, default=1.0)
    ap_.add_argument("--max-s", type=float, default=10.0)
    ap_.add_argument("--seed", type=int, default=0)
    ap_.add_argument("--warmup", type=int, default=2)
    ap_.add_argument("--iters", type=int, default=5)
    ap_.add_argument("--layers", type=int, default=6)
    ap_.add_argument("--rows-per-launch", type=int, default=1 << 19)
    a = ap_.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(a.seed)
    lens = [int(s * 16000) for s in rng.uniform(a.min_s, a.max_s, a.streams)]
    streams = [torch.from_numpy(recipe_wave(f"apollo-bench{i}", 1, n, amp=0.3)[0]).to(dev) for i, n in enumerate(lens)]
    ap = AudioProcessor(is_restore_audio=True, restorer_state_dict=recipe_apollo_state_dict(0, a.layers), cuda_device=0, verbose_log=False)
    assert ap.is_restore_audio, "restorer failed to initialise"
    ap.restorer.max_frames = a.rows_per_launch // 80
    ups = ap._resample_many(streams, 16000, 44100)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    ms = timed(lambda: ap.restore_streams_device(streams, 16000), a.warmup, a.iters)
    peak = torch.cuda.max_memory_allocated(dev)
    ms_model = timed(lambda: ap.restorer(ups), 1, a.iters)
    audio_s = sum(lens) / 16000.0
    flops = ap.restorer.flops([int(u.shape[0]) for u in ups])
    print(json.dumps({"workload": f"apollo restore_audio loop B: {a.streams} x U[{a.min_s},{a.max_s}] s @16 kHz, {a.layers} layers",
                      "audio_s": round(audio_s, 2), "ms": round(ms, 2), "x_real_time": round(audio_s / (ms / 1e3), 1),
                      "tflops_end_to_end": round(flops / (ms / 1e3) / 1e12, 2), "ms_restorer_only": round(ms_model, 2),
                      "tflops_restorer_only": round(flops / (ms_model / 1e3) / 1e12, 2), "model_gflop": round(flops / 1e9, 1),
                      "launches": len(ap.restorer.plan([int(u.shape[0]) for u in ups])), "rows_per_launch": a.rows_per_launch,
                      "peak_device_mem_gb": round(peak / 2**30, 2)}), flush=True)


if __name__ == "__main__":
    main()
