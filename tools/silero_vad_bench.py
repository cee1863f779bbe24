"""silero-VAD packed forward (tdx_silero_forward: windows, STFT, four convolutions, the LSTM chain, the head) at three shapes:
1 clip x 32 chunks (one 1 s stream chunk), 1 x 938 (a full 30 s buffer: what the stream class runs on every incoming chunk) and
32 x 313 (a batch of 10 s clips), audio already on the device.

    python tools/silero_vad_bench.py [--shapes 1x32,1x938,32x313] [--warmup 5] [--iters 30] [--out profiles/silero_vad_bench.json]

Weights: the recipe with the calibrated head (tests/silero_vad_oracle.py); audio: seeded N(0, 0.1) (the kernels' time does not
depend on the values).  Device-event time of every forward on its own; per shape: median, min, max and the inter-quartile
spread in microseconds, the real-time factor, microseconds per launch (launches: a constant read off the forward's source).
The recurrence alone: the same chunks are run again cut into as many clips as the limits allow (one chunk per clip up to 1024
clips), which shortens every chain and leaves the eight other launches' work unchanged; the difference of the two medians
divided by the steps taken off the longest chain is the time of one step of the chain.  Baseline, in the same run: the fp32
oracle on the CPU with 16 threads — the only other implementation there is.  No threshold is set."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# read off tdx_silero_forward's source, not counted at run time: window + STFT GEMM + 4 conv GEMMs + projection GEMM + recurrence + head
LAUNCHES = 9
W = 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x32,1x938,32x313")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import silero_vad_oracle as orc
    from targetdiarization_amd.silero import SileroVad

    torch.set_num_threads(16)
    sd = orc.calibrated_state_dict()
    m = SileroVad(sd, "cuda:0")
    dev = m.device

    def timed(wav, starts, total):
        nclips = len(starts) - 1
        st = torch.tensor(starts, dtype=torch.int32, device=dev)
        p = torch.empty(total, device=dev)
        ws = torch.empty(m.workspace_bytes(nclips, total), dtype=torch.uint8, device=dev)
        for _ in range(a.warmup):
            m.forward_into(wav, st, p, None, None, ws)
        torch.cuda.synchronize()
        ts = []
        for _ in range(max(a.iters, 20)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); m.forward_into(wav, st, p, None, None, ws); e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return np.array(ts)

    res = []
    for shape in a.shapes.split(","):
        nclips, per = (int(x) for x in shape.split("x"))
        total = nclips * per
        g = torch.Generator().manual_seed(total)
        host = torch.randn(total * W, generator=g) * 0.1
        wav = host.to(dev)
        ts = timed(wav, [c * per for c in range(nclips + 1)], total)
        short_clips = min(total, 1024)
        short_starts = [int(v) for v in np.linspace(0, total, short_clips + 1)]
        short_chain = max(b - a_ for a_, b in zip(short_starts, short_starts[1:]))
        tshort = timed(wav, short_starts, total)
        med, smed = float(np.median(ts)), float(np.median(tshort))
        q1, q3 = np.percentile(ts, [25, 75])
        t0 = time.perf_counter()
        for c in range(nclips):
            orc.forward(sd, host[c * per * W:(c + 1) * per * W].numpy(), torch.float32)
        cpu_us = (time.perf_counter() - t0) * 1e6
        res.append({"clips": nclips, "chunks_per_clip": per, "iters": len(ts), "median_us": round(med, 1), "min_us": round(float(ts.min()), 1),
                    "max_us": round(float(ts.max()), 1), "iqr_us": round(float(q3 - q1), 1), "rtf": float(f"{med * 1e-6 / (total * 0.032):.3e}"),
                    "us_per_launch": round(med / LAUNCHES, 1), "gflops": round(m.flops(total) / (med * 1e-6) / 1e9, 2),
                    "short_chain_clips": short_clips, "short_chain_steps": short_chain, "short_chain_median_us": round(smed, 1),
                    "recurrence_us_per_step": round((med - smed) / max(per - short_chain, 1), 3) if per > short_chain else None,
                    "cpu_oracle_fp32_16_threads_us": round(cpu_us, 1), "workspace_mb": round(m.workspace_bytes(nclips, total) / 2**20, 2)})
    line = json.dumps({"workload": "tdx_silero_forward, packed audio on the device, device events per forward",
                       "launches_per_forward_from_source": LAUNCHES, "shapes": res})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
