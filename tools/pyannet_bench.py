"""PyanNet forward (tdx_pyannet_forward: waveform norm, SincNet, 4-layer bidirectional LSTM, head, log-softmax) on 10 s chunks
already on the device, at three batch sizes: 1 (the stream class: one released buffer), 21 (a 30 s clip) and 64 (one full
launch of a long clip).

    python tools/pyannet_bench.py [--batches 1,21,64] [--warmup 3] [--iters 20] [--out FILE.json] [--lib LIBTDX.so]

--lib measures another build of the library, e.g. one compiled with -DTDX_PYANNET_REC_TILE=1 (the recurrence kernel's chunks
per workgroup; the JSON records the value the loaded library reports).

Weights: the calibrated recipe (tests/pyannet_oracle.py); chunks: the seeded synthetic clips (the kernels' time does not
depend on the values).  Device-event time of every forward on its own; prints one JSON line with, per batch: median, min, max
and the inter-quartile spread in microseconds, the real-time factor (forward time / audio time of the chunks), launches per
forward (a constant read off the forward's source, labelled so in the JSON), GFLOP/s from tdx_pyannet_flops and the workspace.
No threshold is set: the stage has no earlier time to compare with."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# read off tdx_pyannet_forward's source, not counted at run time: wav_stats + sinc + 3 x (stats, apply) + 2 conv GEMMs
# + 4 x (projection GEMM, recurrence) + 3 GEMMs + log-softmax
LAUNCHES = 22


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,21,64")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()

    import torch
    import pyannet_oracle as orc
    from targetdiarization_amd import _lib
    from targetdiarization_amd.segmentation import PyanNet
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)

    m = PyanNet(orc.calibrated_state_dict(), "cuda:0")
    dev = m.device
    T = orc.CHUNK
    base = np.stack([orc.clip(T, 7000 + i) for i in range(4)])
    res = []
    for B in (int(x) for x in a.batches.split(",")):
        x = torch.from_numpy(base[np.arange(B) % 4]).to(dev).contiguous()
        logp = torch.empty(B, m.frames(T), 7, device=dev)
        ws = torch.empty(m.workspace_bytes(B, T), dtype=torch.uint8, device=dev)
        for _ in range(a.warmup):
            m.forward_into(x, logp, None, None, ws)
        torch.cuda.synchronize()
        ts = []
        for _ in range(max(a.iters, 20)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); m.forward_into(x, logp, None, None, ws); e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts = np.array(ts)
        med = float(np.median(ts))
        q1, q3 = np.percentile(ts, [25, 75])
        res.append({"chunks": B, "samples": T, "iters": len(ts), "median_us": round(med, 1), "min_us": round(float(ts.min()), 1),
                    "max_us": round(float(ts.max()), 1), "iqr_us": round(float(q3 - q1), 1), "rtf": float(f"{med * 1e-6 / (B * T / 16000.0):.3e}"),
                    "us_per_launch": round(med / LAUNCHES, 1), "gflops": round(m.flops(B, T) / (med * 1e-6) / 1e9, 1),
                    "workspace_mb": round(m.workspace_bytes(B, T) / 2**20, 2)})
    line = json.dumps({"workload": "tdx_pyannet_forward, 10 s chunks on the device, device events per forward",
                       "launches_per_forward_from_source": LAUNCHES, "recurrence_chunk_tile": m.chunk_tile, "sizes": res})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    m.close()


if __name__ == "__main__":
    main()
