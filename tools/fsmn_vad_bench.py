"""FSMN-VAD packed forward (tdx_fsmnvad_forward: LFR + CMVN, the network, softmax) at two sizes: 300 frames (one 3 s stream
chunk) and 180 000 frames (30 minutes), fbank frames already on the device.

    python tools/fsmn_vad_bench.py [--frames 300,180000] [--clips 1] [--warmup 5] [--iters 30] [--out FILE.json]

Weights: the recipe with the calibrated CMVN and silence row (tests/fsmn_vad_oracle.py); features: seeded N(0,1) scaled to the
level of real log-mel frames (the kernels' time does not depend on the values).  Device-event time of every forward on its
own; prints one JSON line with, per size: median, min, max and the inter-quartile spread in microseconds, the real-time
factor (forward time / audio time), launches per forward (a constant read off the forward's source, labelled so in the JSON) and GFLOP/s from tdx_fsmnvad_flops.  No threshold is set: the stage has
no earlier time to compare with."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# read off tdx_fsmnvad_forward's source, not counted at run time: lfr_cmvn + GEMM + 4 x (GEMM, memory, GEMM) + GEMM + softmax
LAUNCHES = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="300,180000")
    ap.add_argument("--clips", type=int, default=1, help="clips the frames are split into (equal parts)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import fsmn_vad_oracle as orc
    from targetdiarization_amd.vad import FsmnVad

    sd, cmvn = orc.calibrated_state_dict()
    m = FsmnVad(sd, cmvn, "cuda:0")
    dev = m.device
    res = []
    for rows in (int(x) for x in a.frames.split(",")):
        g = torch.Generator().manual_seed(rows)
        feat = (torch.randn(rows, 80, generator=g) * 3.0 + 8.0).to(dev)
        starts = torch.tensor(np.linspace(0, rows, a.clips + 1).astype(np.int32), device=dev)
        p0 = torch.empty(rows, device=dev)
        ws = torch.empty(m.workspace_bytes(rows), dtype=torch.uint8, device=dev)
        for _ in range(a.warmup):
            m.forward_into(feat, starts, p0, None, ws)
        torch.cuda.synchronize()
        ts = []
        for _ in range(max(a.iters, 20)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); m.forward_into(feat, starts, p0, None, ws); e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts = np.array(ts)
        med = float(np.median(ts))
        q1, q3 = np.percentile(ts, [25, 75])
        res.append({"frames": rows, "clips": a.clips, "iters": len(ts), "median_us": round(med, 1), "min_us": round(float(ts.min()), 1),
                    "max_us": round(float(ts.max()), 1), "iqr_us": round(float(q3 - q1), 1), "rtf": float(f"{med * 1e-6 / (rows * 0.01):.3e}"),
                    "us_per_launch": round(med / LAUNCHES, 1), "gflops": round(m.flops(rows) / (med * 1e-6) / 1e9, 1),
                    "workspace_mb": round(m.workspace_bytes(rows) / 2**20, 2)})
    line = json.dumps({"workload": "tdx_fsmnvad_forward, packed fbank frames on the device, device events per forward",
                       "launches_per_forward_from_source": LAUNCHES, "sizes": res})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
