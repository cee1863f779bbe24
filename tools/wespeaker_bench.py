"""WeSpeaker ResNet34 forward with masked pooling (tdx_wespk_forward: stem, 33 convolutions + 3 shortcuts, pooling under 3
masks, seg_1) at the pipeline's sizes: 1, 21 and 64 chunks of 998 frames x 3 masks of 589 frames (the stream class, a 30 s
buffer, a long clip's batch), features and masks already on the device, cut into launches of at most --cap chunks as the host
class does (64 chunks: four launches of 16).

    python tools/wespeaker_bench.py [--chunks 1,21,64] [--cap 16] [--warmup 5] [--iters 30] [--out profiles/wespeaker_bench.json]

Two models from the same weights are held in one process, one created under TDX_WESPK_NARROW=0 (the 13 stride-1 3x3
convolutions of the 32- and 64-channel stages on the shared GEMM core) and one under TDX_WESPK_NARROW=1 (conv3x3_narrow_kernel);
their timed forwards alternate (--only narrow | shared_core times one of them alone, for a kernel trace).  Device-event
time of every forward (all its launches) on its own; per size and setting: median, min, max and the inter-quartile spread in microseconds, and the algorithmic TFLOP/s (speaker.WeSpeakerResNet34.flops
over the median; one trunk pass per chunk).  The narrow kernel keeps the default only if its median is lower than the
shared core's at both 21 and 64 chunks by more than the sum of the two spreads; the verdict is printed with the figures."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F, S, FW = 998, 3, 589


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", default="1,21,64")
    ap.add_argument("--cap", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--only", default=None, choices=("narrow", "shared_core"), help="time one setting alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import wespeaker_oracle as orc
    from targetdiarization_amd import _lib
    from targetdiarization_amd.speaker import WeSpeakerResNet34

    assert torch.cuda.is_available(), "the benchmark needs a HIP device"
    sd = orc.calibrated_state_dict()
    os.environ["TDX_WESPK_NARROW"] = "0"
    shared = WeSpeakerResNet34(sd, "cuda:0", max_chunks_per_launch=a.cap)
    os.environ["TDX_WESPK_NARROW"] = "1"
    narrow = WeSpeakerResNet34(sd, "cuda:0", max_chunks_per_launch=a.cap)
    del os.environ["TDX_WESPK_NARROW"]
    models = {"narrow": narrow, "shared_core": shared}
    if a.only:
        models = {a.only: models[a.only]}
    dev = narrow.device
    l = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream

    res = []
    for B in (int(x) for x in a.chunks.split(",")):
        base = orc.shape_feat(1, F)[0]
        feat = torch.stack([base * (1.0 + 0.01 * b) for b in range(B)]).to(dev).contiguous()
        g = torch.Generator().manual_seed(B)
        w = (torch.rand(B, S, FW, generator=g) > 0.4).float().to(dev).contiguous()
        out = torch.empty(B, S, 256, device=dev)
        cuts = [(b0, min(a.cap, B - b0)) for b0 in range(0, B, a.cap)]
        ws = torch.empty(narrow.workspace_bytes(cuts[0][1], F, S), dtype=torch.uint8, device=dev)

        def forward(m):
            for b0, nb in cuts:
                _lib.check(l.tdx_wespk_forward(m._h, feat[b0:b0 + nb].data_ptr(), nb, F, w[b0:b0 + nb].data_ptr(), S, FW,
                                               out[b0:b0 + nb].data_ptr(), ws.data_ptr(), ws.numel(), st))
        ts = {k: [] for k in models}
        for k, m in models.items():
            for _ in range(a.warmup):
                forward(m)
        torch.cuda.synchronize()
        for _ in range(a.iters):
            for k, m in models.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); forward(m); e1.record()
                e1.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3)
        row = {"chunks": B, "launches_of": [nb for _, nb in cuts], "iters": a.iters, "gflop": round(narrow.flops(B, F) / 1e9, 1),
               "workspace_mb": round(ws.numel() / 2**20, 1)}
        for k in models:
            t = np.array(ts[k])
            q1, q3 = np.percentile(t, [25, 75])
            med = float(np.median(t))
            row[k] = {"median_us": round(med, 1), "min_us": round(float(t.min()), 1), "max_us": round(float(t.max()), 1),
                      "iqr_us": round(float(q3 - q1), 1), "tflops": round(narrow.flops(B, F) / (med * 1e-6) / 1e12, 2),
                      "share_of_157_tflops_fp32_mfma_peak": round(narrow.flops(B, F) / (med * 1e-6) / 157e12, 4)}
        if a.only:
            res.append(row)
            continue
        row["shared_minus_narrow_us"] = round(row["shared_core"]["median_us"] - row["narrow"]["median_us"], 1)
        row["sum_of_iqrs_us"] = round(row["shared_core"]["iqr_us"] + row["narrow"]["iqr_us"], 1)
        row["narrow_wins"] = bool(row["shared_minus_narrow_us"] > row["sum_of_iqrs_us"])
        res.append(row)
    judged = [r for r in res if r["chunks"] in (21, 64)]
    verdict = None if (a.only or len(judged) < 2) else bool(all(r["narrow_wins"] for r in judged))
    line = json.dumps({"workload": f"tdx_wespk_forward, {F} frames x {S} masks of {FW} per chunk, on the device, device events per forward",
                       "cap": a.cap, "sizes": res, "narrow_keeps_the_default": verdict})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
