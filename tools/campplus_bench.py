"""CAM++ diarizer end to end on the benchmark's 30 minutes: `CamppDiarizer(audio)` = window plan, ONE upload, the bucketed
embedding launches (tdx_fbank + tdx_campp_forward), spectral clustering on the host, time post-processing.

    python tools/campplus_bench.py [--seconds 1800] [--seed 0] [--warmup 1] [--iters 3] [--max-batch-frames 40000]
                                   [--profile DIR]

Workload: seeded 16 kHz audio (tests/campplus_oracle.py's three synthetic voices in 15 s turns), recipe weights with the calibrated
final BatchNorm.  Prints one JSON line: ms per call, the share of it spent in the device embedding (device events around
`embed`) and in host clustering (wall clock around `spectral_labels`), windows per second and FLOP/s of the embedding from
tdx_campp_flops.  --profile DIR: first runs itself once under `rocprofv3 --kernel-trace --stats` (a child process of its own) and
copies the kernel-stats CSV to DIR/campplus_kernel_stats.csv."""
from __future__ import annotations

import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def profile(a):
    tmp = tempfile.mkdtemp(prefix="campp_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
           "--seconds", str(a.seconds), "--seed", str(a.seed), "--warmup", "0", "--iters", "1", "--max-batch-frames", str(a.max_batch_frames)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("rocprofv3 run failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        raise SystemExit("rocprofv3 wrote no kernel_stats.csv under " + tmp)
    os.makedirs(a.profile, exist_ok=True)
    shutil.copy(found[0], os.path.join(a.profile, "campplus_kernel_stats.csv"))
    shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=1800)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--max-batch-frames", type=int, default=40000)
    ap.add_argument("--profile", default=None)
    a = ap.parse_args()
    if a.profile:
        profile(a)                      # before this process opens the device

    import torch
    import campplus_oracle as orc
    from targetdiarization_amd import clustering, diarization as dz

    rng = np.random.default_rng(a.seed)
    turn = 15 * 16000
    n = a.seconds * 16000
    audio = np.concatenate([orc.voice(i % 3, turn, rng) for i in range((n + turn - 1) // turn)])[:n]
    d = dz.CamppDiarizer(orc.calibrated_state_dict(), cuda_device=0, max_batch_frames=a.max_batch_frames)
    dev = d.embedder.device
    acc = {"embed_ms": 0.0, "cluster_ms": 0.0, "windows": 0}
    embed0, spectral0 = d.embed, dz.spectral_labels

    def embed(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = embed0(windows)           # ends with the download: the stream has drained
        e1.record(); e1.synchronize()
        acc["embed_ms"] += e0.elapsed_time(e1); acc["windows"] += len(windows)
        return out

    def spectral(X, **kw):
        t = time.perf_counter()
        out = spectral0(X, **kw)
        acc["cluster_ms"] += (time.perf_counter() - t) * 1e3
        return out

    d.embed, dz.spectral_labels = embed, spectral
    res = None
    for _ in range(a.warmup):
        res = d(audio)
    for k in acc:
        acc[k] = 0
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    for _ in range(a.iters):
        res = d(audio)
    ms = (time.perf_counter() - t0) * 1e3 / a.iters
    it = max(a.iters, 1)
    emb_ms, cl_ms, nw = acc["embed_ms"] / it, acc["cluster_ms"] / it, acc["windows"] // it
    F = 1 + (dz.WINDOW - 400) // 160
    flops = d.embedder.model.flops(1, F) * nw
    print(json.dumps({"workload": f"CamppDiarizer on {a.seconds} s of seeded 16 kHz audio (three synthetic voices, 15 s turns)",
                      "windows": nw, "frames_per_window": F, "ms": round(ms, 1), "x_real_time": round(a.seconds / (ms / 1e3), 1),
                      "embed_ms": round(emb_ms, 1), "embed_share": round(emb_ms / ms, 3),
                      "cluster_ms": round(cl_ms, 1), "cluster_share": round(cl_ms / ms, 3),
                      "windows_per_s_embed": round(nw / (emb_ms / 1e3), 1), "gflop_per_window": round(flops / nw / 1e9, 3),
                      "tflops_embed": round(flops / (emb_ms / 1e3) / 1e12, 2),
                      "speakers": len({r[2] for r in res["text"]}), "segments": len(res["text"]),
                      "max_batch_frames": a.max_batch_frames, "peak_device_mem_gb": round(torch.cuda.max_memory_allocated(dev) / 2**30, 2)}), flush=True)


if __name__ == "__main__":
    main()
