"""emotion2vec on the device (tdx_emo2v_forward: clip statistics, conv extractor, projection, grouped positional convolutions,
ALiBi transformer blocks, head) at the large size (C 512, D 1024, 16 heads, 4 + 24 blocks, recipe weights of seed 1), audio
already on the device: 1 x 3 s, 1 x 30 s and 32 x 30 s at 16 kHz.

    python tools/emotion2vec_bench.py [--shapes 1x3,1x30,32x30] [--warmup 5] [--iters 30] [--no-split] [--no-cpu] [--out profiles/emotion2vec_bench.json]

Audio: the test clips of tests/emotion2vec_oracle.py (the kernels' time does not depend on the values).  Device-event time of
every forward on its own; per shape the median, min, max and inter-quartile spread in milliseconds and the real-time factor.
The per-kernel split comes from a fresh child process per shape under `rocprofv3 --kernel-trace --stats` (1 warm-up + 3
forwards; total kernel time / 4 forwards), run before this process opens the device.  For orientation, in the same run: the
oracle in float32 on the CPU on ONE clip of the shape (torch's own thread pool).  No threshold is set: the feature is new, there
is no earlier time to compare with."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SR = 16000
CHILD_FORWARDS = 4


def model():
    from targetdiarization_amd.emotion import Emotion2vec
    from targetdiarization_amd.weights import emotion2vec_config, recipe_emotion2vec_state_dict
    cfg = emotion2vec_config()
    sd = recipe_emotion2vec_state_dict(1, cfg)
    return cfg, sd, Emotion2vec(sd, "cuda:0", workspace_budget_bytes=64 << 30)


def setup(m, B, seconds):
    import torch
    import emotion2vec_oracle as orc
    n = int(seconds * SR)
    host = np.stack([orc.clip(n, f"bench{j}") for j in range(B)])
    x = torch.from_numpy(host).to(m.device)
    c = m.cfg
    T = m.frames(n)
    feats = torch.empty((B, T, c["D"]), dtype=torch.float32, device=m.device)
    scores = torch.empty((B, c["n_classes"]), dtype=torch.float32, device=m.device)

    def run():
        with m._guard.call():
            m.launch(x, feats, None, scores)
    return host, run, dict(clips=B, seconds=seconds, samples=n, frames=T)


def child(B, seconds):
    import torch
    _, _, m = model()
    _, run, _ = setup(m, B, seconds)
    for _ in range(CHILD_FORWARDS):
        run()
    torch.cuda.synchronize()
    m.close()


def kernel_name(name: str):
    if "e2v_" in name:
        key = name.split("e2v_")[1].split("(")[0].split("_kernel")[0]
        if key == "ln_rows":
            key += "_gelu" if "true, true" in name or "false, true" in name else ""
        return key
    if "gemm_f32_kernel" in name:
        if "EpiConvRows" in name:
            return "gemm_conv"
        if "ActGelu" in name:
            return "gemm_fc1"
        if "EpiBiasResN" in name:
            return "gemm_proj_fc2"
        return "gemm_qkv_projection"
    return None


def kernel_split(B, seconds):
    """per-kernel milliseconds per forward from a profiled child process"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", f"{B}x{seconds}"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return {"error": (r.stderr or r.stdout)[-300:]}
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                key = kernel_name(row["Name"])
                if key:
                    out[key] = round(out.get(key, 0.0) + float(row["TotalDurationNs"]) / CHILD_FORWARDS / 1e6, 3)
        return dict(sorted(out.items(), key=lambda kv: -kv[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x3,1x30,32x30")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parse = lambda s: tuple(int(v) for v in s.split("x"))
    if a.child is not None:
        return child(*parse(a.child))
    shapes = [parse(s) for s in a.shapes.split(",")]
    splits = {s: ({} if a.no_split else kernel_split(*s)) for s in shapes}

    import torch
    import emotion2vec_oracle as orc
    cfg, sd, m = model()
    res = []
    for (B, seconds) in shapes:
        host, run, info = setup(m, B, seconds)
        for _ in range(a.warmup):
            run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(); e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts = np.array(ts)
        med = float(np.median(ts))
        q1, q3 = np.percentile(ts, [25, 75])
        row = dict(**info, iters=len(ts), median_ms=round(med, 3), min_ms=round(float(ts.min()), 3), max_ms=round(float(ts.max()), 3),
                   iqr_ms=round(float(q3 - q1), 3), rtf=float(f"{med * 1e-3 / (B * seconds):.3e}"),
                   workspace_mb=round(m._guard._ws.numel() / 2**20, 1), kernels_ms=splits[(B, seconds)])
        if not a.no_cpu:
            t0 = time.perf_counter()
            with torch.no_grad():
                orc.forward(sd, host[0], cfg, dtype=torch.float32)
            row["cpu_oracle_fp32_one_clip_s"] = round(time.perf_counter() - t0, 3)
        res.append(row)
    m.close()
    line = json.dumps({"workload": "tdx_emo2v_forward (frame features + scores), emotion2vec large (C 512, D 1024, 16 heads, 4 + 24 blocks), recipe "
                                   "weights, clips at 16 kHz on the device, device events per forward", "shapes": res})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
