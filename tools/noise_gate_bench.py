"""noisereduce's spectral gate on the device (tdx_ngate_forward: pad, analysis GEMM, scan + mask, two smoothing passes, synthesis
GEMM, gather) on one 30 s clip and one 1800 s clip at 16 kHz, audio already on the device.

    python tools/noise_gate_bench.py [--seconds 30,1800] [--warmup 5] [--iters 30] [--no-split] [--no-cpu] [--out profiles/noise_gate_bench.json]

Audio: the gated tone bursts + noise of tests/noise_gate_oracle.py (the kernels' time does not depend on the values).  Device-event
time of every forward on its own; per shape the median, min, max and inter-quartile spread in microseconds and the real-time
factor.  The per-kernel split comes from a fresh child process per shape under `rocprofv3 --kernel-trace --stats` (2 warm-up + 5
forwards; total kernel time / 7 forwards), run before this process opens the device.  The scan kernel's rate is stated against
two byte counts per frame-bin: 36 B, every access it makes (|S| twice, the forward plane written, fixed up and read back, the
mask plane written, fixed up in place), and 8 B, what has to cross HBM if the rest stays in cache (|S| in, mask out).
Baseline, in the same run: the float64 scipy oracle on the CPU, one thread pool as scipy finds it — the cost of the reference's
CPU package on the same clip.  No threshold is set."""
from __future__ import annotations

import argparse
import csv
import ctypes as C
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

LAUNCHES_PER_ROUND = 7       # read off tdx_ngate_forward's source
SR = 16000


def setup(seconds):
    import torch
    import noise_gate_oracle as orc
    from targetdiarization_amd.noise_gate import SpectralGate, gate_params
    g = SpectralGate("cuda:0")
    n = int(seconds * SR)
    host = orc.burst_signal(n, seed=seconds)
    tab, max_rows = g.table([(1, n)], 600000, 30000)
    tab_h = (C.c_int64 * tab.size)(*tab.reshape(-1).tolist())
    x = torch.from_numpy(host).to(g.device)
    y = torch.empty_like(x)
    tab_d = torch.from_numpy(tab).to(g.device)
    b, nf, nt, _ = gate_params(SR)
    rounds = int((tab[:, 7] == 0).sum())
    frames = int((tab[:, 6] // 256 + 1).sum())

    def run():
        with g._guard.call():
            g.launch(x, y, tab_h, tab_d, tab.shape[0], max_rows, b, nf, nt)
    return g, host, run, dict(buffers=int(tab.shape[0]), rounds=rounds, frames=frames, rows_largest_round=int(max_rows))


def child(seconds, warmup, iters):
    import torch
    _, _, run, _ = setup(seconds)
    for _ in range(warmup + iters):
        run()
    torch.cuda.synchronize()


def kernel_split(seconds):
    """per-kernel microseconds per forward from a profiled child process"""
    forwards = 7
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", str(seconds)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return {"error": (r.stderr or r.stdout)[-300:]}
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row["Name"]
                if "ng_" in name:
                    key = name.split("ng_")[1].split("(")[0].split("_kernel")[0]
                elif "gemm_f32_kernel" in name:
                    key = "gemm_analysis" if "EpiSpecMag" in name else ("gemm_synthesis" if "EpiBiasAct" in name else None)
                else:
                    key = None
                if key:
                    out[key] = round(out.get(key, 0.0) + float(row["TotalDurationNs"]) / forwards / 1e3, 1)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", default="30,1800")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--child", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, 2, 5)
    shapes = [int(s) for s in a.seconds.split(",")]
    splits = {s: ({} if a.no_split else kernel_split(s)) for s in shapes}

    import torch
    import noise_gate_oracle as orc
    res = []
    for s in shapes:
        g, host, run, info = setup(s)
        for _ in range(a.warmup):
            run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(); e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts = np.array(ts)
        med = float(np.median(ts))
        q1, q3 = np.percentile(ts, [25, 75])
        row = dict(seconds=s, **info, iters=len(ts), median_us=round(med, 1), min_us=round(float(ts.min()), 1), max_us=round(float(ts.max()), 1),
                   iqr_us=round(float(q3 - q1), 1), rtf=float(f"{med * 1e-6 / s:.3e}"), launches=LAUNCHES_PER_ROUND * info["rounds"],
                   workspace_mb=round(g._guard._ws.numel() / 2**20, 1), kernels_us=splits[s])
        scan = splits[s].get("scan")
        if scan:
            fb = info["frames"] * 513
            row["scan_gb_per_s_at_36_bytes"] = round(fb * 36 / (scan * 1e-6) / 1e9, 1)
            row["scan_gb_per_s_at_8_bytes"] = round(fb * 8 / (scan * 1e-6) / 1e9, 1)
        if not a.no_cpu:
            t0 = time.perf_counter()
            orc.reduce_noise(host, SR)
            row["cpu_scipy_oracle_fp64_s"] = round(time.perf_counter() - t0, 3)
        res.append(row)
        g.close()
    line = json.dumps({"workload": "tdx_ngate_forward, one clip at 16 kHz on the device, noisereduce defaults, device events per forward",
                       "launches_per_round_from_source": LAUNCHES_PER_ROUND, "shapes": res})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
