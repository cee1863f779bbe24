"""pYIN on the device (tdx_pyin_forward: difference + cumulative mean + shifts, troughs -> observation column, Viterbi) on one 30 s
clip and one 1800 s clip at 16 kHz with librosa's defaults (fmin 50, fmax 300), audio already on the device.

    python tools/pyin_bench.py [--seconds 30,1800] [--warmup 3] [--iters 20] [--no-split] [--no-cpu] [--out profiles/pyin_bench.json]

Audio: the gated gliding tone + noise of tests/pyin_oracle.py (the trough kernel's time depends on the number of troughs, so the
signal matters there; the other two kernels' times do not depend on the values).  Device-event time of every forward on its own;
per shape the median, min, max and inter-quartile spread in microseconds and the real-time factor.  The per-kernel split comes
from a fresh child process per shape under `rocprofv3 --kernel-trace --stats` (2 warm-up + 5 forwards; total kernel time / 7
forwards), run before this process opens the device.  Baseline, in the same run: the float64 numpy / scipy oracle on the CPU (FFT
difference, per-frame Python loop for the troughs, dense 622 x 622 Viterbi — the shape of upstream's own implementation) on the
same clip, stage by stage.  No threshold is set."""
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

LAUNCHES = 3       # read off tdx_pyin_forward's source
SR, FMIN, FMAX = 16000, 50.0, 300.0


def setup(seconds):
    import torch
    import pyin_oracle as orc
    from targetdiarization_amd.pitch import Pyin, pyin_plan
    p = Pyin("cuda:0")
    plan = pyin_plan(SR, FMIN, FMAX)
    n = int(seconds * SR)
    host = orc.voiced_signal(n, SR, seed=seconds)
    T = plan.frames(n)
    tab = np.asarray([[0, n, 0, T]], dtype=np.int64)
    tab_h = (C.c_int64 * 4)(*tab.reshape(-1).tolist())
    x = torch.from_numpy(host).to(p.device)
    tab_d = torch.from_numpy(tab).to(p.device)
    tables = p._tables(plan)
    states = torch.empty(T, dtype=torch.int32, device=p.device)
    vprob = torch.empty(T, dtype=torch.float32, device=p.device)

    def run():
        with p._guard.call():
            p.launch(plan, x, tab_h, tab_d, 1, tables, states, vprob)
    return p, host, run, dict(frames=int(T), lags=int(plan.n_lags), states=int(2 * plan.n_pitch_bins), width=int(plan.width)), states


def child(seconds, warmup, iters):
    import torch
    _, _, run, _, _ = setup(seconds)
    for _ in range(warmup + iters):
        run()
    torch.cuda.synchronize()


def kernel_split(seconds):
    """per-kernel microseconds per forward from a profiled child process"""
    forwards = 7
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", str(seconds)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return {"error": (r.stderr or r.stdout)[-300:]}
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row["Name"]
                if "pyin_" in name:
                    key = name.split("pyin_")[1].split("(")[0].split("_kernel")[0]
                    out[key] = round(out.get(key, 0.0) + float(row["TotalDurationNs"]) / forwards / 1e3, 1)
        return out


def cpu_oracle(host):
    """the float64 restatement on the CPU, stage by stage -> (seconds per stage, states)"""
    import pyin_oracle as orc
    P = orc.params(SR, FMIN, FMAX)
    t0 = time.perf_counter()
    yin, sh = orc.yin_shifts(host, P)
    t1 = time.perf_counter()
    print(f"  cpu oracle: yin {t1 - t0:.1f} s", flush=True)
    obs, vp = orc.observation(yin, sh, P)
    t2 = time.perf_counter()
    print(f"  cpu oracle: observation {t2 - t1:.1f} s", flush=True)
    states = orc.viterbi_dense(obs, P)
    t3 = time.perf_counter()
    print(f"  cpu oracle: viterbi {t3 - t2:.1f} s", flush=True)
    return dict(yin=round(t1 - t0, 2), observation=round(t2 - t1, 2), viterbi=round(t3 - t2, 2), total=round(t3 - t0, 2)), states, P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", default="30,1800")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
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
    res = []
    for s in shapes:
        p, host, run, info, states = setup(s)
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
                   iqr_us=round(float(q3 - q1), 1), rtf=float(f"{med * 1e-6 / s:.3e}"), launches=LAUNCHES,
                   workspace_mb=round(p._guard._ws.numel() / 2**20, 1), kernels_us=splits[s])
        vit = splits[s].get("viterbi")
        if vit:
            row["viterbi_us_per_frame"] = round(vit / info["frames"], 3)
        print(json.dumps(row), flush=True)
        if not a.no_cpu:
            cpu, want, P = cpu_oracle(host)
            row["cpu_oracle_fp64_s"] = cpu
            st = states.cpu().numpy()
            v = want < P.npb
            row["voiced_flags_equal_oracle"] = bool(np.array_equal(st < P.npb, v))
            row["voiced_states_equal_oracle"] = bool(np.array_equal(st[v], want[v])) if row["voiced_flags_equal_oracle"] else False
        res.append(row)
        p.close()
    line = json.dumps({"workload": "tdx_pyin_forward, one clip at 16 kHz on the device, librosa defaults with fmin 50 and fmax 300, device events per forward",
                       "launches_from_source": LAUNCHES, "shapes": res})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
