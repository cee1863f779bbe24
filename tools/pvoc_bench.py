"""Phase-vocoder time stretch (rate 0.8) and pitch shift (+3 semitones) on the device (tdx_pvoc_stretch, tdx_resample_sinc) of one
30 s clip and one 1800 s clip at 16 kHz, audio and plan already on the device.

    python tools/pvoc_bench.py [--seconds 30,1800] [--warmup 3] [--iters 20] [--no-split] [--no-cpu] [--out profiles/pvoc_bench.json]

Audio: noise + chirp (tests/pvoc_cases.py's recipe; the kernels' times do not depend on the values).  Device-event time of every
call on its own; per shape and operation the median, min, max and inter-quartile spread in microseconds and the real-time factor.
The per-kernel split comes from a fresh child process per shape and operation under `rocprofv3 --kernel-trace --stats` (2 warm-up
+ 5 calls; total kernel time / 7 calls), run before this process opens the device.  Baseline, in the same run: the float64 numpy
oracle of tests/pvoc_oracle.py on the CPU on the same clip (the phase vocoder in blocks of bins and the resampler in blocks of
samples, so that the 1800 s clip fits in memory; the arithmetic is the oracle's).  No threshold is set."""
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

SR, RATE, STEPS = 16000, 0.8, 3
LAUNCHES = {"time_stretch": 5, "pitch_shift": 6}       # read off tdx_pvoc_stretch's source (+ tdx_resample_sinc)


def clip(seconds):
    import pvoc_cases as cases
    return np.ascontiguousarray(cases._noise_chirp(int(seconds * SR), seconds), dtype=np.float32)


def setup(seconds, op):
    import torch
    from targetdiarization_amd import effects
    pv = effects.PhaseVocoder("cuda:0", workspace_budget_bytes=64 << 30)
    host = clip(seconds)
    plan = effects.stretch_plan(host.shape[0], RATE) if op == "time_stretch" else effects.pitch_plan(host.shape[0], STEPS)
    x = torch.from_numpy(host).to(pv.device).reshape(1, -1)
    ws = pv._workspace(op, plan["n_fft"], plan["hop"], 1, host.shape[0], plan["T_out"])
    idx, idx_h, idx_d, alpha_d = pv._plan_dev(plan)
    y = torch.empty((1, plan["length"]), dtype=torch.float32, device=pv.device)
    out = torch.empty((1, plan["n_final"]), dtype=torch.float32, device=pv.device) if op == "pitch_shift" else y
    st = torch.cuda.current_stream(pv.device).cuda_stream
    L, chk = pv._l, pv._lib.check

    def run():
        with pv._guard.call():
            chk(L.tdx_pvoc_stretch(pv._h, x.data_ptr(), 1, host.shape[0], idx_h, idx_d.data_ptr(), alpha_d.data_ptr(), plan["T_out"], plan["length"],
                                   y.data_ptr(), None, None, ws.data_ptr(), ws.numel(), st))
            if op == "pitch_shift":
                chk(L.tdx_resample_sinc(y.data_ptr(), 1, plan["length"], plan["ratio"], out.data_ptr(), plan["n_final"], st))
    keep = (idx, idx_d, alpha_d, x, ws)
    return pv, host, run, dict(frames=int(plan["T"]), frames_out=int(plan["T_out"]), samples_out=int(out.shape[1])), out, keep


def child(seconds, op, warmup, iters):
    import torch
    _, _, run, _, _, keep = setup(seconds, op)
    for _ in range(warmup + iters):
        run()
    torch.cuda.synchronize()


def kernel_split(seconds, op):
    """per-kernel microseconds per call from a profiled child process"""
    calls = 7
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", f"{seconds}:{op}"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return {"error": (r.stderr or r.stdout)[-300:]}
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row["Name"]
                if "pv_kernel" in name:
                    key = "vocoder"
                elif "pv_" in name and "_kernel" in name:
                    key = name.split("pv_")[1].split("_kernel")[0]
                elif "resample_sinc_kernel" in name:
                    key = "resample_sinc"
                elif "gemm_f32_kernel" in name:
                    key = "gemm_analysis" if "EpiSpec" in name else "gemm_synthesis"
                else:
                    continue
                out[key] = round(out.get(key, 0.0) + float(row["TotalDurationNs"]) / calls / 1e3, 1)
        return out


def cpu_oracle(host, op):
    """the float64 oracle on the CPU, stage by stage -> (seconds per stage, result)"""
    import pvoc_oracle as orc
    rate = RATE if op == "time_stretch" else 2.0 ** (-STEPS / 12)
    t0 = time.perf_counter()
    D = orc.stft(host)
    t1 = time.perf_counter()
    P = np.concatenate([orc.phase_vocoder(D[k:k + 64], rate, block=(k, 2048)) for k in range(0, D.shape[0], 64)], axis=0)
    t2 = time.perf_counter()
    y = orc.istft(P, length=int(round(host.shape[0] / rate)))
    t3 = time.perf_counter()
    sec = dict(stft=round(t1 - t0, 2), phase_vocoder=round(t2 - t1, 2), istft=round(t3 - t2, 2))
    if op == "pitch_shift":
        n_out = int(np.ceil(y.shape[0] * rate))
        y = orc.fix_length(np.concatenate([orc.resample_sinc(y, rate, idx=np.arange(m, min(m + (1 << 20), n_out))) for m in range(0, n_out, 1 << 20)]),
                           host.shape[0])
        sec["resample"] = round(time.perf_counter() - t3, 2)
    sec["total"] = round(time.perf_counter() - t0, 2)
    return sec, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", default="30,1800")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child is not None:
        s, op = a.child.split(":")
        return child(int(s), op, 2, 5)
    shapes = [(int(s), op) for s in a.seconds.split(",") for op in ("time_stretch", "pitch_shift")]
    splits = {k: ({} if a.no_split else kernel_split(*k)) for k in shapes}

    import torch
    res = []
    for (s, op) in shapes:
        pv, host, run, info, out, keep = setup(s, op)
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
        row = dict(seconds=s, op=op, **info, iters=len(ts), median_us=round(med, 1), min_us=round(float(ts.min()), 1), max_us=round(float(ts.max()), 1),
                   iqr_us=round(float(q3 - q1), 1), rtf=float(f"{med * 1e-6 / s:.3e}"), launches=LAUNCHES[op],
                   workspace_mb=round(pv._guard._ws.numel() / 2**20, 1), kernels_us=splits[(s, op)])
        print(json.dumps(row), flush=True)
        got = out.cpu().numpy()[0]
        del keep, out
        pv.close()
        torch.cuda.empty_cache()
        if not a.no_cpu:
            cpu, want = cpu_oracle(host, op)
            row["cpu_oracle_fp64_s"] = cpu
            row["rel_l2_vs_oracle"] = float(f"{np.linalg.norm(got - want) / np.linalg.norm(want):.3e}")
            print(json.dumps(row), flush=True)
        res.append(row)
    line = json.dumps({"workload": "tdx_pvoc_stretch (+ tdx_resample_sinc for pitch_shift), one mono clip at 16 kHz on the device, rate 0.8 / +3 "
                                   "semitones, n_fft 2048, hop 512, device events per call",
                       "launches_from_source": LAUNCHES, "shapes": res})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
