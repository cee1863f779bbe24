"""The any-length FFT (tdx_fft_c2c) and the band mix (tdx_fft_band_mix) on the device, data already there.

    python tools/fft_bench.py [--warmup 3] [--iters 20] [--no-cpu] [--no-torch] [--out profiles/fft_bench.json]

band_mix at n = 160 000 (10 s at 16 kHz), 4 800 000, 28 800 000 (30 min) and 28 800 001; c2c at 2^20 and 2^24.  Device-event time of
every call on its own, or of as many back-to-back calls as fill a millisecond where one is shorter; per case and call the median, min, max and inter-quartile spread in microseconds, the number of passes over the data
(read off the planner: csrc/fft.hpp plan_pow2 through the test hook), the bytes those passes and the chirp / mix kernels must move
(16 M per pass: every pass reads and writes M complex64 once) and the resulting GB/s next to the 6.3 TB/s a copy reaches on MI355X.
Baselines from the same run: the float64 numpy oracle on the CPU, and torch.fft on the device for the same lengths — a yardstick only,
the product never calls it.  No threshold is set."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_COPY_GBS = 6300.0
TILE_LOG2 = 12
MIX_N = [160000, 4800000, 28800000, 28800001]
C2C_N = [1 << 20, 1 << 24]


def passes_pow2(m):
    from targetdiarization_amd import _lib
    return int(_lib.diag().tdx_test_fft_passes(m, TILE_LOG2))


def c2c_traffic(n):
    """(passes over M points, M, bytes moved) of one complex transform of n points, as csrc/fft.hpp issues it"""
    if n & (n - 1) == 0:
        p = passes_pow2(n.bit_length() - 1)
        return p, n, 16 * n * p
    m = (2 * n - 2).bit_length()
    M, p = 1 << m, passes_pow2(m)
    chirp = 8 * (M + n)
    into = 16 * n + 8 * M
    out = 24 * n
    return 3 * p, M, chirp + into + 3 * p * 16 * M + 8 * M + out        # three transforms of M points, the last one reads the chirp's spectrum too


def mix_traffic(n):
    h = n // 2
    pf, Mf, bf = c2c_traffic(n)
    if n & (n - 1) == 0:
        bf += 16 * n                                                    # the interleave kernel
    pi, Mi, bi = c2c_traffic(h)
    return pf + pi, (Mf, Mi), bf + 2 * 8 * n + 8 * h + bi                   # + the mix kernel: two reads of the spectrum, one write of the inverse's input


def timed(run, warmup, iters):
    import torch
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()

    def section(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    # a timed section lasts about a millisecond at least: short calls are issued back to back, `calls_per_sample` of them between
    # one pair of events, and the figures are per call
    reps = max(1, int(np.ceil(1000.0 / max(section(8), 1e-3))))
    ts = np.array([section(reps) for _ in range(iters)])
    q1, q3 = np.percentile(ts, [25, 75])
    return dict(iters=len(ts), calls_per_sample=reps, median_us=round(float(np.median(ts)), 1), min_us=round(float(ts.min()), 1), max_us=round(float(ts.max()), 1),
                iqr_us=round(float(q3 - q1), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import fft_oracle as orc
    from targetdiarization_amd import fft as tfft
    dev = tfft.DeviceFFT("cuda:0", workspace_budget_bytes=64 << 30)
    L, chk = dev._l, dev._lib.check
    st = torch.cuda.current_stream(dev.device).cuda_stream
    rng = np.random.default_rng(0)
    rows = []

    for n in MIX_N:
        ha, hb = (rng.standard_normal(n) * 0.3).astype(np.float32), (rng.standard_normal(n) * 0.3).astype(np.float32)
        xa, xb = torch.from_numpy(ha).to(dev.device), torch.from_numpy(hb).to(dev.device)
        plan = tfft.band_mix_plan(n, 16000)
        ranges = (C.c_long * 6)(*plan["ranges"])
        y = torch.empty(2 * (n // 2), dtype=torch.float32, device=dev.device)
        ws = dev._workspace("band_mix", L.tdx_fft_band_mix_workspace_bytes(n), f"{n} samples")

        def run():
            chk(L.tdx_fft_band_mix(xa.data_ptr(), xb.data_ptr(), n, ranges, y.data_ptr(), None, None, None, ws.data_ptr(), ws.numel(), st))
        t = timed(run, a.warmup, a.iters)
        passes, Ms, nbytes = mix_traffic(n)
        row = dict(op="band_mix", n=n, seconds_at_16k=round(n / 16000, 1), **t, passes=passes, transform_points=list(Ms), bytes_moved=nbytes,
                   gb_per_s=round(nbytes / t["median_us"] / 1e3, 1), share_of_copy_rate=round(nbytes / t["median_us"] / 1e3 / HBM_COPY_GBS, 3),
                   workspace_mb=round(ws.numel() / 2**20, 1))
        got = y.cpu().numpy()
        if not a.no_torch:
            def run_torch():
                fa, fb = torch.fft.rfft(xa), torch.fft.rfft(xb)
                torch.fft.irfft(fa + fb)                                # two forward transforms, one pointwise pass, one inverse
            row["torch_fft_us"] = timed(run_torch, a.warmup, a.iters)["median_us"]
        if not a.no_cpu:
            t0 = time.perf_counter()
            want = orc.mix_audio_by_freq(ha, hb)
            row["cpu_oracle_fp64_s"] = round(time.perf_counter() - t0, 2)
            row["rel_l2_vs_oracle"] = float(f"{np.linalg.norm(got - want) / np.linalg.norm(want):.3e}")
        print(json.dumps(row), flush=True)
        rows.append(row)
        del xa, xb, y

    for n in C2C_N:
        hx = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        x = torch.from_numpy(hx).to(dev.device)
        y = torch.empty_like(x)
        ws = dev._workspace("fft", L.tdx_fft_workspace_bytes(n, 1), f"{n} points")
        xr, yr = torch.view_as_real(x), torch.view_as_real(y)

        def run():
            chk(L.tdx_fft_c2c(xr.data_ptr(), n, 1, 0, yr.data_ptr(), ws.data_ptr(), ws.numel(), st))
        t = timed(run, a.warmup, a.iters)
        passes, M, nbytes = c2c_traffic(n)
        row = dict(op="c2c", n=n, **t, passes=passes, transform_points=[M], bytes_moved=nbytes, gb_per_s=round(nbytes / t["median_us"] / 1e3, 1),
                   share_of_copy_rate=round(nbytes / t["median_us"] / 1e3 / HBM_COPY_GBS, 3))
        got = y.cpu().numpy()
        if not a.no_torch:
            row["torch_fft_us"] = timed(lambda: torch.fft.fft(x), a.warmup, a.iters)["median_us"]
        if not a.no_cpu:
            t0 = time.perf_counter()
            want = np.fft.fft(hx.astype(np.complex128))
            row["cpu_numpy_fp64_s"] = round(time.perf_counter() - t0, 2)
            row["rel_l2_vs_fp64"] = float(f"{np.linalg.norm(got - want) / np.linalg.norm(want):.3e}")
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, y

    line = json.dumps({"workload": "tdx_fft_band_mix of two mono clips / tdx_fft_c2c of one row, data on the device, device events per call; "
                                   "bytes_moved = 16 M per pass plus the chirp, interleave and mix kernels; torch_fft_us = torch.fft on the same "
                                   "lengths (band_mix: two rfft, one add, one irfft), a yardstick only",
                       "hbm_copy_rate_gb_per_s": HBM_COPY_GBS, "tile": 1 << TILE_LOG2, "cases": rows})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
