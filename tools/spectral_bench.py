"""Spectral clustering of n window embeddings: the device path (clustering.spectral_labels_device = tdx_spectral_laplacian +
tdx_symeig_lowest + the shared host tail) next to the host path (clustering.spectral_labels) on the same machine.

    python tools/spectral_bench.py [--sizes 300,1200,2400] [--warmup 2] [--iters 10] [--no-split] [--out profiles/spectral_bench.json]

Embeddings: the blob generator of tests/spectral_cases.py (4 centres, noise 0.9, seed = n), float32, already on the device.
Device: device-event time of each of the two entries on its own and wall-clock time of the whole spectral_labels_device call
(entries + copies of w, V [n,16] and X to the host + tail), medians over --iters runs after --warmup.  The split by stage
(affinity, prune + Laplacian, tridiagonalisation, bisection + inverse iteration, back-transformation) is the kernel time summed by
kernel name from a fresh child process per size under `rocprofv3 --kernel-trace --stats` (1 warm-up + 3 calls; total / 4), run
before this process opens the device: the entries launch back to back, so the event time of an entry is that sum plus the gaps
between its launches, which the tridiagonalisation row shows (about 2 n launches).  Host: perf_counter around each stage of
spectral_labels, restated stage by stage with the same calls, medians over --host-iters runs.  No threshold is set."""
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

STAGES = {"aff_": "affinity", "prune": "prune_laplacian", "lap_": "prune_laplacian", "tri_": "tridiagonalisation",
          "bis": "bisection_inverse_iteration", "inv": "bisection_inverse_iteration", "back": "back_transformation"}


def embeddings(n):
    import spectral_cases as sc
    return sc.blobs(n, 4, 0.9, n)


def device_calls(n):
    """-> (x on the device, run_laplacian, run_symeig): the two entries on preallocated buffers"""
    import torch
    from targetdiarization_amd import _lib
    from targetdiarization_amd.clustering import spectral_drop
    l = _lib.lib()
    X, _ = embeddings(n)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(X).to(dev)
    d, m = x.shape[1], 16
    nb = int(l.tdx_spectral_workspace_bytes(n, d, m))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    L = torch.empty(n, n, dtype=torch.float64, device=dev)
    w = torch.empty(m, dtype=torch.float64, device=dev)
    V = torch.empty(n, m, dtype=torch.float64, device=dev)
    drop = spectral_drop(n)

    def st():
        return torch.cuda.current_stream(dev).cuda_stream

    def lap():
        _lib.check(l.tdx_spectral_laplacian(x.data_ptr(), n, d, drop, L.data_ptr(), None, ws.data_ptr(), nb, st()))

    def eig():
        _lib.check(l.tdx_symeig_lowest(L.data_ptr(), n, m, w.data_ptr(), V.data_ptr(), ws.data_ptr(), nb, st()))
    return x, lap, eig, nb


def child(n):
    import torch
    _, lap, eig, _ = device_calls(n)
    for _ in range(4):
        lap(); eig()
    torch.cuda.synchronize()


def kernel_split(n):
    """microseconds of kernel time per stage and per laplacian + symeig pair, from a profiled child process"""
    calls = 4
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", str(n)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return {"error": (r.stderr or r.stdout)[-300:]}
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row["Name"]
                if "spec_" not in name:
                    continue
                key = name.split("spec_")[1]
                stage = next((v for k, v in STAGES.items() if key.startswith(k)), "other")
                out[stage] = round(out.get(stage, 0.0) + float(row["TotalDurationNs"]) / calls / 1e3, 1)
        return out


def host_stages(X, iters):
    """seconds per stage of clustering.spectral_labels, restated with the same calls"""
    from scipy.linalg import eigh
    from targetdiarization_amd.clustering import _unit, spectral_drop, spectral_labels, spectral_tail
    n = len(X)
    rows = []
    for _ in range(iters):
        t = [time.perf_counter()]
        X64 = np.asarray(X, dtype=np.float64)
        Un = _unit(X64)
        A = Un @ Un.T
        t.append(time.perf_counter())
        drop = spectral_drop(n)
        idx = np.argsort(A, axis=1, kind="stable")[:, :drop]
        np.put_along_axis(A, idx, 0.0, axis=1)
        A = 0.5 * (A + A.T)
        np.fill_diagonal(A, 0.0)
        L = np.diag(A.sum(axis=1)) - A
        t.append(time.perf_counter())
        w, V = eigh(L, subset_by_index=[0, 15])
        t.append(time.perf_counter())
        lab = spectral_tail(w, V, X64)
        t.append(time.perf_counter())
        spectral_labels(X)
        t.append(time.perf_counter())
        rows.append(np.diff(t))
    med = np.median(np.array(rows), axis=0)
    keys = ["affinity", "prune_laplacian", "eigh_16_lowest", "tail", "spectral_labels_total"]
    return {k: round(float(v), 4) for k, v in zip(keys, med)}, lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="300,1200,2400")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--child", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child)
    sizes = [int(s) for s in a.sizes.split(",")]
    splits = {n: ({} if a.no_split else kernel_split(n)) for n in sizes}

    import torch
    import spectral_cases as sc
    from targetdiarization_amd.clustering import spectral_labels_device
    res = []
    for n in sizes:
        x, lap, eig, nb = device_calls(n)
        for _ in range(a.warmup):
            lap(); eig()
        torch.cuda.synchronize()
        t_lap, t_eig, t_all, t_tail = [], [], [], []
        for _ in range(a.iters):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record(); lap(); e[1].record(); eig(); e[2].record()
            e[2].synchronize()
            t_lap.append(e[0].elapsed_time(e[1]) * 1e3)
            t_eig.append(e[1].elapsed_time(e[2]) * 1e3)
        for _ in range(a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lab_dev = spectral_labels_device(x)
            t_all.append(time.perf_counter() - t0)
        X, y = embeddings(n)
        host, lab_host = host_stages(X, a.host_iters)
        row = dict(n=n, d=int(x.shape[1]), iters=a.iters, launches=5 + 2 * (n - 1) - 1 + 4, workspace_mb=round(nb / 2**20, 1),
                   laplacian_entry_us=round(float(np.median(t_lap)), 1), symeig_entry_us=round(float(np.median(t_eig)), 1),
                   symeig_entry_min_max_us=[round(float(min(t_eig)), 1), round(float(max(t_eig)), 1)],
                   device_path_total_s=round(float(np.median(t_all)), 4), kernels_us=splits[n], host_s=host,
                   same_partition_as_host=bool(sc.same_partition(lab_dev, lab_host)), recovers_truth=bool(sc.same_partition(lab_dev, y)))
        row["host_tail_inside_device_path_s"] = host["tail"]
        print(json.dumps(row), flush=True)
        res.append(row)
    line = json.dumps({"workload": "spectral clustering of n blob embeddings [n,192] resident on the device: device path (two entries + host tail) and host "
                                   "spectral_labels on the same machine; medians", "sizes": res})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
