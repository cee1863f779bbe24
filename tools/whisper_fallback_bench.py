"""What Whisper's sampled decoding costs a decode step at real widths (d 1280, 20 heads, 128 mels, vocabulary 51866, recipe weights;
DESIGN 8.26): decode_ts at B = 1 and 8 through
  old   tdx_whisper_decode_ts (the greedy entry point),
  zero  tdx_whisper_decode_ts_sample with every temperature 0 (the sampling head and step kernels, the noise skipped wholesale),
  hot   tdx_whisper_decode_ts_sample with every temperature 0.6 (the noise computed, every id drawn).

    python tools/whisper_fallback_bench.py [--batches 1,8] [--layers 4] [--warmup 3] [--iters 15] [--steps 16,80] [--variants old,zero,hot]
                                           [--package DIR] [--no-split] [--parent-json A.json,B.json,...] [--out profiles/whisper_fallback_bench.json]
    python tools/whisper_fallback_bench.py --merge NEW.json[,NEW2.json,...] --parent-json A.json,B.json,... --out FILE

The step time is tools/whisper_bench.py's: the difference of the medians of two calls that differ only in the number of generated
tokens (64 steps apart by default), over that difference, by the host clock between synchronisations; end-of-text is suppressed; the
variants alternate inside one run.  --package DIR imports targetdiarization_amd from another checkout (a build of the parent commit,
--variants old): run it several times around this build's run in one session and hand the results to --parent-json; the output then
carries the parent's step times, their run-to-run spread (max - min) and this build's `zero` and `old` against their mean.
--merge does that afterwards, without a device, from the files of runs that alternated in one session (further runs of this build are
kept as "repeat_runs").
The per-step head time comes from fresh child processes under `rocprofv3 --kernel-trace --stats` (run before this process opens the
device): the mean duration of the wh_head_kernel / wh_next_kernel instantiations each variant launches."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.whisper_bench import shader_clock, stats  # noqa: E402

TEMPERATURE = 0.6


def setup(layers, package):
    if package:
        sys.path.insert(0, os.path.abspath(package))
    import torch
    import targetdiarization_amd
    from targetdiarization_amd.whisper import WhisperASR, decode_prefix, default_generation_config
    from targetdiarization_amd.weights import recipe_whisper_state_dict, whisper_config
    assert torch.cuda.is_available(), "the benchmark needs a HIP device"
    cfg = whisper_config(d_model=1280, enc_heads=20, enc_layers=layers, dec_layers=layers, n_mels=128, vocab=51866)
    m = WhisperASR(recipe_whisper_state_dict(0, cfg), cfg, "cuda:0")
    gen = default_generation_config(cfg["vocab"])
    prefix = decode_prefix("chinese", "transcribe", None, gen)
    sup = list(gen["suppress_tokens"]) + [gen["eos_token_id"]]
    beg = gen["begin_suppress_tokens"]

    def calls_for(B):
        g = torch.Generator().manual_seed(B)
        feats = (0.5 * torch.randn(B, cfg["n_mels"], 2 * cfg["n_audio_ctx"], generator=g)).to("cuda:0")
        _, state = m.encode(feats, with_state=True)
        streams = [(b + 1) << 32 for b in range(B)]
        return {"old": lambda n: m.decode_ts(state, [prefix] * B, n, sup, beg, sot_pos=[0] * B),
                "zero": lambda n: m.decode_ts(state, [prefix] * B, n, sup, beg, sot_pos=[0] * B, temperature=0.0, streams=streams, seed=1),
                "hot": lambda n: m.decode_ts(state, [prefix] * B, n, sup, beg, sot_pos=[0] * B, temperature=TEMPERATURE, streams=streams, seed=1)}
    return torch, m, cfg, calls_for, os.path.relpath(os.path.dirname(os.path.abspath(targetdiarization_amd.__file__)), ROOT)


def child(a):
    torch, _, _, calls_for, _ = setup(a.layers, a.package)
    B, n = int(a.batches), int(a.steps.split(",")[1])
    calls = calls_for(B)
    for k in a.variants.split(","):
        for _ in range(3):
            calls[k](n)
    torch.cuda.synchronize()


def kernel_split(a, B, variants):
    """mean microseconds per launch of the head and step kernels a child process ran for `variants` (old and zero launch different
    instantiations and can share a child; zero and hot launch the same one and cannot)"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child",
               "--batches", str(B), "--layers", str(a.layers), "--steps", a.steps, "--variants", variants] + (["--package", a.package] if a.package else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return {"error": (r.stderr or r.stdout)[-300:]}
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row["Name"]
                for kern in ("wh_head_kernel", "wh_next_kernel"):
                    if kern in name:
                        key = kern + name.split(kern)[1].split("(")[0].replace(" ", "")
                        out[key] = {"mean_us": round(float(row["TotalDurationNs"]) / float(row["Calls"]) / 1e3, 2), "calls": int(row["Calls"])}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--steps", default="16,80")
    ap.add_argument("--variants", default="old,zero,hot")
    ap.add_argument("--package", default=None)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.merge:                                             # no device: this build's runs + the parent's runs -> one file
        res = json.load(open(a.merge.split(",")[0]))
        res["repeat_runs"] = [{k: {str(b["B"]): b.get(f"step_us_{k}") for b in r["batches"]} for k in ("old", "zero", "hot")}
                              for r in (json.load(open(p)) for p in a.merge.split(",")[1:])]
        against_parent(res, a.parent_json)
        return write(res, a.out)
    batches = [int(x) for x in a.batches.split(",")]
    variants = a.variants.split(",")
    split = {}
    if not a.no_split:                                      # before this process opens the device
        for B in batches:
            split[B] = {}
            if "old" in variants or "zero" in variants:
                split[B]["old,zero"] = kernel_split(a, B, ",".join(v for v in ("old", "zero") if v in variants))
            if "hot" in variants:
                split[B]["hot"] = kernel_split(a, B, "hot")
    torch, m, cfg, calls_for, package = setup(a.layers, a.package)
    n1, n2 = (int(x) for x in a.steps.split(","))
    rows = []
    for B in batches:
        calls = {k: fn for k, fn in calls_for(B).items() if k in variants}
        td = {(k, n): [] for k in calls for n in (n1, n2)}
        for n in (n1, n2):
            for _ in range(a.warmup):
                for fn in calls.values():
                    fn(n)
        for _ in range(a.iters):
            for n in (n1, n2):                              # alternating, the variants side by side
                for k, fn in calls.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = fn(n)
                    torch.cuda.synchronize()
                    td[(k, n)].append((time.perf_counter() - t0) * 1e6)
                    assert out[2].cpu().tolist() == [n] * B
        st = {k: stats(v) for k, v in td.items()}
        row = {"B": B}
        for k in calls:
            row[f"step_us_{k}"] = round((st[(k, n2)]["median_us"] - st[(k, n1)]["median_us"]) / (n2 - n1), 2)
            row[f"step_spread_us_{k}"] = round((st[(k, n1)]["iqr_us"] + st[(k, n2)]["iqr_us"]) / (n2 - n1), 2)
            row[f"decode_{n2}_new_{k}"] = st[(k, n2)]
        if "zero" in calls and "old" in calls:
            row["zero_minus_old_us"] = round(row["step_us_zero"] - row["step_us_old"], 2)
        if "hot" in calls and "zero" in calls:
            row["noise_us"] = round(row["step_us_hot"] - row["step_us_zero"], 2)
        row["head_weight_read_us_at_8_TB_s"] = round(4.0 * cfg["vocab"] * cfg["d_model"] / 8e12 * 1e6, 1)
        if B in split:
            row["kernels_us"] = split[B]
        rows.append(row)
        print(f"B = {B}: {row}", file=sys.stderr, flush=True)
    res = {"workload": f"Whisper large-v3 widths (d 1280, vocabulary 51866), {a.layers} + {a.layers} layers, recipe weights, fp32; decode step = (median of {n2} "
                       f"new tokens - median of {n1}) / {n2 - n1} by the host clock, the variants alternating in one run; hot = temperature {TEMPERATURE}",
           "package": package, "warmup": a.warmup, "iters": a.iters, "batches": rows, "shader_clock_after_the_loops": shader_clock()}
    if a.parent_json:
        against_parent(res, a.parent_json)
    write(res, a.out)


def against_parent(res, parent_json):
    rows = res["batches"]
    runs = [json.load(open(p)) for p in parent_json.split(",")]
    res["parent_runs"] = [{"package": r["package"], "step_us_old": {str(b["B"]): b["step_us_old"] for b in r["batches"]},
                           "shader_clock_after_the_loops": r["shader_clock_after_the_loops"]} for r in runs]
    cmp = {}
    for row in rows:
        vals = [r["step_us_old"][str(row["B"])] for r in res["parent_runs"] if str(row["B"]) in r["step_us_old"]]
        if vals:
            mean, spread = sum(vals) / len(vals), max(vals) - min(vals)
            cmp[str(row["B"])] = {"parent_step_us_old": vals, "parent_spread_us": round(spread, 2)}
            for k in ("old", "zero"):
                if f"step_us_{k}" in row:
                    cmp[str(row["B"])][f"{k}_minus_parent_us"] = round(row[f"step_us_{k}"] - mean, 2)
                    cmp[str(row["B"])][f"{k}_within_parent_spread"] = bool(row[f"step_us_{k}"] - mean <= spread)
    res["against_parent"] = cmp


def write(res, out):
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
