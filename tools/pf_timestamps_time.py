"""Paraformer's upsampling timestamp head (ParaformerDecoder.upsampled = tdx_pfdec_timestamps: two GEMMs, the BLSTM recurrence,
the alphas and the peak scan) alone, at the two shapes the pipeline runs: B = 1, T = 145 (one clip per call, the reference's
own pattern) and B = 60, T = 500 (a 30 s bucket of the long-audio workload), inputs already on the device, recipe weights with
the full 16-block decoder.  Beside it, for scale, the decoder's predict + decode_embeds at the same shapes (what decode() ran
before the head existed; the host read of the counts is inside, as in decode()).

    python tools/pf_timestamps_time.py [--shapes 1x145,60x500] [--warmup 2] [--iters 10] [--out profiles/pf_timestamps.json]

Device-event time of every call on its own; per shape: median, min, max and inter-quartile spread in milliseconds, the steps of
the recurrence (3T) and the median per step."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ts):
    t = np.array(ts)
    q1, q3 = np.percentile(t, [25, 75])
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t.min()), 3), "max_ms": round(float(t.max()), 3),
            "iqr_ms": round(float(q3 - q1), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x145,60x500")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from targetdiarization_amd import weights as W
    from targetdiarization_amd.paraformer import ParaformerDecoder

    assert torch.cuda.is_available(), "the measurement needs a HIP device"
    sd = dict(W.recipe_paraformer_decoder_state_dict(0))
    sd.update(W.recipe_paraformer_timestamp_state_dict(0))
    dec = ParaformerDecoder(sd, device="cuda:0")
    assert dec.has_timestamps

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    rows = []
    for shape in a.shapes.split(","):
        B, T = (int(x) for x in shape.split("x"))
        enc = torch.randn(B, T, 512, generator=torch.Generator().manual_seed(B * 1000 + T)).to(dec.device)
        counts = dec.predict(enc)[2]

        def head():
            dec.upsampled(enc, counts)

        def decoder():
            _, emb, cnt, _ = dec.predict(enc)
            dec.decode_embeds(emb, cnt, enc, max(int(cnt.max()), 1))

        for _ in range(a.warmup):
            head(); decoder()
        torch.cuda.synchronize()
        th, td = [], []
        for _ in range(a.iters):
            th.append(timed(head)); td.append(timed(decoder))
        row = {"B": B, "T": T, "steps": 3 * T, "iters": a.iters, "tokens_max": int(counts.max()),
               "workspace_mb": round(int(dec._l.tdx_pfdec_timestamps_workspace_bytes(dec._h, B, T)) / 2**20, 1),
               "head": stats(th), "predict_plus_decode": stats(td)}
        row["head_us_per_step"] = round(row["head"]["median_ms"] * 1e3 / (3 * T), 2)
        rows.append(row)
    line = json.dumps({"workload": "ParaformerDecoder.upsampled (tdx_pfdec_timestamps) vs predict + decode_embeds, 16 decoder blocks, on the device, "
                                   "device events per call", "recurrence": "barrier-free, one workgroup per (4 clips, direction)", "shapes": rows})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
