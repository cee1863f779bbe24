"""SenseVoiceSmall forward (tdx_sv_forward: prompt + 50 + 20 SANM layers + CTC head over 25055 words + collapse) at the pipeline's
sizes: 120 segments of 30 s (500 LFR frames each, cut into launch sequences of at most --rows LFR rows as HotPath does: 65 + 55
segments) and one 10 s clip (167 frames), features already on the device.

    python tools/sensevoice_bench.py [--shapes 120x500,1x167] [--rows 32768] [--warmup 3] [--iters 10] [--only fused|chunks|encoder|paraformer]
                                     [--out profiles/sensevoice_bench.json]

Four models from the same recipe weights are held in one process and their timed forwards alternate:
  fused     TDX_SV_HEAD=1 at create: the fused head kernel
  chunks    TDX_SV_HEAD=0 at create: row chunks through the x3 Linear + row kernel
  encoder   the same 70 layers with a 2-word vocabulary: the model without a head worth speaking of
  paraformer  tdx_pfenc_forward, Paraformer's 50 layers, at the same shapes (no prompt rows)
Device-event time of every forward (all its launch sequences) on its own; per shape and model: median, min, max and the
inter-quartile spread in microseconds.  The head's own time is (fused | chunks) - encoder, its TFLOP/s 2 * rows * 512 * 25055 over
that, next to the 157 TFLOP/s fp32 MFMA peak.  The verdict: the default of TDX_SV_HEAD is the path whose median at
the 120-segment shape is lower by more than the sum of the two spreads; if neither is, the fused path for its footprint."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOCAB = 25055


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="120x500,1x167")
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--blocks", default="50,20")
    ap.add_argument("--only", default=None, choices=("fused", "chunks", "encoder", "paraformer"), help="time one model alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from targetdiarization_amd import _lib
    from targetdiarization_amd.paraformer import ParaformerEncoder
    from targetdiarization_amd.sensevoice import SenseVoiceSmall
    from targetdiarization_amd.weights import recipe_sensevoice_state_dict

    assert torch.cuda.is_available(), "the benchmark needs a HIP device"
    nb, tp = (int(x) for x in a.blocks.split(","))
    sd = recipe_sensevoice_state_dict(0, nb, tp, VOCAB)
    want = [a.only] if a.only else ["fused", "chunks", "encoder", "paraformer"]
    models = {}
    for name, head in (("fused", "1"), ("chunks", "0")):
        if name in want:
            os.environ["TDX_SV_HEAD"] = head
            models[name] = SenseVoiceSmall(sd, "cuda:0")
    os.environ.pop("TDX_SV_HEAD", None)
    if "encoder" in want:
        sd2 = dict(sd)
        sd2["ctc.ctc_lo.weight"], sd2["ctc.ctc_lo.bias"] = sd["ctc.ctc_lo.weight"][:2].contiguous(), sd["ctc.ctc_lo.bias"][:2].contiguous()
        models["encoder"] = SenseVoiceSmall(sd2, "cuda:0")
    if "paraformer" in want:
        models["paraformer"] = ParaformerEncoder({k: v for k, v in sd.items() if k.startswith("encoder.") and ".tp_" not in k}, "cuda:0", num_blocks=nb, graph_rows=0)
    dev = torch.device("cuda:0")
    l = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    prompt = (C.c_int * 4)(0, 1, 2, 14)

    res = []
    for shape in a.shapes.split(","):
        B, T = (int(x) for x in shape.split("x"))
        S = T + 4
        per = max(1, a.rows // S)
        cuts = [(b0, min(per, B - b0)) for b0 in range(0, B, per)]
        g = torch.Generator().manual_seed(B * 1000 + T)
        feats = torch.randn(B, T, 560, generator=g).to(dev).contiguous()
        i32 = dict(dtype=torch.int32, device=dev)
        fid, fsc, tok, frm, cnt = torch.empty(B, S, **i32), torch.empty(B, S, device=dev), torch.empty(B, S, **i32), torch.empty(B, S, **i32), torch.empty(B, **i32)
        enc = torch.empty(B, T, 512, device=dev)
        wsb = {k: (int(l.tdx_pfenc_workspace_bytes(m._h, cuts[0][1], T)) if k == "paraformer" else m.workspace_bytes(cuts[0][1], T)) for k, m in models.items()}
        ws = torch.empty(max(wsb.values()), dtype=torch.uint8, device=dev)

        def forward(k, m):
            for b0, n in cuts:
                if k == "paraformer":
                    _lib.check(l.tdx_pfenc_forward(m._h, feats[b0:].data_ptr(), None, n, T, enc[b0:].data_ptr(), ws.data_ptr(), ws.numel(), st))
                else:
                    _lib.check(l.tdx_sv_forward(m._h, feats[b0:].data_ptr(), n, T, prompt, None, fid[b0:].data_ptr(), fsc[b0:].data_ptr(), tok[b0:].data_ptr(),
                                                frm[b0:].data_ptr(), cnt[b0:].data_ptr(), ws.data_ptr(), ws.numel(), st))
        ts = {k: [] for k in models}
        for k, m in models.items():
            for _ in range(a.warmup):
                forward(k, m)
        torch.cuda.synchronize()
        for _ in range(a.iters):
            for k, m in models.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); forward(k, m); e1.record()
                e1.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3)
        head_flop = 2.0 * B * S * 512 * VOCAB
        row = {"segments": B, "lfr_frames": T, "rows": B * S, "launch_sequences_of": [n for _, n in cuts], "iters": a.iters,
               "workspace_mb": {k: round(v / 2**20, 1) for k, v in wsb.items()}, "head_gflop": round(head_flop / 1e9, 1)}
        for k, m in models.items():
            t = np.array(ts[k])
            q1, q3 = np.percentile(t, [25, 75])
            med = float(np.median(t))
            fl = sum(float(l.tdx_pfenc_flops(m._h, n, T)) if k == "paraformer" else m.flops(n, T) for _, n in cuts)
            row[k] = {"median_us": round(med, 1), "min_us": round(float(t.min()), 1), "max_us": round(float(t.max()), 1), "iqr_us": round(float(q3 - q1), 1),
                      "gflop": round(fl / 1e9, 1), "tflops": round(fl / (med * 1e-6) / 1e12, 2)}
        if "encoder" in row:
            for k in ("fused", "chunks"):
                if k in row:
                    ht = row[k]["median_us"] - row["encoder"]["median_us"]
                    row[k]["head_us"] = round(ht, 1)
                    row[k]["head_share_of_model"] = round(ht / row[k]["median_us"], 4)
                    if ht > 0:
                        row[k]["head_tflops"] = round(head_flop / (ht * 1e-6) / 1e12, 2)
                        row[k]["head_share_of_157_tflops_fp32_mfma_peak"] = round(head_flop / (ht * 1e-6) / 157e12, 4)
        if "fused" in row and "chunks" in row:
            row["chunks_minus_fused_us"] = round(row["chunks"]["median_us"] - row["fused"]["median_us"], 1)
            row["sum_of_iqrs_us"] = round(row["chunks"]["iqr_us"] + row["fused"]["iqr_us"], 1)
        res.append(row)
    verdict = None
    big = [r for r in res if r["segments"] == 120 and "chunks_minus_fused_us" in r]
    if big:
        d, s = big[0]["chunks_minus_fused_us"], big[0]["sum_of_iqrs_us"]
        verdict = "fused: faster beyond the spread" if d > s else "chunks: faster beyond the spread" if -d > s else "fused: neither is faster beyond the spread, the footprint decides"
    line = json.dumps({"workload": f"tdx_sv_forward, {nb}+{tp} layers, vocabulary {VOCAB}, features on the device, device events per forward",
                       "rows_per_launch_sequence": a.rows, "shapes": res, "default_of_TDX_SV_HEAD": verdict})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
