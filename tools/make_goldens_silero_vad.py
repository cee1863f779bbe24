"""Mint tests/golden/silero_vad_calibration.json.  The recipe's random head does not separate voiced from silent chunks, which
tests nothing behind the network; the head (decoder.decoder.2.weight / .bias, 128 weights and a bias) is fitted in closed
form in fp64 — ridge regression (lambda 1e-3) on relu(h) of the oracle over a seeded calibration clip (400 chunks: silence,
1e-4 N(0,1), alternating with bursts of the synthetic voices on chunk boundaries), target logit +2.5 on voiced and -2.5 on silent
chunks — and the fit is accepted only if every voiced chunk of that clip lands above 0.5 and every silent one below 0.35.
Moderate logits on purpose: the GPU test recovers the logit from p as log(p / (1 - p)), which loses its digits as p nears 0 or 1.
It then prints, for the test clips, the agreement with the chunk labels and the smallest distance of any chunk's p from 0.5 and
0.35, and stores the largest |p_fp32 - p_fp64| of the oracle over the test clips together with the device bound derived from
it (10x: the MFMA tiles and the recurrence's lanes sum in another order).  Deterministic; runs on the CPU.

    python tools/make_goldens_silero_vad.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import silero_vad_oracle as orc                                          # noqa: E402
from targetdiarization_amd.weights import recipe_silero_vad_state_dict   # noqa: E402

SEED, LAMBDA = 0, 1e-3
TARGET_VOICED, TARGET_SILENT = 2.5, -2.5


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = recipe_silero_vad_state_dict(SEED)
    clip, lab = orc.calibration_clip()
    _, _, h = orc.forward(sd, clip)
    X = torch.cat([torch.relu(h), torch.ones(h.shape[0], 1, dtype=torch.float64)], dim=1)
    y = torch.where(torch.from_numpy(lab) > 0, torch.tensor(TARGET_VOICED, dtype=torch.float64), torch.tensor(TARGET_SILENT, dtype=torch.float64))
    theta = torch.linalg.solve(X.t() @ X + LAMBDA * torch.eye(X.shape[1], dtype=torch.float64), X.t() @ y)
    w, b = theta[:-1].float(), theta[-1].float()                                    # as stored
    sdc = {k: v.clone() for k, v in sd.items()}
    sdc["decoder.decoder.2.weight"] = w.reshape(1, 128, 1)
    sdc["decoder.decoder.2.bias"] = b.reshape(1)
    p = orc.forward(sdc, clip)[0].numpy()
    voiced_min, silent_max = float(p[lab > 0].min()), float(p[lab == 0].max())
    print(f"calibration clip: {len(p)} chunks, voiced min p {voiced_min:.4f}, silent max p {silent_max:.4f}")
    assert voiced_min > 0.5 and silent_max < 0.35, "the fitted head does not separate the calibration clip"
    out = {"seed": SEED, "lambda": LAMBDA, "calibration_chunks": int(len(p)), "calibration_voiced_min_p": voiced_min,
           "calibration_silent_max_p": silent_max, "head_weight": w.double().tolist(), "head_bias": float(b)}
    # the test clips: label agreement, distance from the two thresholds, fp32 against fp64 of the oracle
    clips = orc.prob_clips() + orc.e2e_clips()
    labs = orc.prob_labels() + orc.e2e_labels()
    worst, margin, agree, total = 0.0, 1.0, 0, 0
    for c, l in zip(clips, labs):
        a = orc.forward(sdc, c, torch.float64)[0]
        f = orc.forward(sdc, c, torch.float32)[0]
        worst = max(worst, float((a - f.double()).abs().max()))
        a = a.numpy()
        margin = min(margin, float(np.minimum(np.abs(a - 0.5), np.abs(a - 0.35)).min()))
        agree += int(((a >= 0.5) == (l > 0)).sum()); total += len(a)
        print(f"  clip of {len(c)} samples, {len(a)} chunks: p in [{a.min():.4f}, {a.max():.4f}], share >= 0.5 {(a >= 0.5).mean():.3f}, "
              f"label agreement {((a >= 0.5) == (l > 0)).mean():.3f}")
    out["check_label_agreement"] = agree / total
    out["check_min_distance_from_thresholds"] = margin
    out["p_fp32_vs_fp64_max_abs"] = worst
    out["p_device_bound"] = 10.0 * worst
    os.makedirs(os.path.dirname(orc.CALIBRATION), exist_ok=True)
    with open(orc.CALIBRATION, "w") as f:
        json.dump(out, f)
    print(f"test clips: label agreement {agree / total:.4f}, smallest distance of a chunk's p from 0.5 / 0.35: {margin:.4f}")
    print(f"oracle fp32 vs fp64: max |p| difference {worst:.3e} -> device bound {10 * worst:.3e}")
    print(orc.CALIBRATION, os.path.getsize(orc.CALIBRATION), "bytes")


if __name__ == "__main__":
    main()
