"""Mint tests/golden/fsmn_vad_calibration.json.  Recipe weights alone give p0 ~ 1/248 on every frame, which tests nothing
behind the network; three things are fitted in closed form on a seeded calibration clip (silence, 1e-4 N(0,1), alternating
with bursts of the synthetic voices):
  * cmvn: shift = -mean, scale = 1/std of the LFR features;
  * row 0 of out_linear2 (140 weights and a bias): ridge regression (lambda 1e-3) on the fp64 oracle's out_linear1
    activations, so that logit0 - logsumexp(other logits) is +3 on silent frames and -6 on voiced ones.
It then prints, for a DIFFERENT clip, the share of speech frames, the agreement with the frame labels and the number of
frames with |p0 - 0.2| < 0.02 (0.2 is the decision point of `1 - p0 >= p0 + 0.6`), and stores the largest
|p0_fp32 - p0_fp64| of the oracle over the posterior test's clips together with the device bound derived from it (10x: the
MFMA tiles sum in another order and the device folds two pairs of linears).

    python tools/make_goldens_fsmn_vad.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fsmn_vad_oracle as orc                                          # noqa: E402
from oracle import frontend_oracle as fo                                # noqa: E402
from targetdiarization_amd.weights import recipe_fsmn_vad_state_dict    # noqa: E402

SEED, CAL_SEED, LAMBDA = 0, 910, 1e-3
TARGET_SIL, TARGET_VOICED = 3.0, -6.0


def bursts_every(n, period, duty, first_voice=0):
    out, k = [], 0
    for a in range(period // 2, n - period // 4, period):
        out.append((a, a + int(period * duty), (first_voice + k) % 3)); k += 1
    return out


def frame_labels(T, bursts):
    """1 where the frame's centre (sample 160 t + 200) lies in a burst"""
    c = 160 * np.arange(T) + 200
    lab = np.zeros(T, dtype=bool)
    for a, b, _ in bursts:
        lab |= (c >= a) & (c < b)
    return lab


def main():
    sd = recipe_fsmn_vad_state_dict(SEED)
    sdd = {k: v.double() for k, v in sd.items()}
    n = orc.frames_to_samples(473)
    bursts = bursts_every(n, 16000, 0.55)
    wave = torch.from_numpy(orc.mix(n, bursts, CAL_SEED)).double()
    lfr = fo.apply_lfr(fo.kaldi_fbank(wave, "hamming", 32768.0), 5, 1)
    shift, scale = -lfr.mean(dim=0), 1.0 / lfr.std(dim=0, unbiased=True)
    shift, scale = shift.float().double(), scale.float().double()                  # as stored
    H = orc.encoder(sdd, (lfr + shift) * scale, upto="out_linear1")                # [T,140]
    W, b = sdd["encoder.out_linear2.linear.weight"], sdd["encoder.out_linear2.linear.bias"]
    others = torch.logsumexp(H @ W[1:].t() + b[1:], dim=-1)
    lab = torch.from_numpy(frame_labels(H.shape[0], bursts))
    y = others + torch.where(lab, torch.tensor(TARGET_VOICED, dtype=torch.float64), torch.tensor(TARGET_SIL, dtype=torch.float64))
    X = torch.cat([H, torch.ones(H.shape[0], 1, dtype=torch.float64)], dim=1)
    theta = torch.linalg.solve(X.t() @ X + LAMBDA * torch.eye(X.shape[1], dtype=torch.float64), X.t() @ y)
    out = {"seed": SEED, "calibration_seed": CAL_SEED, "lambda": LAMBDA, "calibration_frames": int(H.shape[0]),
           "cmvn_shift": shift.tolist(), "cmvn_scale": scale.tolist(),
           "row0_weight": theta[:-1].float().double().tolist(), "row0_bias": float(theta[-1].float())}
    # the calibrated model, from the values as they will be stored
    sdc = {k: v.clone() for k, v in sd.items()}
    sdc["encoder.out_linear2.linear.weight"][0] = theta[:-1].float()
    sdc["encoder.out_linear2.linear.bias"][0] = theta[-1].float()
    cmvn = (shift.float(), scale.float())
    # the three figures on another clip
    n2 = orc.frames_to_samples(500)
    b2 = bursts_every(n2, 13000, 0.6, first_voice=1)
    p0, _ = orc.forward(sdc, cmvn, orc.mix(n2, b2, CAL_SEED + 1))
    p0 = p0.numpy()
    lab2 = frame_labels(len(p0), b2)
    speech = p0 <= 0.2
    near = int((np.abs(p0 - 0.2) < 0.02).sum())
    print(f"check clip: {len(p0)} frames, speech share {speech.mean():.3f}, agreement with the frame labels "
          f"{(speech == lab2).mean():.3f}, frames with |p0 - 0.2| < 0.02: {near}")
    # fp32 against fp64 of the oracle over the posterior test's clips -> the device bound on p0
    worst = 0.0
    for clip in orc.posterior_clips():
        a, _ = orc.forward(sdc, cmvn, clip, torch.float64)
        c, _ = orc.forward(sdc, cmvn, clip, torch.float32)
        worst = max(worst, float((a - c.double()).abs().max()))
    out["check_speech_share"], out["check_label_agreement"], out["check_frames_near_threshold"] = float(speech.mean()), float((speech == lab2).mean()), near
    out["p0_fp32_vs_fp64_max_abs"] = worst
    out["p0_device_bound"] = 10.0 * worst
    os.makedirs(os.path.dirname(orc.CALIBRATION), exist_ok=True)
    with open(orc.CALIBRATION, "w") as f:
        json.dump(out, f)
    print(f"oracle fp32 vs fp64: max |p0| difference {worst:.3e} -> device bound {10 * worst:.3e}")
    print(orc.CALIBRATION, os.path.getsize(orc.CALIBRATION), "bytes")


if __name__ == "__main__":
    main()
