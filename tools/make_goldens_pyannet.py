"""Mint tests/golden/pyannet_calibration.json.  The recipe weights give logits of modest spread whose class means differ by
more than the spread, so one class would win every frame; two things are set in closed form on the posterior test clips
(tests/pyannet_oracle.py posterior_clips, fp64 oracle):
  * bias: class c's logit gets -gain * mean_c, so that every class's logit has zero mean over the clips;
  * gain = 1 / (standard deviation of the centred logits): the calibrated logits have unit spread.
It stores the spread before the gain, the oracle's own fp32-vs-fp64 difference on those clips (rel-L2 and max abs of the
log-probabilities and of each tap) and logp_device_bound = 10 x that max abs (the MFMA tiles and the device's reductions sum
in another order), then searches seeds for two end-to-end clips (12 s, 4 s) in which every frame of every chunk has a top-2
margin of at least 20 x logp_device_bound.

    python tools/make_goldens_pyannet.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pyannet_oracle as orc                                             # noqa: E402
from targetdiarization_amd import overlap                                # noqa: E402
from targetdiarization_amd.weights import recipe_pyannet_state_dict      # noqa: E402

SEED = 0
E2E_FIRST_SEED, E2E_TRIES = 4000, 400
# The fp32-vs-fp64 figures are rounding residue of the host's fp32 kernels: another CPU or thread count sums in another order.
# A rerun reproduces them, and logp_device_bound with them, within this factor; it is stored in the JSON next to them, and
# tests/test_pyannet_host.py holds a rerun to it.  Everything else in the file reproduces to 1e-6.
FP32_RESIDUE_TOLERANCE = 3.0


def rel_l2(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm())


def calibrate(seed: int = SEED) -> dict:
    """everything but the end-to-end seeds"""
    sd = recipe_pyannet_state_dict(seed)
    clips = orc.posterior_clips()
    z = torch.cat([orc.forward(sd, c, logits=True).reshape(-1, orc.NUM_CLASSES) for c in clips])
    mean = z.mean(dim=0)
    std = float((z - mean).std(unbiased=False))
    gain = float(np.float32(1.0 / std))
    bias = [float(np.float32(-gain * m)) for m in mean.tolist()]
    out = {"seed": seed, "gain": gain, "bias": bias, "pre_gain_logit_std": std}
    sdc = orc.apply_calibration(sd, gain, bias)
    worst = {"logp": [0.0, 0.0], "sincnet": [0.0, 0.0], "lstm": [0.0, 0.0]}
    seen = np.zeros(orc.NUM_CLASSES, dtype=np.int64)
    for c in clips:
        a = orc.forward(sdc, c, torch.float64, taps=True)
        b = orc.forward(sdc, c, torch.float32, taps=True)
        for name, x, y in zip(("logp", "sincnet", "lstm"), a, b):
            worst[name][0] = max(worst[name][0], rel_l2(y, x))
            worst[name][1] = max(worst[name][1], float((y.double() - x).abs().max()))
        seen += np.bincount(a[0].argmax(dim=-1).reshape(-1).numpy(), minlength=orc.NUM_CLASSES)
    for name, (r, m) in worst.items():
        out[f"{name}_fp32_vs_fp64_rel_l2"], out[f"{name}_fp32_vs_fp64_max_abs"] = r, m
    out["logp_device_bound"] = 10.0 * worst["logp"][1]
    out["fp32_residue_tolerance_factor"] = FP32_RESIDUE_TOLERANCE
    out["frames_per_class"] = seen.tolist()
    return out


def all_clear(sd, wave, floor: float) -> bool:
    starts, _ = overlap.chunk_plan(len(wave))
    return bool(orc.margins(orc.forward(sd, overlap.cut_chunks(wave, starts)).numpy()).min() >= floor)


def main():
    out = calibrate()
    sdc = orc.apply_calibration(recipe_pyannet_state_dict(SEED), out["gain"], out["bias"])
    floor = orc.MARGIN_FACTOR * out["logp_device_bound"]
    seeds = []
    for n in (12 * orc.SR, 4 * orc.SR):
        found = next((s for s in range(E2E_FIRST_SEED, E2E_FIRST_SEED + E2E_TRIES) if all_clear(sdc, orc.clip(n, s), floor)), None)
        if found is None:
            raise SystemExit(f"no seed in {E2E_TRIES} tries keeps every frame of a {n // orc.SR} s clip clear of {floor:.3e}")
        seeds.append(found)
    out["e2e_seeds"] = seeds
    os.makedirs(os.path.dirname(orc.CALIBRATION), exist_ok=True)
    with open(orc.CALIBRATION, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))
    print(orc.CALIBRATION, os.path.getsize(orc.CALIBRATION), "bytes")


if __name__ == "__main__":
    main()
