"""Mint tests/golden/campplus_calibration.json: running mean / var of CAM++'s final (affine-free) BatchNorm, taken from the
fp64 oracle's pre-BN outputs over a seeded calibration signal (the test voices with other phases, vibrato and noise than the
test conversations use).  With the plain recipe statistics the embeddings of different inputs have cosine >= 0.998: a
device-vs-oracle comparison would miss input-dependent bugs and merge-by-cosine would collapse every conversation.

    python tools/make_goldens_campplus.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import campplus_oracle as orc                                       # noqa: E402
from oracle import frontend_oracle as fo                            # noqa: E402
from targetdiarization_amd.weights import recipe_campplus_state_dict   # noqa: E402

SEED, CAL_SEED, PER_VOICE = 0, 900, 16


def main():
    sd = recipe_campplus_state_dict(SEED)
    rng = np.random.default_rng(CAL_SEED)
    feats = []
    for vid in sorted(orc.VOICES):
        x = orc.voice(vid, PER_VOICE * 12000 + 12000, rng)
        for i in range(PER_VOICE):
            feats.append(fo.sv_features(torch.from_numpy(x[i * 12000:i * 12000 + 24000]).double()))
    pre = torch.cat([orc.forward(sd, torch.stack(feats[c:c + 8]), torch.float64, pre_bn=True) for c in range(0, len(feats), 8)])
    out = {"seed": SEED, "calibration_seed": CAL_SEED, "windows": len(feats),
           "running_mean": pre.mean(dim=0).tolist(), "running_var": pre.var(dim=0, unbiased=True).tolist()}
    path = orc.CALIBRATION
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f)
    print(path, len(feats), "windows; var range", min(out["running_var"]), max(out["running_var"]))


if __name__ == "__main__":
    main()
