"""Mint tests/golden/wespeaker_calibration.json.  The recipe weights (weights.recipe_wespeaker_state_dict) are random and
fan-in scaled; what keeps 33 convolutions of them alive is BatchNorm statistics that match the activations, so the running
mean / variance of all 36 BatchNorms are taken from ONE fp64 pass of the oracle over six seeded synthetic voices
(tests/wespeaker_oracle.py calibration_voices), each BatchNorm normalising with the statistics it has just measured.

The file also records what the tests rest on:
  * fp32_vs_fp64: the oracle's own fp32-vs-fp64 rel-L2 (worst row) on every test input, unmasked and masked.  It must come
    out <= 1e-5, a tenth of the embedding bar; otherwise the recipe is to be re-tuned, not the bar.
  * mask_separation: on the masked test inputs, the rel-L2 between the oracle embeddings of the two disjoint masks of one
    chunk (smallest over the chunks).  It must come out >= 1e-2, 100 bars: a device that ignored the mask would fail.
  * e2e: the 12 s end-to-end clip (a seed of tests/pyannet_oracle.py clip, searched from the PyanNet goldens' own) whose
    centroid-linkage merge heights over the two oracles all lie further than 1e-2 from the published threshold.

    python tools/make_goldens_wespeaker.py
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pyannet_oracle as porc                                            # noqa: E402
import wespeaker_oracle as orc                                           # noqa: E402
from targetdiarization_amd import overlap                                # noqa: E402
from targetdiarization_amd.weights import recipe_wespeaker_state_dict    # noqa: E402

SEED = 0
SHAPES = ((1, 1), (1, 2), (2, 9), (3, 17), (2, 298), (1, 998))          # tests/test_gpu_wespeaker.py
MASKED = ((2, 298, 3, 589), (1, 998, 3, 589), (3, 17, 2, 7), (1, 9, 1, 2))
E2E_TRIES = 8
E2E_MARGIN = 1e-2


def worst_row(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    ok = np.isfinite(b).all(axis=1)
    return max(orc.rel_l2(x, y) for x, y in zip(a[ok], b[ok]))


def e2e_heights(sd_seg, sd_emb, wave):
    """-> (merge heights of the training embeddings' centroid linkage, tracks) of overlap.diarize over the two oracles"""
    from scipy.cluster.hierarchy import linkage
    seen = {}

    def segment(chunks):
        return porc.forward(sd_seg, torch.from_numpy(chunks)).numpy()

    def embed_masked(chunks, masks):
        seen["E"] = orc.embed_masked(sd_emb, chunks, masks)
        return seen["E"]

    tracks = overlap.diarize(wave, segment, None, embed_masked=embed_masked)
    starts, _ = overlap.chunk_plan(wave.shape[0])
    chunks = overlap.cut_chunks(wave, starts)
    seg = overlap.powerset_to_speakers(segment(chunks))
    emb, owner = overlap.masked_embeddings(chunks, seg, lambda c, m: seen["E"])
    train = np.array([seg[k, :, j].mean() >= 0.2 for k, j in owner], dtype=bool)
    U = overlap._unit(emb[train])
    h = linkage(U, method="centroid", metric="euclidean")[:, 2] if train.sum() > 1 else np.zeros(0)
    return h, tracks


def main():
    t0 = time.time()
    sd = recipe_wespeaker_state_dict(SEED)
    bn = orc.calibrate(sd)
    for k, v in bn.items():
        sd[k] = v
    out = {"seed": SEED, "bn": {k: [float(x) for x in v.tolist()] for k, v in bn.items()}}
    print(f"calibrated {len(bn) // 2} BatchNorms, {sum(v.numel() for v in bn.values())} floats  ({time.time() - t0:.0f} s)")

    fp, sep = {}, {}
    trunks = {}
    for B, F in SHAPES:
        feat = orc.shape_feat(B, F)
        with torch.no_grad():
            t64, t32 = orc.trunk(sd, feat, torch.float64), orc.trunk(sd, feat, torch.float32)
        trunks[(B, F)] = (t64, t32)
        e64, e32 = orc.head(sd, t64, None, torch.float64), orc.head(sd, t32, None, torch.float32)
        fp[f"{B}x{F}"] = worst_row(e32, e64)
        alive = float((t64 > 0).double().mean())
        print(f"({B},{F}): fp32 vs fp64 rel-L2 {fp[f'{B}x{F}']:.3e}   trunk output > 0: {alive:.2f}   |emb| {float(e64.norm(dim=-1).mean()):.3f}")
    for B, F, S, Fw in MASKED:
        feat = orc.shape_feat(B, F)
        if (B, F) not in trunks:
            with torch.no_grad():
                trunks[(B, F)] = (orc.trunk(sd, feat, torch.float64), orc.trunk(sd, feat, torch.float32))
        t64, t32 = trunks[(B, F)]
        m = orc.shape_masks(B, S, Fw, t64.shape[2])
        e64 = orc.head(sd, t64, torch.from_numpy(m), torch.float64).numpy()
        e32 = orc.head(sd, t32, torch.from_numpy(m), torch.float32).numpy()
        key = f"{B}x{F}x{S}x{Fw}"
        fp[key] = worst_row(e32, e64)
        line = f"({B},{F},{S},{Fw}): fp32 vs fp64 rel-L2 {fp[key]:.3e}   NaN rows {int(np.isnan(e64).all(axis=-1).sum())}"
        if S >= 2:
            # masks 0 and 1 of a chunk are disjoint halves (chunk 0's may be the special rows: take the chunks where both are finite)
            d = [orc.rel_l2(e64[b, 0], e64[b, 1]) for b in range(B) if np.isfinite(e64[b, :2]).all()]
            if d:
                sep[key] = min(d)
                line += f"   disjoint masks differ by {sep[key]:.3e}"
        print(line)
    out["fp32_vs_fp64"] = fp
    out["mask_separation"] = sep
    assert max(fp.values()) <= 1e-5, "re-tune the recipe: the oracle's own fp32 run is not within a tenth of the bar"
    assert sep and min(sep.values()) >= 1e-2, "re-tune the recipe: the embedding hardly depends on the mask"

    sd_seg = porc.calibrated_state_dict(0)
    first = porc.calibration()["e2e_seeds"][0]
    for seed in [first] + [first + 1000 + i for i in range(E2E_TRIES)]:
        wave = porc.clip(12 * porc.SR, seed)
        h, tracks = e2e_heights(sd_seg, sd, wave)
        gap = float(np.abs(h - overlap.DEFAULT_THRESHOLD).min()) if len(h) else float("inf")
        print(f"e2e seed {seed}: heights {np.round(h, 4).tolist()}  gap to the threshold {gap:.4f}  {len(tracks)} tracks  ({time.time() - t0:.0f} s)")
        if gap > E2E_MARGIN and seed == first:
            out["e2e"] = {"seed": int(seed), "gap": gap, "margin": E2E_MARGIN, "heights": [float(x) for x in h]}
            break
        if gap > E2E_MARGIN:
            # another seed than the PyanNet goldens': its frames must be clear of the segmentation margin as well
            starts, _ = overlap.chunk_plan(wave.shape[0])
            lp = porc.forward(sd_seg, torch.from_numpy(overlap.cut_chunks(wave, starts))).numpy()
            if porc.margins(lp).min() >= porc.MARGIN_FACTOR * porc.calibration()["logp_device_bound"]:
                out["e2e"] = {"seed": int(seed), "gap": gap, "margin": E2E_MARGIN, "heights": [float(x) for x in h]}
                break
    assert "e2e" in out, "no end-to-end clip clear of the threshold"
    path = orc.CALIBRATION
    with open(path, "w") as f:
        json.dump(out, f)
        f.write("\n")
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {time.time() - t0:.0f} s)")


if __name__ == "__main__":
    main()
