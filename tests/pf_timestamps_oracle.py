"""CPU restatement of Paraformer's upsampling timestamp predictor (the second head of funasr's CifPredictorV3 and
ts_prediction_lfr6_standard), in plain torch, written from the formulas of DESIGN §8.16 — checker only, never imported by the
product.  Third-party architecture restated from memory of the published code: parity with funasr is unpinned.  Runs in the
dtype of its inputs (fp32 or fp64)."""
import torch
import torch.nn.functional as F

THRESHOLD = 1.0 - 1e-4


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def cif_alphas(enc, sd, residual: bool):
    """the main predictor branch up to the alphas with the tail frame appended (CifPredictorV2: residual; V3: none): [B,T+1]"""
    ctx = enc.transpose(1, 2)
    mem = F.conv1d(F.pad(ctx, (1, 1)), sd["predictor.cif_conv1d.weight"], sd["predictor.cif_conv1d.bias"])
    out = F.relu((mem + ctx) if residual else mem).transpose(1, 2)
    a = torch.sigmoid(F.linear(out, sd["predictor.cif_output.weight"], sd["predictor.cif_output.bias"]))[..., 0]
    return torch.cat((a, torch.full((enc.shape[0], 1), 0.45, dtype=enc.dtype)), dim=1)


def cif_wo_hidden(alphas, threshold: float = THRESHOLD):
    """alphas [B,U] -> the running integral at every frame [B,U], reset by `threshold` where it reaches it (sequential, in alphas' dtype)"""
    thr = torch.tensor(threshold, dtype=alphas.dtype)
    integ = torch.zeros(alphas.shape[0], dtype=alphas.dtype)
    out = []
    for u in range(alphas.shape[1]):
        integ = integ + alphas[:, u]
        out.append(integ)
        integ = torch.where(integ >= thr, integ - thr, integ)
    return torch.stack(out, 1)


def upsampled_head(enc, counts, sd, smooth: float = 0.25, noise: float = 0.01):
    """enc [B,T,512], counts [B] -> dict(tap [B,3T,1024], raw [B,3T], alphas [B,3T], peaks [B,3T])"""
    dt = enc.dtype
    y = F.conv_transpose1d(enc.transpose(1, 2), sd["predictor.upsample_cnn.weight"], sd["predictor.upsample_cnn.bias"], stride=3).transpose(1, 2)
    lstm = torch.nn.LSTM(512, 512, 1, batch_first=True, bidirectional=True).to(dt)
    with torch.no_grad():
        for n, p in lstm.named_parameters():
            p.copy_(sd["predictor.blstm." + n])
        tap, _ = lstm(y)
    z = F.linear(tap, sd["predictor.cif_output2.weight"], sd["predictor.cif_output2.bias"])[..., 0]
    raw = F.relu(smooth * torch.sigmoid(z) - noise)
    s = raw.sum(-1)
    scale = torch.where(s > 0, counts.to(dt) / s, torch.ones_like(s))
    alphas = raw * scale[:, None]
    return {"tap": tap, "raw": raw, "alphas": alphas, "peaks": cif_wo_hidden(alphas)}


def timestamps(alphas, peaks, nchars: int, shift: float = -1.5, rate: int = 3):
    """ts_prediction_lfr6_standard for one clip and nchars characters (none of them </s>) -> [[start_ms, end_ms]] per character"""
    if nchars == 0:
        return []
    tr = 0.06 / rate
    fire = [u + shift for u in range(peaks.shape[0]) if peaks[u] >= THRESHOLD]
    if len(fire) != nchars + 1 and float(alphas.sum()) > 0:
        a = alphas / (alphas.sum() / (nchars + 1))
        peaks = cif_wo_hidden(a[None])[0]
        fire = [u + shift for u in range(peaks.shape[0]) if peaks[u] >= THRESHOLD]
    if not fire:
        return []
    U = peaks.shape[0]
    ent = []                                       # (is_token, start, end) in frames
    if fire[0] > 5:
        ent.append([False, 0.0, fire[0]])
    for i in range(min(len(fire) - 1, nchars)):
        if fire[i + 1] - fire[i] <= 12:
            ent.append([True, fire[i], fire[i + 1]])
        else:
            ent.append([True, fire[i], fire[i] + 12])
            ent.append([False, fire[i] + 12, fire[i + 1]])
    if U - fire[-1] > 5:
        mid = (U + fire[-1]) * 0.5
        if ent:
            ent[-1][2] = mid
        ent.append([False, mid, float(U)])
    elif ent:
        ent[-1][2] = float(U)
    return [[int(s * tr * 1000), int(e * tr * 1000)] for tok, s, e in ent if tok]


def decode_timestamps(enc, sd, num_blocks: int, eos_id: int = 2):
    """Paraformer.inference after the encoder with the V3 predictor: per clip (token count kept, timestamps, head outputs)"""
    from oracle import paraformer_oracle as po
    B, T, _ = enc.shape
    alphas = cif_alphas(enc, sd, residual=False)
    hidden = torch.cat((enc, torch.zeros(B, 1, 512, dtype=enc.dtype)), dim=1)
    fired, _ = po.cif(hidden, alphas)
    counts = torch.floor(alphas.sum(-1)).long()
    L = int(counts.max())
    emb = torch.zeros(B, L, 512, dtype=enc.dtype)
    for b in range(B):
        n = min(int(counts[b]), fired[b].shape[0])
        emb[b, :n] = fired[b][:n]
    ids = po.sanm_decoder_forward(emb, counts, enc, sd, num_blocks).argmax(-1)
    head = upsampled_head(enc, counts, sd)
    res = []
    for b in range(B):
        n = int(counts[b])
        if n > 0 and int(ids[b, n - 1]) == eos_id:
            n -= 1
        ts = timestamps(head["alphas"][b], head["peaks"][b], n)
        res.append((min(n, len(ts)), ts))
    return res, counts, head
