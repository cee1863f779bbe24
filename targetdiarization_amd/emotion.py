"""emotion2vec over the C-ABI (tdx_emo2v_*): funasr's `AutoModel(model=emotion_model_dir)` and its call
`self.emotion(wav_file, granularity="utterance", extract_embedding=False)` behind the reference's `emotion_detection`
(ASRProcessor.py:277-283, :935-973).  A data2vec 2.0 audio encoder (7 strided convolutions, a grouped positional convolution
stack, post-LN transformer blocks with a symmetric ALiBi bias and 10 learned prefix tokens) and a 9-way head, fp32.

    m = Emotion2vec(state_dict, "cuda:0")                       # funasr's model.pt tensors, upstream names
    res = m.generate([wav0, wav1], granularity="utterance")     # [{"key", "labels", "scores"[, "feats"]}, ...]
    feats = m.features([wav0])                                  # [T_i, D] device tensors

Neither funasr nor the checkpoint is available here: the model, the parameter names (weights.EMOTION2VEC_NAMES, the one table
a correction goes into) and the labels are restated from upstream, and parity with iic/emotion2vec_plus_large is unpinned; what
the tests pin is a float64 torch restatement of the same steps, whose convolutional front end is checked against
transformers' Data2VecAudio modules.  A launch takes clips of equal length (upstream has no padding mask at
batch 1): clips are bucketed by exact length."""
from __future__ import annotations

import os
import re

import numpy as np
import torch

from . import _lib
from .weights import (EMOTION2VEC_BLOCK_LEAVES, EMOTION2VEC_IGNORED, EMOTION2VEC_NAMES, emotion2vec_config, emotion2vec_frames,
                      emotion2vec_param_shapes, emotion2vec_upstream_name, pack_blob)

PARAM_NAMES = EMOTION2VEC_NAMES
# the 9 lines of the checkpoint's tokens.txt [upstream-recall]
DEFAULT_LABELS = ("生气/angry", "厌恶/disgusted", "恐惧/fearful", "开心/happy", "中立/neutral", "其他/other", "难过/sad", "吃惊/surprised", "<unk>")
MIN_SAMPLES = 400


def ignored_key(name: str) -> bool:
    return "mask_emb" in name or any(name.startswith(p) for p in EMOTION2VEC_IGNORED)


def _indices(state_dict, blob_pattern: str):
    """the sorted indices n (as the blob counts them) for which a key matching the pattern's upstream name exists"""
    up, off = next((u, o) for p, u, o in PARAM_NAMES if p == blob_pattern)
    rx = re.compile("^" + re.escape(up).replace(r"\{n\}", r"(\d+)"))
    return sorted({int(m.group(1)) - off for k in state_dict for m in [rx.match(k)] if m})


def infer_config(state_dict, config=None) -> dict:
    """The sizes read from the tensors: D from proj.weight, H from alibi_scale, E from extra_tokens, the depths from the block
    indices, C, the kernels and the group count from the convolution shapes.  Strides are not in the weights: they come from
    `config` (conv_strides) or default to (5, 2, 2, 2, 2, 2, 2).  A missing tensor is named."""
    up = emotion2vec_upstream_name

    def need(name):
        if name not in state_dict:
            raise _lib.TdxError(f"emotion2vec: tensor missing: {name}")
        return state_dict[name]

    head = need(up("head.weight"))
    if head.dim() != 2:
        raise _lib.TdxError(f"emotion2vec: wrong shape: {up('head.weight')} is {tuple(head.shape)}, expected [classes, D]")
    D = int(head.shape[1])
    convs = _indices(state_dict, "conv.{n}.weight")
    if not convs or convs != list(range(len(convs))):
        raise _lib.TdxError(f"emotion2vec: tensor missing: {up('conv.{n}.weight', 0)} (conv layers found: {convs})")
    w0 = need(up("conv.{n}.weight", 0))
    kernels = tuple(int(need(up("conv.{n}.weight", i)).shape[-1]) for i in convs)
    pos = _indices(state_dict, "pos.{n}.weight")
    if not pos or pos != list(range(len(pos))):
        raise _lib.TdxError(f"emotion2vec: tensor missing: {up('pos.{n}.weight', 0)} (positional layers found: {pos})")
    pw = need(up("pos.{n}.weight", 0))
    if pw.dim() != 3 or int(pw.shape[1]) < 1 or D % int(pw.shape[1]):
        raise _lib.TdxError(f"emotion2vec: wrong shape: {up('pos.{n}.weight', 0)} is {tuple(pw.shape)}, expected [D, D / groups, k] with D = {D}")
    pre = _indices(state_dict, "prenet.blocks.{n}.")
    main = _indices(state_dict, "blocks.{n}.")
    for name, idx in (("context_encoder.blocks", pre), ("blocks", main)):
        if idx != list(range(len(idx))):
            raise _lib.TdxError(f"emotion2vec: tensor missing: the indices of {name} are {idx}, not 0 .. {len(idx) - 1}")
    c = dict(config or {})
    got = {"C": int(w0.shape[0]), "D": D, "H": int(need(up("alibi_scale")).numel()), "E": int(need(up("extra_tokens")).shape[-2]),
           "prenet_depth": len(pre), "depth": len(main), "conv_kernels": kernels, "pos_layers": len(pos), "pos_k": int(pw.shape[2]),
           "pos_groups": D // int(pw.shape[1]), "n_classes": int(head.shape[0])}
    for k, v in got.items():
        if k in c and (tuple(c[k]) if k == "conv_kernels" else int(c[k])) != v:
            raise _lib.TdxError(f"emotion2vec: config says {k} = {c[k]}, the tensors say {v}")
    c.update(got)
    if "conv_strides" in c and len(c["conv_strides"]) != len(kernels):
        raise _lib.TdxError(f"emotion2vec: {len(kernels)} conv layers but {len(c['conv_strides'])} strides in the config")
    if "conv_strides" not in c and len(kernels) > 7:
        raise _lib.TdxError(f"emotion2vec: {len(kernels)} conv layers: the strides must come from the config")
    return emotion2vec_config(c)


def to_blob_state(state_dict, cfg) -> dict:
    """upstream names -> the names of the TDXW blob (PARAM_NAMES).  Ignored prefixes are dropped; every listed tensor is
    required with its strict shape; anything else is an error.  Errors name the upstream key."""
    shapes = emotion2vec_param_shapes(cfg)
    sd = {k: v for k, v in state_dict.items() if not ignored_key(k)}
    for name, shp in shapes.items():
        if name not in sd:
            raise _lib.TdxError(f"emotion2vec: tensor missing: {name}")
        if tuple(sd[name].shape) != tuple(shp):
            raise _lib.TdxError(f"emotion2vec: wrong shape: {name} is {tuple(sd[name].shape)}, expected {tuple(shp)}")
    extra = [k for k in sd if k not in shapes]
    if extra:
        raise _lib.TdxError(f"emotion2vec: unexpected tensor: {extra[0]}")
    out = {}
    counts = {"conv.": len(cfg["conv_kernels"]), "pos.": cfg["pos_layers"], "prenet.blocks.": cfg["prenet_depth"], "blocks.": cfg["depth"]}
    for pat, _, _ in PARAM_NAMES:
        if "{n}" not in pat:
            out[pat] = sd[emotion2vec_upstream_name(pat)]
            continue
        n = counts[pat.split("{n}")[0]]
        leaves = [""] if not pat.endswith("{n}.") else [f"{leaf}.{wb}" for leaf in EMOTION2VEC_BLOCK_LEAVES for wb in ("weight", "bias")]
        for i in range(n):
            for leaf in leaves:
                out[pat.replace("{n}", str(i)) + leaf] = sd[emotion2vec_upstream_name(pat, i, leaf)]
    return out


def load_state_dict(model_dir: str):
    """(state dict, labels or None) of a funasr model directory: model.pt through torch.load(weights_only=True), its ["model"]
    or ["state_dict"] when present; tokens.txt, one label per line, when present"""
    obj = torch.load(os.path.join(model_dir, "model.pt"), map_location="cpu", weights_only=True)
    for k in ("model", "state_dict"):
        if isinstance(obj, dict) and k in obj and isinstance(obj[k], dict):
            obj = obj[k]
            break
    labels = None
    tok = os.path.join(model_dir, "tokens.txt")
    if os.path.isfile(tok):
        with open(tok, encoding="utf-8") as f:
            labels = [ln.rstrip("\n") for ln in f if ln.strip()]
    return obj, labels


def bucket_by_length(lengths):
    """{length: [clip indices in call order]} in order of first appearance"""
    out = {}
    for i, n in enumerate(lengths):
        out.setdefault(int(n), []).append(i)
    return out


class Emotion2vec:
    def __init__(self, state_dict, device="cuda:0", config=None, labels=None, workspace_budget_bytes: int = 8 << 30):
        self._l = _lib.lib()
        self.cfg = infer_config(state_dict, config)
        c = self.cfg
        self.labels = list(labels) if labels is not None else list(DEFAULT_LABELS)
        if len(self.labels) != c["n_classes"]:
            raise _lib.TdxError(f"Emotion2vec: {len(self.labels)} labels for a head of {c['n_classes']} classes")
        self.workspace_budget_bytes = int(workspace_budget_bytes)
        cc = _lib.Emo2vConfig()
        cc.C, cc.D, cc.H, cc.E, cc.prenet_depth, cc.depth = c["C"], c["D"], c["H"], c["E"], c["prenet_depth"], c["depth"]
        if len(c["conv_kernels"]) > 8:
            raise _lib.TdxError("Emotion2vec: at most 8 conv layers")
        cc.n_conv = len(c["conv_kernels"])
        for i, (k, s) in enumerate(zip(c["conv_kernels"], c["conv_strides"])):
            cc.conv_k[i], cc.conv_s[i] = k, s
        cc.pos_layers, cc.pos_k, cc.pos_groups, cc.n_classes = c["pos_layers"], c["pos_k"], c["pos_groups"], c["n_classes"]
        blob = pack_blob(to_blob_state(state_dict, c))
        self._own = _lib.Handle(device, "Emotion2vec", self._l.tdx_emo2v_create, self._l.tdx_emo2v_destroy, _lib.C.byref(cc), blob=blob)
        self.device, self._h, self._guard = self._own.device, self._own.ptr, self._own.guard

    def frames(self, n: int) -> int:
        return emotion2vec_frames(n, self.cfg)

    # ---- one launch: B clips of equal length, already on the device as [B, N]
    def launch(self, x, feats=None, emb=None, scores=None, taps=(None, None, None, None)):
        """enqueue tdx_emo2v_forward on the current stream (inside `with self._guard.call():`; tools/emotion2vec_bench.py times
        this).  taps: (projection [B,T,D], x + P(x) [B,T,D], first block's qkv [B,S,3D], first block's attention [B,S,D])."""
        B, N = x.shape
        ws = self._guard.workspace(int(self._l.tdx_emo2v_workspace_bytes(self._h, B, N)))
        st = torch.cuda.current_stream(self.device).cuda_stream
        p = lambda t: t.data_ptr() if t is not None else None
        if any(t is not None for t in taps):
            _lib.check(self._l.tdx_emo2v_forward_taps(self._h, x.data_ptr(), B, N, p(feats), p(emb), p(scores), *[p(t) for t in taps],
                                                      ws.data_ptr(), ws.numel(), st))
        else:
            _lib.check(self._l.tdx_emo2v_forward(self._h, x.data_ptr(), B, N, p(feats), p(emb), p(scores), ws.data_ptr(), ws.numel(), st))

    def _plan(self, arrs, keys):
        """[(N, [clip indices])]: buckets of equal length cut into sub-batches whose workspace fits the budget"""
        if not self._h:
            raise _lib.TdxError("Emotion2vec: the model is closed")
        for a, k in zip(arrs, keys):
            if a.size < MIN_SAMPLES or self.frames(a.size) < 1:
                raise _lib.TdxError(f"Emotion2vec: clip {k!r} has {a.size} samples; at least {MIN_SAMPLES} are needed for one frame")
        plan = []
        for n, idx in bucket_by_length([a.size for a in arrs]).items():
            one = int(self._l.tdx_emo2v_workspace_bytes(self._h, 1, n))
            if one == 0 or one > self.workspace_budget_bytes:
                raise _lib.TdxError(f"Emotion2vec: clip {keys[idx[0]]!r} of {n} samples needs a workspace of {one} bytes; the budget is "
                                    f"{self.workspace_budget_bytes}")
            bmax = max(1, min(len(idx), self.workspace_budget_bytes // one))
            while bmax > 1 and int(self._l.tdx_emo2v_workspace_bytes(self._h, bmax, n)) > self.workspace_budget_bytes:
                bmax -= 1
            plan += [(n, idx[i:i + bmax]) for i in range(0, len(idx), bmax)]
        return plan

    def _run(self, wavs, keys, want_feats: bool, want_emb: bool, want_scores: bool, taps=None):
        arrs = [np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(-1)) for w in wavs]
        c = self.cfg
        out = [dict() for _ in arrs]
        with torch.cuda.device(self.device), self._guard.call():
            for n, idx in self._plan(arrs, keys):
                B, T, S = len(idx), self.frames(n), c["E"] + self.frames(n)
                x = torch.from_numpy(np.stack([arrs[i] for i in idx])).to(self.device)
                new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
                feats = new(B, T, c["D"]) if want_feats else None
                emb = new(B, c["D"]) if want_emb else None
                scores = new(B, c["n_classes"]) if want_scores else None
                tp = (None,) * 4
                if taps is not None:
                    tp = (new(B, T, c["D"]), new(B, T, c["D"]), new(B, S, 3 * c["D"]), new(B, S, c["D"]))
                self.launch(x, feats, emb, scores, tp)
                for j, i in enumerate(idx):
                    if want_feats:
                        out[i]["feats"] = feats[j]
                    if want_emb:
                        out[i]["emb"] = emb[j]
                    if want_scores:
                        out[i]["scores"] = scores[j]
                    if taps is not None:
                        out[i]["taps"] = dict(zip(("proj", "pos", "qkv", "attn"), (t[j] for t in tp)))
        return out

    def features(self, wavs, taps=None):
        """list of [T_i, D] device tensors (funasr's frame-level `feats`).  `taps`: a list that receives, per clip, the dict of
        device tensors proj, pos, qkv, attn (see launch)."""
        res = self._run(wavs, [str(i) for i in range(len(wavs))], True, False, False, taps)
        if taps is not None:
            taps.extend(r["taps"] for r in res)
        return [r["feats"] for r in res]

    def generate(self, wavs, granularity: str = "utterance", extract_embedding: bool = False, keys=None):
        """funasr's result shape: [{"key", "labels", "scores"[, "feats"]}], feats [D] (utterance) or [T, D] (frame) as numpy"""
        if granularity not in ("utterance", "frame"):
            raise ValueError(f"Emotion2vec.generate: granularity must be 'utterance' or 'frame', got {granularity!r}")
        wavs = list(wavs) if isinstance(wavs, (list, tuple)) else [wavs]
        keys = [str(k) for k in keys] if keys is not None else [f"rand_key_{i}" for i in range(len(wavs))]
        if len(keys) != len(wavs):
            raise ValueError("Emotion2vec.generate: one key per clip")
        frame = extract_embedding and granularity == "frame"
        res = self._run(wavs, keys, frame, extract_embedding and not frame, True)
        out = []
        for k, r in zip(keys, res):
            d = {"key": k, "labels": list(self.labels), "scores": [float(v) for v in r["scores"].cpu().tolist()]}
            if extract_embedding:
                d["feats"] = (r["feats"] if frame else r["emb"]).cpu().numpy()
            out.append(d)
        return out

    def __call__(self, wavs, granularity="utterance", extract_embedding=False, **kw):
        return self.generate(wavs, granularity=granularity, extract_embedding=extract_embedding, **kw)

    def close(self):
        self._own.close()


def build_emotion(state_dict=None, config=None, labels=None, model_dir: str = "", cuda_device: int = 0):
    """the model from weights, or from a directory holding model.pt (None when neither is there)"""
    if state_dict is None and isinstance(model_dir, str) and model_dir and os.path.isfile(os.path.join(model_dir, "model.pt")):
        state_dict, file_labels = load_state_dict(model_dir)
        labels = labels if labels is not None else file_labels
    if state_dict is None:
        return None
    return Emotion2vec(state_dict, device=f"cuda:{cuda_device}", config=config, labels=labels)
