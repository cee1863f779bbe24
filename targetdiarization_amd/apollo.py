"""Apollo band-split RoFormer restorer over the C-ABI (tdx_apollo_*): the model the reference builds in
`AudioProcessor.init_restorer_model` (AudioProcessor.py:277-281; look2hear/models/apollo.py, sr=44100, win=20, feature_dim=256,
layer=6) and runs in `restore_audio` (:959-980).

    rest = ApolloRestorer(state_dict, device="cuda:0")        # the reference's state-dict names (BaseModel.from_pretrain format)
    outs = rest([clip0, clip1, ...])                          # 1-D float32 device tensors at 44.1 kHz -> list of the same shapes

Clips are independent (the reference runs the channels of [1, C, n] as batch items).  Device memory is bounded by
`rows_per_launch` (token rows = 80 per STFT frame): whole clips are batched up to the budget, a longer clip is cut into frame
windows with a 54-frame halo on each cut side (the net's receptive field), whose outputs are exact.  No trained checkpoint ships
with the reference; tests and tools use weights.recipe_apollo_state_dict."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .weights import pack_blob

HOP, HALO, MAX_ITEMS, MIN_SAMPLES = 441, 54, 64, 442


def frames_of(n: int) -> int:
    return 1 + n // HOP


def load_state_dict(weights_folder: str):
    """`BaseModel.from_pretrain` (base_model.py:52-64): torch.load(<folder>/pytorch_model.bin)["state_dict"]"""
    conf = torch.load(os.path.join(weights_folder, "pytorch_model.bin"), map_location="cpu", weights_only=False)
    return conf["state_dict"]


class ApolloRestorer:
    def __init__(self, state_dict, device="cuda:0", num_layers: int = 6, rows_per_launch: int = 1 << 19):
        self._l = _lib.lib()
        self.num_layers = num_layers
        self.max_frames = int(rows_per_launch) // 80
        if self.max_frames < 2 * (HALO + 1) + 1:
            raise _lib.TdxError(f"ApolloRestorer: rows_per_launch must hold at least {80 * (2 * HALO + 3)} rows")
        self._own = _lib.Handle(device, "ApolloRestorer", self._l.tdx_apollo_create, self._l.tdx_apollo_destroy, num_layers, blob=pack_blob(state_dict))
        self.device, self._h, self._guard = self._own.device, self._own.ptr, self._own.guard

    def eval(self):
        return self

    def flops(self, lengths) -> float:
        """model FLOPs of restoring clips of these lengths (halo recomputation of cut clips not counted)"""
        return float(sum(self._l.tdx_apollo_flops(self._h, frames_of(int(n))) for n in lengths))

    def plan(self, lengths):
        """launches as lists of items (clip, frame_lo, frame_hi, sample_lo, sample_hi), each launch <= max_frames frames"""
        items = []
        for c, n in enumerate(lengths):
            T = frames_of(n)
            if T <= self.max_frames:
                items.append((c, 0, T, 0, n))
                continue
            step = self.max_frames - 2 * HALO - 1           # owned frames per window
            for a in range(0, T, step):
                b = min(T, a + step)
                items.append((c, max(0, a - HALO), min(T, b + HALO + 1), a * HOP, n if b == T else b * HOP))
        launches, cur, fr = [], [], 0
        for it in items:
            f = it[2] - it[1]
            if cur and (fr + f > self.max_frames or len(cur) == MAX_ITEMS):
                launches.append(cur); cur, fr = [], 0
            cur.append(it); fr += f
        if cur:
            launches.append(cur)
        return launches

    def __call__(self, clips):
        """list of 1-D float32 device tensors (44.1 kHz, >= 442 samples each) -> list of restored 1-D device tensors"""
        clips = [c.to(self.device, torch.float32).reshape(-1) for c in clips]
        if not clips:
            return []
        lens = [int(c.shape[0]) for c in clips]
        if min(lens) < MIN_SAMPLES:
            raise _lib.TdxError(f"ApolloRestorer: every clip needs >= {MIN_SAMPLES} samples (the STFT's reflect pad), got {min(lens)}")
        lens_h = (C.c_int64 * len(lens))(*lens)
        with torch.cuda.device(self.device), self._guard.call():
            x = torch.cat(clips) if len(clips) > 1 else clips[0].contiguous()
            y = torch.empty_like(x)
            st = torch.cuda.current_stream(self.device).cuda_stream
            for launch in self.plan(lens):
                frames = sum(it[2] - it[1] for it in launch)
                items = np.asarray(launch, dtype=np.int32).reshape(-1)
                it_h = (C.c_int32 * items.size)(*items.tolist())
                nb = int(self._l.tdx_apollo_workspace_bytes(self._h, frames))
                ws = self._guard.workspace(nb)
                _lib.check(self._l.tdx_apollo_forward(self._h, x.data_ptr(), lens_h, len(lens), it_h, len(launch), y.data_ptr(),
                                                      ws.data_ptr(), ws.numel(), st))
        return list(y.split(lens))

    def close(self):
        self._own.close()
