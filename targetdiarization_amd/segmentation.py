"""PyanNet: pyannote segmentation-3.0 on the device over the C-ABI (tdx_pyannet_*, csrc/pyannet.hip) — the network inside
`self.od_pipeline` (TargetDiarization.py:84,132,143).  Third-party model, restated from the published code
[upstream-recall]; parity with the published checkpoint is unpinned (none is at hand).  16 kHz chunks [B,T] in, per frame
(270 samples) the log-probabilities of the 7 powerset classes out; overlap.py builds speaker tracks from them."""
from __future__ import annotations

import torch

from . import _lib
from .weights import pack_pyannet_blob

NUM_CLASSES = 7
T_MIN, T_MAX = 1261, 160000


class PyanNet:
    """state_dict: pyannote's names (sincnet.*, lstm.*, linear.*, classifier.*)."""

    def __init__(self, state_dict, device="cuda:0", max_chunks_per_launch: int = 64):
        self._l = _lib.lib()
        self._own = _lib.Handle(device, "PyanNet", self._l.tdx_pyannet_create, self._l.tdx_pyannet_destroy, blob=pack_pyannet_blob(state_dict))
        self.device, self._h, self._guard = self._own.device, self._own.ptr, self._own.guard
        self.max_chunks_per_launch = int(max_chunks_per_launch)
        self.chunk_tile = int(self._l.tdx_pyannet_chunk_tile())          # chunks per workgroup of the recurrence kernel

    def frames(self, T: int) -> int:
        return int(self._l.tdx_pyannet_frames(int(T)))

    def workspace_bytes(self, B: int, T: int) -> int:
        return int(self._l.tdx_pyannet_workspace_bytes(self._h, int(B), int(T)))

    def flops(self, B: int, T: int) -> float:
        return float(self._l.tdx_pyannet_flops(self._h, int(B), int(T)))

    def forward_into(self, wav, logp, tap_sincnet=None, tap_lstm=None, ws=None):
        """the bare C call on the current stream: wav [B,T] float32 (device, contiguous), logp [B,F,7], taps None or
        [B,F,60] / [B,F,256]; ws: a uint8 device tensor of workspace_bytes(B, T) (None: the object's grow-only workspace;
        hold `self._guard.call()` around it then).  No allocation when ws is given: this is what a graph capture records."""
        B, T = int(wav.shape[0]), int(wav.shape[1])
        if ws is None:
            ws = self._guard.workspace(self.workspace_bytes(B, T))
        st = torch.cuda.current_stream(self.device).cuda_stream
        ptr = lambda t: t.data_ptr() if t is not None else None
        _lib.check(self._l.tdx_pyannet_forward(self._h, wav.data_ptr(), B, T, logp.data_ptr(), ptr(tap_sincnet), ptr(tap_lstm),
                                               ws.data_ptr(), ws.numel(), st))

    def log_probs(self, chunks, taps: bool = False):
        """chunks [B,T] device tensor -> log-probabilities [B,F,7] (device); taps: (logp, sincnet [B,F,60], lstm [B,F,256]).
        B is split into launches of at most max_chunks_per_launch chunks."""
        if chunks.ndim != 2 or chunks.device != self.device:
            raise _lib.TdxError(f"PyanNet.log_probs: chunks must be [B,T] on {self.device}")
        B, T = int(chunks.shape[0]), int(chunks.shape[1])
        F = self.frames(T)
        if F == 0:
            raise _lib.TdxError(f"PyanNet: T = {T} outside [{T_MIN}, {T_MAX}]")
        x = chunks.to(torch.float32).contiguous()
        with torch.cuda.device(self.device):
            logp = torch.empty(B, F, NUM_CLASSES, device=self.device)
            ts = torch.empty(B, F, 60, device=self.device) if taps else None
            tl = torch.empty(B, F, 256, device=self.device) if taps else None
            with self._guard.call():
                for a in range(0, B, self.max_chunks_per_launch):
                    b = min(B, a + self.max_chunks_per_launch)
                    self.forward_into(x[a:b], logp[a:b], ts[a:b] if taps else None, tl[a:b] if taps else None)
        return (logp, ts, tl) if taps else logp

    def close(self):
        self._own.close()
