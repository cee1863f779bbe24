"""-m gpu: the gated attention launch of a FLASH layer on the model's own path, through the diag hook tdx_attn_gate_planes: it calls
attention_core_h3 (csrc/mf2_attention.hpp) as tdx_mf2_forward does, with the planes-out gate EpiAttnGatePlOut on gemm_h3a (the
128-row paired tile with two segments and their scale-domain change, v unpacked from the K-major planes, u in fp32, the exp2 / rcp
sigmoid, the staging tile, one scale and one sum of squares per (token, 128-channel segment), the padding-row predicate, the
default segment swap) or on the wide kernel.  ops.cal_attention never reaches any of that: it stores att_v / att_u in fp32.

Reference: oracle.mossformer2_oracle.cal_attention in fp64, then o = (att_u*v) * sigmoid(att_v*u) in fp64 (attention_gate_ref.py).
Bar: rel-L2 of the reconstruction (hi + lo) * os against it below 3 * err32, err32 = the rel-L2 of the oracle run in torch fp32, per
case; 3 is the margin test_static_scales_under_heavy_tailed_weights gives this gate.  The cases and why each is there are in
test_attention_paths.py (checked there against a mirror of attn_plan / h3a_fits).  Every output buffer has two guard rows in
front of and behind the B*S real ones, pre-filled with a sentinel.

The kernel choice (h3a) and the segment order (swap) are arguments of the hook — in the model they are the process-wide TDX_H3A /
TDX_H3A_SWAP — so the bit-identity claims of gemm_h3a.hpp and mf2_attention.hpp are asserted here in one process:
(h3a=1, swap=0) == (h3a=0) in oP, os, oss and Kvu, and Kvu is the same under every setting."""
import pytest
import torch

import attention_gate_ref as ref
from test_attention_paths import CASES, attn_plan

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0")
GUARD = 2
FILL_F, FILL_B = 7.0, 0x5A
SETTINGS = [(1, 1), (1, 0), (0, 0), (0, 1)]          # (h3a, swap); swap means nothing to the wide kernel


@pytest.fixture(scope="module")
def diag():
    from targetdiarization_amd import _lib
    return _lib.diag()


class Out:
    """oP [GUARD + M + GUARD][4E] bytes, os / oss [GUARD | E/128 x M | GUARD] floats, kvu [B][128][2E]"""

    def __init__(self, B, S, E):
        self.M, self.E, self.nseg = B * S, E, E // 128
        self.oP = torch.full((self.M + 2 * GUARD, 4 * E), FILL_B, dtype=torch.uint8, device=dev)
        self.os = torch.full((self.nseg * self.M + 2 * GUARD,), FILL_F, device=dev)
        self.oss = torch.full((self.nseg * self.M + 2 * GUARD,), FILL_F, device=dev)
        self.kvu = torch.full((B, 128, 2 * E), FILL_F, device=dev)

    def ptrs(self):
        return (self.oP.data_ptr() + GUARD * 4 * self.E, self.os.data_ptr() + 4 * GUARD, self.oss.data_ptr() + 4 * GUARD, self.kvu.data_ptr())

    def guards_intact(self):
        oP, os_, oss = self.oP.cpu(), self.os.cpu(), self.oss.cpu()
        return (bool((oP[:GUARD] == FILL_B).all()) and bool((oP[-GUARD:] == FILL_B).all())
                and all(bool((t[:GUARD] == FILL_F).all()) and bool((t[-GUARD:] == FILL_F).all()) for t in (os_, oss)))

    def planes(self):
        """hi, lo [M][nseg][128] (f16 values as fp64), os, oss [M][nseg] as fp64, on the CPU"""
        p = self.oP[GUARD:-GUARD].cpu().view(torch.float16).reshape(self.M, self.E // 8, 2, 8).double()
        hi, lo = (p[:, :, i].reshape(self.M, self.nseg, 128) for i in (0, 1))
        os_, oss = (t[GUARD:-GUARD].cpu().reshape(self.nseg, self.M).T.double() for t in (self.os, self.oss))
        return hi, lo, os_, oss


def run(diag, case, h3a, swap):
    B, S, E = case
    ts = [t.to(dev) for t in ref.inputs(case)]
    nb = int(diag.tdx_attn_gate_planes_workspace_bytes(B, S, E))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    out = Out(B, S, E)
    rc = diag.tdx_attn_gate_planes(*[t.data_ptr() for t in ts], B, S, E, h3a, swap, *out.ptrs(), ws.data_ptr(), nb, None)
    assert rc == 0, diag.tdx_diag_last_error()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_gate_planes_vs_fp64(diag, case):
    B, S, E = case
    M, nseg = B * S, E // 128
    o64, err32 = ref.reference(case)
    assert err32 > 0
    outs = {}
    for h3a, swap in SETTINGS:
        what = f"{case} h3a={h3a} swap={swap}"
        out = outs[(h3a, swap)] = run(diag, case, h3a, swap)
        hi, lo, os_, oss = out.planes()
        rec = (hi + lo) * os_[:, :, None]
        # ---- accuracy
        err = float((rec.reshape(M, E) - o64).norm() / o64.norm())
        print(f"{what}: kvu launch {attn_plan(*case).kvu if h3a else 'wide'}  rel-L2 {err:.3e}  err32 {err32:.3e}  bar {3 * err32:.3e}")
        assert err < 3 * err32, (what, err, err32)
        # ---- plane format, per (row, segment)
        mant, _ = torch.frexp(os_)
        assert bool((mant == 0.5).all()), what + ": a scale is not a power of two"
        # the scale puts the segment's largest |value| into [2^14, 2^15): asserted on hi + lo, which is that scaled value to 2^-22.
        # |hi| alone is its f16 rounding (spacing 16 there): a value within 8 of 2^15 rounds UP to 2^15 itself (lo < 0), which the
        # (3, 600, 256) case contains — so |hi| is held to [2^14, 2^15], the value itself to the half-open interval.
        himax = hi.abs().amax(dim=2)
        smax = (hi + lo).abs().amax(dim=2)
        zero = (rec == 0).all(dim=2)
        assert bool(((smax >= 2.0 ** 14) & (smax < 2.0 ** 15))[~zero].all()), (what, float(smax[~zero].min()), float(smax[~zero].max()))
        assert bool(((himax >= 2.0 ** 14) & (himax <= 2.0 ** 15))[~zero].all()), (what, float(himax[~zero].min()), float(himax[~zero].max()))
        z = ref.zero_segment(case)
        if z is not None:
            assert bool(zero[z]) and int(zero.sum()) == 1, what + ": the all-zero segment (and only it) must come out as zero"
            assert float(hi[z].abs().max()) == 0.0 and float(lo[z].abs().max()) == 0.0 and float(oss[z]) == 0.0, what
        else:
            assert not bool(zero.any()), what
        # ---- sum of squares over the segment's 128 columns.  Bound: 128 fp32 additions at 2^-24 each (7.6e-6) plus twice the split's
        # 2^-21 relative precision (9.5e-7) = 8.6e-6, doubled
        q = rec.pow(2).sum(dim=2)
        assert bool(((oss - q).abs() <= 2e-5 * q).all()), (what, float(((oss - q).abs() / q.clamp(min=1e-300)).max()))
        # ---- guard rows
        assert out.guards_intact(), what + ": a guard row was written"
    # ---- bit identity
    a, w, d = outs[(1, 0)], outs[(0, 0)], outs[(1, 1)]
    same = {n: torch.equal(getattr(a, n), getattr(w, n)) for n in ("oP", "os", "oss", "kvu")}
    same["kvu(1,1)==kvu(1,0)"] = torch.equal(d.kvu, a.kvu)
    same["kvu(1,1)==kvu(0,0)"] = torch.equal(d.kvu, w.kvu)
    same["(0,1)==(0,0)"] = all(torch.equal(getattr(outs[(0, 1)], n), getattr(w, n)) for n in ("oP", "os", "oss", "kvu"))
    print(f"{case}: (h3a=1, swap=0) against (h3a=0): {same}")
    assert all(same.values()), (case, same)


def test_bad_arguments_are_refused(diag):
    x = torch.zeros(1 << 16, device=dev)
    p = x.data_ptr()
    nb = int(diag.tdx_attn_gate_planes_workspace_bytes(1, 4, 128))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    good = [p] * 7 + [1, 4, 128, 1, 1] + [p] * 4 + [ws.data_ptr(), nb, None]
    assert diag.tdx_attn_gate_planes_workspace_bytes(1, 4, 64) == 0
    bad = list(good); bad[9] = 64
    assert diag.tdx_attn_gate_planes(*bad) != 0                                   # E = 64: not a multiple of 128
    assert b"128" in diag.tdx_diag_last_error()
    bad = list(good); bad[9] = 192
    assert diag.tdx_attn_gate_planes(*bad) != 0
    for i in list(range(7)) + [12, 13, 14, 15, 16]:                               # every pointer
        bad = list(good); bad[i] = None
        assert diag.tdx_attn_gate_planes(*bad) != 0, i
    bad = list(good); bad[17] = nb - 1
    assert diag.tdx_attn_gate_planes(*bad) != 0                                   # workspace too small
    torch.cuda.synchronize()
