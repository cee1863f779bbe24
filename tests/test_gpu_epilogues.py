"""-m gpu: the shared GEMM epilogue family (csrc/epilogues.hpp: EpiBiasAct, EpiBiasActN, EpiBiasRes, EpiBiasResN) reached
directly through the diag hook tdx_linear_epi, on the exact-fp32 MFMA core.

Reference: torch in fp64 on the CPU, out = act((A W^T + b) + res).  Bar: rel-L2 < 2e-6 — the bar test_linear_vs_fp64
(test_gpu_mossformer2.py) holds this core to at up to ten times this K.  M = 130 is one full 128-row tile plus two rows (the
row-checked epilogue path); Npad/nreal cover an unguarded width, a guard inside the only column tile and a guard inside the
second of two.  out has two extra rows and is pre-filled with 7.0: rows >= M and columns >= nreal must come back untouched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0")
M = 130
ACTS = {
    0: lambda x: x,
    1: lambda x: x.clamp(min=0.0),
    2: lambda x: x.clamp(0.0, 20.0),
    3: lambda x: x * torch.sigmoid(x),
    4: lambda x: torch.where(x >= 0, x, 0.01 * x),
}


@pytest.fixture(scope="module")
def diag():
    from targetdiarization_amd import _lib
    return _lib.diag()


@pytest.mark.parametrize("K", [32, 96])
@pytest.mark.parametrize("Npad,nreal", [(128, 128), (128, 100), (256, 200)])
def test_epilogue_family_vs_fp64(diag, Npad, nreal, K):
    g = torch.Generator(device="cpu").manual_seed(1000 * Npad + 10 * nreal + K)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(Npad, K, generator=g) * (8.0 / K ** 0.5)         # pre-activations of std ~8: ReLU20 clamps on both sides
    bias = torch.randn(Npad, generator=g) * 2.0
    res = torch.randn(M, Npad, generator=g) * 4.0
    pre = a.double() @ w.double().T                                   # shared by every case below, never modified
    a_d, w_d, bias_d, res_d = a.to(dev), w.to(dev), bias.to(dev), res.to(dev)
    for act, f in ACTS.items():
        for with_bias in (True, False):
            for res_mode in ("none", "separate", "alias"):
                what = f"act={act} bias={with_bias} res={res_mode}"
                ref = pre + bias.double() if with_bias else pre.clone()
                if res_mode != "none":
                    ref = ref + res.double()
                ref = f(ref)[:, :nreal]
                out = torch.full((M + 2, Npad), 7.0, device=dev)
                if res_mode == "alias":
                    out[:M, :nreal] = res_d[:, :nreal]
                res_ptr = {"none": None, "separate": res_d.data_ptr(), "alias": out.data_ptr()}[res_mode]
                rc = diag.tdx_linear_epi(a_d.data_ptr(), w_d.data_ptr(), bias_d.data_ptr() if with_bias else None, res_ptr,
                                         out.data_ptr(), M, Npad, nreal, K, act, None)
                assert rc == 0, (what, diag.tdx_diag_last_error())
                got = out.cpu()
                err = float((got[:M, :nreal].double() - ref).norm() / ref.norm())
                print(f"{what} Npad={Npad} nreal={nreal} K={K}: rel-L2 {err:.3e}")
                assert err < 2e-6, (what, err)
                assert bool((got[M:] == 7.0).all()), what + ": rows >= M were written"
                assert bool((got[:, nreal:] == 7.0).all()), what + ": columns >= nreal were written"


def test_bad_arguments_are_refused(diag):
    x = torch.zeros(256, 128, device=dev)
    p = x.data_ptr()
    assert diag.tdx_linear_epi(p, p, None, None, p, 4, 100, 100, 32, 0, None) != 0       # Npad not a multiple of 128
    assert diag.tdx_linear_epi(p, p, None, None, p, 4, 128, 129, 32, 0, None) != 0       # nreal beyond Npad
    assert diag.tdx_linear_epi(p, p, None, None, p, 4, 128, 128, 32, 5, None) != 0       # unknown activation
