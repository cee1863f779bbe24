"""-m gpu: the fp32-A operand form of the split-f16 x3 core (csrc/gemm_h3f.hpp: fp32 NHWC rows split with a static scale while they are
staged) through the diag hook tdx_h3_gemm_f32a.  For every shape and value range the result must be BIT-IDENTICAL to the two-launch path
it replaces — tdx_h3_split_rows_static, then the planes GEMM of tdx_h3_gemm_ex (A_CONV, one tap, sa_mul = 0) on the same data — and
within the bar tests/test_gpu_h3.py holds against an fp64 product (rel-L2 < 2e-6).  Shapes: K = 64 .. 512 (4 .. 32 k-tiles: the
rings are deeper than the shortest loop), N = 96 -> 128 and 192 -> 256 padded weights with nreal, 256, 512, M not a multiple of 256,
and a stride-2 case with odd H and W (5 x 17 pixels -> 3 x 9)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
GUARD, SENT, NAN = 3, 7.0, float("nan")

# (B, Hin, Win, stride, K, N, lda)
CASES = [
    (1, 1, 720, 1, 64, 96, 64),
    (1, 1, 1360, 1, 96, 256, 96),
    (1, 1, 257, 1, 192, 512, 192),
    (1, 1, 513, 1, 256, 192, 256),
    (1, 1, 300, 1, 512, 192, 544),       # rows with a pitch beyond K
    (11, 5, 17, 2, 256, 192, 256),       # stride 2, odd H and W: 11 x 3 x 9 = 297 rows in two M tiles
]
RANGES = [((0.0, 20.0), 1024.0), ((-40.0, 40.0), 512.0)]      # the model's two static scales: ReLU20 outputs, sums of two


@pytest.fixture(scope="module")
def diag():
    from targetdiarization_amd import _lib
    return _lib.diag()


def _weights(diag, N, K, seed):
    """weight planes [Npad][4K] + row scales, rows >= N zero (as the model pads its 1x1 weights to a multiple of 128)"""
    Npad = (N + 127) // 128 * 128
    w = torch.zeros(Npad, K)
    w[:N] = torch.randn(N, K, generator=torch.Generator().manual_seed(seed)) / K ** 0.5
    w = w.to(dev)
    P = torch.empty(Npad, 4 * K, dtype=torch.uint8, device=dev)
    s = torch.empty(Npad, device=dev)
    assert diag.tdx_h3_split_rows(w.data_ptr(), K, P.data_ptr(), s.data_ptr(), Npad, K, None) == 0, diag.tdx_diag_last_error()
    return w, P, s, Npad


def _out(M, Npad, N):
    out = torch.full((M + GUARD, Npad), SENT, device=dev)
    out[:M, :N] = NAN
    return out


@pytest.mark.parametrize("rng", RANGES, ids=["0_20_s1024", "pm40_s512"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%dx%dx%d_s%d_K%d_N%d" % c[:6])
def test_f32a_matches_split_then_planes_gemm(diag, case, rng):
    from targetdiarization_amd._lib import H3Seg
    B, Hin, Win, stride, K, N, lda = case
    (lo, hi), a_mul = rng
    Hout, Wout = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    M, R = B * Hout * Wout, B * Hin * Win
    g = torch.Generator().manual_seed(1000 * K + N + int(a_mul))
    x = torch.full((R, lda), NAN)
    x[:, :K] = torch.rand(R, K, generator=g) * (hi - lo) + lo
    x[0, 0], x[R - 1, K - 1] = hi, lo                 # the ends of the range
    x = x.to(dev)
    w, Pw, sw, Npad = _weights(diag, N, K, K + N)
    inv = torch.full((1,), 1.0 / a_mul, device=dev)

    # the path it replaces: one split pass over every pixel row, then the planes GEMM (implicit 1x1 convolution)
    Px = torch.empty(R, 4 * K, dtype=torch.uint8, device=dev)
    assert diag.tdx_h3_split_rows_static(x.data_ptr(), lda, Px.data_ptr(), R, K, a_mul, None) == 0, diag.tdx_diag_last_error()
    zero_row = torch.zeros(4 * K, dtype=torch.uint8, device=dev)
    seg = H3Seg()
    seg.A, seg.B, seg.sa, seg.sb, seg.lda, seg.ldb, seg.K, seg.zdiv, seg.sa_mul, seg.sb_mul = \
        Px.data_ptr(), Pw.data_ptr(), inv.data_ptr(), sw.data_ptr(), 4 * K, 4 * K, K, 1, 0, 1
    ref = _out(M, Npad, N)
    rc = diag.tdx_h3_gemm_ex(0, 0, 0, 1, C.byref(seg), None, M, Npad, 0, 1, Hin, Win, Hout, Wout, stride, 1, K, 0, zero_row.data_ptr(),
                             ref.data_ptr(), Npad, 0, N, None, None)
    assert rc == 0, diag.tdx_diag_last_error()

    out = _out(M, Npad, N)
    rc = diag.tdx_h3_gemm_f32a(x.data_ptr(), lda, a_mul, inv.data_ptr(), Pw.data_ptr(), sw.data_ptr(), M, Npad, K, Hin, Win, Hout, Wout, stride,
                               out.data_ptr(), Npad, N, None)
    assert rc == 0, diag.tdx_diag_last_error()
    torch.cuda.synchronize()

    for name, o in (("planes", ref), ("f32a", out)):
        assert bool((o[M:] == SENT).all()) and bool((o[:M, N:] == SENT).all()), f"{name}: wrote outside the valid region"
        assert bool(torch.isfinite(o[:M, :N]).all()), f"{name}: valid elements not stored or not finite"
    assert torch.equal(out, ref), f"not bit-identical: {int((out != ref).sum())} elements differ, max |d| = {float((out - ref).abs().max())}"

    xs = x[:, :K].reshape(B, Hin, Win, K)[:, ::stride, ::stride].reshape(M, K)
    r64 = xs.double() @ w[:N].double().T
    rel = float((out[:M, :N].double() - r64).norm() / r64.norm())
    print(f"rel-L2 vs fp64 = {rel:.3e}")
    assert rel < 2e-6, rel


def test_f32a_refusals(diag):
    K, N, M = 64, 128, 64
    x = torch.zeros(M, K, device=dev); out = torch.zeros(M, N, device=dev); inv = torch.ones(1, device=dev)
    P = torch.zeros(N, 4 * K, dtype=torch.uint8, device=dev); s = torch.ones(N, device=dev)

    def call(**kw):
        a = dict(lda=K, a_mul=1024.0, M=M, N=N, K=K, Hin=1, Win=M, Hout=1, Wout=M, stride=1, nreal=N)
        a.update(kw)
        return diag.tdx_h3_gemm_f32a(x.data_ptr(), a["lda"], a["a_mul"], inv.data_ptr(), P.data_ptr(), s.data_ptr(), a["M"], a["N"], a["K"],
                                     a["Hin"], a["Win"], a["Hout"], a["Wout"], a["stride"], out.data_ptr(), N, a["nreal"], None)
    assert call() == 0, diag.tdx_diag_last_error()
    for bad in (dict(K=24), dict(lda=K - 4), dict(lda=K + 2), dict(a_mul=0.0), dict(M=M - 1), dict(stride=2), dict(nreal=N + 1), dict(Win=M - 1)):
        assert call(**bad) == 1, bad
        assert diag.tdx_diag_last_error().decode().startswith("tdx_h3_gemm_f32a: "), bad
    torch.cuda.synchronize()
