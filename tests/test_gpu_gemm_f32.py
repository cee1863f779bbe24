"""The fp32 MFMA GEMM core (csrc/gemm.hpp: gemm_f32_kernel / launch_gemm) in every operand mode and on both block-to-tile maps,
reached directly through the diag hooks tdx_gemm_f32 / tdx_gemm_f32_conv (csrc/diag.hip), which build a GemmArgs from their arguments
and call launch_gemm itself with a plain store out[z][m][n] = v (n < nreal).  Epilogue arithmetic is test_gpu_epilogues.py's business;
this file is about operands and tiling: CONV (9 / 1 taps, strides, cv_stride_w, zero padding), A_KMAJOR / B_KMAJOR with the kvalid
row mask, PAIRED with pair_off, two K segments, the zdiv / kchunk / ktotal batch split, n_valid tile skipping and both tile maps
(map_mode 0 with its remainder N group and with blockIdx.y batches, map_mode 1 with z = 8j + x).

SHIFT is not instantiated: no launch_gemm call site on the fp32 core sets it (every `launch_gemm<` under csrc/ passes false as its
fourth argument), so there is no product configuration to reproduce.

Reference: the same product in torch fp64 on the CPU (matmul, conv2d, explicit sums over segments) from seeded randn inputs.
Bars, both derived and not measured on the code under test:
  * rel-L2 < 2e-6 — the bar this core holds in test_gpu_epilogues.py and test_linear_vs_fp64 at K up to 1024; no case here exceeds
    K_total = 1056;
  * elementwise |got - ref| <= K_total * 2**-23 * (|A| @ |B|), the standard fp32 summation bound with |A| @ |B| in fp64.  It pins a
    single wrong element and the message names its (z, m, n).

Buffer discipline, in every case: `out` is pre-filled with NaN inside the valid region (every valid element must come back finite)
and with 7.0 in two sentinel rows after row M and in the columns from nreal on (they must come back untouched); row-major A has NaN
guard rows after row M; K-major operands have NaN rows from kvalid on.  The kernel clamps its addresses and masks when it writes to
LDS, so a result is finite only if both work.  Row-major B (a weight) is zero-padded to the tile, as the product's loaders do.

test_remainder_group_of_two stands beside the N = 384 shapes of test_tile_maps for a reason: with a remainder group of ONE N tile
`n = ngf*gw + j % rem` is `ngf*gw` whatever the code does with j, so a broken remainder branch needs rem >= 2 to show.

Checked against three value-only mutations of gemm.hpp (every address stays in bounds): cdy / cdx swapped fails the six 9-tap CONV
cases; va / vb forced true in the K-major loads fails tdf2_kvalid_fb_16_of_32, the <T,T> z split and the two-segment PAIRED case; the
remainder branch pinned to n = ngf*gw fails test_remainder_group_of_two alone."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
dev = torch.device("cuda:0")
NAN = float("nan")
SENT = 7.0
GUARD = 2                       # sentinel rows of out / NaN guard rows of a row-major A
L2_BUDGET = 1536 * 1024         # launch_gemm: the weight slice of one N group stays under this many bytes


@pytest.fixture(scope="module")
def diag():
    from targetdiarization_amd import _lib
    return _lib.diag()


def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1009 + int(k)
    return torch.Generator(device="cpu").manual_seed(seed % (2 ** 31))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _seg(A, B, lda, ldb, K, strideA=0, strideB=0, zdiv=1, strideA2=0, strideB2=0, kchunk=0, ktotal=None):
    from targetdiarization_amd._lib import GemmSeg
    return GemmSeg(A.data_ptr(), B.data_ptr(), lda, ldb, strideA, strideB, strideA2, strideB2, K, zdiv, kchunk, K if ktotal is None else ktotal)


def _plan(M, N, ktot, batches, paired=False):
    """(map_mode, mp, gw, tiles_m, tiles_n) by the formulas of launch_gemm"""
    tm, tn = -(-M // 128), N // (64 if paired else 128)
    if tm >= 16 and batches <= 4:
        return (0, -(-tm // 8), max(1, min(L2_BUDGET // (128 * ktot * 4), tn)), tm, tn)
    return (1, 0, 1, tm, tn)


def _out(Z, M, ncols, cols):
    """out [Z][M + GUARD][ncols]: NaN where the kernel has to store (rows < M, columns `cols`), 7.0 elsewhere"""
    out = torch.full((Z, M + GUARD, ncols), SENT)
    out[:, :M, cols] = NAN
    return out.to(dev)


def _check(got, M, cols, ref, absprod, ktot, what):
    """got [Z][M + GUARD][ncols] (CPU); ref, absprod [Z][M][len(cols)] fp64"""
    mask = torch.zeros_like(got, dtype=torch.bool)
    mask[:, :M, cols] = True
    touched = (~mask) & (got != SENT)
    assert not bool(touched.any()), f"{what}: wrote outside the valid region, first at (z, m, n) = {touched.nonzero()[0].tolist()}"
    v = got[:, :M, cols].double()
    nonfinite = ~torch.isfinite(v)
    assert not bool(nonfinite.any()), (f"{what}: {int(nonfinite.sum())} valid elements not stored or not finite, first at (z, m, col index) = "
                                       f"{nonfinite.nonzero()[0].tolist()}")
    err = float((v - ref).norm() / ref.norm())
    diff = (v - ref).abs()
    bound = ktot * 2.0 ** -23 * absprod
    worst = float((diff / bound.clamp(min=1e-300)).max())
    print(f"{what}: rel-L2 {err:.3e}, worst |diff| / bound {worst:.3f}")
    assert err < 2e-6, (what, err)
    bad = diff > bound
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} elements beyond the fp32 summation bound, first at (z, m, col index) = "
                                 f"{bad.nonzero()[0].tolist()}: got {float(v[bad][0])!r}, ref {float(ref[bad][0])!r}")


def _launch(diag, ak, bk, paired, segs, M, N, n_valid, pair_off, batches, out, nreal):
    plan = (C.c_int * 5)()
    ncols = out.shape[2]
    rc = diag.tdx_gemm_f32(ak, bk, paired, C.byref(segs[0]), C.byref(segs[1]) if len(segs) > 1 else None, M, N, n_valid, pair_off, batches,
                           out.data_ptr(), ncols, (M + GUARD) * ncols, nreal, plan, None)
    assert rc == 0, diag.tdx_diag_last_error()
    torch.cuda.synchronize()
    return out.cpu(), tuple(plan)


def _rowmajor_a(g, Z, M, K, lda=None):
    """[Z][M + GUARD][lda], NaN guard rows after row M and NaN beyond column K; logical view [Z][M][K]"""
    lda = lda or K
    buf = torch.full((Z, M + GUARD, lda), NAN)
    buf[:, :M, :K] = _randn(g, Z, M, K)
    return buf, buf[:, :M, :K].double()


def _weight(g, Z, N, K, nreal):
    """row-major B [Z][N][K], rows >= nreal zero; logical view [Z][nreal][K]"""
    buf = torch.zeros(Z, N, K)
    buf[:, :nreal] = _randn(g, Z, nreal, K)
    return buf, buf[:, :nreal].double()


def _nt(diag, M, N, K, batches, n_valid=None, nreal=None, what=""):
    """plain NT, one segment, per-batch A and B; returns the plan"""
    n_valid, nreal = n_valid or N, nreal or N
    g = _gen(M, N, K, batches, n_valid, nreal)
    a, A = _rowmajor_a(g, batches, M, K)
    w, W = _weight(g, batches, N, K, nreal)
    a_d, w_d = a.to(dev), w.to(dev)
    cols = slice(0, nreal)
    got, plan = _launch(diag, 0, 0, 0, [_seg(a_d, w_d, K, K, K, strideA=(M + GUARD) * K, strideB=N * K)], M, N, n_valid, 0, batches,
                        _out(batches, M, N, cols), nreal)
    _check(got, M, cols, A @ W.transpose(1, 2), A.abs() @ W.abs().transpose(1, 2), K, what or f"NT M={M} N={N} K={K} Z={batches}")
    return plan


# ------------------------------------------------------------------------------------------------------------------ 1: tile maps
# (M, N, K, batches) -> (map_mode, mp, gw, remainder N group)
TILE_CASES = [
    ((130, 256, 64, 1), (1, 0, 1, 0)),
    ((70, 128, 32, 9), (1, 0, 1, 0)),           # z = 8j + x: the second round of eight holds one batch
    ((1921, 384, 1056, 1), (0, 2, 2, 1)),       # tiles_m 16, ragged last tile; one full N group + a remainder group of one
    ((2049, 384, 1056, 1), (0, 3, 2, 1)),       # tiles_m 17: XCD 5 holds two panels, XCDs 6 and 7 return early
    ((1921, 384, 32, 1), (0, 2, 3, 0)),         # a single N group
    ((2049, 384, 32, 1), (0, 3, 3, 0)),
    ((2049, 384, 1056, 3), (0, 3, 2, 1)),       # map_mode 0 with z = blockIdx.y
]


def _tile_case(diag, shape, expect):
    M, N, K, batches = shape
    mode, mp, gw, rem = expect
    want = _plan(M, N, K, batches)
    assert (want[0], want[1], want[2], want[4] % want[2]) == (mode, mp, gw, rem), f"{shape}: the case is off its branch: {want}"
    plan = _nt(diag, M, N, K, batches)
    assert plan == want, f"{shape}: launch_gemm planned {plan} (map_mode, mp, gw, tiles_m, tiles_n), the test expects {want}"


@gpu
@pytest.mark.parametrize("shape,expect", TILE_CASES, ids=["x".join(map(str, s)) for s, _ in TILE_CASES])
def test_tile_maps(diag, shape, expect):
    _tile_case(diag, shape, expect)


@gpu
def test_remainder_group_of_two(diag):
    """gw = 3 over 5 N tiles: the remainder group holds TWO tiles, so j / rem and j % rem of the `p >= ngf` branch are not trivial
    (a 768-wide QKV Linear, N = 2304, K = 768, has this shape of remainder from 1921 rows on)."""
    _tile_case(diag, (1921, 640, 1024, 1), (0, 2, 3, 2))


# ------------------------------------------------------------------------------------------------------- 2: n_valid and nreal
@gpu
@pytest.mark.parametrize("n_valid,nreal", [(32, 32), (64, 40), (96, 96), (160, 130), (256, 256)])
def test_n_valid_and_nreal(diag, n_valid, nreal):
    _nt(diag, 130, 256, 64, 1, n_valid=n_valid, nreal=nreal, what=f"n_valid={n_valid} nreal={nreal}")


# ----------------------------------------------------------------------------------------------------------------- 3: row pitch
@gpu
def test_lda_wider_than_k(diag):
    M, N, K, lda = 130, 128, 64, 96
    g = _gen(3, M, N, K, lda)
    a, A = _rowmajor_a(g, 1, M, K, lda)
    w, W = _weight(g, 1, N, K, N)
    a_d, w_d = a.to(dev), w.to(dev)
    got, _ = _launch(diag, 0, 0, 0, [_seg(a_d, w_d, lda, K, K)], M, N, N, 0, 1, _out(1, M, N, slice(0, N)), N)
    _check(got, M, slice(0, N), A @ W.transpose(1, 2), A.abs() @ W.abs().transpose(1, 2), K, "lda 96 > K 64")


@gpu
def test_lda_narrower_than_k_overlapping_rows(diag):
    """lda = HOP < K = NFFT: how silero, Whisper and the noise gate frame audio in place"""
    M, N, K, lda = 130, 128, 96, 32
    g = _gen(3, M, N, K, lda)
    n = (M - 1) * lda + K
    wav = torch.full((n + GUARD * lda,), NAN)
    wav[:n] = _randn(g, n)
    A = wav[:n].unfold(0, K, lda).double().unsqueeze(0)
    assert A.shape == (1, M, K)
    w, W = _weight(g, 1, N, K, N)
    a_d, w_d = wav.to(dev), w.to(dev)
    got, _ = _launch(diag, 0, 0, 0, [_seg(a_d, w_d, lda, K, K)], M, N, N, 0, 1, _out(1, M, N, slice(0, N)), N)
    _check(got, M, slice(0, N), A @ W.transpose(1, 2), A.abs() @ W.abs().transpose(1, 2), K, "lda 32 < K 96")


# ---------------------------------------------------------------------------------------------------------------------- 4: CONV
# (B, Hin, Win, cin, n_valid (N = 128), stride_h, stride_w, taps, lda - cin)
CONV_CASES = {
    "M165_crosses_a_tile_inside_an_image": (3, 5, 11, 32, 32, 1, 1, 9, 0),
    "three_k_tiles_per_tap": (2, 5, 7, 96, 96, 1, 1, 9, 0),
    "stride2_odd_Hin": (2, 5, 8, 64, 64, 2, 2, 9, 0),              # Hout 3: the last row's lower taps fall outside
    "campplus_head_stride_w_1": (2, 6, 9, 32, 32, 2, 1, 9, 0),
    "shortcut_1tap_stride2": (2, 6, 8, 64, 64, 2, 2, 1, 0),
    "lda_cin_plus_32": (3, 5, 11, 32, 32, 1, 1, 9, 32),
    "M2046_map_mode_0": (2, 31, 33, 32, 32, 1, 1, 9, 0),
}


@gpu
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_vs_fp64_conv2d(diag, name):
    B, Hin, Win, cin, nv, sh, sw, taps, extra = CONV_CASES[name]
    N, lda, pad = 128, cin + extra, 1 if taps == 9 else 0
    Hout, Wout = (Hin - 1) // sh + 1, (Win - 1) // sw + 1
    M = B * Hout * Wout
    g = _gen(4, B, Hin, Win, cin, nv, sh, sw, taps, extra)
    x = torch.full((B * Hin * Win + GUARD, lda), NAN)                       # NHWC rows, NaN guard rows and NaN beyond cin
    x[:B * Hin * Win, :cin] = _randn(g, B * Hin * Win, cin)
    w = torch.zeros(N, taps * cin)                                          # [N][tap][cin], rows >= n_valid zero
    w[:nv] = _randn(g, nv, taps * cin)
    xi = x[:B * Hin * Win, :cin].reshape(B, Hin, Win, cin).permute(0, 3, 1, 2).double()
    k = 3 if taps == 9 else 1
    wi = w[:nv].reshape(nv, k, k, cin).permute(0, 3, 1, 2).double()
    ref = F.conv2d(xi, wi, stride=(sh, sw), padding=pad).permute(0, 2, 3, 1).reshape(1, M, nv)
    absprod = F.conv2d(xi.abs(), wi.abs(), stride=(sh, sw), padding=pad).permute(0, 2, 3, 1).reshape(1, M, nv)
    assert ref.shape[1] == M

    x_d, w_d = x.to(dev), w.to(dev)
    out = _out(1, M, N, slice(0, nv))
    plan = (C.c_int * 5)()
    stride_w = sw if sw != sh else 0                                        # conv_gemm leaves cv_stride_w 0, head_conv sets it to 1
    rc = diag.tdx_gemm_f32_conv(x_d.data_ptr(), lda, w_d.data_ptr(), B, Hin, Win, Hout, Wout, sh, stride_w, taps, cin, N, nv,
                                out.data_ptr(), N, nv, plan, None)
    assert rc == 0, diag.tdx_diag_last_error()
    torch.cuda.synchronize()
    got = out.cpu()
    want = _plan(M, N, taps * cin, 1)
    assert tuple(plan) == want, (tuple(plan), want)
    if name == "M2046_map_mode_0":
        assert want[:3] == (0, 2, 1)
    else:
        assert want[0] == 1

    # the borders of every image first, so that a wrong tap at an edge is reported as such
    m = torch.arange(M)
    ho, wo = (m % (Hout * Wout)) // Wout, m % Wout
    edges = {"top row": ho == 0, "bottom row": ho == Hout - 1, "left column": wo == 0, "right column": wo == Wout - 1}
    v = got[0, :M, :nv].double()
    for edge, sel in edges.items():
        assert bool(torch.isfinite(v[sel]).all()), f"{name}: {edge} not stored or not finite"
        err = float((v[sel] - ref[0, sel]).norm() / ref[0, sel].norm())
        worst = float(((v[sel] - ref[0, sel]).abs() / (taps * cin * 2.0 ** -23 * absprod[0, sel])).max())
        print(f"{name} {edge}: rel-L2 {err:.3e}, worst |diff| / bound {worst:.3f}")
        assert err < 2e-6, f"{name}: {edge} of the images is wrong (rel-L2 {err:.3e})"
        assert worst <= 1.0, f"{name}: an element of the {edge} of the images is beyond the fp32 summation bound ({worst:.3g} x)"
    _check(got, M, slice(0, nv), ref, absprod, taps * cin, name)


# --------------------------------------------------------------------------------------------------------- 5: K-major operands
@gpu
def test_a_kmajor_as_stft_inverse(diag):
    """<T,F>: A is [K][M] per batch with strideA, the weight is shared"""
    M, N, K, R = 128, 256, 64, 3
    g = _gen(5, 1, M, N, K, R)
    a = torch.full((R, K + 1, M), NAN)                                      # one NaN row behind the K valid ones
    a[:, :K] = _randn(g, R, K, M)
    A = a[:, :K].transpose(1, 2).double()
    w, W = _weight(g, 1, N, K, N)
    a_d, w_d = a.to(dev), w.to(dev)
    got, plan = _launch(diag, 1, 0, 0, [_seg(a_d, w_d, M, K, K, strideA=(K + 1) * M)], M, N, N, 0, R, _out(R, M, N, slice(0, N)), N)
    assert plan == _plan(M, N, K, R) and plan[0] == 1
    _check(got, M, slice(0, N), A @ W.transpose(1, 2), A.abs() @ W.abs().transpose(1, 2), K, "<T,F>")


@gpu
@pytest.mark.parametrize("M,K,kvalid", [(16, 64, 64), (64, 32, 16)], ids=["tdf1_K_f", "tdf2_kvalid_fb_16_of_32"])
def test_b_kmajor_as_mdx_tdf(diag, M, K, kvalid):
    """<F,T> as run_tfc_tdf issues it: A a weight [M][K], B [K][c] per batch with ldb = c = 96 < 128 (N = 128, n_valid = 96), Z = 5.
    The second Linear has kvalid = fb = 16 of K = fbp = 32; A's columns 16..31 hold finite values, so only the mask on B zeroes them."""
    c, N, Z = 96, 128, 5
    g = _gen(5, 2, M, K, kvalid)
    a, A = _rowmajor_a(g, 1, M, K)
    b = torch.full((Z * K * c + 64,), NAN)                                  # the 128-column reads of the last valid row run 32 floats on
    bv = b[:Z * K * c].view(Z, K, c)
    bv[:, :kvalid] = _randn(g, Z, kvalid, c)
    Bm = bv[:, :kvalid].double()
    Av = A[:, :, :kvalid]
    a_d, b_d = a.to(dev), b.to(dev)
    cols = slice(0, c)
    got, plan = _launch(diag, 0, 1, 0, [_seg(a_d, b_d, K, c, K, strideB=K * c, ktotal=kvalid)], M, N, c, 0, Z, _out(Z, M, N, cols), c)
    assert plan[0] == 1
    _check(got, M, cols, Av @ Bm, Av.abs() @ Bm.abs(), K, f"<F,T> M={M} K={K} kvalid={kvalid}")


@gpu
def test_both_kmajor_with_z_split_as_attention_core(diag):
    """<T,T>: slab[b][split] = lin_k^T [v|u] over the split's token range; S = 70 in chunks of 32 -> the last split holds 6 rows"""
    S, kchunk, splits, Bt, M, N = 70, 32, 3, 2, 128, 128
    Sp = splits * kchunk
    g = _gen(5, 3, S, kchunk, Bt)
    link = torch.full((Bt, Sp, M), NAN)
    link[:, :S] = _randn(g, Bt, S, M)
    vu = torch.full((Bt, Sp, N), NAN)
    vu[:, :S] = _randn(g, Bt, S, N)
    l_d, v_d = link.to(dev), vu.to(dev)
    seg = _seg(l_d, v_d, M, N, kchunk, strideA=Sp * M, strideB=Sp * N, zdiv=splits, strideA2=kchunk * M, strideB2=kchunk * N, kchunk=kchunk,
               ktotal=S)
    cols = slice(0, N)
    got, plan = _launch(diag, 1, 1, 0, [seg], M, N, N, 0, Bt * splits, _out(Bt * splits, M, N, cols), N)
    assert plan[0] == 1
    ref = torch.zeros(Bt * splits, M, N, dtype=torch.float64)
    absprod = torch.zeros_like(ref)
    for b in range(Bt):
        for sp in range(splits):
            lo, hi = sp * kchunk, min((sp + 1) * kchunk, S)
            ref[b * splits + sp] = link[b, lo:hi].double().T @ vu[b, lo:hi].double()
            absprod[b * splits + sp] = link[b, lo:hi].double().abs().T @ vu[b, lo:hi].double().abs()
    _check(got, M, cols, ref, absprod, kchunk, "<T,T> per split")
    # the sum over the splits is lin_k^T [v|u]
    total = got[:, :M].double().view(Bt, splits, M, N).sum(1)
    full = link[:, :S].double().transpose(1, 2) @ vu[:, :S].double()
    fullabs = link[:, :S].double().abs().transpose(1, 2) @ vu[:, :S].double().abs()
    err = float((total - full).norm() / full.norm())
    print(f"<T,T> summed over splits: rel-L2 {err:.3e}")
    assert err < 2e-6
    assert bool(((total - full).abs() <= Sp * 2.0 ** -23 * fullabs).all())


# -------------------------------------------------------------------------------------------------------------------- 6: PAIRED
@gpu
@pytest.mark.parametrize("nreal", [128, 100], ids=["unguarded", "nreal_100"])
def test_paired_nt_as_frontend(diag, nreal):
    """N = 128 pair columns, pair_off = 128: column c pairs weight rows c and 128 + c (re / im of a DFT bin)"""
    M, N, K, off = 130, 128, 64, 128
    g = _gen(6, 1, nreal)
    a, A = _rowmajor_a(g, 1, M, K)
    w = torch.zeros(1, off + N, K)
    w[:, :nreal] = _randn(g, 1, nreal, K)
    w[:, off:off + nreal] = _randn(g, 1, nreal, K)
    cols = list(range(nreal)) + list(range(off, off + nreal))
    W = w[:, cols].double()
    a_d, w_d = a.to(dev), w.to(dev)
    got, plan = _launch(diag, 0, 0, 1, [_seg(a_d, w_d, K, K, K)], M, N, N, off, 1, _out(1, M, off + N, cols), nreal)
    assert plan == _plan(M, N, K, 1, paired=True) and plan[4] == 2
    _check(got, M, cols, A @ W.transpose(1, 2), A.abs() @ W.abs().transpose(1, 2), K, f"PAIRED NT nreal={nreal}")


@gpu
def test_paired_two_segments_as_attention_core(diag):
    """<F,T,PAIRED> at E = 64: [A_quad | lin_q] x [VU ; Kvu].  seg0: K-major B with zdiv = G, kchunk = 256, ktotal = S = 300 (G = 2, the
    second group holds 44 valid rows); seg1: a constant B per batch (strideB2 = 0).  pair_off = E."""
    E, S, Bt, QK = 64, 300, 2, 128
    G = (S + 255) // 256
    Sp = G * 256
    g = _gen(6, 2, E, S, Bt)
    abuf = _randn(g, Bt, G, 256, 256)                                       # finite everywhere: only the mask on B zeroes k >= kvalid
    vu = torch.full((Bt, Sp, 2 * E), NAN)
    vu[:, :S] = _randn(g, Bt, S, 2 * E)
    linq = _randn(g, Bt, Sp, QK)
    kvu = _randn(g, Bt, QK, 2 * E)
    a_d, v_d, q_d, k_d = abuf.to(dev), vu.to(dev), linq.to(dev), kvu.to(dev)
    s0 = _seg(a_d, v_d, 256, 2 * E, 256, strideA=G * 65536, strideB=Sp * 2 * E, zdiv=G, strideA2=65536, strideB2=256 * 2 * E, kchunk=256,
              ktotal=S)
    s1 = _seg(q_d, k_d, QK, 2 * E, QK, strideA=Sp * QK, strideB=QK * 2 * E, zdiv=G, strideA2=256 * QK, strideB2=0, kchunk=0, ktotal=QK)
    M, cols = 256, slice(0, 2 * E)
    got, plan = _launch(diag, 0, 1, 1, [s0, s1], M, E, E, E, Bt * G, _out(Bt * G, M, 2 * E, cols), E)
    assert plan == _plan(M, E, 256 + QK, Bt * G, paired=True) and plan[0] == 1
    ref = torch.zeros(Bt * G, M, 2 * E, dtype=torch.float64)
    absprod = torch.zeros_like(ref)
    for b in range(Bt):
        for grp in range(G):
            kv = min(256, S - grp * 256)
            a0, b0 = abuf[b, grp, :, :kv].double(), vu[b, grp * 256:grp * 256 + kv].double()
            a1, b1 = linq[b, grp * 256:(grp + 1) * 256].double(), kvu[b].double()
            ref[b * G + grp] = a0 @ b0 + a1 @ b1
            absprod[b * G + grp] = a0.abs() @ b0.abs() + a1.abs() @ b1.abs()
    assert S - (G - 1) * 256 == 44
    _check(got, M, cols, ref, absprod, 256 + QK, "<F,T,PAIRED> two segments")


# --------------------------------------------------------------------------------------------------------- 7: refused arguments
def test_unsafe_arguments_are_refused(diag):
    """Not marked gpu: libtdx_diag.so loads without a device and every refusal comes before the first device call.  The pointers are
    real all the same (device memory where there is a device) and point into the middle of a large zero buffer, so a refusal that
    went missing would end in a wrong status, not in a stray access."""
    from targetdiarization_amd._lib import GemmSeg
    on_gpu = torch.cuda.is_available()
    buf = torch.zeros(1 << 22, device=dev if on_gpu else "cpu")
    p = buf.data_ptr() + (1 << 23)

    def general(ak=0, bk=0, paired=0, M=128, N=128, n_valid=None, pair_off=0, batches=1, nreal=None, out=p, seg0=True, seg1=None, **kw):
        s = dict(A=p, B=p, lda=64, ldb=128 if bk else 64, strideA=0, strideB=0, strideA2=0, strideB2=0, K=64, zdiv=1, kchunk=0, ktotal=64)
        s.update(kw)
        s0 = GemmSeg(**s)
        s1 = GemmSeg(**dict(s, **seg1)) if seg1 else None
        return diag.tdx_gemm_f32(ak, bk, paired, C.byref(s0) if seg0 else None, C.byref(s1) if s1 else None, M, N, N if n_valid is None else n_valid,
                                 pair_off, batches, out, 256, 0, N if nreal is None else nreal, None, None)

    def conv(a=p, w=p, out=p, lda=32, ntaps=9, cin=32, N=128, n_valid=32, nreal=32):
        return diag.tdx_gemm_f32_conv(a, lda, w, 1, 4, 4, 4, 4, 1, 0, ntaps, cin, N, n_valid, out, 128, nreal, None, None)

    refused = {
        "K % 32": (lambda: general(K=48), b"K % 32"),
        "K % 32 in the second segment": (lambda: general(seg1=dict(K=40)), b"K % 32"),
        "N % 128": (lambda: general(N=192), b"N % 128"),
        "PAIRED N % 64": (lambda: general(paired=1, N=96, pair_off=128), b"N % 64"),
        "lda % 4": (lambda: general(lda=66), b"lda % 4"),
        "ldb % 4": (lambda: general(ldb=66), b"ldb % 4"),
        "M < 1": (lambda: general(M=0), b"M >= 1"),
        "A_KMAJOR M % 128": (lambda: general(ak=1, lda=256, M=130), b"M % 128"),
        "kvalid < 1 in the last split": (lambda: general(ak=1, bk=1, lda=128, K=32, zdiv=3, kchunk=32, ktotal=64, batches=3), b"ktotal"),
        "kvalid < 1, K-major B only": (lambda: general(bk=1, K=32, zdiv=2, kchunk=32, ktotal=32, batches=2), b"ktotal"),
        "zdiv < 1": (lambda: general(zdiv=0), b"zdiv"),
        "nreal > n_valid": (lambda: general(n_valid=64, nreal=65), b"nreal"),
        "null A": (lambda: general(A=None), b"null"),
        "null B": (lambda: general(B=None), b"null"),
        "null B in the second segment": (lambda: general(seg1=dict(B=None)), b"null"),
        "null out": (lambda: general(out=None), b"null"),
        "null segment": (lambda: general(seg0=False), b"null"),
        "conv cin % 32": (lambda: conv(cin=48, lda=48), b"cin % 32"),
        "conv ntaps 3": (lambda: conv(ntaps=3), b"ntaps"),
        "conv ntaps 0": (lambda: conv(ntaps=0), b"ntaps"),
        "conv N % 128": (lambda: conv(N=96), b"N % 128"),
        "conv lda % 4": (lambda: conv(lda=34), b"lda % 4"),
        "conv null a": (lambda: conv(a=None), b"null"),
        "conv null w": (lambda: conv(w=None), b"null"),
        "conv null out": (lambda: conv(out=None), b"null"),
    }
    for what, (call, word) in refused.items():
        rc = call()
        assert rc == 1, f"{what}: status {rc}, expected TDX_E_INVALID"
        msg = diag.tdx_diag_last_error()
        assert msg.startswith(b"tdx_gemm_f32") and word in msg, (what, msg)
