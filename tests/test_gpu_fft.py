"""GPU tests of the any-length FFT and the band mix (csrc/fft.hpp, targetdiarization_amd/fft.py).

The error criterion of every comparison: relative L2 against numpy's float64 result on the same float32 input, at most 8 times the
error of numpy's own float32 transform of that input, and below 1e-5 (the cap tests/test_gpu_pvoc.py uses for its analysis stage).
numpy >= 2 transforms float32 input in single precision; where it does not (the result is not complex64 / float32) only the cap
applies.  Every test prints the device's figure next to numpy's.

numpy's single-precision FORWARD transform is taken with norm="forward".  With the default norm numpy 2.2 passes the factor 1 as a
Python int, its ufunc then resolves to the double-precision loop, and the complex64 it returns is the float64 transform rounded once
(its error equals that rounding's, 2.5e-8 at every length) — not a float32 transform, and not a figure any float32 algorithm stays
within 8 times of.  With norm="forward" the factor 1 / n is a float32, the single-precision loop runs, and the result is the
spectrum times that factor: it is compared with the float64 spectrum times the same factor, so nothing but numpy's own arithmetic
enters the figure.  ifft and irfft take the single-precision loop with their default norm.  test_c2c prints the default-norm figure
as well.

Measured on MI355X: all 277 cases pass.  The worst ratios: 5.4 (band mix, n = 6, disjoint ranges: the output is one constant, device
2.5e-8 against numpy's 4.6e-9), 4.2 (c2c, n = 4095, impulse, forward: 2.7e-7 against 6.4e-8) and 4.1 (c2c, n = 160000, tone, forward).
Where numpy's float32 error is exactly 0 the bound is 0 and the device's is 0 too (powers of two on a constant; the inverse transform
of a constant at n = 3, which numpy's radix-3 butterfly and the device's paired fp64 sum both return exactly)."""
import ast
import ctypes as C
import os

import numpy as np
import pytest

import fft_oracle as orc
from targetdiarization_amd import _lib
from targetdiarization_amd import fft as tfft

pytestmark = pytest.mark.gpu

TILE = tfft.TILE
CAP = 1e-5
_IN = {}


@pytest.fixture(scope="module")
def dev():
    return tfft.DeviceFFT("cuda:0")


def l2(a, ref):
    a, ref = np.asarray(a).astype(np.complex128).ravel(), np.asarray(ref).astype(np.complex128).ravel()
    den = np.linalg.norm(ref)
    return float(np.linalg.norm(a - ref) / den) if den > 0 else float(np.linalg.norm(a - ref))


def fct32(n):
    """the factor numpy's norm="forward" applies in single precision, as a float64"""
    return float(np.reciprocal(n, dtype=np.float32))


def check(what, got, ref64, f32, single, scale=1.0):
    """the criterion; `f32` numpy's own single-precision result (times `scale`, see the head of the file), `single` its expected dtype"""
    err, base = l2(got, ref64), l2(f32, np.asarray(ref64) * scale)
    is_single = np.asarray(f32).dtype == single
    print(f"{what}: device {err:.3e}  numpy float32 {base:.3e}  ratio {err / base if base > 0 else float('inf') if err > 0 else 0.0:.2f}")
    assert err < CAP, what
    if is_single:
        assert err <= 8 * base, what
    return err, base


def signal(n, kind):
    """complex64 [n]"""
    if (n, kind) not in _IN:
        j = np.arange(n)
        if kind == "noise":
            rng = np.random.default_rng(n)
            x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        elif kind == "impulse":
            x = np.zeros(n, dtype=np.complex128)
            x[(n // 3 + 1) % n if n > 1 else 0] = 1.0
        elif kind == "constant":
            x = np.full(n, 0.3 - 0.7j)
        else:                                  # one tone on the bin k0, amplitude 0.5
            x = 0.5 * np.exp(2j * np.pi * ((j * tone_bin(n)) % n) / n)
        _IN.clear()                            # one input at a time: the largest is 38 MB
        _IN[n, kind] = x.astype(np.complex64)
    return _IN[n, kind]


def tone_bin(n):
    return (n // 5 + 1) % n


# ---- 1. c2c, forward and inverse
SIZES = [1, 2, 3, 4, 5, 7, 8, 16, 64, TILE // 2, TILE, 2 * TILE, TILE - 1, TILE + 1, 1009, 8191, 65537, 160000, 1 << 20, 4800001]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("kind", ["noise", "impulse", "constant", "tone"])
@pytest.mark.parametrize("n", SIZES)
def test_c2c(dev, n, kind, inverse):
    x = signal(n, kind)
    np_f = np.fft.ifft if inverse else np.fft.fft
    got = dev.ifft(x) if inverse else dev.fft(x)
    assert got.shape == (n,) and got.dtype == np.complex64
    ref = np_f(x.astype(np.complex128))
    f32, scale = (np.fft.ifft(x), 1.0) if inverse else (np.fft.fft(x, norm="forward"), fct32(n))
    err, base = check(f"c2c n={n} {kind} {'inverse' if inverse else 'forward'}", got, ref, f32, np.complex64, scale)
    if not inverse:
        print(f"    numpy default norm (float64, rounded once): {l2(np.fft.fft(x), ref):.3e}")
    if kind == "tone" and not inverse and n > 1:
        # the energy outside the tone's bin stays below the bound times n * amplitude — over what the float32 samples themselves
        # hold there (their rounding is part of the input: the float64 spectrum shows it)
        off, own = got.astype(np.complex128), ref.copy()
        off[tone_bin(n)] = own[tone_bin(n)] = 0
        leak, leak_own = float(np.linalg.norm(off)) / (n * 0.5), float(np.linalg.norm(own)) / (n * 0.5)
        bound = min(8 * base, CAP) if f32.dtype == np.complex64 else CAP
        print(f"    leak outside bin {tone_bin(n)}: {leak:.3e} of n * amplitude (the input's own {leak_own:.3e}), bound {bound:.3e}")
        assert leak <= leak_own + bound


def test_c2c_split_twiddles(dev):
    """Beyond 2^24 points the inter-pass twiddle is the product of two roots (csrc/fft.hpp root()): 2^25 points, a unit impulse, whose
    spectrum exp(-2 pi i j0 k / n) is known without a transform; 2^20 bins of it are compared.  Every output is the impulse times the
    product of the roots of 4 passes and 13 in-tile stages, each good to about 2^-24: the bound is 1e-6 for their rms."""
    import torch
    n, j0 = 1 << 25, (1 << 25) // 3 + 1
    x = torch.zeros(n, dtype=torch.complex64, device="cuda:0")
    x[j0] = 1.0
    X = dev.fft(x)
    k = np.random.default_rng(0).integers(0, n, 1 << 20)
    got = X[torch.from_numpy(k).to("cuda:0")].cpu().numpy().astype(np.complex128)
    ref = np.exp(-2j * np.pi * ((k * j0) % n) / n)
    err = float(np.sqrt(np.mean(np.abs(got - ref) ** 2)))
    print(f"c2c n=2^25 impulse: rms error of 2^20 bins {err:.3e}, worst {np.abs(got - ref).max():.3e}")
    assert err < 1e-6


# ---- 2. multi-pass plans at small sizes (the test hook: the same kernels under a small tile)
def hook_c2c(x, inverse, tile_log2):
    import torch
    d = _lib.diag()
    b, n = (1, x.shape[0]) if x.ndim == 1 else x.shape
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.complex64)).to("cuda:0")
    y = torch.empty_like(t)
    need = d.tdx_test_fft_workspace_bytes(n, b, tile_log2)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda:0")
    rc = d.tdx_test_fft_c2c(torch.view_as_real(t).data_ptr(), n, b, int(inverse), torch.view_as_real(y).data_ptr(), ws.data_ptr(), need,
                            torch.cuda.current_stream().cuda_stream, tile_log2)
    assert rc == 0, d.tdx_diag_last_error()
    torch.cuda.synchronize()
    return y.cpu().numpy()


def test_planner_depths():
    """what the sizes below rest on: the passes of 2^m points under the tiles 2^6, 2^9 and the product's"""
    d = _lib.diag()
    passes = lambda m, t: d.tdx_test_fft_passes(m, t)
    assert [passes(m, 6) for m in (6, 7, 9, 10, 12, 13, 15, 16, 18)] == [1, 3, 3, 4, 4, 5, 5, 6, 6]
    assert [passes(m, 9) for m in (9, 10, 11, 15, 16)] == [1, 2, 3, 3, 4]
    assert [passes(m, 12) for m in (12, 13, 16, 17, 24, 25, 27)] == [1, 2, 2, 3, 3, 4, 4]
    assert passes(28, 12) == 0 and passes(10, 3) == 0 and passes(10, 13) == 0


# (tile_log2, n): both ends of every plan depth up to 2^18, and one Bluestein length whose M lands on each depth
MULTI = [(6, 1 << 7), (6, 1 << 9), (6, 1 << 10), (6, 1 << 12), (6, 1 << 13), (6, 1 << 15), (6, 1 << 16), (6, 1 << 18),
         (9, 1 << 10), (9, 1 << 11), (9, 1 << 15), (9, 1 << 16), (9, 1 << 18),
         (6, 100), (6, 1009), (6, 5000), (6, 40000), (9, 400), (9, 1009), (9, 20000)]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("tile_log2,n", MULTI)
def test_multi_pass_plans(tile_log2, n, inverse):
    x = signal(n, "noise")
    np_f = np.fft.ifft if inverse else np.fft.fft
    got = hook_c2c(x, inverse, tile_log2)
    f32, scale = (np.fft.ifft(x), 1.0) if inverse else (np.fft.fft(x, norm="forward"), fct32(n))
    check(f"hook tile 2^{tile_log2} n={n} {'inverse' if inverse else 'forward'}", got, np_f(x.astype(np.complex128)), f32, np.complex64, scale)


@pytest.mark.parametrize("n", [1, 8, 64, TILE // 2, TILE, 1009, TILE + 1])
def test_hook_with_the_product_tile_is_the_product(dev, n):
    x = signal(n, "noise")
    for inverse in (False, True):
        a, b = hook_c2c(x, inverse, TILE.bit_length() - 1), (dev.ifft(x) if inverse else dev.fft(x))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 3. determinism
@pytest.mark.parametrize("n", [64, 1009, 2 * TILE, 160000])
def test_batch_rows_and_repeats_are_bit_identical(dev, n):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))).astype(np.complex64)
    r = rng.standard_normal((3, n)).astype(np.float32)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for f, data in ((dev.fft, x), (dev.ifft, x), (dev.rfft, r)):
        whole = f(data)
        assert whole.shape[0] == 3
        for b in range(3):
            assert np.array_equal(bits(whole[b]), bits(f(data[b]))), (n, b)
        assert np.array_equal(bits(whole), bits(f(data)))
    X = dev.rfft(r)
    whole = dev.irfft(X, n)
    for b in range(3):
        assert np.array_equal(bits(whole[b]), bits(dev.irfft(X[b], n)))
    plan = tfft.band_mix_plan(n, 16000)
    y = dev.band_mix(r[0], r[1], plan)
    assert np.array_equal(bits(y), bits(dev.band_mix(r[0], r[1], plan)))


# ---- 4. r2c / c2r
@pytest.mark.parametrize("n", [2, 3, 6, 7, 2 * TILE, 2 * TILE + 1, 160000, 160001])
def test_r2c_c2r(dev, n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    X = dev.rfft(x)
    assert X.shape == (n // 2 + 1,) and X.dtype == np.complex64
    check(f"r2c n={n}", X, np.fft.rfft(x.astype(np.float64)), np.fft.rfft(x, norm="forward"), np.complex64, fct32(n))
    S = (rng.standard_normal(n // 2 + 1) + 1j * rng.standard_normal(n // 2 + 1)).astype(np.complex64)
    S[0] = S[0].real + 0.75j                       # imaginary parts that irfft ignores: bin 0 and, for even n, the last bin
    if n % 2 == 0:
        S[-1] = S[-1].real - 1.25j
    y = dev.irfft(S, n)
    assert y.shape == (n,) and y.dtype == np.float32
    check(f"c2r n={n}", y, np.fft.irfft(S.astype(np.complex128), n), np.fft.irfft(S, n), np.float32)
    Z = S.copy()
    Z[0] = Z[0].real
    if n % 2 == 0:
        Z[-1] = Z[-1].real
    assert np.array_equal(y.view(np.uint32), dev.irfft(Z, n).view(np.uint32))        # they have no effect at all


# ---- 5. the band mix
SR = 16000
_CLIPS = {}


def clips(n):
    """two float32 clips and their spectra in float64 and in numpy's single precision, once per n"""
    if n not in _CLIPS:
        _CLIPS.clear()
        rng = np.random.default_rng(1000 + n)
        a, b = (rng.standard_normal(n) * 0.3).astype(np.float32), (rng.standard_normal(n) * 0.3).astype(np.float32)
        _CLIPS[n] = (a, b, (np.fft.rfft(a.astype(np.float64)), np.fft.rfft(b.astype(np.float64))), (rfft32(a), rfft32(b)))
    return _CLIPS[n]


def settings(n):
    f = float(np.float64(max(1, (n // 2 + 1) // 3) if n > 3 else 0) * (1.0 / (n * (1 / SR))))       # a limit exactly on a bin
    return {"default": ([0, 4000], [0, 8000]), "none": (None, None), "disjoint": ([0, 1000], [3000, 5000]), "onebin": ([0, f], [f, 8000]),
            "reversed": ([3000, 100], [0, 8000]), "cover": ([0, 8000], [1000, 3000])}


def rfft32(x):
    """numpy's single-precision rfft: the spectrum times fct32(n) (the head of the file)"""
    return np.fft.rfft(x, norm="forward")


def single_mix(n, f32, mr, ar, sr=SR):
    """the oracle's steps in numpy's single precision on the two spectra of rfft32: (output, mix spectrum), both times fct32(n) — every
    step is linear in the spectra"""
    fa, fb = f32
    in_main, in_aux, in_both, _, _ = orc.band_sets(n, sr, mr, ar)
    mix = np.zeros_like(fa)
    mix[in_main] = fa[in_main]
    mix[in_aux] = fb[in_aux]
    if in_both.any():
        w = np.linspace(1, 0, int(in_both.sum())).astype(fa.real.dtype)
        mix[in_both] = fa[in_both] * w + fb[in_both] * (1 - w)
    return np.fft.irfft(mix), mix


@pytest.mark.parametrize("name", ["default", "none", "disjoint", "onebin", "reversed", "cover"])
@pytest.mark.parametrize("n", [2, 5, 6, 257, 1009, 4096, 160000, 160001, 4800001])
def test_band_mix(dev, n, name):
    a, b, f64, f32 = clips(n)
    mr, ar = settings(n)[name]
    plan = tfft.band_mix_plan(n, SR, mr, ar)
    if name == "onebin":
        assert plan["count"] == 1
    taps, sp = {}, {}
    y = dev.band_mix(a, b, plan, taps=taps)
    ref = orc.mix_audio_by_freq(a, b, SR, mr, ar, spectra=sp, ffts=f64)
    assert y.shape == ref.shape == (2 * (n // 2),) and y.dtype == np.float32
    y32, mix32 = single_mix(n, f32, mr, ar)
    what = f"band_mix n={n} {name}"
    check(what + " output", y, ref, y32, np.float32, fct32(n))
    check(what + " main spectrum", taps["main"], sp["main"], f32[0], np.complex64, fct32(n))
    check(what + " aux spectrum", taps["aux"], sp["aux"], f32[1], np.complex64, fct32(n))
    check(what + " mixed spectrum", taps["mix"], sp["mix"], mix32, np.complex64, fct32(n))
    for key in ("main", "aux", "mix"):
        assert taps[key].shape == (n // 2 + 1,) and taps[key].dtype == np.complex64
    masks = orc.band_sets(n, SR, mr, ar)
    outside = ~(masks[0] | masks[1] | masks[2])
    assert np.all(sp["mix"][outside] == 0) and np.all(taps["mix"][outside] == 0)          # a zeroed bin is exactly 0


# ---- 6. AudioProcessor.mix_audio_by_freq end to end
@pytest.fixture(scope="module")
def ap():
    from targetdiarization_amd.audio_processor import AudioProcessor
    return AudioProcessor(verbose_log=False, cuda_device=0)


def test_mix_audio_by_freq_end_to_end(ap, dev):
    rng = np.random.default_rng(5)
    a, b = (rng.standard_normal(1009) * 0.3).astype(np.float32), (rng.standard_normal(1300) * 0.3).astype(np.float32)
    bits = lambda v: v.view(np.uint32)
    # the result is float32 and is DeviceFFT.band_mix of the same plan, bit for bit
    y = ap.mix_audio_by_freq(a, b[:1009], 16000, [100, 3000], [2000, 7000])
    assert y.dtype == np.float32 and y.shape == (1008,)
    assert np.array_equal(bits(y), bits(dev.band_mix(a, b[:1009], tfft.band_mix_plan(1009, 16000, [100, 3000], [2000, 7000]))))
    # force_align, main shorter: aux is truncated
    assert np.array_equal(bits(ap.mix_audio_by_freq(a, b, force_align=True)), bits(dev.band_mix(a, b[:1009], tfft.band_mix_plan(1009, 16000))))
    # force_align, main longer: aux is padded with silence
    padded = np.concatenate((a, np.zeros(291, dtype=np.float32)))
    y = ap.mix_audio_by_freq(b, a, force_align=True)
    assert y.shape == (1300,) and np.array_equal(bits(y), bits(dev.band_mix(b, padded, tfft.band_mix_plan(1300, 16000))))
    check("force_align, main longer", y, orc.mix_audio_by_freq(b, a, force_align=True), single_mix(1300, (rfft32(b), rfft32(padded)),
          [0, 4000], [0, 8000])[0], np.float32, fct32(1300))
    # nothing to mix: audio_main itself
    assert ap.mix_audio_by_freq(a, b) is a
    m2 = np.zeros((16, 2), dtype=np.float32)
    assert ap.mix_audio_by_freq(m2, m2) is m2
    one = np.ones(1, dtype=np.float32)
    assert ap.mix_audio_by_freq(one, one) is one
    # the default ranges are not shared between calls
    assert ap.mix_audio_by_freq.__func__.__defaults__[1:3] == ([0, 4000], [0, 8000])


def test_mix_audio_by_freq_reproduces_the_goldens(ap, gold):
    G = np.load(os.path.join(gold, "band_mix.npz"))
    done = 0
    for name, n, n_aux, sr, mr, ar, align in [ast.literal_eval(str(c)) for c in G["mixf_cases"]]:
        a, b = G[f"mixf_{name}_main"], G[f"mixf_{name}_aux"]
        assert a.dtype == np.float32
        y = ap.mix_audio_by_freq(a, b, sr, mr, ar, align)
        if bool(G[f"mixf_{name}_same"]):
            assert y is a
            continue
        ref = G[f"mixf_{name}_out"]
        assert y.shape == ref.shape and y.dtype == np.float32
        bb = b[:n]
        check(f"golden {name}", y, ref, single_mix(n, (rfft32(a), rfft32(bb)), mr, ar, sr)[0], np.float32, fct32(n))
        done += 1
    assert done >= 14
