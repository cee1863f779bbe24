"""CPU test of the block -> tile map of the split-f16 x3 GEMM core (csrc/gemm_h3.hpp: plan_gemm_h3 and H3_TILE_OF_BLOCK, the one text
the kernel and the host copy h3_tile_of_block are both made of), through the host-only hooks tdx_h3_plan / tdx_h3_tile_of_block of
libtdx_diag.so.  No device is touched.

For every launch the blocks of the whole grid are enumerated: each tile (z, bm, bn) with z < batches, bm < tiles_m, bn < tiles_n must
be produced by exactly one block, and no block may produce anything else.  That is the whole contract of the map: a tile computed
twice costs time, a tile never computed leaves its output unwritten, a tile outside the ranges writes out of bounds.

The plans come from plan_gemm_h3 itself over a few hundred (M, N, ktot, batches), chosen so that every branch is met: map_mode 1 with
batches not a multiple of 8; map_mode 0 with one N group, with several groups and a remainder group of one and of more tiles, with
M chunks (mc > 0) whose last chunk is short, with XCDs that own no tile.  A second test walks plans the launcher can be steered to with
TDX_H3_GW_KB / TDX_H3_MC: every gw in [1, tiles_n] and every mc in [0, mp) for a few tilings.

The plan formulas are restated here (and asserted) only when those two variables are unset."""
import ctypes as C
import os

import pytest

from targetdiarization_amd import _lib

ENV_PLAN = [v for v in ("TDX_H3_GW_KB", "TDX_H3_MC") if v in os.environ]


@pytest.fixture(scope="module")
def diag():
    from targetdiarization_amd.build import build_lib
    build_lib()
    return _lib.diag()


def expected_plan(M, N, ktot, batches, paired):
    """(map_mode, mp, gw, mc, tiles_m, tiles_n) by the formulas of plan_gemm_h3"""
    tm = -(-M // 256)
    tn = N // 128 if paired else -(-N // 256)
    if tm >= 16 and batches <= 4:
        mp = -(-tm // 8)
        gw = max(1, min(1536 * 1024 // (256 * ktot * 4), tn))
        mc = 0
        if gw < tn:
            c = 6 * 1024 * 1024 // (256 * ktot * 4)
            if 0 < c < mp:
                mc = c
        return (0, mp, gw, mc, tm, tn), (8 * mp * tn, batches)
    return (1, 0, 1, 0, tm, tn), (8 * (-(-batches // 8)) * tm * tn, 1)


def enumerate_tiles(diag, plan, grid, batches):
    """{(z, bm, bn): number of blocks that compute it} over the whole grid, and the number of blocks that return at once"""
    p = (C.c_int * 6)(*plan)
    z, bm, bn = C.c_int(), C.c_int(), C.c_int()
    seen, idle = {}, 0
    for by in range(grid[1]):
        for bx in range(grid[0]):
            r = diag.tdx_h3_tile_of_block(p, batches, bx, by, C.byref(z), C.byref(bm), C.byref(bn))
            assert r in (0, 1), diag.tdx_diag_last_error()
            if r:
                key = (z.value, bm.value, bn.value)
                seen[key] = seen.get(key, 0) + 1
            else:
                idle += 1
    return seen, idle


def assert_exact_cover(diag, plan, grid, batches, what):
    _, _, _, _, tm, tn = plan
    seen, idle = enumerate_tiles(diag, plan, grid, batches)
    want = {(z, m, n) for z in range(batches) for m in range(tm) for n in range(tn)}
    extra = sorted(set(seen) - want)
    assert not extra, f"{what}: plan {plan} produces tiles outside the launch, first (z, bm, bn) = {extra[0]}"
    missing = sorted(want - set(seen))
    assert not missing, f"{what}: plan {plan} never produces {len(missing)} tiles, first (z, bm, bn) = {missing[0]}"
    twice = sorted(k for k, c in seen.items() if c != 1)
    assert not twice, f"{what}: plan {plan} produces {len(twice)} tiles more than once, first (z, bm, bn) = {twice[0]}"
    assert idle == grid[0] * grid[1] - len(want)


def launches():
    out = []
    # map_mode 1: few M tiles, or more than four batches
    for M in (1, 256, 257, 3840):
        for N in (128, 256, 300, 1280):
            for batches in (1, 2, 5, 8, 9, 11, 16):
                out.append((M, N, 512, batches, False))
    for batches in (5, 11):
        out.append((4200, 1280, 512, batches, False))
    # map_mode 0: tiles_m 16 .. 97, 1 .. 9 N tiles, K from one L2-resident group down to gw = 1 with chunks
    for M in (3841, 4096, 4200, 4353, 6500, 8193, 12345, 24600):
        for N in (128, 256, 768, 1280, 2304):
            for ktot in (64, 512, 768, 1024, 2048, 2304):
                for batches in (1, 3, 4):
                    if batches == 1 or (M, N) in ((4200, 1280), (6500, 768)):
                        out.append((M, N, ktot, batches, False))
    # PAIRED: 128 pair columns per tile
    for M, N, ktot, batches in ((300, 384, 512, 2), (4200, 640, 512, 2), (6500, 384, 2048, 1), (24600, 640, 512, 1)):
        out.append((M, N, ktot, batches, True))
    return out


def test_every_tile_exactly_once(diag):
    cases = launches()
    assert len(cases) > 300
    met = set()
    for (M, N, ktot, batches, paired) in cases:
        plan, grid = (C.c_int * 6)(), (C.c_int * 2)()
        assert diag.tdx_h3_plan(M, N, ktot, batches, int(paired), plan, grid) == 0, diag.tdx_diag_last_error()
        plan, grid = tuple(plan), tuple(grid)
        what = f"M={M} N={N} ktot={ktot} batches={batches} paired={paired}"
        if not ENV_PLAN:
            assert (plan, grid) == expected_plan(M, N, ktot, batches, paired), what
        assert_exact_cover(diag, plan, grid, batches, what)
        mode, mp, gw, mc, tm, tn = plan
        if mode == 1:
            met.add("map1" if batches % 8 == 0 or batches == 1 else "map1_ragged_round")
        else:
            rem = tn % gw
            met.add("one_group" if gw == tn else "rem0" if rem == 0 else "rem1" if rem == 1 else "rem2plus")
            if mc:
                met.add("chunks_even" if mp % mc == 0 else "chunks_short_last")
            if 8 * mp - tm >= mp:
                met.add("idle_xcd")
            if batches > 1:
                met.add("map0_batches")
    if not ENV_PLAN:
        assert met >= {"map1", "map1_ragged_round", "one_group", "rem0", "rem1", "rem2plus", "chunks_even", "chunks_short_last", "idle_xcd",
                       "map0_batches"}, met


def test_every_gw_and_mc(diag):
    """what TDX_H3_GW_KB / TDX_H3_MC can steer the launcher to: every group width and every chunk height of a few tilings"""
    for tm, tn, batches in ((16, 2, 1), (17, 5, 1), (26, 3, 2), (41, 7, 1), (97, 5, 1)):
        mp = -(-tm // 8)
        for gw in range(1, tn + 1):
            for mc in range(0, mp):
                if mc and gw == tn:
                    continue                # the launcher chunks only when several groups re-read the A rows
                plan = (0, mp, gw, mc, tm, tn)
                assert_exact_cover(diag, plan, (8 * mp * tn, batches), batches, "steered plan")


def test_bad_arguments_are_refused(diag):
    z = C.c_int()
    plan = (C.c_int * 6)(0, 0, 1, 0, 16, 2)          # map_mode 0 with mp = 0 would divide by zero
    assert diag.tdx_h3_tile_of_block(plan, 1, 0, 0, C.byref(z), C.byref(z), C.byref(z)) == -1
    plan = (C.c_int * 6)(0, 2, 0, 0, 16, 2)          # gw = 0
    assert diag.tdx_h3_tile_of_block(plan, 1, 0, 0, C.byref(z), C.byref(z), C.byref(z)) == -1
    assert diag.tdx_h3_plan(0, 256, 64, 1, 0, plan, (C.c_int * 2)()) != 0
    assert diag.tdx_h3_plan(300, 200, 64, 1, 1, plan, (C.c_int * 2)()) != 0        # PAIRED: N % 128
