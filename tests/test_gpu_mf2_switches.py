"""-m gpu: the process-level A/B switches of the MossFormer2 forward (csrc/mf2.hip), once, on the 2-block recipe model.  Each is a
function-local static read once per process, so every setting runs tests/mf2_switch_child.py in a fresh interpreter (one after
another).  What the code claims about them, asserted on the SHA-256 of the output bytes:

  TDX_FUSE_CONV=0   the separate conv17<4> pass: "the same arithmetic in the same order: bit-identical results"
  TDX_FORK_ROWS=0   only moves the q/k-head branch of a FLASH layer onto the caller's stream: a difference would be a race
  TDX_H3A=0         the wide attention kernel: bit-identical to gemm_h3a in the same segment order, which is TDX_H3A_SWAP=0
                    (the default order, lin_q x Kvu first, changes the accumulation order and is compared with fp64 instead:
                    tests/test_gpu_attention_gate.py)

and in every process the eager forward and the HIP-graph replay give the same bytes."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "mf2_switch_child.py")
SWITCHES = ("TDX_H3A", "TDX_H3A_SWAP", "TDX_H3A_ORDER", "TDX_H3_DEBUG", "TDX_FUSE_CONV", "TDX_FORK_ROWS")
# one child = one interpreter start with torch, the recipe weights, two model creates and three 1198-row forwards (one of them
# the graph capture): 2.3 - 2.8 s per child measured on MI355X machines inside two runs of the whole suite (12.3 and 12.8 s for
# the five); the limit is three times the slowest
CHILD_MEASURED_S = 2.8
CHILD_LIMIT_S = 3 * CHILD_MEASURED_S


def _child(setting):
    """digests of one child, or pytest.fail: the caller starts no further child after an abnormal exit"""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(setting)
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, CHILD], env=env, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"child {setting or 'default'} did not finish in {CHILD_LIMIT_S:.0f} s; stderr:\n{e.stderr}")
    if r.returncode != 0:
        pytest.fail(f"child {setting or 'default'} exited with status {r.returncode}; stderr:\n{r.stderr[-4000:]}")
    d = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"{setting or 'default'}: {time.perf_counter() - t0:.1f} s  {d}")
    assert d["env"] == {k: v for k, v in env.items() if k.startswith("TDX_")}
    assert d["finite"] and d["captures"] == 1, (setting, d)
    assert d["eager"] == d["graph"], f"{setting or 'default'}: eager forward and graph replay differ"
    return d["eager"]


def test_switches_are_bit_identical():
    base = _child({})
    assert _child({"TDX_FUSE_CONV": "0"}) == base, "TDX_FUSE_CONV=0 changes the result"
    assert _child({"TDX_FORK_ROWS": "0"}) == base, "TDX_FORK_ROWS=0 changes the result: the forked branches race"
    noswap = _child({"TDX_H3A_SWAP": "0"})
    assert _child({"TDX_H3A": "0"}) == noswap, "the wide attention kernel (TDX_H3A=0) differs from gemm_h3a in the same segment order"
