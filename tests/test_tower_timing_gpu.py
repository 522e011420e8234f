"""The timed path of the BERT towers (gemm_events, what bench.py's per-GEMM roofline reads): a forward with
gemm_events = {} records one HIP event pair per layer for each of the four GEMMs, computes what the untimed
forward computes, and leaves no trace once gemm_events is None again.

Geometry: BERT-base per-layer shapes (hidden 768, 12 heads, intermediate 3072) with 2 layers, vocab 1000,
128 positions; B = 2 x L = 128 with one row's mask shortened = 256 rows, the smallest count that takes the
LayerNorm-folded bf16 path and the fp8 fast path.

Timed vs untimed output:
  bf16 (folded path, and the plain path with ln_fold = False) and fp8 (fast path): the events wrap the very
      launches the untimed forward makes -> torch.equal.
  x3: the timed chain is another order of f32 operations (no residual in the O-proj / FFN2 epilogues, a plain
      LayerNorm that adds the residual itself, FFN1 -> FFN2 as two GEMMs), so a tolerance: max|timed - untimed|
      / max|untimed| <= X3_BAR = twice X3_MEASURED = 1.152e-6, the value measured on an MI355X with this
      geometry and these inputs on the commit before this test was added.
"""
import math

import pytest
import torch

from mmr_amd import ops
from mmr_amd.towers import BERT_BASE, BertTower, init_bert_state
from mmr_amd.towers_x3 import BertTowerX3

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = dict(BERT_BASE, vocab_size=1000, num_hidden_layers=2, max_position_embeddings=128)
NAMES = {"qkv", "o", "ffn1", "ffn2"}
X3_MEASURED = 1.152e-6
X3_BAR = 2 * X3_MEASURED


@pytest.fixture(scope="module")
def state():
    return init_bert_state(CFG, 31)


@pytest.fixture(scope="module")
def batch():
    g = torch.Generator().manual_seed(32)
    ids = torch.randint(0, CFG["vocab_size"], (2, 128), generator=g)
    mask = torch.ones(2, 128, dtype=torch.int64)
    mask[1, 77:] = 0
    return ids.to(DEV), mask.to(DEV)


def _rel(a, b):
    return (a.float() - b.float()).abs().max().item() / b.float().abs().max().item()


def _timed_vs_untimed(tw, batch):
    """(untimed, timed) outputs of tw; checks the recorded events and that gemm_events = None afterwards
    gives the untimed bits again."""
    ref = tw.forward(*batch).clone()
    tw.gemm_events = {}
    timed = tw.forward(*batch).clone()
    torch.cuda.synchronize()
    ev = tw.gemm_events
    tw.gemm_events = None
    assert set(ev) == NAMES, sorted(ev)
    for name, pairs in ev.items():
        assert len(pairs) == CFG["num_hidden_layers"], (name, len(pairs))
        for e0, e1 in pairs:
            ms = e0.elapsed_time(e1)
            assert math.isfinite(ms) and ms >= 0, (name, ms)
    again = tw.forward(*batch)
    assert torch.equal(again, ref), "gemm_events = None does not reproduce the untimed forward"
    return ref, timed


def test_bf16_folded_and_plain(state, batch):
    tw = BertTower(state, CFG, device=DEV)
    assert tw.ln_fold and ops.linear_ln_parts(256, tw.hidden, 2) > 0, "256 rows must take the folded path"
    ref, timed = _timed_vs_untimed(tw, batch)
    print(f"bf16 folded: timed vs untimed {_rel(timed, ref):.3e}")
    assert torch.equal(timed, ref)
    tw.ln_fold = False  # the plain path: same kernels timed and untimed
    ref, timed = _timed_vs_untimed(tw, batch)
    print(f"bf16 plain: timed vs untimed {_rel(timed, ref):.3e}")
    assert torch.equal(timed, ref)


def test_fp8_fast_path(state, batch):
    tw = BertTower(state, CFG, device=DEV, fp8=True)
    assert all(ly["qkv_w8"].kp == tw.hidden and ly["i_w8"].layout == 2 for ly in tw.layers), \
        "256 rows x hidden 768 must take the fp8 fast path"
    ref, timed = _timed_vs_untimed(tw, batch)
    print(f"fp8 fast: timed vs untimed {_rel(timed, ref):.3e}")
    assert torch.equal(timed, ref)


def test_x3(state, batch):
    tw = BertTowerX3(state, CFG, device=DEV)
    ref, timed = _timed_vs_untimed(tw, batch)
    print(f"x3: timed vs untimed {_rel(timed, ref):.3e} (bar {X3_BAR})")
    assert _rel(timed, ref) <= X3_BAR
