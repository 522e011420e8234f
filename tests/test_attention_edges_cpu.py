"""CPU: the reference helper of the attention edge tests (attention_edges_ref.py) holds what the GPU tests
rely on: the selection cases' gap, one-hot softmax and power-of-two target scores, HF's uniform softmax on
an all-masked sequence, the additive mask against -inf fill, the mask shapes and the rising row maximum."""
import math

import pytest
import torch

from attention_edges_ref import (GAP_NATS, attn_f64, edge_targets, mask_geometries, rising_max_case, selection_case,
                                 selection_expected, selection_gap, selection_logits)

# every head dim of the GPU grids at its extreme lengths, plus a few shapes off those grids
SEL = [(lq, lk, heads, dh) for dh in (8, 24, 40, 72, 104, 120, 136, 168) for heads in (1, 3)
       for lq, lk in ((1, 1), (1, 160), (33, 31), (65, 33), (130, 160))]
SEL += [(40, 64, 2, 8), (40, 300, 2, 16), (40, 65, 2, 24),   # (dh = 8 has only 256 distinct sign keys)
        (40, 129, 2, 64), (40, 160, 2, 192), (40, 31, 2, 40)]


@pytest.mark.parametrize("lq,lk,heads,dh", SEL)
def test_selection_case_gap_and_one_hot(lq, lk, heads, dh):
    c = selection_case(lq, lk, heads, dh, seed=lq + lk + dh)
    assert c["q"].dtype == c["k"].dtype == c["v"].dtype == torch.bfloat16
    assert c["q"].shape == (lq, heads * dh) and c["k"].shape == c["v"].shape == (lk, heads * dh)
    if lk > 1:
        assert selection_gap(c) >= GAP_NATS
    s = selection_logits(c)
    # the target's raw score is a power of two (its product with scale * log2 e is then exact in f32)
    raw = torch.gather(s, 2, c["pi"][:, :, None]) / c["scale"]
    assert torch.equal(torch.exp2(torch.round(torch.log2(raw))), torch.round(raw))
    assert raw.max().item() * c["scale"] < 1e4
    p = s.softmax(-1)
    onehot = torch.zeros_like(p).scatter_(2, c["pi"][:, :, None], 1.0)
    tiny = lk * math.exp(-GAP_NATS)                                 # 160 e^-120 = 1e-50: nothing in f32
    assert torch.equal(torch.gather(p, 2, c["pi"][:, :, None]), torch.ones(heads, lq, 1, dtype=torch.float64))
    assert (p - onehot).abs().max().item() <= tiny
    out, mean, probs = selection_expected(c)
    ref = attn_f64(c["q"], c["k"], c["v"], 1, lq, lk, heads, dh, c["scale"])[0]
    assert (ref - out.double()).abs().max().item() <= 10 * tiny
    assert torch.allclose(mean, ref.mean(0), rtol=0, atol=1e-12)
    assert (probs - p.mean(0)).abs().max().item() <= tiny
    # every head reaches key 0, key lk - 1 and both sides of every tile edge once lq allows
    et = edge_targets(lk)
    if lq >= len(et):
        for h in range(heads):
            assert set(et) <= set(c["pi"][h].tolist())


def test_selection_case_explicit_targets():
    pi = torch.tensor([[3, 0, 64], [64, 63, 1]])
    c = selection_case(3, 65, 2, 40, seed=1, targets=pi)
    assert torch.equal(c["pi"], pi) and selection_gap(c) >= GAP_NATS


def test_edge_targets():
    assert edge_targets(1) == [0]
    assert edge_targets(32) == [0, 31]
    assert edge_targets(33) == [0, 31, 32]
    assert edge_targets(160) == [0, 31, 32, 63, 64, 95, 96, 127, 128, 159]


def _qkv(b, lq, lk, heads, dh, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b * lq, heads * dh, generator=g), torch.randn(b * lk, heads * dh, generator=g),
            torch.randn(b * lk, heads * dh, generator=g))


def test_attn_f64_all_masked_row_is_mean_of_v():
    b, lq, lk, heads, dh = 2, 5, 70, 3, 40
    q, k, v = _qkv(b, lq, lk, heads, dh, 3)
    mask = torch.ones(b, lk, dtype=torch.int64)
    mask[0] = 0
    out = attn_f64(q, k, v, b, lq, lk, heads, dh, dh ** -0.5, mask)
    mean = v.double().view(b, lk, heads * dh)[0].mean(0)
    assert torch.allclose(out[0], mean.expand(lq, -1), rtol=0, atol=1e-14)
    assert torch.equal(out[1], attn_f64(q, k, v, b, lq, lk, heads, dh, dh ** -0.5)[1])


@pytest.mark.parametrize("L", [33, 64, 96, 160])
def test_attn_f64_partial_mask_equals_inf_fill(L):
    b, heads, dh = 5, 2, 40
    q, k, v = _qkv(b, L, L, heads, dh, L)
    mask = mask_geometries(L, L)[1:]
    got = attn_f64(q, k, v, b, L, L, heads, dh, dh ** -0.5, mask)
    hd = lambda t: t.double().view(b, L, heads, dh).transpose(1, 2)  # noqa: E731
    s = (hd(q) @ hd(k).transpose(-1, -2) * dh ** -0.5).masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    ref = (s.softmax(-1) @ hd(v)).transpose(1, 2).reshape(b, L, heads * dh)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("L", [33, 64, 96, 160])
def test_mask_geometries(L):
    m = mask_geometries(L, 7)
    assert m.shape == (6, L) and m.dtype == torch.int64 and set(m.unique().tolist()) <= {0, 1}
    assert m[0].sum() == 0 and m[5].sum() == L
    lead = 64 if L > 64 else 32
    assert m[1, :lead].sum() == 0 and m[1, lead:].sum() == L - lead > 0
    assert m[2].sum() == 1 and m[2, L - 1] == 1
    tiles = [m[3, t:t + 32] for t in range(0, L, 32)]
    assert all(t.sum() == 0 for t in tiles[1::2]) and all(0 < t.sum() for t in tiles[0::2])
    assert any(t.sum() < t.numel() for t in tiles[0::2])            # holes inside the live tiles
    assert m[4, :L // 2 + 1].sum() == L // 2 + 1 and m[4, L // 2 + 1:].sum() == 0


def test_rising_max_case():
    lq, lk, heads = 65, 160, 2
    for dh in (64, 40):
        q, k, v = rising_max_case(lq, lk, heads, dh, seed=5)
        for t in (q, k, v):
            assert torch.equal(t, t.to(torch.bfloat16).float())
        s = (q.double().view(lq, heads, dh).transpose(0, 1) @ k.double().view(lk, heads, dh).permute(1, 2, 0)) / math.sqrt(dh)
        assert 6.0 <= s.std().item() <= 11.0
        tmax = torch.stack([s[..., t:t + 32].max(-1).values for t in range(0, lk, 32)], -1)  # (heads, lq, 5)
        assert (tmax[..., 1:] > tmax[..., :-1]).all()
