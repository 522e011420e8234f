"""f64 restatement of the classification head and the predict() tail (src/Model/model.py:271-277, 481,
491-537), shared by test_classifier_cpu.py and test_classifier_gpu.py:

    a = x W1^T + b1,  h = GELU_erf(a),  logits = h W2^T + b2,  probs = 1 / (1 + exp(-logits)),
    preds = probs >= float32(threshold),  top-K by (prob desc, class asc).

Per-element error bound of the bf16x3 head (csrc/cls_head.hip), derived from the project's linear bar
(test_x3_gpu.py: |err| <= 2^-15 |x| |W|^T + 1e-6 max|ref| for one bf16x3 linear), not fitted:
    e_h   = 2^-15 (|x| |W1|^T) + 1e-7 (1 + |a|)     fc1's bar, plus mmr::erf_as's 1.5e-7 through 1/2 a (1 + erf)
    bound = 1.13 e_h |W2|^T + 2^-15 (|h| |W2|^T) + 1e-6 max|ref|      (1.13 >= GELU's Lipschitz constant)
    pbound = bound / 4 + 2^-22                       sigmoid' <= 1/4, plus the f32 exp / divide / rounding
Comparisons that an error within the bound can flip are tie-aware: preds are compared outside the band
|p_ref - threshold| <= pbound, and top-K lists up to permutations inside a tie group (classes, in reference
order, whose [p - pbound, p + pbound] intervals chain-overlap).  test_classifier_cpu.py caps both sets on the
reference alone for every case below."""
import functools
import math

import numpy as np
import torch

# (B, D, H, C): the GPU test's shapes.  H = 4 D with D % 128 == 0, D <= 1024 is the fused kernel (C <= 64 / <= 128 /
# <= 256 are its three builds; B on both sides of the 32-row tile, several tiles); D = 96 and H = 2 D are the two
# chain routes (exact f32 / bf16x3 linears)
CASES = [(1, 128, 512, 1), (31, 128, 512, 17), (33, 128, 512, 43), (257, 128, 512, 43), (33, 128, 512, 200),
         (33, 256, 1024, 64), (31, 256, 1024, 65), (257, 256, 1024, 65),
         (1, 768, 3072, 43), (33, 768, 3072, 43), (257, 768, 3072, 43),
         (33, 96, 384, 43), (31, 128, 256, 43), (64, 1024, 4096, 43)]
THRESHOLD = 0.5
KS = (1, 5, None)  # None: K = C


def case_ks(c):
    return sorted({min(k, c) if k is not None else c for k in KS})


def make_inputs(B, D, H, C):
    """Seeded f32 inputs of one case: x ~ N(0, 1), W1 ~ N(0, 1 / D) (pre-activations of order 1), W2 ~
    N(0, 0.05^2 / H), b2 ~ N(0, 1).  The bound above sums absolute values through both layers and grows like
    sqrt(D H) against the data's own cancelling sums: with unit-scale W2 it reaches ~0.05 on logits of spread ~1
    at D = 768, and the sets left out of the exact comparisons (threshold band, tie groups) would hold several
    per cent of the entries.  The small W2 keeps the bound (which scales with W2, so the logits check is as tight
    per product) near 1e-3 while b2 spreads the logits over about +-2.5: probabilities from ~0.08 to ~0.92,
    neighbours in a row's order typically 1e-2 apart, pbound <= ~5e-4."""
    g = torch.Generator().manual_seed(1000 * D + 10 * C + B + H)
    x = torch.randn(B, D, generator=g)
    w1 = torch.randn(H, D, generator=g) * D ** -0.5
    b1 = torch.randn(H, generator=g) * 0.1
    w2 = torch.randn(C, H, generator=g) * (0.05 * H ** -0.5)
    b2 = torch.randn(C, generator=g)
    return x, w1, b1, w2, b2


SPARSE_CASES = [(33, 128, 512, 43), (33, 768, 3072, 43), (40, 1024, 4096, 65)]


def make_sparse_inputs(B, D, H, C):
    """Inputs on which the bound is tight: W1 rows with ONE non-zero (hidden j reads x[:, j % D]) and W2 rows with
    four, all N(0, 1) f32 values (non-zero lo parts).  |x| |W|^T is then the magnitude of the few products
    themselves, so the bound is ~2^-15 of each product, 4x the bf16x3 split's own ~2^-17: a dropped hi.lo / lo.hi
    term (2^-9 of a product) or a hidden unit read at the wrong k position exceeds it at once."""
    g = torch.Generator().manual_seed(7 * D + C + B)
    x = torch.randn(B, D, generator=g)
    w1 = torch.zeros(H, D)
    w1[torch.arange(H), torch.arange(H) % D] = torch.randn(H, generator=g)
    b1 = torch.randn(H, generator=g) * 0.1
    w2 = torch.zeros(C, H)
    cols = torch.stack([torch.randperm(H, generator=g)[:4] for _ in range(C)])
    w2.scatter_(1, cols, torch.randn(C, 4, generator=g))
    b2 = torch.randn(C, generator=g) * 0.1
    return x, w1, b1, w2, b2


def head_f64(x, w1, b1, w2, b2):
    """(logits, probs, bound, pbound) as f64 tensors from f32 / f64 inputs."""
    x, w1, b1, w2, b2 = (torch.as_tensor(t).double() for t in (x, w1, b1, w2, b2))
    a = x @ w1.T + b1
    h = 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0)))
    logits = h @ w2.T + b2
    e_h = 2.0 ** -15 * (x.abs() @ w1.abs().T) + 1e-7 * (1.0 + a.abs())
    bound = 1.13 * (e_h @ w2.abs().T) + 2.0 ** -15 * (h.abs() @ w2.abs().T) + 1e-6 * logits.abs().max()
    probs = 1.0 / (1.0 + torch.exp(-logits))
    return logits, probs, bound, 0.25 * bound + 2.0 ** -22


@functools.lru_cache(maxsize=None)
def case(B, D, H, C):
    """Inputs and the f64 reference of one case, computed once per process; treat as read-only."""
    inp = make_inputs(B, D, H, C)
    return inp, head_f64(*inp)


def preds_of(probs, threshold):
    """(probs >= float32(threshold)) as int32, the comparison predict() makes on f32 probabilities."""
    return (torch.as_tensor(probs).double() >= float(np.float32(threshold))).to(torch.int32)


def band(p_ref, pbound, threshold):
    """Entries whose prediction an error within pbound can flip."""
    return (p_ref - float(np.float32(threshold))).abs() <= pbound


def order_of(probs):
    """Per row the class indices by (prob desc, class asc), (B, C) int64."""
    p = torch.as_tensor(probs).double()
    return torch.argsort(-p, dim=1, stable=True)


def tie_groups(p_ref, pbound):
    """(order, gid): the reference order per row and, per position of it, the id of its tie group — consecutive
    classes whose error intervals overlap (p_i - e_i <= p_next + e_next) share a group."""
    order = order_of(p_ref)
    ps, es = torch.gather(p_ref, 1, order), torch.gather(pbound, 1, order)
    split = (ps[:, :-1] - es[:, :-1]) > (ps[:, 1:] + es[:, 1:])  # clearly ahead of the next one
    gid = torch.cat([torch.zeros_like(order[:, :1]), split.long().cumsum(1)], 1)
    return order, gid


def max_tie_group_in_topk(p_ref, pbound, k):
    """Largest tie group that touches the first k positions of the reference order (over all rows)."""
    _, gid = tie_groups(p_ref, pbound)
    worst = 0
    for row in gid:
        sizes = torch.bincount(row)
        worst = max(worst, int(sizes[row[:k]].max()))
    return worst


def topk_mismatches(idx, p_ref, pbound):
    """Rows of idx (B, K) that are NOT tie-aware equal to the reference's top-K: position j must hold a class of
    the tie group of the reference's j-th class, and no class twice."""
    idx = torch.as_tensor(idx).long()
    k = idx.shape[1]
    order, gid = tie_groups(p_ref, pbound)
    group_of_class = torch.empty_like(gid)
    group_of_class.scatter_(1, order, gid)
    bad = (torch.gather(group_of_class, 1, idx) != gid[:, :k]).any(1)
    dup = torch.tensor([len(set(r.tolist())) != k for r in idx])
    return torch.nonzero(bad | dup).flatten().tolist()


def exact_topk(probs, k):
    """(vals, idx) of the first k of (prob desc, class asc) on the given probabilities, exactly."""
    o = order_of(probs)[:, :k]
    return torch.gather(torch.as_tensor(probs), 1, o), o
