"""Plain-torch f64 reference and adversarial inputs for the attention cores (csrc/fusion.hip mha_small,
csrc/x3.hip x3_mha), shared by test_attention_edges_cpu.py and test_attention_edges_gpu.py.

attn_f64         softmax(q k^T * scale + (1 - mask) * finfo(f32).min) v, HF BertSelfAttention's additive key
                 mask (a sequence whose keys are all masked gets a uniform softmax: the mean of V).
selection_case   q / k / v for which softmax picks exactly one key per (head, query): every off-target logit is
                 >= 120 nats below the target's, so every off-target exp2 argument in the kernels is below
                 -150 and that weight is exactly 0 in f32; the context row must then be one V row bit for bit.
mask_geometries  the six key-mask shapes of the mask tests.
rising_max_case  soft logits (std ~ 8) whose row maximum rises with every 32-key tile.

The selection keys: the obvious recipe (Gaussian keys of equal norm, q = beta k) leaves the target's raw
score s an arbitrary f32, and the bf16 core computes p = exp2(fma(s, c2, -fl(s c2))) = 2^(rounding error of
s c2), about 1 +- 5e-5 at logits near 1e3.  P is rounded to bf16 (exactly 1) but the softmax denominator
sums the f32 p, so out = V / p: harmless after the bf16 rounding of `out`, but 5e-5 in the f32 mean_out,
far above the 1e-6 that output is held to.  Here every key of a head has 2^m entries of +-1 (m =
floor(log2 dh), the other entries 0), so |k|^2 = 2^m, and q = beta k with beta a power of two: the target's
raw score beta 2^m is a power of two, s c2 is exact, p = 1 and alpha = 1 exactly, and `out`, `mean_out` and
the probabilities carry nothing but f32 summation error.  All products and sums of the scores are exact
integers times beta, in both kernels."""
import math

import torch

F32_MIN = torch.finfo(torch.float32).min
GAP_NATS = 120.0


def _heads(t, b, l, heads, dh):
    return t.double().reshape(b, l, heads, dh).transpose(1, 2)


def attn_f64(q, k, v, b, lq, lk, heads, dh, scale, mask=None):
    """(b, lq, heads*dh) f64; q (b*lq, heads*dh), k / v (b*lk, heads*dh), mask (b, lk) of 0 / 1 or None."""
    s = _heads(q, b, lq, heads, dh) @ _heads(k, b, lk, heads, dh).transpose(-1, -2) * scale
    if mask is not None:
        s = s + (1.0 - mask.double())[:, None, None, :] * F32_MIN
    return (s.softmax(-1) @ _heads(v, b, lk, heads, dh)).transpose(1, 2).reshape(b, lq, heads * dh)


def edge_targets(lk):
    """Key 0, key lk - 1 and both sides of every 32-key tile edge (which include the 64- / 128-key block
    edges of every launch)."""
    t = {0, lk - 1}
    for e in range(32, lk, 32):
        t |= {e - 1, e}
    return sorted(t)


def _sign_keys(lk, dh, m, g):
    """lk distinct rows of 2^m entries +-1 at random positions of dh, the rest 0 (f64)."""
    def rows(n):
        pos = torch.rand(n, dh, generator=g).argsort(-1)[:, :m]
        sgn = torch.randint(0, 2, (n, m), generator=g).double() * 2 - 1
        return torch.zeros(n, dh, dtype=torch.float64).scatter_(1, pos, sgn)
    k = rows(lk)
    for _ in range(1000):
        gram = k @ k.T - 2.0 * m * torch.eye(lk, dtype=torch.float64)
        dup = torch.nonzero(torch.triu(gram >= m, 1).any(0)).flatten()  # equal to an earlier row
        if dup.numel() == 0:
            return k
        k[dup] = rows(dup.numel())
    raise RuntimeError(f"no {lk} distinct keys at dh={dh}")


def selection_case(lq, lk, heads, dh, seed, targets=None):
    """One sequence: {q (lq, heads*dh), k, v (lk, heads*dh)} bf16, pi (heads, lq) the selected key of every
    (head, query), scale = dh^-0.5.  targets: (heads, lq) key indices; default: head h walks edge_targets(lk)
    from its h-th entry for two rounds (every head hits all of them once lq >= their number), then random keys."""
    g = torch.Generator().manual_seed(seed)
    m = 1 << (dh.bit_length() - 1)
    scale = 1.0 / math.sqrt(dh)
    if targets is None:
        et = edge_targets(lk)
        pi = torch.randint(0, lk, (heads, lq), generator=g)
        for h in range(heads):
            for i in range(min(lq, 2 * len(et))):
                pi[h, i] = et[(i + h) % len(et)]
    else:
        pi = torch.as_tensor(targets, dtype=torch.int64).reshape(heads, lq)
    k = torch.stack([_sign_keys(lk, dh, m, g) for _ in range(heads)])            # (heads, lk, dh)
    gram = k @ k.transpose(-1, -2)
    gram -= 4.0 * m * torch.eye(lk, dtype=torch.float64)                         # the diagonal out of the max
    room = m - gram.max(-1).values.clamp(min=-float(m))                          # (heads, lk): 2^m - max_j k_j.k_t
    need = GAP_NATS / (room * scale)
    beta = torch.exp2(torch.ceil(torch.log2(need))).clamp(min=1.0) if lk > 1 else torch.ones_like(need)
    kt = torch.gather(k, 1, pi[:, :, None].expand(heads, lq, dh))                # (heads, lq, dh)
    q = kt * torch.gather(beta, 1, pi)[:, :, None]
    v = torch.randn(lk, heads * dh, generator=g).to(torch.bfloat16)
    qb, kb = (t.permute(1, 0, 2).reshape(-1, heads * dh).to(torch.bfloat16) for t in (q, k))
    assert torch.equal(qb.double().reshape(lq, heads, dh).permute(1, 0, 2), q)  # bf16-representable
    return {"q": qb, "k": kb, "v": v, "pi": pi, "scale": scale, "lq": lq, "lk": lk, "heads": heads, "dh": dh}


def selection_logits(c):
    """(heads, lq, lk) f64 scaled scores of a selection case."""
    return (_heads(c["q"], 1, c["lq"], c["heads"], c["dh"])[0]
            @ _heads(c["k"], 1, c["lk"], c["heads"], c["dh"])[0].transpose(-1, -2)) * c["scale"]


def selection_gap(c):
    """min over (head, query) of target logit - largest other logit (inf with one key)."""
    s = selection_logits(c)
    t = torch.gather(s, 2, c["pi"][:, :, None])
    rest = s.scatter(2, c["pi"][:, :, None], -float("inf")).max(-1, keepdim=True).values
    return (t - rest).min().item()


def selection_expected(c):
    """out (lq, heads*dh) bf16 = V[pi_h(i)] per head, mean (heads*dh) f64 over the queries, probs (lq, lk) f64
    = count_h[pi_h(i) == key] / heads."""
    lq, lk, heads, dh = c["lq"], c["lk"], c["heads"], c["dh"]
    vh = c["v"].reshape(lk, heads, dh).permute(1, 0, 2)                           # (heads, lk, dh)
    out = torch.gather(vh, 1, c["pi"][:, :, None].expand(heads, lq, dh)).permute(1, 0, 2).reshape(lq, heads * dh)
    probs = torch.zeros(heads, lq, lk, dtype=torch.float64).scatter_(2, c["pi"][:, :, None], 1.0).mean(0)
    return out.contiguous(), out.double().mean(0), probs


def mask_geometries(L, seed):
    """(6, L) int64 key masks: 0 all keys masked; 1 keys 0..31 masked (0..63 when that leaves a live key);
    2 only key L - 1 live; 3 every other 32-key tile masked (tile 0 live) plus random holes; 4 right padding;
    5 no masking."""
    g = torch.Generator().manual_seed(seed)
    m = torch.ones(6, L, dtype=torch.int64)
    m[0] = 0
    m[1, :64 if L > 64 else 32] = 0
    m[2, :L - 1] = 0
    tile = torch.arange(L) // 32
    m[3] = ((tile % 2 == 0) & (torch.rand(L, generator=g) > 0.3)).to(torch.int64)
    m[3, 0] = 1
    m[4, L // 2 + 1:] = 0
    return m


def rising_max_case(lq, lk, heads, dh, seed, step=6.0, noise=2.0):
    """q (lq, heads*dh), k, v (lk, heads*dh) f32 (bf16-representable): logits = noise * N(0, 1) + step * (key
    // 32), by a shared direction u in q and k whose weight in k grows with the key's 32-key tile."""
    g = torch.Generator().manual_seed(seed)
    u = torch.ones(dh) / math.sqrt(dh)
    a = math.sqrt(step) * dh ** 0.25                     # q.u = a, k_j.u = a * tile(j): logit += step * tile
    q = torch.randn(lq, heads, dh, generator=g) * math.sqrt(noise)
    k = torch.randn(lk, heads, dh, generator=g) * math.sqrt(noise)
    q = q - (q @ u)[..., None] * u + a * u
    k = k - (k @ u)[..., None] * u + a * (torch.arange(lk) // 32).float()[:, None, None] * u
    v = torch.randn(lk, heads * dh, generator=g)
    return tuple(t.reshape(t.shape[0], heads * dh).to(torch.bfloat16).float() for t in (q, k, v))
