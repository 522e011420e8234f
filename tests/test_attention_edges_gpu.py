"""GPU: the attention cores at the inputs where such kernels go wrong (csrc/fusion.hip mha_small behind
ops.mha / ops.bert_attention and their MX-fp8 forms, csrc/x3.hip x3_mha behind ops.x3_attention /
x3_attention_split, the probability kernels of csrc/attn_probs.hip, the Swin window kernels at ws != 7).

Bars:
  * selection (attention_edges_ref.selection_case: softmax picks one key): `out` equals the selected V row
    bit for bit in both cores (P = 1 exactly, V bf16-representable so x3's lo terms vanish), mean_out within
    1e-6 * max|ref| of the f64 mean (f32 summation over <= 130 rows), the probabilities within 1e-6;
  * masks and soft logits against attn_f64 (HF's additive finfo.min mask) at each kernel's existing bound,
    max|err| <= 2e-2 * max|ref| for bf16 and 5e-5 for x3, and no NaN / Inf;
  * MX-fp8 forms bit-identical to quantize_mxfp8 of the bf16 output; x3 split rows to the split of the f32 rows;
  * nothing outside [b*lq) x [heads*dh) of a padded, strided output is written."""
import itertools
import json
import math

import pytest
import torch

from attention_edges_ref import attn_f64, mask_geometries, rising_max_case, selection_case, selection_expected
from attn_maps_ref import towers_mini
from mmr_amd import ops
from mmr_amd.towers import BERT_BASE, BertTower
from oracle import towers as otw
from test_towers_gpu import _check_emb, _swin_attn_ref
from test_x3_gpu import _split_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {"bf16": 2e-2, "q8": 2e-2, "x3": 5e-5}
LQS, LKS = (1, 33, 65, 129, 130), (1, 31, 32, 33, 64, 65, 96, 129, 160)
DH_BF16, DH_X3 = (8, 24, 40, 72, 104, 136, 168), (8, 24, 40, 72, 104, 120)
PAT16, PAT32 = 0x5A5A, 0x5A5A5A5A  # guard fill (bf16 / f32 bits)


def _rel(got, ref):
    ref = ref.detach().double().cpu()
    return (got.detach().double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _guarded(rows, cols, dtype, pad_rows=0, pad_cols=8):
    """(buffer filled with the guard pattern, its [rows x cols] interior view at row stride cols + pad_cols)."""
    it = torch.int16 if dtype == torch.bfloat16 else torch.int32
    buf = torch.full((rows + 2 * pad_rows, cols + pad_cols), PAT16 if it == torch.int16 else PAT32, dtype=it,
                     device=DEV).view(dtype)
    return buf, buf[pad_rows:pad_rows + rows, :cols]


def _guard_intact(buf, rows, cols, pad_rows=0):
    g = buf.view(torch.int16 if buf.element_size() == 2 else torch.int32).clone()
    pat = g.new_full((), PAT16 if buf.element_size() == 2 else PAT32)
    g[pad_rows:pad_rows + rows, :cols] = pat
    return bool((g == pat).all())


def _selection_batch(b, lq, lk, heads, dh, seed, f32):
    """b selection cases as one launch: operands as strided views of packed (rows, 3C) projections on the
    device (junk in the other columns), expected out (b*lq, C), mean (b, C) f64, probs (b, lq, lk) f64."""
    cs = [selection_case(lq, lk, heads, dh, seed + i) for i in range(b)]
    C = heads * dh
    g = torch.Generator().manual_seed(seed)
    qp, kvp = torch.randn(b * lq, 3 * C, generator=g), torch.randn(b * lk, 3 * C, generator=g)
    qp[:, C:2 * C] = torch.cat([c["q"] for c in cs]).float()
    kvp[:, :C] = torch.cat([c["k"] for c in cs]).float()
    kvp[:, 2 * C:] = torch.cat([c["v"] for c in cs]).float()
    dt = torch.float32 if f32 else torch.bfloat16
    qp, kvp = qp.to(dt).to(DEV), kvp.to(dt).to(DEV)
    exp = [selection_expected(c) for c in cs]
    out = torch.cat([e[0] for e in exp]).to(dt)
    return (qp[:, C:2 * C], kvp[:, :C], kvp[:, 2 * C:], cs[0]["scale"], out, torch.stack([e[1] for e in exp]),
            torch.stack([e[2] for e in exp]))


def _selection_grid(kind, heads, dh):
    """One (core, heads, dh) over the lq x lk grid; returns the list of failed checks."""
    f32 = kind == "x3"
    dt = torch.float32 if f32 else torch.bfloat16
    core = ops.x3_attention if f32 else ops.mha
    probs_fn = ops.x3_attention_probs if f32 else ops.mha_probs
    bad, worst = [], {"mean": 0.0, "probs": 0.0}
    b, C = 2, heads * dh
    for lq, lk in itertools.product(LQS, LKS):
        q, k, v, scale, exp, exp_mean, exp_probs = _selection_batch(b, lq, lk, heads, dh, 1000 * lq + lk + dh, f32)
        buf, out = _guarded(b * lq, C, dt)                                # ldo = heads*dh + 8
        mean = torch.empty(b, C, device=DEV)
        core(q, k, v, b, lq, lk, heads, dh, scale, out=out, mean_out=mean)
        probs = probs_fn(q, k, b, lq, lk, heads, dh, scale)
        torch.cuda.synchronize()
        tag = f"{kind} heads={heads} dh={dh} lq={lq} lk={lk}"
        if not torch.equal(_bits(out.cpu()), _bits(exp)):
            d = (out.cpu().double() - exp.double())
            bad.append(f"{tag}: out != V[pi], {int((_bits(out.cpu()) != _bits(exp)).sum())} elements, "
                       f"max|diff| {d.abs().max().item():.3g}, nan {int(torch.isnan(d).sum())}")
        if not _guard_intact(buf, b * lq, C):
            bad.append(f"{tag}: columns past heads*dh of the strided out written")
        em, ep = _rel(mean, exp_mean), (probs.double().cpu() - exp_probs).abs().max().item()
        worst["mean"], worst["probs"] = max(worst["mean"], em), max(worst["probs"], ep)
        if not em <= 1e-6:
            bad.append(f"{tag}: mean_out rel {em:.3g} > 1e-6")
        if not ep <= 1e-6:
            bad.append(f"{tag}: probs err {ep:.3g} > 1e-6")
        if lq == lk:  # the BERT entries: packed [q | k | v] rows, all-ones key mask
            qkv = torch.cat([q, k, v], 1).view(b, lq, 3 * C)
            ones = torch.ones(b, lk, dtype=torch.int64, device=DEV)
            if f32:
                got = torch.empty(b * lq, C, device=DEV)
                ops.x3_attention(qkv.view(-1, 3 * C)[:, :C], qkv.view(-1, 3 * C)[:, C:2 * C], qkv.view(-1, 3 * C)[:, 2 * C:],
                                 b, lq, lk, heads, dh, scale, out=got, mask=ones)
            else:
                got = ops.bert_attention(qkv, ones, heads, dh).view(b * lq, C)
            if not torch.equal(_bits(got.cpu()), _bits(exp)):
                bad.append(f"{tag}: masked entry (all-ones mask) != V[pi]")
    print(json.dumps({"kind": kind, "heads": heads, "dh": dh, "worst": worst, "failed": len(bad)}))
    return bad


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("dh", DH_BF16)
def test_mha_selects_one_value_row_bitwise(dh, heads):
    """mmr_mha / mmr_bert_attention / mmr_mha_probs when softmax picks a single key per (head, query): the
    key-to-value pairing inside a tile (P^T's register order against the ds_read_tr16_b64 V^T fragment), the
    alpha / m_run updates with the maximum in the first block, the last block and rising over every block,
    the zero-padded Q columns and clamped K / V chunks of head dims that are no multiple of 32."""
    bad = _selection_grid("bf16", heads, dh)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("dh", DH_X3)
def test_x3_attention_selects_one_value_row_bitwise(dh, heads):
    """The same grid on mmr_x3_attention (plain and with an all-ones key mask) / mmr_x3_attention_probs: exact
    too — P = 1 splits into hi = 1, lo = 0, and V's lo image is zero."""
    bad = _selection_grid("x3", heads, dh)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("lk", [96, 160])
def test_selection_tile_filling_forms(lk):
    """The forms that need b*lq % 256 == 0 (b = 2, lq = 128): mmr_mha_q8 (heads*dh = 256) returns V[pi] and
    its MX-fp8 operand equals quantize_mxfp8 of it; mmr_x3_attention_xs (heads*dh = 120, kp = 128) returns
    hi = V[pi], lo = 0 and zero padding columns."""
    b, lq = 2, 128
    heads, dh = 4, 64
    q, k, v, scale, exp, exp_mean, _ = _selection_batch(b, lq, lk, heads, dh, lk, False)
    buf, out = _guarded(b * lq, heads * dh, torch.bfloat16)
    mean = torch.empty(b, heads * dh, device=DEV)
    _, _, o8 = ops.mha(q, k, v, b, lq, lk, heads, dh, scale, out=out, mean_out=mean, q8=True)
    ref8 = ops.quantize_mxfp8(exp.to(DEV), layout=0)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out.cpu()), _bits(exp)) and _guard_intact(buf, b * lq, heads * dh)
    assert torch.equal(o8.q, ref8.q) and torch.equal(o8.s, ref8.s)
    assert _rel(mean, exp_mean) <= 1e-6
    heads, dh = 3, 40
    q, k, v, scale, exp, exp_mean, _ = _selection_batch(b, lq, lk, heads, dh, lk + 1, True)
    mean = torch.empty(b, heads * dh, device=DEV)
    for mask in (None, torch.ones(b, lk, dtype=torch.int64, device=DEV)):
        xr = ops.x3_attention_split(q, k, v, b, lq, lk, heads, dh, scale, mask=mask, mean_out=mean)
        torch.cuda.synchronize()
        assert isinstance(xr, ops.X3Rows) and xr.kp == 128
        assert torch.equal(xr.t.view(torch.int16).cpu(), _split_bits(exp, xr.kp))
        assert _rel(mean, exp_mean) <= 1e-6


def _mask_case(kind, L, dh):
    """(b, heads, mask (b, L), qkv (b*L, 3C) in the kind's input type, f64 reference (b, L, C))."""
    heads = 4 if kind == "q8" else 2
    m6 = mask_geometries(L, L + dh)
    mask = torch.cat([m6, m6[:2]]) if kind == "q8" else m6    # q8: b*L % 256 == 0
    b, C = mask.shape[0], heads * dh
    g = torch.Generator().manual_seed(L * dh)
    qkv = torch.randn(b * L, 3 * C, generator=g)
    qkv = qkv * 0.7 if kind == "x3" else qkv.to(torch.bfloat16)
    ref = attn_f64(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], b, L, L, heads, dh, 1.0 / math.sqrt(dh), mask)
    return b, heads, mask, qkv, ref


# the MX-fp8 form needs head_dim % 32 == 0, b*L % 256 == 0 (b = 8) and heads*dh % 256 == 0 (heads = 4)
MASK_CASES = [(kind, L, dh) for kind in ("bf16", "x3") for L in (33, 64, 96, 160) for dh in (64, 40)]
MASK_CASES += [("q8", L, 64) for L in (64, 96, 160)]


@pytest.mark.parametrize("kind,L,dh", MASK_CASES)
def test_attention_mask_geometries(kind, L, dh):
    """Six key-mask shapes in one launch (attention_edges_ref.mask_geometries) against HF's additive mask in
    f64: all keys masked (HF: uniform softmax, the mean of V over the L keys), fully masked leading tiles,
    one live key in the last (ragged) tile, interior masked tiles + holes, right padding, none.

    Before the all-masked fix in mha_small (fusion.hip) sequence 0 of the bf16 / q8 forms was NaN at every
    shape here: every score of tile 0 is -FLT_MAX, p = exp2(fma(s, c2, -fl(m c2))) = exp2(-(rounding error of
    FLT_MAX c2)) = 0 for every key, l_run = 0 and the row is 0 * inf."""
    b, heads, mask, qkv, ref = _mask_case(kind, L, dh)
    C = heads * dh
    qd, md = qkv.to(DEV), mask.to(DEV)
    if kind == "x3":
        out = torch.empty(b * L, C, device=DEV)
        ops.x3_attention(qd[:, :C], qd[:, C:2 * C], qd[:, 2 * C:], b, L, L, heads, dh, 1.0 / math.sqrt(dh), out=out,
                         mask=md)
    else:
        out = ops.bert_attention(qd.view(b, L, 3 * C), md, heads, dh)
        if kind == "q8":
            ctx, c8 = ops.bert_attention(qd.view(b, L, 3 * C), md, heads, dh, q8=True)
            _, c8b = ops.bert_attention(qd.view(b, L, 3 * C), md, heads, dh, q8=True, bf16=False)
            ref8 = ops.quantize_mxfp8(out.view(b * L, C), layout=0)
            torch.cuda.synchronize()
            assert torch.equal(_bits(ctx), _bits(out))
            for x8 in (c8, c8b):
                assert torch.equal(x8.q, ref8.q) and torch.equal(x8.s, ref8.s)
    torch.cuda.synchronize()
    got = out.view(b, L, C).float().cpu()
    errs = [_rel(got[i], ref[i]) if torch.isfinite(got[i]).all() else float("nan") for i in range(b)]
    print(json.dumps({"kind": kind, "L": L, "dh": dh, "rel_per_sequence": errs,
                      "nonfinite_per_sequence": [int((~torch.isfinite(got[i])).sum()) for i in range(b)]}))
    assert torch.isfinite(got).all(), "NaN / Inf in the context"
    assert max(errs) <= TOL[kind], errs


@pytest.mark.parametrize("dh", [64, 40])
@pytest.mark.parametrize("kind", ["bf16", "x3"])
def test_attention_rising_row_maximum(kind, dh):
    """Logits of std ~ 8 whose row maximum rises with every 32-key tile (lk = 160, lq = 65): every online-softmax
    step rescales O and l by a small alpha, where N(0, 1) logits leave the running maximum almost still."""
    b, lq, lk, heads = 2, 65, 160, 2
    C = heads * dh
    cases = [rising_max_case(lq, lk, heads, dh, seed=5 + i) for i in range(b)]
    q, k, v = (torch.cat([c[j] for c in cases]) for j in range(3))
    scale = 1.0 / math.sqrt(dh)
    ref = attn_f64(q, k, v, b, lq, lk, heads, dh, scale)
    dt = torch.float32 if kind == "x3" else torch.bfloat16
    qd, kd, vd = (t.to(dt).to(DEV) for t in (q, k, v))
    out = torch.empty(b * lq, C, dtype=dt, device=DEV)
    mean = torch.empty(b, C, device=DEV)
    (ops.x3_attention if kind == "x3" else ops.mha)(qd, kd, vd, b, lq, lk, heads, dh, scale, out=out, mean_out=mean)
    torch.cuda.synchronize()
    rep = {"kind": kind, "dh": dh, "out": _rel(out.view(b, lq, C), ref), "mean": _rel(mean, ref.mean(1))}
    print(json.dumps(rep))
    assert rep["out"] <= TOL[kind] and rep["mean"] <= TOL[kind]


@pytest.mark.parametrize("lq", [1, 33, 130])
@pytest.mark.parametrize("kind", ["bf16", "x3"])
def test_attention_output_guards(kind, lq):
    """out with 2 guard rows before and after and ldo = heads*dh + 8, mean_out with 2 guard rows before and
    after, both pre-filled with a bit pattern: padded queries are never stored and nothing outside
    [b*lq) x [heads*dh) changes; the interior equals a plain (unpadded) launch bit for bit."""
    b, lk, heads, dh = 2, 65, 3, 40
    C = heads * dh
    dt = torch.float32 if kind == "x3" else torch.bfloat16
    g = torch.Generator().manual_seed(lq)
    q = (torch.randn(b * lq, C, generator=g) * 0.7).to(dt).to(DEV)
    k = (torch.randn(b * lk, C, generator=g) * 0.7).to(dt).to(DEV)
    v = (torch.randn(b * lk, C, generator=g) * 0.7).to(dt).to(DEV)
    core = ops.x3_attention if kind == "x3" else ops.mha
    scale = 1.0 / math.sqrt(dh)
    plain, plain_mean = torch.empty(b * lq, C, dtype=dt, device=DEV), torch.empty(b, C, device=DEV)
    core(q, k, v, b, lq, lk, heads, dh, scale, out=plain, mean_out=plain_mean)
    obuf, out = _guarded(b * lq, C, dt, pad_rows=2)
    mbuf, mean = _guarded(b, C, torch.float32, pad_rows=2, pad_cols=0)
    core(q, k, v, b, lq, lk, heads, dh, scale, out=out, mean_out=mean)
    torch.cuda.synchronize()
    assert _guard_intact(obuf, b * lq, C, pad_rows=2), "out: written outside [b*lq) x [heads*dh)"
    assert _guard_intact(mbuf, b, C, pad_rows=2), "mean_out: guard rows written"
    assert torch.equal(_bits(out), _bits(plain)) and torch.equal(_bits(mean), _bits(plain_mean))
    assert _rel(out.view(b, lq, C), attn_f64(q, k, v, b, lq, lk, heads, dh, scale)) <= TOL[kind]


def test_bert_tower_all_zero_attention_mask_row():
    """The bf16 BERT tower (towers_mini.npz weights) on a batch of 3 whose middle attention_mask row is all
    zero: that row follows HF (uniform attention in every layer) within the tower's usual bound instead of
    turning NaN, and the other rows are bit-identical to the same batch with the row's own mask."""
    f, w = towers_mini()
    cfg = dict(BERT_BASE, **json.loads(bytes(f["cfg"]).decode())["bert"])
    ids = torch.from_numpy(f["input_ids"])[[0, 1, 0]]
    mask = torch.from_numpy(f["attention_mask"])[[0, 1, 0]]
    zeroed = mask.clone()
    zeroed[1] = 0
    bt = BertTower(w["bert"], cfg, device=DEV)
    got = bt.forward(ids.to(DEV), zeroed.to(DEV)).float().cpu()
    base = bt.forward(ids.to(DEV), mask.to(DEV)).float().cpu()
    with torch.no_grad():
        ref = otw.bert_forward(ids, zeroed, w["bert"], cfg["num_hidden_layers"], cfg["num_attention_heads"])
    print(json.dumps({"nonfinite": int((~torch.isfinite(got)).sum()),
                      "rel_zeroed_row": _rel(got[1], ref[1]) if torch.isfinite(got[1]).all() else float("nan")}))
    assert torch.isfinite(got).all()
    _check_emb(got, ref)
    assert torch.equal(got[[0, 2]], base[[0, 2]])


# ------------------------------------------------------------------ Swin windows at ws != 7
SWIN = [(8, 16, 0), (8, 16, 3), (4, 8, 0), (4, 8, 1), (4, 8, 3)]  # ws, hw, shift: 64 keys (none padded) / 16 keys


def _swin_inputs(B, ws, hw, shift, heads, f32):
    g = torch.Generator().manual_seed(100 * ws + 10 * shift + heads + B)
    C = heads * 32
    qkv = torch.randn(B, hw, hw, 3 * C, generator=g)
    qkv = qkv * 0.7 if f32 else qkv.to(torch.bfloat16)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g) * (0.5 if f32 else 1.0)
    return qkv, table


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("ws,hw,shift", SWIN)
def test_swin_attn_bias_other_windows(ws, hw, shift, heads):
    """mmr_swin_attn_bias against the dense bias assembled from the oracle's relative_position_index and
    shift_mask (hw / ws = 2 windows a side: window index == the kernel's type), the same f32 sum: bitwise;
    key columns past ws*ws are -FLT_MAX."""
    N = ws * ws
    table = _swin_inputs(2, ws, hw, shift, heads, True)[1]
    got = ops.swin_attn_bias(table.to(DEV), heads, ws, hw, shift).cpu()
    exp = table[otw.relative_position_index(ws).view(-1)].view(N, N, heads).permute(2, 0, 1)[None]
    if shift:
        exp = exp + otw.shift_mask(hw, hw, ws, shift)[:, None]
    assert got.shape == (4 if shift else 1, heads, 64, 64)
    assert torch.equal(got[:, :, :N, :N], exp)
    assert (got[:, :, :N, N:] == torch.finfo(torch.float32).min).all()


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("ws,hw,shift", SWIN)
def test_swin_window_attention_other_windows(ws, hw, shift, heads):
    """mmr_swin_window_attention at 8 x 8 and 4 x 4 windows against the oracle restatement (2e-2), and its
    MX-fp8 form (B = 4: rows % 256 == 0) bit-identical to quantize_mxfp8 of the bf16 output, K padding included."""
    qkv, table = _swin_inputs(4, ws, hw, shift, heads, False)
    C = heads * 32
    ref = _swin_attn_ref(qkv.double(), table.double(), hw, heads, ws, shift)
    qd = qkv.to(DEV)
    bias = ops.swin_attn_bias(table.to(DEV), heads, ws, hw, shift)
    y = ops.swin_window_attention(qd, bias, hw, heads, ws, shift)
    y2 = ops.swin_window_attention(qd[:2].contiguous(), bias, hw, heads, ws, shift)  # B = 2
    a8 = ops.swin_window_attention_q8(qd, bias, hw, heads, ws, shift)
    ref8 = ops.quantize_mxfp8(y.reshape(-1, C), layout=0, kp=256)
    torch.cuda.synchronize()
    rep = {"ws": ws, "shift": shift, "heads": heads, "rel": _rel(y, ref)}
    print(json.dumps(rep))
    assert torch.isfinite(y.float()).all() and rep["rel"] <= 2e-2
    assert torch.equal(_bits(y2), _bits(y[:2]))
    assert a8.kp == 256 and a8.k == C
    assert torch.equal(a8.q, ref8.q) and torch.equal(a8.s, ref8.s)


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("ws,hw,shift", SWIN)
def test_x3_swin_window_attention_other_windows(ws, hw, shift, heads):
    """mmr_x3_swin_window_attention at 8 x 8 and 4 x 4 windows against f64 (5e-5), and its split-row form
    (B = 4: tokens % 256 == 0) bit-identical to the split of the f32 output, padding columns zero."""
    qkv, table = _swin_inputs(4, ws, hw, shift, heads, True)
    C = heads * 32
    ref = _swin_attn_ref(qkv.double(), table.double(), hw, heads, ws, shift)
    qd = qkv.to(DEV)
    bias = ops.swin_attn_bias(table.to(DEV), heads, ws, hw, shift)
    y = ops.x3_swin_window_attention(qd, bias, hw, heads, ws, shift)
    y2 = ops.x3_swin_window_attention(qd[:2].contiguous(), bias, hw, heads, ws, shift)  # B = 2
    xr = ops.x3_swin_window_attention_split(qd, bias, hw, heads, ws, shift)
    torch.cuda.synchronize()
    rep = {"ws": ws, "shift": shift, "heads": heads, "rel": _rel(y, ref)}
    print(json.dumps(rep))
    assert torch.isfinite(y).all() and rep["rel"] <= 5e-5
    assert torch.equal(y2, y[:2])
    assert isinstance(xr, ops.X3Rows) and xr.lead == (4, hw, hw)
    assert torch.equal(xr.t.view(torch.int16), _split_bits(y.reshape(-1, C), xr.kp))
