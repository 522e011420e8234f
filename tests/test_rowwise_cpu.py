"""CPU: the self-test of the row-kernel tests (rowwise_ref.py).  A plain f32 two-pass LayerNorm with fully
sequential sums (the worst summation order a kernel could have) passes both rules, the per-element bound and the
99 % bit-equality share, on every (family, width, variant) test_rowwise_gpu.py launches, within 1.0 of the bf16
bound and 0.5 of the f32 bounds; each mutant of that model breaks a rule at every width on the family named in
rowwise_ref.CAUGHT_BY; the `constant` family gives beta exactly."""
import json

import pytest
import torch

import rowwise_ref as R


def _judge(cases, out):
    """Run the model over the cases: (worst ratio, lowest bit share, list of failures)."""
    worst, share, bad = 0.0, 1.0, []
    for k in cases:
        y = R.model_f32(k["v32"], k["g_rows"], k["b_rows"], k["eps"], out=out, extra32=k["extra32"])
        tag = f"{k['fam']} c={k['c']} eps={k['eps']} alpha={k.get('alpha')} res={k.get('r') is not None}"
        if out == "bf16":
            ra, sh = R.measure(y, k["ref"], k["tol_bf16"]), R.bit_share(y, k["ref"])
            if not ra <= R.MODEL_BF16 or not sh >= R.BIT_SHARE:
                bad.append(f"{tag}: err/tol {ra:.3g}, bit share {sh:.4f}")
            share = min(share, sh)
        else:
            ra = R.measure(y, k["ref"], k["tol_f32"])
            if not ra <= R.MODEL_F32:
                bad.append(f"{tag}: err/tol {ra:.3g} > {R.MODEL_F32}")
        if k["exact_beta"]:
            exp = R.bf16_rn(k["b_rows"]) if out == "bf16" else k["b_rows"].float()
            if not torch.equal(R.bits(y), R.bits(exp.expand(y.shape))):
                bad.append(f"{tag}: constant rows != beta")
        worst = max(worst, ra)
    return worst, share, bad


@pytest.mark.parametrize("c", R.LN_WIDTHS)
def test_model_passes_layernorm_cases(c):
    worst, share, bad = _judge(R.layernorm_cases(c), "bf16")
    print(json.dumps({"c": c, "worst": worst, "share": share}))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c", R.LNROWS_BF16)
def test_model_passes_ln_rows_bf16_cases(c):
    worst, share, bad = _judge(R.lnrows_cases(c, torch.bfloat16), "bf16")
    print(json.dumps({"c": c, "worst": worst, "share": share}))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c", [c for c, _ in R.LNROWS_F32])
def test_model_passes_ln_rows_f32_cases(c):
    worst, _, bad = _judge(R.lnrows_cases(c, torch.float32), "f32")
    print(json.dumps({"c": c, "worst": worst}))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c", R.EMBED_WIDTHS)
def test_model_passes_bert_embed_cases(c):
    b, l = R.EMBED_BL[-1]
    worst, share, bad = _judge(R.embed_cases(c, b, l), "bf16")
    print(json.dumps({"c": c, "worst": worst, "share": share}))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c", R.MERGE_WIDTHS)
def test_model_passes_patch_merge_cases(c):
    B, H = R.MERGE_BH[-1]
    worst, share, bad = _judge([R.merge_case(B, H, c, c)], "bf16")
    print(json.dumps({"c": c, "worst": worst, "share": share}))
    assert not bad, "\n".join(bad)


def test_patch_merge_quadrant_order_is_visible():
    """Swapping two source pixels of the merge (any of the six pairs) breaks both rules at every width (the row's
    statistics survive a permutation, so the two untouched quarters stay right)."""
    for c in R.MERGE_WIDTHS:
        k = R.merge_case(3, 6, c, c)
        v = k["v32"].view(-1, 4, c)
        for i, j in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            p = list(range(4))
            p[i], p[j] = j, i
            y = R.model_f32(v[:, p].reshape(-1, 4 * c), k["g"], k["b"], k["eps"])
            assert not R.measure(y, k["ref"], k["tol_bf16"]) <= 1.0 and R.bit_share(y, k["ref"]) < R.BIT_SHARE, (c, i, j)


@pytest.mark.parametrize("c", R.HEAD_WIDTHS)
def test_model_passes_swin_head_cases(c):
    bad, worst = [], {"patches": 0.0, "glob": 0.0, "pool": 0.0}
    for fam in R.FAMILIES:
        for t in R.HEAD_T:
            k = R.head_case(fam, max(R.HEAD_B), t, c, c + t)
            got = dict(zip(("patches", "glob", "pool"), R.model_head(k["x"], k["g"], k["b_"], k["eps"])))
            for name in worst:
                ra = R.measure(got[name], k[name], k["tol_" + name])
                worst[name] = max(worst[name], ra)
                if not ra <= R.MODEL_F32:
                    bad.append(f"{fam} t={t} {name}: err/tol {ra:.3g}")
    print(json.dumps({"c": c, "worst": worst}))
    assert not bad, "\n".join(bad)


def test_model_passes_mean_tokens_cases():
    for c in R.MEAN_WIDTHS:
        for l in R.MEAN_L:
            k = R.mean_case(2, l, c, c + l)
            s = torch.zeros(2, c)
            for t in range(l):
                s = s + k["x"][:, t].float()
            assert R.measure(s / l, k["ref"], k["tol"]) <= R.MODEL_F32, (c, l)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_is_caught_at_every_width(mutant):
    """The plain (no alpha, no residual) case of the named family breaks a rule under the mutant, at every width
    of the layernorm_launch tests."""
    fam = R.CAUGHT_BY[mutant]
    report = {}
    for c in R.LN_WIDTHS:
        k = R.ln_case(fam, max(R.LN_ROWS), c, c)
        y = R.model_f32(k["v32"], k["g_rows"], k["b_rows"], k["eps"], mutant=mutant)
        ra, sh = R.measure(y, k["ref"], k["tol_bf16"]), R.bit_share(y, k["ref"])
        report[c] = (round(ra, 3), round(sh, 4))
        if mutant == "onepass" and c == 8:
            # no mutant here: squares of bf16 values near 40 are multiples of 2^-4 below 2^11, eight of them
            # sum exactly in f32, and the one-pass variance is the correctly rounded one
            assert torch.equal(R.bits(y), R.bits(R.model_f32(k["v32"], k["g_rows"], k["b_rows"], k["eps"])))
            continue
        assert not ra <= 1.0 or sh < R.BIT_SHARE, f"{mutant} passes on {fam} at c={c}: err/tol {ra:.3g}, share {sh:.4f}"
    print(json.dumps({"mutant": mutant, "family": fam, "err/tol, share by c": report}))


def test_outlier_sits_in_the_last_chunk():
    for c in (8, 96, 1000, 4096):
        x = R.family("outlier", 20, c, 1).float()
        pos = (x == 30.0).nonzero()
        assert pos.shape[0] == 20 and bool((pos[:, 1] >= c - 8).all())
        assert len(set(pos[:, 1].tolist())) == min(8, c)


def test_constant_family_gives_beta_exactly():
    for c in R.LN_WIDTHS:
        for res in (False, True):
            k = R.ln_case("constant", 5, c, c, res=res)
            assert k["exact_beta"] and torch.equal(k["ref"], k["b"].double().expand(5, c))
            y = R.model_f32(k["v32"], k["g"], k["b"], k["eps"])
            assert torch.equal(R.bits(y), R.bits(R.bf16_rn(k["b"]).expand(5, c)))
            y32 = R.model_f32(k["v32"], k["g"], k["b"], k["eps"], out="f32")
            assert torch.equal(y32, k["b"].expand(5, c))


def test_cases_are_reproducible_and_row_prefixes_agree():
    """The GPU file computes a reference at the largest row count and launches on its leading rows."""
    a, b = R.ln_case("gauss", 67, 160, 3, alpha=0.7, res=True), R.ln_case("gauss", 67, 160, 3, alpha=0.7, res=True)
    assert torch.equal(a["ref"], b["ref"]) and torch.equal(R.bits(a["x"]), R.bits(b["x"]))
    k = R.ln_case("gauss", 13, 100, 3, alpha=0.7, res=True, groups=3, group_div=2, post=True)
    r9, *_ = R.ln_f64(R.operand_f64(k["x"][:9], k["alpha"][(torch.arange(9) // 2) % 3][:, None], k["r"][:9]),
                      k["g_rows"][:9], k["b_rows"][:9], k["eps"])
    assert torch.equal(r9 + k["extra32"][:9].double(), k["ref"][:9])
