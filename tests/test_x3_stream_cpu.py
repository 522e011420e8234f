"""CPU: the self-test of the streamed x3 kernel tests (x3_stream_ref.py); needs no GPU and no built library.

On every case test_x3_stream_gpu.py launches in part C, the bf16x3 model in its second summation order ("seq":
16-wide k-steps added in sequence) stays within rule 2 at 6 s and rules 3 and 4 at 2 s, with s taken from the
first order, and |e(Mdl)| <= 0.05 (MLP) / 0.2 (x3_rowlin and the stem: bare linears) in both orders; every mutant
of CAUGHT_BY breaks the named rule on the named family at every size launched; the bf16 stem's model meets its
per-element rule; the families are what the module docstring says.

Measured worst ratios of the model, both orders (max|e|, rule 2, rule 3, rule 4, in s):
  MLP C = 96 0.004, 5.43, 1.60, 1.40;  MLP C = 192 0.002, 5.12, 1.31, 1.51;  x3_rowlin 0.089, 5.95, 1.49, 1.45;
  stem 0.074, 5.97, 1.61, 2.00.
Mutants, the named rule's ratio over all sizes (rule 1: max|e| against 1; rule 3: worst row against 3 s):
  fc2_kstep_one 25 ... 81 s, fc2_kstep_all 27 ... 92 s, fc1_xlo 237 ... 392 s, tanh 12.6 ... 20.3 s, lncm1 291 ... 853 s
  (x3_rowlin 631 ... 1527 s), noeps > 7000 s, onepass 7.2 ... 12.4 s (x3_rowlin 17.4 ... 18.3 s); gshift, bshift,
  nores_tail, ky_swap, nobias: max|e| > 110."""
import json

import pytest
import torch

import x3_stream_ref as S


def _model_ok(tag, y_seq, y_mm, k, bad, worst, sanity=S.W_SANITY):
    j = S.judge(y_seq, k["R"], k["W"], k["s"])
    m = S.judge(y_mm, k["R"], k["W"], k["s"])
    if S.verdict(j, S.CAP2, S.CAP34):
        bad.append(f"{tag}: model (seq) at {[round(v, 3) for v in j]}")
    if not (j[0] <= sanity and m[0] <= sanity):
        bad.append(f"{tag}: |e(Mdl)| = {j[0]:.4f} / {m[0]:.4f} > {sanity}")
    for i in range(4):
        worst[i] = max(worst[i], j[i], m[i])


@pytest.mark.parametrize("C", S.MLP_C)
def test_model_meets_rules_mlp(C):
    bad, worst = [], [0.0] * 4
    for fam, T in S.MLP_CASES:
        k = S.mlp_case(fam, T, C)
        _model_ok(f"mlp C={C} T={T} {fam}", S.mlp_M(k["x"], k["p"], "seq"), S.mlp_M(k["x"], k["p"]), k, bad, worst)
    print(json.dumps({"kernel": "mlp", "C": C, "max|e|, rule2, rule3, rule4": worst}))
    assert not bad, "\n".join(bad)


def test_model_meets_rules_rowlin():
    bad, worst = [], [0.0] * 4
    for c, n, mode, fam, T in S.ROW_CASES:
        k = S.row_case(c, n, mode, fam, T)
        _model_ok(f"rowlin {c}x{n} {mode} T={T} {fam}", S.rowlin_M(k["x"], k["p"], mode, k["res"], "seq"),
                  S.rowlin_M(k["x"], k["p"], mode, k["res"]), k, bad, worst, S.W_BARE)
    print(json.dumps({"kernel": "rowlin", "max|e|, rule2, rule3, rule4": worst}))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("fam,B,hw", S.STEM_CASES)
def test_model_meets_rules_stem(fam, B, hw):
    bad, worst = [], [0.0] * 4
    k = S.stem_case(fam, B, hw)
    _model_ok(f"stem B={B} hw={hw} {fam}", S.stem_M(k["img"], k["p"], True, "seq"), S.stem_M(k["img"], k["p"]), k, bad,
              worst, S.W_BARE)
    yb = S.bf(S.stem_M(k["img"], k["p"], x3=False))
    err = (yb.double() - k["Rb"]).abs()
    if not bool((err <= S.stem_bf16_tol(k["Rb"])).all()):
        bad.append(f"stem bf16 B={B} hw={hw} {fam}: model outside 2^-8 |R| + 2e-3")
    print(json.dumps({"kernel": "stem", "case": [fam, B, hw], "max|e|, rule2, rule3, rule4": worst}))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ mutants
def _mutant_rows(kernel, mutant, fam):
    """[(tag, judge())] of the mutant of Mdl over every case of `fam` that the GPU file launches and the mutant
    touches (LayerNorm mutants: the ln modes; residual mutants: the residual modes with a partial last workgroup)."""
    out = []
    if kernel == "mlp":
        for C in S.MLP_C:
            for f, T in S.MLP_CASES:
                if f != fam or (mutant == "nores_tail" and T % 128 == 0):
                    continue
                k = S.mlp_case(f, T, C)
                out.append((f"C={C} T={T}", S.judge(S.mlp_M(k["x"], k["p"], "mm", mutant), k["R"], k["W"], k["s"])))
    elif kernel == "rowlin":
        for c, n, mode, f, T in S.ROW_CASES:
            if f != fam:
                continue
            if mutant in ("lncm1", "noeps", "onepass", "gshift") and not mode.startswith("ln"):
                continue
            if mutant == "nores_tail" and (not mode.endswith("res") or T % 256 == 0):
                continue
            k = S.row_case(c, n, mode, f, T)
            y = S.rowlin_M(k["x"], k["p"], mode, k["res"], "mm", mutant)
            out.append((f"{c}x{n} {mode} T={T}", S.judge(y, k["R"], k["W"], k["s"])))
    else:
        for f, B, hw in S.STEM_CASES:
            if f != fam:
                continue
            k = S.stem_case(f, B, hw)
            out.append((f"B={B} hw={hw}", S.judge(S.stem_M(k["img"], k["p"], True, "mm", mutant), k["R"], k["W"],
                                                  k["s"])))
    return out


@pytest.mark.parametrize("mutant,kernel,rule,fam", [(m, *v) for m, vs in S.CAUGHT_BY.items() for v in vs])
def test_mutant_breaks_its_rule_at_every_size(mutant, kernel, rule, fam):
    rows = _mutant_rows(kernel, mutant, fam)
    print(json.dumps({f"{mutant}/{kernel}": [(t, [round(v, 2) for v in j]) for t, j in rows]}))
    assert rows
    missed = [t for t, j in rows if rule not in (S.verdict(j) or [])]
    assert not missed, (mutant, kernel, rule, missed)


def test_every_mutant_is_listed():
    assert set(S.CAUGHT_BY) == set(S.MLP_MUTANTS) | set(S.ROW_MUTANTS) | set(S.STEM_MUTANTS)
    for m in S.ROW_MUTANTS:
        assert any(v[0] == "rowlin" for v in S.CAUGHT_BY[m]), m


# ------------------------------------------------------------------------------------------------ the inputs
def test_constant_rows_are_exact_for_the_model():
    """The constant rows' LayerNorm gives beta exactly (module docstring), so their branch is one clean vector."""
    for C in S.MLP_C:
        for T in (257, 1000):
            x = S.rows("constant", T, C)
            flat = (x == x[:, :1]).all(1)
            assert int(flat.sum()) == S.N_CONST and bool(flat[:S.N_CONST].all())
            assert x[:S.N_CONST, 0].unique().numel() == S.N_CONST
            assert 4 <= x[:S.N_CONST].min() and x[:S.N_CONST].max() <= 12
            p = S.mlp_params(C)
            z = S._ln_m(x, p["g"], p["b"], S.EPS)
            assert torch.equal(z[:S.N_CONST], p["b"].expand(S.N_CONST, C))


def test_families():
    x = S.rows("spike", 200, 96)
    i = torch.arange(200)
    assert bool((x[i, (7 * i) % 96] > 4.5).all())
    for B, hw in ((1, 32), (3, 32), (1, 64), (3, 224)):
        pt = S.patches(S.images("constant", B, hw)).view(B, -1, 48)
        flat = (pt == pt[..., :1]).all(-1)
        assert int(flat.sum()) == (pt.shape[0] * pt.shape[1] if B * pt.shape[1] < 256 else S.N_CONST)
        px = S.patches(S.images("pixel", B, hw)).view(B, -1, 48)
        assert bool(((px == 50.0).sum(-1) == 1).all())
    # patches() is the conv's own im2col: the f32 conv of torch agrees with the product over it
    p, img = S.stem_params(), S.images("gauss", 2, 32)
    v = torch.nn.functional.conv2d(img.double(), p["w"].double(), stride=4).permute(0, 2, 3, 1).reshape(-1, 96)
    assert torch.allclose(S.patches(img).double() @ p["w"].double().reshape(96, 48).T, v, rtol=0, atol=1e-12)


def test_split_rows_hold_the_exact_operand():
    x = S.rows("gauss", 33, 96)
    t = S.split_rows(x, 128)
    hi, lo = S.split(x)
    assert torch.equal(t[:, :96].float(), hi) and torch.equal(t[:, 128:224].float(), lo)
    assert not t[:, 96:128].any() and not t[:, 224:].any()
