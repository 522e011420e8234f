"""CPU: the self-test of the fused-Swin kernel tests (swin_fused_ref.py); needs no GPU and no built library.

The rounding-point model Mdl (f32 torch, the kernels' documented bf16 rounding points) meets rule 1 and rule 2 at a
worst ratio <= 0.5 before its output rounding, and <= 1 after it, on every case test_swin_fused_gpu.py launches in
part C; the spike family does reach GELU pre-activations beyond +-7; the part-B predicate holds for the model at
every perturbed token; every mutant of CAUGHT_BY breaks its rule on its family at every size launched; the
structural mutants break the part-B predicate.

What the rules do not resolve at T <= 1000 (measured here on gauss, asserted as measured so that a change shows):
  lncm1 (variance over C - 1)        worst rule 1 / rule 2 ratio over all sizes: MLP 1.13 / 1.34 (both at C = 96,
                                     T = 1000; every other size below 1), attention block 1.02 / 0.98.
  tanh (tanh-GELU), qscale_after     no case above 0.84: their error against f64 has the RMS of the model's own
                                     (within 10 %), so no rule against f64 that admits the model can see them.
  pad_key                            seen on the shifted cases (shift 3, every geometry: 1.35 ... 2.6), where the
                                     corner windows' small mask regions let one extra key weigh; at shift 0 one key
                                     among 50 moves the output by less than the output rounding (0.8).
Measured worst ratios of the model (rule 1, rule 2): MLP 0.489, 0.064; attention block 0.459, 0.148; linear_rw
0.355, 4e-4 (its sigma is f32 summation noise alone).  Caught mutants, rule 1 ratio over all sizes: b2drop 47 ... 179
(rule 2: 239 ... 1246), lnhalf 3.5 ... 12.8, nores_tail > 200, projb_shift > 90, relpos_T > 25, rw_order > 1e5."""
import json

import pytest
import torch

import swin_fused_ref as S


def _model_ok(k, tag, bad, worst):
    r1, r2 = S.judge(k["mdl"], k["R"], k["sigma"])
    b1, b2 = S.judge(S.bf(k["mdl"]), k["R"], k["sigma"])
    if not (r1 <= S.MODEL_MAX and r2 <= S.MODEL_MAX):
        bad.append(f"{tag}: model at {r1:.3f} / {r2:.3f} > {S.MODEL_MAX}")
    if not (b1 <= 1.0 and b2 <= 1.0):
        bad.append(f"{tag}: bf16(model) at {b1:.3f} / {b2:.3f} > 1")
    worst[0], worst[1] = max(worst[0], r1), max(worst[1], r2)


@pytest.mark.parametrize("C", S.MLP_C)
def test_model_meets_rules_mlp(C):
    bad, worst = [], [0.0, 0.0]
    for T in S.MLP_T:
        for fam in S.FAMILIES:
            _model_ok(S.mlp_case(fam, T, C), f"mlp C={C} T={T} {fam}", bad, worst)
    print(json.dumps({"kernel": "mlp", "C": C, "rule1": worst[0], "rule2": worst[1]}))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("B,hw", S.ATTN_GEO)
def test_model_meets_rules_attn(B, hw):
    bad, worst = [], [0.0, 0.0]
    for shift in S.ATTN_SHIFTS:
        for fam in S.FAMILIES:
            _model_ok(S.attn_case(fam, B, hw, shift), f"attn B={B} hw={hw} shift={shift} {fam}", bad, worst)
    print(json.dumps({"kernel": "attn", "B": B, "hw": hw, "rule1": worst[0], "rule2": worst[1]}))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("N,K,bias,res", S.RW_CASES)
def test_model_meets_rules_rw(N, K, bias, res):
    bad, worst = [], [0.0, 0.0]
    for M in S.RW_M:
        for fam in S.FAMILIES:
            _model_ok(S.rw_case(fam, M, N, K, bias, res), f"rw {N}x{K} M={M} {fam}", bad, worst)
    print(json.dumps({"kernel": "rw", "N": N, "K": K, "rule1": worst[0], "rule2": worst[1]}))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("C", S.MLP_C)
def test_spike_family_leaves_the_gelu_fit_interval(C):
    """gelu_fast was fitted on [-7, 7] (common.h): the spike cases put fc1 pre-activations outside it."""
    for T in (33, 257, 1000):
        pre = S.mlp_preact(S.rows("spike", T, C, 0), S.mlp_params(C))
        assert int((pre > 7).sum()) >= 10 and int((pre < -7).sum()) >= 10, (T, pre.abs().max().item())


def test_constant_rows_are_capped_where_rule2_applies():
    for T in S.MLP_T:
        x = S.rows("constant", T, 96, 0).float()
        flat = (x == x[:, :1]).all(1)
        assert int(flat.sum()) == S.n_const(T) and bool(flat[:S.n_const(T)].all())
        m = S.rows("mixed", T, 96, 0).float()
        assert 1 <= int((m == m[:, :1]).all(1).sum()) <= max(S.n_const(T), 1) or T < 4
    assert S.n_const(1000) == 15 and S.n_const(257) == 8 and S.n_const(33) == 33


# ------------------------------------------------------------------------------------------------ mutants
def _mutant_ratios(kernel, mutant, fam):
    """[(tag, rule 1 ratio, rule 2 ratio)] of bf16(mutant of Mdl) over every size launched."""
    out = []
    if kernel == "mlp":
        for C in S.MLP_C:
            for T in S.MLP_T:
                k = S.mlp_case(fam, T, C)
                y = S.bf(S.mlp_chain(k["x"], k["p"], torch.float32, True, mutant))
                out.append((f"C={C} T={T}",) + S.judge(y, k["R"], k["sigma"]))
    elif kernel == "attn":
        for B, hw in S.ATTN_GEO:
            for shift in S.ATTN_SHIFTS:
                k = S.attn_case(fam, B, hw, shift)
                y = S.bf(S.attn_chain(k["x"], k["p"], shift, torch.float32, True, mutant))
                out.append((f"B={B} hw={hw} shift={shift}",) + S.judge(y, k["R"], k["sigma"]))
    else:
        for N, K, bias, res in S.RW_CASES:
            for M in S.RW_M:
                k = S.rw_case(fam, M, N, K, bias, res)
                y = S.bf(S.rw_chain(k["x"], k["p"], k["r"], torch.float32, mutant))
                out.append((f"{N}x{K} M={M}",) + S.judge(y, k["R"], k["sigma"]))
    return out


@pytest.mark.parametrize("mutant", [m for m, v in S.CAUGHT_BY.items() if v[1] != "locality"])
def test_mutant_breaks_its_rule_at_every_size(mutant):
    kernel, rule, fam = S.CAUGHT_BY[mutant]
    rows = _mutant_ratios(kernel, mutant, fam)
    if mutant == "pad_key":
        rows = [r for r in rows if "shift=3" in r[0]]
    if mutant == "nores_tail":
        assert all(T % 32 for T in S.MLP_T)          # every launched size has a ragged last tile
    print(json.dumps({mutant: [(t, round(a, 2), round(b, 2)) for t, a, b in rows]}))
    assert rows and all(r[1] > 1.0 for r in rows), rows
    if mutant in ("b2drop", "projb_shift"):          # a wrong bias entry is also what rule 2 is for
        assert all(r[2] > 1.0 for r in rows if r[2] > 0), rows


def _locality_all(hw, shift, mutant, B=2):
    """Part B on the model: verdicts for every perturbed token (image 1 of B)."""
    p = S.attn_params(0)
    x = S.rows("gauss", B * hw * hw, S.AC, 7 * hw + shift).view(B, hw, hw, S.AC)
    y = S.bf(S.attn_chain(x, p, shift, torch.float32, True, mutant))
    out = []
    for row, col in S.locality_tokens(hw, shift):
        y2 = S.bf(S.attn_chain(S.perturb(x, (1, row, col)), p, shift, torch.float32, True, mutant))
        out.append(S.locality_verdict(S.changed_tokens(y, y2), hw, shift, 1, row, col))
    return out


@pytest.mark.parametrize("hw,shift", [(14, 0), (14, 3), (14, 5), (21, 0), (21, 3), (21, 5)])
def test_locality_predicate_holds_for_the_model(hw, shift):
    """The -100 mask leaves e^-100: below a bf16 P and below an f32 ulp of the row sum, so the model (f32, P
    rounded to bf16) keeps everything outside the allowed region bit for bit."""
    assert _locality_all(hw, shift, None) == [None] * len(S.locality_tokens(hw, shift))


@pytest.mark.parametrize("mutant", [m for m, v in S.CAUGHT_BY.items() if v[1] == "locality"])
@pytest.mark.parametrize("hw,shift", [(14, 3), (14, 5), (21, 3), (21, 5)])
def test_structural_mutant_leaves_the_allowed_region(mutant, hw, shift):
    verdicts = _locality_all(hw, shift, mutant)
    print(json.dumps({mutant: verdicts}))
    assert sum(v is not None and "outside" in v for v in verdicts) >= 2, verdicts


def test_allowed_region_geometry():
    """The predicate's own construction: unshifted it is the token's 7 x 7 window; shifted, a token of an interior
    window keeps the whole (rolled) window, a token of the corner window only its mask region."""
    a = S.allowed_region(14, 0, 3, 10)
    assert int(a.sum()) == 49 and bool(a[:7, 7:].all())
    a = S.allowed_region(14, 3, 6, 6)             # rolled (3, 3): window (0, 0), no mask
    assert int(a.sum()) == 49 and bool(a[3:10, 3:10].all())
    a = S.allowed_region(14, 3, 1, 1)             # rolled (12, 12): corner window, the 3 x 3 wrapped region
    assert int(a.sum()) == 9 and bool(a[:3, :3].all())
    a = S.allowed_region(14, 3, 13, 1)            # rolled (10, 12): corner window, rows 7..10 x cols 11..13
    assert int(a.sum()) == 12 and bool(a[10:14, :3].all())


def test_mutants_the_rules_do_not_resolve():
    """Module docstring: measured, and asserted as measured."""
    worst = {}
    for m, kernel in (("tanh", "mlp"), ("lncm1", "mlp"), ("lncm1", "attn"), ("qscale_after", "attn")):
        rr = _mutant_ratios(kernel, m, "gauss")
        worst[f"{m}/{kernel}"] = (max(r[1] for r in rr), max(r[2] for r in rr))
    print(json.dumps(worst))
    assert worst["tanh/mlp"][0] < 1 and worst["tanh/mlp"][1] < 1
    assert worst["qscale_after/attn"][0] < 1 and worst["qscale_after/attn"][1] < 1
    assert worst["lncm1/mlp"][1] > 1                                  # rule 2 at C = 96, T = 1000
    for m, chain, k in (("tanh", S.mlp_chain, S.mlp_case("gauss", 1000, 96)),
                        ("qscale_after", None, S.attn_case("gauss", 1, 56, 3))):
        mut = (S.mlp_chain(k["x"], k["p"], torch.float32, True, m) if chain else
               S.attn_chain(k["x"], k["p"], 3, torch.float32, True, m))
        assert S.sigma(mut, k["R"]) <= 1.1 * k["sigma"], m
    pk = [r for r in _mutant_ratios("attn", "pad_key", "gauss") if "shift=0" in r[0]]
    assert all(r[1] < 1 for r in pk), pk
