"""CPU: the self-test of the small-linear tests (small_linear_ref.py).  The f32 models of linear_f32, linear_x3 and
gemm_rw stay within MODEL_F32 / MODEL_X3 / MODEL_RW of the per-element bounds on every case test_small_linear_gpu.py
launches and reproduce the exact families bit for bit; each mutant breaks a rule on the family named in CAUGHT_BY at
every case where it changes the computation at all (where it cannot, that is asserted instead); the integer and
split families are exact by construction; erf_as is within 1.5e-7 of erf."""
import json

import pytest
import torch

import rowwise_ref as R
import small_linear_ref as L

BMAX = max(L.LIN_B)


def _nws(cin, cout):
    return sorted({L.x3_nw(cin, cout, BMAX, pin=p) for p in L.X3_PINS})


def _judge(kind, inp, nw, share):
    """The model over the 8 epilogues of one case: (worst err / tol, failures)."""
    x, w, cin = inp["x"], inp["w"], inp["cin"]
    parts = L.model_partials(kind, x.float(), w.float(), nw)
    P, A = L.products(x, w)
    worst, bad = 0.0, []
    for act, bias_on, res_on in L.EPILOGUES:
        bias, r = (inp["bias"] if bias_on else None), (inp["r"] if res_on else None)
        y = L.model_epilogue(parts, bias, r, act)
        ref, tol = L.lin_ref(kind, P, A, bias, r, act, cin, nw)
        ra = L.measure(y, ref, tol)
        worst = max(worst, ra)
        tag = f"{kind} {inp['fam']} cin={cin} cout={inp['cout']} nw={nw} act={act} bias={bias_on} res={res_on}"
        if not ra <= share:
            bad.append(f"{tag}: err / tol {ra:.3g} > {share}")
        exp = L.expected_exact(inp, bias_on, res_on) if not act else None
        if exp is not None and not torch.equal(L.bits(y), L.bits(exp)):
            bad.append(f"{tag}: not bit-exact")
    return worst, bad


@pytest.mark.parametrize("cin", L.X3_CIN)
def test_model_passes_linear_x3_cases(cin):
    worst, bad = 0.0, []
    for cout in L.X3_COUT:
        for fam in L.families("x3"):
            inp = L.lin_inputs("x3", fam, BMAX, cin, cout, 0)
            for nw in _nws(cin, cout):
                wo, b = _judge("x3", inp, nw, L.MODEL_X3)
                worst, bad = max(worst, wo), bad + b
    print(json.dumps({"kernel": "linear_x3", "cin": cin, "worst": worst}))
    assert not bad, "\n".join(bad[:20])


def test_model_passes_linear_x3_auto4_case():
    b, cin, cout = L.X3_AUTO4
    assert L.x3_nw(cin, cout, b) == 4 and L.x3_nw(cin, cout, BMAX) == 8
    for fam in ("integer", "gauss"):
        worst, bad = _judge("x3", L.lin_inputs("x3", fam, b, cin, cout, 0), 4, L.MODEL_X3)
        assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("cin", L.F32_CIN)
def test_model_passes_linear_f32_cases(cin):
    worst, bad = 0.0, []
    for cout in L.F32_COUT:
        for fam in L.families("f32"):
            wo, b = _judge("f32", L.lin_inputs("f32", fam, BMAX, cin, cout, 0), None, L.MODEL_F32)
            worst, bad = max(worst, wo), bad + b
    print(json.dumps({"kernel": "linear_f32", "cin": cin, "worst": worst}))
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("n,k", L.RW_NK)
def test_model_passes_linear_rw_cases(n, k):
    worst, share, bad = 0.0, 1.0, []
    for fam in L.families("rw"):
        inp = L.lin_inputs("rw", fam, max(L.RW_M), k, n, 0)
        P, A = L.products(inp["x"], inp["w"])
        for bias_on in (False, True):
            for res_on in (False, True):
                bias, r = (inp["bias"] if bias_on else None), (inp["r"] if res_on else None)
                y = L.model_rw(inp["x"], inp["w"], bias, r)
                ref, tol = L.lin_ref("rw", P, A, bias, r, 0, k)
                ra, sh = L.measure(y, ref, tol), L.bit_share(y, ref)
                worst, share = max(worst, ra), min(share, sh)
                tag = f"rw {fam} N={n} K={k} bias={bias_on} res={res_on}"
                if not ra <= L.MODEL_RW or not sh >= L.BIT_SHARE:
                    bad.append(f"{tag}: err / tol {ra:.3g}, bit share {sh:.4f}")
                exp = L.expected_exact(inp, bias_on, res_on)
                if exp is not None and not torch.equal(L.bits(y), L.bits(exp)):
                    bad.append(f"{tag}: not bit-exact")
    print(json.dumps({"kernel": "linear_rw", "N": n, "K": k, "worst": worst, "share": share}))
    assert not bad, "\n".join(bad[:20])


# ---------------------------------------------------------------------------------------------- mutants
def _caught(kind, inp, nw, mutant, act, bias_on, res_on, **kw):
    """(the mutant breaks a rule, its output differs from the model's at all)."""
    bias, r = (inp["bias"] if bias_on else None), (inp["r"] if res_on else None)
    y = L.model_linear(kind, inp["x"], inp["w"], bias, r, act, nw, mutant, **kw)
    y0 = L.model_linear(kind, inp["x"], inp["w"], bias, r, act, nw)
    P, A = L.products(inp["x"], inp["w"])
    ref, tol = L.lin_ref(kind, P, A, bias, r, act, inp["cin"], nw)
    broke = not L.measure(y, ref, tol) <= 1.0
    if kind == "rw":
        broke = broke or L.bit_share(y, ref) < L.BIT_SHARE
    exp = L.expected_exact(inp, bias_on, res_on) if not act else None
    if exp is not None:
        broke = broke or not torch.equal(L.bits(y), L.bits(exp))
    return broke, not torch.equal(L.bits(y), L.bits(y0))


def _shapes(kind):
    if kind == "x3":
        return [(cin, cout, nw) for cin in L.X3_CIN for cout in L.X3_COUT for nw in _nws(cin, cout)]
    if kind == "f32":
        return [(cin, cout, None) for cin in L.F32_CIN for cout in L.F32_COUT]
    return [(k, n, None) for n, k in L.RW_NK]


@pytest.mark.parametrize("kind,mutant", [(k, m) for k in ("f32", "x3", "rw") for m in L.MUTANTS[k]
                                         if m not in ("resstride", "bias0")])
def test_mutant_is_caught_at_every_case(kind, mutant):
    fam = L.CAUGHT_BY[mutant]
    act = 1 if mutant in ("actlate", "tanh") else 0
    rows = max(L.RW_M) if kind == "rw" else BMAX
    for cin, cout, nw in _shapes(kind):
        inp = L.lin_inputs(kind, fam, rows, cin, cout, 0)
        broke, differs = _caught(kind, inp, nw, mutant, act, True, True)
        idle = (mutant == "nopart" and kind == "f32" and L.f32_route(cin)[7] == 0) or (mutant == "biastile" and cout == 32)
        if idle:
            # no mutant here: wave 7 has no k-step (cin / 16 < 8 or 9 steps at per = 2), or the only tile's columns
            # are the bias indices
            assert not differs, (kind, mutant, cin, cout)
            continue
        assert broke, f"{mutant} passes on {fam} at {kind} cin={cin} cout={cout} nw={nw}"


@pytest.mark.parametrize("kind", ("f32", "x3"))
def test_resstride_mutant_is_caught_at_the_stride_cases(kind):
    for cin, cout in L.STRIDE_SHAPES[kind]:
        nw = L.x3_nw(cin, cout, BMAX) if kind == "x3" else None
        inp = L.lin_inputs(kind, L.CAUGHT_BY["resstride"], BMAX, cin, cout, 1)
        for name, _, dy, dr in L.STRIDES:
            if dr is not None and dr != dy:
                broke, _ = _caught(kind, inp, nw, "resstride", 0, True, True, ldr=cout + dr, ldy=cout + dy)
                assert broke, (kind, cin, cout, name)


@pytest.mark.parametrize("kind", ("f32", "x3"))
def test_bias0_mutant_is_caught_at_the_batched_cases(kind):
    for cin, cout in L.BATCH_SHAPES[kind]:
        for nb in L.BATCH_N:
            b = max(L.BATCH_B)
            nw = L.x3_nw(cin, cout, b, nb) if kind == "x3" else None
            inps = [L.lin_inputs(kind, L.CAUGHT_BY["bias0"], b, cin, cout, 10 + i) for i in range(nb)]
            args = ([i["x"] for i in inps], [i["w"] for i in inps], [i["bias"] for i in inps], [i["r"] for i in inps])
            good, mut = L.model_batched(kind, *args, 0, nw), L.model_batched(kind, *args, 0, nw, "bias0")
            for i, inp in enumerate(inps):
                exp = L.expected_exact(inp, True, True)
                assert torch.equal(L.bits(good[i]), L.bits(exp)), (kind, cin, cout, nb, i)
                assert i == 0 or not torch.equal(L.bits(mut[i]), L.bits(exp)), (kind, cin, cout, nb, i)


# ---------------------------------------------------------------------------------------------- the families
def test_integer_and_split_families_are_exact():
    """sum |terms| stays below 2^24 units of the smallest term, so every f32 partial sum in any order is exact, and
    the kernel's split reproduces the parts of the split family."""
    for kind in ("f32", "x3", "rw"):
        for cin, cout, _ in _shapes(kind):
            rows = max(L.RW_M) if kind == "rw" else BMAX
            inp = L.lin_inputs(kind, "integer", rows, cin, cout, 0)
            assert L.abs_term_sum(inp).max().item() < 2.0 ** 24, (kind, cin, cout)
            if kind == "x3":
                for t in (inp["x"], inp["w"]):
                    hi, lo = L.split_bf16(t)
                    assert torch.equal(hi, t) and not lo.any()
    for cin in L.X3_CIN:
        for cout in L.X3_COUT:
            inp = L.lin_inputs("x3", "split", BMAX, cin, cout, 0)
            for t, h, l in ((inp["x"], inp["xh"], inp["xl"]), (inp["w"], inp["wh"], inp["wl"])):
                hi, lo = L.split_bf16(t)
                assert torch.equal(hi, h) and torch.equal(lo, l) and bool(l.any())
            hh = inp["xh"].double().abs() @ inp["wh"].double().abs().t()
            assert hh.max().item() / 2.0 ** -10 < 2.0 ** 24 and L.abs_term_sum(inp).max().item() / 2.0 ** -10 < 2.0 ** 24
            # the expectation is the three-term sum, not x w: they differ by the lo lo term
            P, _ = L.products(inp["x"], inp["w"])
            three = L.expected_exact(inp, False, False).double()
            assert torch.equal(P - three, inp["xl"].double() @ inp["wl"].double().t()) and bool((P != three).any())


def test_onehot_family_covers_every_k_and_splits_exactly():
    for cin in L.X3_CIN:
        inp = L.lin_inputs("x3", "onehot", 1, cin, 32, 0)
        assert inp["rows"] == cin and torch.equal(inp["x"], torch.eye(cin))
        hi, lo = L.split_bf16(inp["w"])
        assert torch.equal((hi.double() + lo.double()).float(), inp["w"]) and torch.equal(hi.double() + lo.double(),
                                                                                          inp["w"].double())
        assert bool(lo.any())


def test_rowscale_rows_differ_by_a_factor_of_two():
    inp = L.lin_inputs("f32", "rowscale", 20, 128, 32, 0)
    g = L.lin_inputs("f32", "gauss", 20, 128, 32, 0)
    sc = 2.0 ** (torch.arange(20) % 9 - 4).float()[:, None]
    assert torch.equal(inp["x"], g["x"] * sc) and torch.equal(inp["r"], g["r"] * sc)


def test_routes_match_the_dispatch_code():
    assert [L.x3_route(c, L.x3_nw(c, 32, 70)) for c in L.X3_CIN] == [(4, 1, 1), (8, 1, 1), (4, 3, 3), (8, 2, 2),
                                                                     (4, 5, 2), (8, 6, 3)]
    assert L.x3_route(512, 4) == (4, 4, 1) and L.x3_nw(640, 32, 70, pin=8) == 4 and L.x3_nw(128, 32, 70, pin=8) == 4
    assert L.f32_route(16) == [1, 0, 0, 0, 0, 0, 0, 0] and L.f32_route(144) == [2, 2, 2, 2, 1, 0, 0, 0]
    assert L.f32_route(1552) == [13] * 7 + [6] and L.f32_route(768) == [6] * 8 and L.f32_route(128) == [1] * 8
    got = [(L.rw_route(n, k, 261, 256)["parts"], L.rw_route(n, k, 261, 256)["ct"]) for n, k in L.RW_NK]
    assert got == [(1, 1), (1, 2), (1, 3), (1, 1), (2, 3), (3, 3)]
    assert all(L.rw_route(n, k, m, 256)["tiles_per_wave"] == 1 for n, k in L.RW_NK for m in L.RW_M)
    m = L.rw_persistent_m(*L.RW_PERSISTENT, 256)
    rt = L.rw_route(*L.RW_PERSISTENT, m, 256)
    assert m == 2 * 680 * 32 + 3 * 32 + 5 and (rt["per_cu"], rt["grid_x"], rt["tiles_per_wave"]) == (1, 85, 3)
    assert rt["tiles"] > 2 * rt["grid_x"] * 8


def test_erf_as_is_within_its_stated_error():
    """common.h cites |erf error| <= 1.5e-7 for Abramowitz-Stegun 7.1.26: the restatement, evaluated in f64, holds it
    on a grid over [-8, 8].  The bound's GELU term counts that error alone; the roundings of an f32 evaluation
    (0.5 |z| times the erf error) must hide below the smallest pre-activation term 1.13 n 2^-24 S, n >= 25, S >= |z|:
    an f32 erf error below 2 * 1.13 * 25 * 2^-24."""
    x = torch.linspace(-8, 8, 320001, dtype=torch.float64)
    e64 = (L.erf_as(x) - torch.erf(x)).abs().max().item()
    e32 = (L.erf_as(x.float()).double() - torch.erf(x.float().double())).abs().max().item()
    print(json.dumps({"erf_as f64": e64, "erf_as f32": e32}))
    assert min(L.n_roundings("f32", 16), L.n_roundings("x3", 128, 4)) >= 25
    assert e64 <= 1.5e-7 and e32 <= 2 * 1.13 * 25 * L.U24


# ---------------------------------------------------------------------------------------------- x3 row kernels
@pytest.mark.parametrize("c", L.X3_EMBED_C)
def test_model_passes_x3_bert_embed_cases(c):
    b, l = L.X3_EMBED_BL[-1]
    for fam in R.FAMILIES:
        for eps in ((1e-12, 1e-5) if fam == "tinyvar" else (1e-12,)):
            k = L.x3_embed_case(fam, b, l, c, c + l, eps)
            y = R.model_f32(k["v32"], k["g"], k["b"], eps, out="f32")
            ra = L.measure(y, k["ref"], k["tol_f32"])
            assert ra <= R.MODEL_F32, (fam, c, eps, ra)
            if k["exact_beta"]:
                assert torch.equal(y, k["b"].expand(b * l, c))


def test_model_passes_x3_mean_rows_cases():
    worst = 0.0
    for c in L.X3_MEAN_C:
        for l in L.X3_MEAN_L:
            for b in L.X3_MEAN_B:
                for extra in (False, True):
                    for fam in ("gauss", "integer"):
                        k = L.x3_mean_case(fam, b, l, c, c + l, extra)
                        y = L.model_mean_rows(k["x"], k["extra"])
                        ra = L.measure(y, k["ref"], k["tol"])
                        worst = max(worst, ra)
                        assert ra <= L.MODEL_MEAN, (c, l, b, extra, fam, ra)
                        if k["exact"] is not None:
                            assert torch.equal(L.bits(y), L.bits(k["exact"]))
    print(json.dumps({"kernel": "x3_mean_rows", "worst": worst}))
