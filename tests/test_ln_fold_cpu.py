"""CPU: the data, the kernel model, the statistics order and the mutants that test_ln_fold_gpu.py holds
mmr_linear_bf16_ln and mmr_ln_row_coef to (tests/ln_fold_ref.py).
  data           the coefficient, vector and operand families are what the docstring says; every f32 operation of the
                 three modes is exact on them (equal to the f64 value); rows' coefficients are distinct.
  model, mutants the model passes every check on every case and built combination (on the case cut to two row panels
                 and two tile columns); wherever a mutant changes the model's output or statistics the checks fail; every
                 mutant is caught.
  statistics     the f32 restatement of the kernel's order: part sums bit-equal to the f64 sum, worst M2 error / bound
                 printed.
  coefficients   the f32 restatement of ln_row_coef within the derived bound on every case; worst ratio printed.
Each printed line records the worst ratio to each derived bound."""
import functools

import pytest
import torch

import gemm_routes_ref as G
import ln_fold_ref as L


def test_tile_width_rule():
    for c in L.CASES:
        assert L.ln_nt(c.m, c.n) == c.nt, L.case_id(c)
    assert L.ln_nt(256, 768) == 3 and L.ln_nt(4096, 768) == 3      # 4 > 3 tiles of 256 CUs; 64 > 48
    assert L.ln_nt(32768, 768) == 3 and L.ln_nt(32768, 3072) == 4 and L.ln_nt(256, 200) == 0
    assert {c.nt for c in L.CASES} == {3, 4}


def _operands(c, act, rows, cols):
    d = G.data(G.family_of(act), c.m, c.n, c.k, rows=rows, cols=cols)
    return d, L.extras(c, act, rows, cols)


@pytest.mark.parametrize("c", L.CASES[:6], ids=[L.case_id(c) for c in L.CASES[:6]])
def test_families_exact(c):
    rows, cols = L.cut(c)
    d, e = _operands(c, 0, rows, cols)
    ra, rb = e["coef"][:, 0], e["coef"][:, 1]
    assert set(ra.tolist()) <= {0.25, 0.5, 1.0, 2.0} and len(set(ra.tolist())) == 4
    assert rb.abs().max() <= 4 and torch.equal(rb * 4, (rb * 4).round())
    assert e["c"].abs().max() == 8 and set(e["gamma"].tolist()) == {0.5, 1.0, 2.0}
    assert torch.equal(e["beta"] * 4, (e["beta"] * 4).round())
    pair = e["coef"][:, 0] * 100 + e["coef"][:, 1]
    assert (pair[:128] != pair[128:256]).double().mean() > 0.9                 # the two halves differ
    if rows > 256:
        assert (pair[:256] != pair[256:512]).double().mean() > 0.9             # and the next tile's rows
    acc = G.preact(d["x"], d["w"])
    for mode, r in ((0, None), (0, d["r"]), (1, None), (2, d["r"])):
        v = L.pre_f32(mode, acc, d["b"], r, e)
        assert torch.equal(v.double(), L.exact_f64(mode, acc, d["b"], r, e)), mode
        assert (G.bf2f(G.rne_bits(v)) != v).double().mean() > 0.1, mode          # rounding is exercised (K = 128: |acc| ~ 60)
    dg, eg = _operands(c, 1, rows, cols)
    z = L.exact_f64(1, G.preact(dg["x"], dg["w"]), dg["b"], None, eg)
    assert z.abs().max() <= G.ZMAX and torch.equal(z * 8, (z * 8).round())


@functools.lru_cache(maxsize=None)
def _run_case(ci):
    c = L.CASES[ci]
    rows, cols = L.cut(c)
    bad, escaped, caught, worst_g, worst_m2 = [], [], set(), 0.0, 0.0
    for name, mode, act, hr, so in L.COMBOS:
        if not L.built(c, mode):
            continue
        d, e = _operands(c, act, rows, cols)
        r = d["r"] if hr else None
        nt = L.nt_of(c, mode)
        acc = G.preact(d["x"], d["w"])
        if act:
            ref, tol = G.gelu_ref_tol(L.exact_f64(mode, acc, d["b"], r, e), None, "round1")
            chk = (lambda buf: G.verify_gelu(buf, rows, ref, tol))
        else:
            exp = G.rne_bits(L.pre_f32(mode, acc, d["b"], r, e))
            chk = (lambda buf: G.verify_exact(buf, rows, exp))

        def ok(bufs):
            res = chk(bufs[0])
            if not so:
                return G.passes(res), res, None
            rs = L.verify_stats(bufs[1], bufs[0][L.GUARD:L.GUARD + rows], nt)
            return G.passes(res) and L.stats_pass(rs), res, rs

        base = L.model(c, mode, act, d["x"], d["w"], d["b"], r, e, so)
        good, res, rs = ok(base)
        if not good:
            bad.append((name, res, rs))
        if act:
            worst_g = max(worst_g, res[2])
        if so:
            worst_m2 = max(worst_m2, rs[3])
        for mu in L.MUTANTS:
            mb = L.model(c, mode, act, d["x"], d["w"], d["b"], r, e, so, mutant=mu)
            if torch.equal(mb[0], base[0]) and (not so or torch.equal(mb[1], base[1])):
                continue
            if ok(mb)[0]:
                escaped.append((name, mu))
            else:
                caught.add(mu)
    return bad, escaped, caught, worst_g, worst_m2


@pytest.mark.parametrize("ci", range(len(L.CASES)), ids=[L.case_id(c) for c in L.CASES])
def test_model_and_mutants(ci):
    bad, escaped, caught, worst_g, worst_m2 = _run_case(ci)
    print(f"{L.case_id(L.CASES[ci])}: model gelu error / bound {worst_g:.3f}, M2 error / bound {worst_m2:.3f}, "
          f"mutants caught {sorted(caught)}")
    assert not bad, bad
    assert not escaped, escaped
    assert worst_g <= 1.0 and worst_m2 <= 1.0


def test_every_mutant_caught():
    caught = set().union(*(_run_case(ci)[2] for ci in range(len(L.CASES))))
    assert caught == set(L.MUTANTS), set(L.MUTANTS) - caught


def test_constant_part_floor():
    """A constant part (M2_ref = 0) with a mean that 1 / 48 does not divide exactly stays inside the absolute floor."""
    y = torch.full((16, 96), 193.0)
    y[:, 48:] = torch.arange(16)[:, None] * 3.0 + 0.25
    st = L.model_stats(y, 3)
    s, m2, mean = L.stats_ref(G.rne_bits(y), 3)
    assert torch.equal(st[..., 0].double(), s)
    ratio = ((st[..., 1].double() - m2).abs() / L.m2_tol(m2, mean, 3).clamp(min=1e-300))
    print(f"constant parts: worst M2 / floor {ratio.max().item():.3f}")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("m,nparts,fam,eps", L.COEF_CASES, ids=[f"{m}-{p}-{f}-{e:g}" for m, p, f, e in L.COEF_CASES])
def test_coef_model_within_bound(m, nparts, fam, eps):
    st, y = L.coef_parts(m, nparts, fam)
    n = y.shape[1]
    ref, tol = L.coef_ref_tol(st, n, eps)
    mean, var = y.mean(1), y.var(1, unbiased=False)
    direct = torch.stack([1 / torch.sqrt(var + eps), -mean / torch.sqrt(var + eps)], 1)
    assert torch.allclose(ref, direct, rtol=1e-5, atol=1e-9)          # Chan's merge of the f32 parts is the row's LayerNorm
    got = L.model_coef(st, n, eps).double()
    ratio = ((got - ref).abs() / tol).max().item()
    print(f"ln_row_coef model m {m} parts {nparts} {fam} eps {eps:g}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0
