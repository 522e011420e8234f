"""CPU: the route table, the kernel models and the bounds that test_gemm_routes_gpu.py holds mmr_linear_bf16 to
(tests/gemm_routes_ref.py).
  route table    mmr_linear_bf16_route with cus = 256 (no GPU needed) gives every case's intended route, without and
                 with a residual; the table reaches all 11 routes; the binding's names are the header's.
  model, mutants the model of each route passes the checks on every case and epilogue (exact family bit for bit, gelu
                 family within the bound, guard rows intact) on the case data cut to gemm_routes_ref.cut; wherever a
                 mutant changes the model's output at all the checks fail, and every mutant is caught on every route
                 it applies to.
  rounding       round1 and round2 differ in >= 0.1 % of the elements of every residual case of the exact family.
  GELU           the fit error of gelu_fast / gelu_fast2 and the f32-evaluation slack, measured."""
import functools
import os
import re
import subprocess

import pytest
import torch

import __graft_entry__ as ge
import gemm_routes_ref as G


@pytest.fixture(scope="module")
def ops():
    if not os.path.exists(os.path.join(ge.PKG, "libmmr.so")):
        subprocess.run(["make", "-j8"], cwd=os.path.join(ge.PKG, "csrc"), check=True)
    from mmr_amd import ops
    return ops


def test_route_names(ops):
    assert ops.GEMM_ROUTES == G.ROUTES
    txt = open(os.path.join(ge.ROOT, "include", "mmr.h")).read()
    ids = {n.lower(): int(v) for n, v in re.findall(r"MMR_GEMM_ROUTE_(\w+) = (\d+)", txt)}
    assert ids == G.RID
    assert int(re.search(r"MMR_GEMM_N_ROUTES = (\d+)", txt).group(1)) == len(G.ROUTES) == 11
    from mmr_amd import _lib
    assert _lib.lib().mmr_linear_bf16_n_variants() == G.N_VARIANTS


def test_route_table(ops):
    for c in G.CASES:
        for res in (False, True):
            got = ops.linear_route(c.m, c.n, c.k, res, c.variant, G.CUS)
            assert got == G.RID[G.route_of(c, res)], (G.case_id(c), res, G.ROUTES[got] if got >= 0 else got)
    assert {c.route for c in G.CASES} == set(G.ROUTES)
    # the w4 kernels take no residual: no variant reaches them with one
    for c in G.CASES:
        for v in range(G.N_VARIANTS):
            assert not G.ROUTES[ops.linear_route(c.m, c.n, c.k, True, v, G.CUS)].startswith("w4")
    # the tuner test's shape: variant 0 with a residual (the untuned in-place call) is the base kernel
    assert ops.linear_route(*G.TUNER_SHAPE, True, 0, G.CUS) == G.RID["base_128x128"]
    # what mmr_linear_bf16 refuses, and variants outside the table
    for m, n, k, v in ((0, 8, 8, 0), (-1, 8, 8, 0), (4, 12, 8, 0), (4, 8, 12, 0), (4, 0, 8, 0), (4, 8, 0, 0),
                       (4, 8, 8, -1), (4, 8, 8, G.N_VARIANTS)):
        assert ops.linear_route(m, n, k, False, v, G.CUS) == -1


def test_table_has_the_edges():
    """K, M and N tails on every route that admits them (the base and big kernels; N tails: the base kernel alone),
    a shifted last row tile on both w4 routes, one-tile and multi-tile walks on both 8-phase routes."""
    for r in G.ROUTES:
        tm, tn, kb = G.TILE[r]
        mine = [c for c in G.CASES if c.route == r]
        if r.startswith(("base", "big")):
            assert any(c.k % kb for c in mine) and any(c.m % tm for c in mine), r
        if r.startswith("base"):
            assert any(c.n % tn for c in mine) and any(c.m == 1 for c in mine) and any(c.k == 8 for c in mine)
        if r.startswith("w4"):
            assert any(c.m % 256 for c in mine), r
        if r.startswith("p8"):
            tiles = sorted((c.m // tm) * (c.n // tn) for c in mine)
            assert tiles[0] == 1 and tiles[1] % 8 != 0 and tiles[-1] > G.CUS, r


def test_exact_family_is_exact():
    for c in G.CASES:
        assert G.abs_term_bound(c.k) < 2 ** 24
    d = G.data("exact", 300, 200, 72)
    assert d["x"].abs().max() == 4 and d["w"].abs().max() == 4 and d["b"].abs().max() == 8 and d["r"].abs().max() == 64
    assert torch.equal(d["b"] * 4, (d["b"] * 4).round()) and torch.equal(d["r"], d["r"].round())
    assert G.data("exact", 8, 8, 8)["x"].abs().max() == 32
    for t in d.values():                                           # bf16 operands hold the values exactly
        G.to_bf16(t) if t.dim() == 2 else None
    # a cut is a slice of the full case
    full, part = G.data("gelu", 300, 200, 72), G.data("gelu", 300, 200, 72, rows=17, cols=40)
    assert torch.equal(full["x"][:17], part["x"]) and torch.equal(full["w"][:40], part["w"])
    assert torch.equal(full["r"][:17, :40], part["r"]) and torch.equal(full["b"][:40], part["b"])
    # rne_bits is torch's own conversion on finite values, ties included
    v = torch.cat([torch.randn(4096, generator=torch.Generator().manual_seed(3)) * 300,
                   torch.tensor([257.0, 259.0, -257.0, -259.0, 1.00390625, 0.0, -0.0])])
    assert torch.equal(G.rne_bits(v), G.bits(v.to(torch.bfloat16)))
    assert torch.equal(G.half_ulp(torch.tensor([1.0, 1.99, 2.0, 0.75, 300.0])).float(),
                       torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 1.0]))


@functools.lru_cache(maxsize=None)
def _run_case(ci):
    """Model and mutants over one case's epilogues: (failures of the unmutated model, mutants that changed the output
    and passed, {(mutant, route)} caught, worst gelu ratio of the model)."""
    c = G.CASES[ci]
    bad, escaped, caught, worst = [], [], set(), 0.0
    for name, act, hb, hr, inplace in G.EPILOGUES:
        fam, route = G.family_of(act), G.route_of(c, hr)
        rows, cols = G.cut(c, hr)
        d = G.data(fam, c.m, c.n, c.k, rows=rows, cols=cols)
        x, w, b, r = d["x"], d["w"], (d["b"] if hb else None), (d["r"] if hr else None)
        acc = G.preact(x, w)
        if act:
            z = acc + b.double() if hb else acc
            assert z.abs().max() <= G.ZMAX
            ref, tol = G.gelu_ref_tol(z, r, G.RES_MODEL[route])
            check = (lambda buf: G.verify_gelu(buf, rows, ref, tol))
        else:
            exp = G.expected_exact(acc, b, r, G.RES_MODEL[route])
            check = (lambda buf: G.verify_exact(buf, rows, exp))
        base = G.model(route, x, w, b, r, act, inplace=inplace)
        res = check(base)
        if not G.passes(res):
            bad.append((name, res))
        if act:
            worst = max(worst, res[2])
        for mu in G.MUTANTS:
            if mu == "round" and act:
                continue          # both models lie inside the gelu bound of either; the exact family tells them apart
            buf = G.model(route, x, w, b, r, act, mutant=mu, inplace=inplace)
            if torch.equal(buf, base):
                continue          # not a mutant on this case and epilogue
            if G.passes(check(buf)):
                escaped.append((name, mu))
            else:
                caught.add((mu, route))
    return bad, escaped, caught, worst


@pytest.mark.parametrize("ci", range(len(G.CASES)), ids=[G.case_id(c) for c in G.CASES])
def test_model_and_mutants(ci):
    bad, escaped, _, worst = _run_case(ci)
    assert not bad, bad
    assert not escaped, escaped
    assert worst <= 1.0


def test_every_mutant_caught_on_every_route():
    caught = set().union(*(_run_case(ci)[2] for ci in range(len(G.CASES))))
    missing = [(mu, r) for mu in G.MUTANTS for r in G.MUTANT_ROUTES[mu] if (mu, r) not in caught]
    assert not missing, missing


def test_rounding_models_differ():
    """Every residual case of the exact family tells round1 from round2: >= 0.1 % of the elements differ (and at
    least one)."""
    for c in G.CASES:
        rows, cols = G.cut(c, True)
        d = G.data("exact", c.m, c.n, c.k, rows=rows, cols=cols)
        acc = G.preact(d["x"], d["w"])
        diff = (G.expected_exact(acc, d["b"], d["r"], "round1") != G.expected_exact(acc, d["b"], d["r"], "round2"))
        assert diff.sum() >= 1 and diff.double().mean() >= 1e-3, (G.case_id(c), diff.double().mean().item())


def test_gelu_fit_and_slack():
    slack = 0.0
    for form in ("fast", "fast2"):
        err, z = G.measure_fit(form)
        print(f"gelu_{form}: fit error {err:.4e} at z = {z:.3f}")
        assert 1.19e-5 <= err <= G.FIT and 3.85 <= abs(z) <= 3.91
        s, zs = G.measure_slack(form)
        print(f"gelu_{form}: f32 evaluation {s:.4e} at z = {zs:.3f}")
        slack = max(slack, s)
    assert 2 * slack <= G.SLACK <= 2.05 * slack            # SLACK is twice the measured maximum, rounded up
