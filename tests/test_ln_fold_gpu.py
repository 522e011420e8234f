"""GPU: the LayerNorm-fold forms of the 8-phase GEMM (csrc/gemm.hip gemm_bf16_tn_p8<LNM, STO>: mmr_linear_bf16_ln) and
mmr_ln_row_coef against the exact expectations of tests/ln_fold_ref.py (module docstring there: the coefficient and vector
families, why each mode is exact, the statistics and coefficient bounds; test_ln_fold_cpu.py holds the model and the
mutants these checks are proved against).

test_case      every case of ln_fold_ref.CASES (NT = 3: n in {192, 576, 4416}; NT = 4: n in {256, 4352}; n = 768 where the
               launcher chooses by fill; (m, K) in {(256, 128), (768, 384), (4096, 128)}: one tile, nine tiles, 1-2 tiles per
               workgroup so both tile parities of the coefficient and vector slots carry different data) under every
               built combination: fold, fold + GELU, normalised residual with and without statistics, statistics with and
               without a residual.  The tile width is recovered from linear_ln_parts and asserted.  Outputs bit for bit
               (GELU: per-element bound), the statistics in a sentinel-filled buffer with guards: every slot written,
               part sums bit-equal to the f64 sum of the stored outputs, M2 within the derived bound.
test_unbuilt   the combinations that are not built are refused, output and statistics untouched.
test_row_coef  mmr_ln_row_coef per element against f64 on parts built by the test (nparts 4, 16, 36, 48; m 1, 7, 256; rows
               with |mean| ~ 1e3 spreads; constant rows; eps 1e-12 and 1e-5), and m = 0.
test_zz_report cases per combination, the worst gelu, M2 and coefficient ratios, the file's runtime.

Measured on an MI355X (256 CUs).  The file's 147 tests spend 0.3 s inside them (the slowest case 0.03 s; operands are hashed
on the device).  Every exact case came out bit for bit in all six combinations on both tile widths, every guard intact, every
statistics slot written once, every part sum bit-equal to the f64 sum; no defect was found in gemm.hip.  Cases per combination:
fold 18, fold + GELU 18, normalised residual 12, with statistics 12, statistics 18, statistics + residual 18, row_coef 48.
Worst gelu error / bound 0.969 (the CPU model: 0.969); worst M2 error / bound 0.050 (the CPU model's f32 restatement: 0.041);
worst coefficient error / bound 0.107 (the CPU model: 0.089)."""
import collections
import json
import time

import pytest
import torch

import gemm_routes_ref as G
import ln_fold_ref as L
from mmr_amd import _lib, ops
from test_gemm_routes_gpu import DEV, _cus, _sync

pytestmark = pytest.mark.gpu
_SHAPES = collections.OrderedDict()
_STATS = {"t0": None, "cases": collections.Counter(), "gelu": 0.0, "m2": 0.0, "coef": 0.0, "slowest": (0.0, "")}


@pytest.fixture(scope="module", autouse=True)
def _clock():
    _STATS["t0"] = time.perf_counter()
    yield
    _SHAPES.clear()


def _shape(c, act):
    key = (c, act)
    if key not in _SHAPES:
        while len(_SHAPES) >= 2:
            _SHAPES.popitem(last=False)
        d = G.data(G.family_of(act), c.m, c.n, c.k, device=DEV)
        e = L.extras(c, act, device=DEV)
        _SHAPES[key] = {"x": G.to_bf16(d["x"]), "w": G.to_bf16(d["w"]), "b": d["b"], "r": G.to_bf16(d["r"]),
                        "acc": d["x"].double() @ d["w"].double().t(), "e": e}
    return _SHAPES[key]


def _buffers(m, n, parts):
    buf = torch.full((m + 2 * L.GUARD, n), L.SENT, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    sbuf = torch.full((m * parts * 2 + 2 * L.GUARD_ST,), L.SENT_F, device=DEV)
    return buf, buf[L.GUARD:L.GUARD + m], sbuf, sbuf[L.GUARD_ST:L.GUARD_ST + m * parts * 2]


def _call(s, y, m, n, k, mode, act, hr, st):
    e, p = s["e"], _lib.ptr
    v1 = e["c"] if mode == 1 else (e["gamma"] if mode == 2 else None)
    return _lib.lib().mmr_linear_bf16_ln(p(s["x"]), p(s["w"]), p(s["b"]), p(s["r"] if hr else None), p(y), m, n, k, act, mode,
                                         p(e["coef"] if mode else None), p(v1), p(e["beta"] if mode == 2 else None), p(st),
                                         _lib.stream_ptr(s["x"].device))


_FORMS = sorted(((ci, co) for ci in range(len(L.CASES)) for co in L.COMBOS if L.built(L.CASES[ci], co[1])),
                key=lambda f: (f[0], f[1][2]))


@pytest.mark.parametrize("ci,combo", _FORMS, ids=[f"{L.case_id(L.CASES[ci])}-{co[0]}" for ci, co in _FORMS])
def test_case(ci, combo):
    if _cus() != G.CUS:
        pytest.skip(f"the case table is derived for {G.CUS} CUs, this device has {_cus()}")
    t0 = time.perf_counter()
    c = L.CASES[ci]
    name, mode, act, hr, so = combo
    nt = L.nt_of(c, mode)
    parts = ops.linear_ln_parts(c.m, c.n, mode)
    assert parts == 4 * c.n // (64 * nt), f"tile width: {parts} parts for n = {c.n}, expected NT = {nt}"
    s = _shape(c, act)
    buf, y, sbuf, st = _buffers(c.m, c.n, parts)
    assert _call(s, y, c.m, c.n, c.k, mode, act, hr, st if so else None) == 0, _lib.lib().mmr_last_error()
    _sync()
    got, e = buf.view(torch.int16), s["e"]
    r = s["r"].float() if hr else None
    if act:
        z = L.exact_f64(mode, s["acc"], s["b"], r, e)
        assert z.abs().max().item() <= G.ZMAX
        ref, tol = G.gelu_ref_tol(z, None, "round1")
        res = G.verify_gelu(got, c.m, ref, tol)
        _STATS["gelu"] = max(_STATS["gelu"], res[2])
    else:
        res = G.verify_exact(got, c.m, G.rne_bits(L.pre_f32(mode, s["acc"], s["b"], r, e)))
    rs = L.verify_stats(sbuf, got[L.GUARD:L.GUARD + c.m], nt) if so else None
    if so:
        _STATS["m2"] = max(_STATS["m2"], rs[3])
    else:
        assert bool((sbuf == L.SENT_F).all())
    dt = time.perf_counter() - t0
    _STATS["cases"][name] += 1
    _STATS["slowest"] = max(_STATS["slowest"], (dt, f"{L.case_id(c)}-{name}"))
    print(f"{L.case_id(c)} {name}: NT {nt}, (guards, sentinels, {'err / tol' if act else '!= expected'}) {res}, statistics "
          f"(guards, unwritten, sums != f64, worst M2 err / tol) {rs}, {dt:.2f} s")
    assert res[0] and res[1] == 0 and G.passes(res), res
    assert rs is None or L.stats_pass(rs), rs


def test_unbuilt():
    c = L.CASES[0]
    s = _shape(c, 0)
    c4 = next(k for k in L.CASES if k.n == 256 and k.m == 256)
    s4 = _shape(c4, 0)
    for cc, ss, combos in ((c, s, L.UNBUILT), (c4, s4, ((2, 0, True, False), (2, 0, True, True)))):   # ln_mode 2: n % 192
        buf, y, sbuf, st = _buffers(cc.m, cc.n, 4 * cc.n // (64 * cc.nt))
        for mode, act, hr, so in combos:
            assert _call(ss, y, cc.m, cc.n, cc.k, mode, act, hr, st if so else None) != 0, (mode, act, hr, so)
            _sync()
            assert _lib.lib().mmr_last_error()
            assert bool((buf.view(torch.int16) == L.SENT).all()) and bool((sbuf == L.SENT_F).all()), (mode, act, hr, so)
    buf, y, sbuf, st = _buffers(c.m, c.n, 4)
    for m, n, k in ((128, c.n, c.k), (c.m, 200, c.k), (c.m, c.n, 64)):                              # m % 256, n, k % 128
        assert _call(s, y, m, n, k, 0, 0, False, st) != 0
    e = dict(s["e"])
    for hole in ("coef", "c"):                                                                        # the fold's inputs
        s2 = dict(s, e=dict(e, **{hole: None}))
        assert _call(s2, y, c.m, c.n, c.k, 1, 0, False, None) != 0
    _sync()
    assert bool((buf.view(torch.int16) == L.SENT).all()) and bool((sbuf == L.SENT_F).all())


@pytest.mark.parametrize("m,nparts,fam,eps", L.COEF_CASES, ids=[f"{m}-{p}-{f}-{e:g}" for m, p, f, e in L.COEF_CASES])
def test_row_coef(m, nparts, fam, eps):
    st, y = L.coef_parts(m, nparts, fam)
    n = y.shape[1]
    ref, tol = L.coef_ref_tol(st, n, eps)
    out = torch.full((m + 2, 2), L.SENT_F, device=DEV)
    std = st.to(DEV)
    assert _lib.lib().mmr_ln_row_coef(_lib.ptr(std), m, nparts, n, eps, _lib.ptr(out[1:m + 1]), _lib.stream_ptr(std.device)) == 0
    _sync()
    out = out.cpu()
    assert bool((out[0] == L.SENT_F).all() and (out[m + 1] == L.SENT_F).all())
    ratio = ((out[1:m + 1].double() - ref).abs() / tol).max().item()
    _STATS["coef"] = max(_STATS["coef"], ratio)
    _STATS["cases"]["row_coef"] += 1
    print(f"ln_row_coef m {m} parts {nparts} {fam} eps {eps:g}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


def test_row_coef_m0():
    st = torch.zeros(1, 4, 2, device=DEV)
    out = torch.full((2, 2), L.SENT_F, device=DEV)
    assert _lib.lib().mmr_ln_row_coef(_lib.ptr(st), 0, 4, 192, 1e-5, _lib.ptr(out), _lib.stream_ptr(st.device)) == 0
    _sync()
    assert bool((out == L.SENT_F).all())


def test_zz_report():
    print(json.dumps({"cases_per_combination": dict(_STATS["cases"]), "worst_gelu_err_over_tol": round(_STATS["gelu"], 4),
                      "worst_m2_err_over_tol": round(_STATS["m2"], 4), "worst_coef_err_over_tol": round(_STATS["coef"], 4),
                      "runtime_s": round(time.perf_counter() - _STATS["t0"], 1),
                      "slowest": (round(_STATS["slowest"][0], 2), _STATS["slowest"][1])}))
