"""GPU: mmr_linear_bf16 on every one of its 11 routes (csrc/gemm.hip), pinned variant by variant, against the exact
expectations of tests/gemm_routes_ref.py (module docstring there: routes, data families, residual rounding models,
the gelu bound; test_gemm_routes_cpu.py holds the models and mutants these checks are proved against).

test_route_case  every case of gemm_routes_ref.CASES (the smallest shape that reaches each route for 256 CUs, and the
                 route's M / N / K tails, shifted tiles, one-tile and multi-tile persistent walks) under six
                 epilogues: none, bias, bias + GELU, bias + residual, bias + GELU + residual, bias + residual in
                 place.  The variant is pinned (ops.pinned), ops.linear_route must name the intended route on this
                 device, and the output is the middle M rows of an (M + 2 GUARD, N) buffer pre-filled with a bf16
                 NaN pattern.  Raw 16-bit views: exact family bit for bit under the route's rounding model (round2
                 on the LDS-staged base / big kernels, round1 on the 8-phase kernel), gelu family within the
                 per-element bound, guard rows untouched, no sentinel left inside.  The exact pre-activation of a
                 shape is computed once in f64 on the CPU and shared by its epilogues.
test_tuner       an unpinned call on a fresh shape: exact result, a variant in range reported, and the untuned
                 in-place call (out = residual) exact under variant 0's route.
test_refusals    K or N not a multiple of 8, act = 2, NULL operands: refused, the sentinel-filled output untouched.
test_zz_report   cases per route, the largest gelu error / bound per route, the file's runtime.

Measured on an MI355X (256 CUs).  The file runs in 4.8 s (219 tests, 2.6 s inside them; the slowest is the first,
0.6 s with the library's start-up; an 8192 x 4096 case takes 0.08 s).  Every exact-family case came out bit for bit
on all 11 routes and epilogues, every guard row intact, no sentinel left inside; no defect was found in gemm.hip.
Cases run per route: base 45, w4 256x256 9, w4 256x192 9, big 256x256 KB64x2 27, KB32x4 18, big 256x192 12, big
256x128 KB32x2 18, KB32x3 18, KB64x3 24, 8-phase 256x256 18, 256x192 18.  Largest gelu error / bound: 0.969 without a
residual (the same on every route: z takes the same multiples of 1/8 in every case, and the worst one is a value
that lands next to a bf16 tie), 0.996 with one on the round2 routes, 0.993 on the 8-phase routes.  The tuner settled
on variant 4 (the base kernel) for TUNER_SHAPE."""
import collections
import json
import time

import pytest
import torch

import gemm_routes_ref as G
from mmr_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ORDER = sorted(range(len(G.CASES)), key=lambda i: (G.CASES[i].m, G.CASES[i].n, G.CASES[i].k))   # shapes adjacent
_SHAPES = collections.OrderedDict()      # (m, n, k, family) -> operands and exact pre-activation; the last two kept
_STATS = {"t0": None, "cases": collections.Counter(), "gelu": {}, "slowest": (0.0, "")}


@pytest.fixture(scope="module", autouse=True)
def _clock():
    _STATS["t0"] = time.perf_counter()
    yield
    _SHAPES.clear()


def _shape(m, n, k, fam):
    """x, w (bf16, device), b (f32, device), acc = x w^T exact (f64 on the CPU, then on the device) and the residual
    (made on first use), once per shape and family."""
    key = (m, n, k, fam)
    if key not in _SHAPES:
        while len(_SHAPES) >= 2:
            _SHAPES.popitem(last=False)
        d = G.data(fam, m, n, k, parts="xwb")
        _SHAPES[key] = {"x": G.to_bf16(d["x"]).to(DEV), "w": G.to_bf16(d["w"]).to(DEV), "b": d["b"].to(DEV),
                        "acc": G.preact(d["x"], d["w"]).to(DEV)}
    s = _SHAPES[key]
    s["r"] = s.get("r")
    return s


def _residual(s, m, n, k, fam):
    if s["r"] is None:
        s["r"] = G.to_bf16(G.data(fam, m, n, k, device=DEV, parts="r")["r"])
    return s["r"]


def _buffer(m, n):
    """(buf, out): the sentinel-filled (m + 2 GUARD, n) bf16 buffer and its middle m rows."""
    buf = torch.full((m + 2 * G.GUARD, n), G.SENT, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    return buf, buf[G.GUARD:G.GUARD + m]


def _sync():
    """Wait for the launch; a device error ends the session, so that nothing more starts on a faulted GPU."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, nothing more is launched: {e}", returncode=3)


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@pytest.mark.parametrize("epi", G.EPILOGUES, ids=[e[0] for e in G.EPILOGUES])
@pytest.mark.parametrize("ci", ORDER, ids=[G.case_id(G.CASES[i]) for i in ORDER])
def test_route_case(ci, epi):
    if _cus() != G.CUS:
        pytest.skip(f"the case table is derived for {G.CUS} CUs, this device has {_cus()}")
    t0 = time.perf_counter()
    c = G.CASES[ci]
    name, act, hb, hr, inplace = epi
    fam, route = G.family_of(act), G.route_of(c, hr)
    s = _shape(c.m, c.n, c.k, fam)
    b = s["b"] if hb else None
    r = _residual(s, c.m, c.n, c.k, fam) if hr else None
    buf, out = _buffer(c.m, c.n)
    if inplace:
        out.copy_(r)
    with ops.pinned(ops.PIN_GEMM_BF16, c.variant):
        got_route = ops.linear_route(c.m, c.n, c.k, hr, c.variant)
        assert got_route == G.RID[route], (G.ROUTES[got_route], route)
        ops.linear(s["x"], s["w"], b, out if inplace else r, act=act, out=out)
    _sync()
    got = buf.view(torch.int16)
    rf = r.float() if hr else None
    if act:
        z = s["acc"] + b.double() if hb else s["acc"]
        assert z.abs().max().item() <= G.ZMAX
        ref, tol = G.gelu_ref_tol(z, rf, G.RES_MODEL[route])
        res = G.verify_gelu(got, c.m, ref, tol)
        _STATS["gelu"][route] = max(_STATS["gelu"].get(route, 0.0), res[2])
    else:
        res = G.verify_exact(got, c.m, G.expected_exact(s["acc"], b, rf, G.RES_MODEL[route]))
    dt = time.perf_counter() - t0
    print(f"{G.case_id(c)} {name} -> {route}: guards intact {res[0]}, sentinels inside {res[1]}, "
          f"{'worst err / tol' if act else 'elements != expected'} {res[2]}, {dt:.2f} s")
    _STATS["cases"][route] += 1
    _STATS["slowest"] = max(_STATS["slowest"], (dt, f"{G.case_id(c)}-{name}"))
    assert res[0], "guard rows written"
    assert res[1] == 0, f"{res[1]} elements never written"
    assert G.passes(res), res


def test_tuner():
    if _cus() != G.CUS:
        pytest.skip(f"the case table is derived for {G.CUS} CUs, this device has {_cus()}")
    m, n, k = G.TUNER_SHAPE
    L = _lib.lib()
    s = _shape(m, n, k, "exact")
    assert L.mmr_linear_bf16_variant(m, n, k, 0, 1, 0) == -1, "not a fresh shape: another test tuned it"
    buf, out = _buffer(m, n)
    ops.linear(s["x"], s["w"], s["b"], None, act=0, out=out)
    _sync()
    v = L.mmr_linear_bf16_variant(m, n, k, 0, 1, 0)
    assert 0 <= v < G.N_VARIANTS
    route = G.ROUTES[ops.linear_route(m, n, k, False, v)]
    res = G.verify_exact(buf.view(torch.int16), m, G.expected_exact(s["acc"], s["b"], None, G.RES_MODEL[route]))
    print(f"tuner: variant {v} -> {route}: {res}")
    assert G.passes(res), res
    # out aliases the residual: no tuning (the timing launches would add it again and again), variant 0's route
    r = _residual(s, m, n, k, "exact")
    buf, out = _buffer(m, n)
    out.copy_(r)
    ops.linear(s["x"], s["w"], s["b"], out, act=0, out=out)
    _sync()
    assert L.mmr_linear_bf16_variant(m, n, k, 0, 1, 1) == -1
    route = G.ROUTES[ops.linear_route(m, n, k, True, 0)]
    res = G.verify_exact(buf.view(torch.int16), m, G.expected_exact(s["acc"], s["b"], r.float(), G.RES_MODEL[route]))
    print(f"untuned in place: variant 0 -> {route}: {res}")
    assert G.passes(res), res


def test_refusals():
    m, n, k = 16, 16, 16
    x = torch.ones(m, 2 * k, dtype=torch.bfloat16, device=DEV)
    w = torch.ones(n + 8, 2 * k, dtype=torch.bfloat16, device=DEV)
    buf, out = _buffer(m, n + 8)
    L = _lib.lib()

    def refused(xp, wp, yp, n_, k_, act):
        st = L.mmr_linear_bf16(_lib.ptr(xp), _lib.ptr(wp), None, None, _lib.ptr(yp), m, n_, k_, act, _lib.stream_ptr(x.device))
        _sync()
        assert st != 0 and L.mmr_last_error()
        assert bool((buf.view(torch.int16) == G.SENT).all()), "a refused call wrote its output"

    refused(x, w, out, n, k + 4, 0)        # K % 8
    refused(x, w, out, n + 4, k, 0)        # N % 8
    refused(x, w, out, n, k, 2)            # act
    refused(None, w, out, n, k, 0)
    refused(x, None, out, n, k, 0)
    refused(x, w, None, n, k, 0)
    with pytest.raises(_lib.MMRError):
        ops.linear(x[:, :k + 4], w[:n, :k + 4], act=0, out=out)


def test_zz_report():
    """Cases run per route, the largest gelu error / bound per route and the file's runtime, for the record."""
    print(json.dumps({"cases_per_route": dict(_STATS["cases"]),
                      "worst_gelu_err_over_tol": {k: round(v, 4) for k, v in _STATS["gelu"].items()},
                      "runtime_s": round(time.perf_counter() - _STATS["t0"], 1),
                      "slowest": (round(_STATS["slowest"][0], 2), _STATS["slowest"][1])}))
