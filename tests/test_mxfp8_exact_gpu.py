"""GPU: the MX-fp8 forms of the 8-phase GEMM (csrc/gemm.hip gemm_bf16_tn_p8<FP8>: mmr_linear_mxfp8 with weight layouts 1
and 2, mmr_linear_mxfp8_q8) and mmr_quantize_mxfp8's edges, against the exact expectations of tests/mxfp8_exact_ref.py
(module docstring there: how the operands are built without the quantiser, the data families and why each is exact;
test_mxfp8_exact_cpu.py holds the model and the mutants these checks are proved against).

test_case        every case of mxfp8_exact_ref.CASES (for 256 CUs: one tile, nine tiles with uneven XCD shares, 1-2 tiles
                 per workgroup, zero-padded tail blocks; the first four carry rows and columns with exponents -100 / +100)
                 under six bf16-out epilogues on both layouts and three OUT8 epilogues on layout 2.  The output is the
                 middle of sentinel-filled buffers with guards (OUT8: bytes and scale image).  Exact and out8 families
                 bit for bit in every element (OUT8 against oracle.mxfp8.quantize of bf16_rn of the exact pre-activation),
                 GELU within gemm_routes_ref.gelu_ref_tol, OUT8 + GELU by the boundary-aware check on the exact z.
test_big_*       outputs above 128 MiB (non-temporal stores): >= 32 whole tiles bit for bit (first, last, every share's
                 ends, second tiles of a workgroup, every residue mod 8), guards and sentinels over the whole buffer.
test_quantiser   mmr_quantize_mxfp8 through the C entry: k % 32 != 0, kp beyond the next multiple of 256, threshold
                 mantissa and its bf16 neighbours, bf16 subnormals, the largest finite bf16, -0.0, e4m3 ties: bytes and
                 scale bytes equal oracle.mxfp8, padding zero, guards intact.
test_refusals    shape, act, layout and NULL violations leave every output byte at the sentinel.
test_zz_report   cases per form, the worst gelu ratio, the file's runtime.

Measured on an MI355X (256 CUs).  The file's 83 tests spend 4.6 s inside them (the slowest, OUT8 + GELU at 4096 x 4352 with its
numpy check, 1.5 s; a 138 MB case 0.1-0.3 s).  Cases per form: layout 1 bf16 24 + 2 large, layout 2 bf16 24 + 2 large, OUT8 12
+ 2 large, quantiser 15.  Every exact-family case came out bit for bit on the first run, on both layouts and all six epilogues,
the rows and columns with exponents -100 / +100 and the 37 tiles of each large case included; so did the quantiser's edges.
Worst gelu error / bound 0.9999; OUT8 + GELU: at most 9.0 % of the codes differ, all at a rounding boundary and by one step.
The one disagreement was the reference's: torch.ldexp on the device returned some powers of two an ulp off, so the f64
product held -1e-13 where a sum cancels, and the OUT8 expectation turned that into byte 0x80 where the kernel, rightly, wrote
0x00 (3 cases, 2 to 196 bytes each); mxfp8_exact_ref._pow2 now builds 2^e from the exponent field.  No defect was found in gemm.hip."""
import collections
import json
import time

import numpy as np
import pytest
import torch

import gemm_routes_ref as G
import mxfp8_exact_ref as R
from mmr_amd import _lib, ops
from oracle import mxfp8 as mx
from test_gemm_routes_gpu import DEV, _cus, _sync

pytestmark = pytest.mark.gpu
_SHAPES = collections.OrderedDict()
_STATS = {"t0": None, "cases": collections.Counter(), "gelu": 0.0, "out8_gelu": 0.0, "slowest": (0.0, "")}


@pytest.fixture(scope="module", autouse=True)
def _clock():
    _STATS["t0"] = time.perf_counter()
    yield
    _SHAPES.clear()


def _need_256():
    if _cus() != G.CUS:
        pytest.skip(f"the case table is derived for {G.CUS} CUs, this device has {_cus()}")


def _mx(q, e, k, layout):
    """Element values and exponents -> ops.MXFP8 on the device (bytes by e4m3_encode, scales through the offsets)."""
    return ops.MXFP8(R.e4m3_encode(q).to(DEV), torch.from_numpy(R.image(e, layout)).to(DEV), k, layout)


def _shape(c, fam):
    """The operands of (case, family) as MXFP8, the bias, the exact pre-activation (f64 on the device), once."""
    key = (c, fam)
    if key not in _SHAPES:
        while len(_SHAPES) >= 2:
            _SHAPES.popitem(last=False)
        d = R.operands(c, fam, parts="xwb")
        xd, wd = R.dense(d["xq"].to(DEV), d["xe"].to(DEV)), R.dense(d["wq"].to(DEV), d["we"].to(DEV))
        acc = R.exact_acc(xd, wd)
        _SHAPES[key] = {"x8": _mx(d["xq"], d["xe"], c.k, 0), "w8": _mx(d["wq"], d["we"], c.k, c.layout),
                        "b": d["b"].to(DEV), "acc": acc, "r": None}
    return _SHAPES[key]


def _residual(s, c, fam):
    if s["r"] is None:
        s["r"] = G.to_bf16(R.operands(c, fam, device=DEV, parts="r")["r"])
    return s["r"]


def _buf16(m, n):
    buf = torch.full((m + 2 * R.GUARD, n), R.SENT, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    return buf, buf[R.GUARD:R.GUARD + m]


def _buf8(m, n):
    """OUT8: (byte buffer, its middle m rows, scale buffer, the image inside it)."""
    buf = torch.full((m + 2 * R.GUARD, n), R.SENT8, dtype=torch.uint8, device=DEV)
    nsc = m // 256 * (n // 128) * 1024
    sbuf = torch.full((nsc + 2 * R.GUARD_S,), R.SENT_S, dtype=torch.uint8, device=DEV)
    return buf, buf[R.GUARD:R.GUARD + m], sbuf, sbuf[R.GUARD_S:R.GUARD_S + nsc]


def _q8(x8, w8, b, act, yq, ys, m, n):
    st = _lib.lib().mmr_linear_mxfp8_q8(_lib.ptr(x8.q), _lib.ptr(x8.s), _lib.ptr(w8.q), _lib.ptr(w8.s), _lib.ptr(b),
                                        _lib.ptr(yq), _lib.ptr(ys), m, n, x8.kp, act, _lib.stream_ptr(x8.q.device))
    assert st == 0, _lib.lib().mmr_last_error()


def _note(t0, form, name):
    dt = time.perf_counter() - t0
    _STATS["cases"][form] += 1
    _STATS["slowest"] = max(_STATS["slowest"], (dt, name))
    return dt


_FORMS = [(ci, False, e) for ci in range(len(R.CASES)) for e in R.EPILOGUES] + \
         [(ci, True, e) for ci in range(len(R.CASES)) if R.CASES[ci].layout == 2 for e in R.EPILOGUES8]
_FORMS.sort(key=lambda f: (f[0], bool(f[2][1]), f[1]))          # a case's families adjacent: the shape cache holds two


@pytest.mark.parametrize("ci,out8,epi", _FORMS,
                         ids=[f"{R.case_id(R.CASES[f[0]])}-{'out8' if f[1] else 'bf16'}-{f[2][0]}" for f in _FORMS])
def test_case(ci, out8, epi):
    _need_256()
    t0 = time.perf_counter()
    c = R.CASES[ci]
    name, act, hb, hr, inplace = epi
    fam = "gelu" if act else ("out8" if out8 else "exact")
    s = _shape(c, fam)
    b = s["b"] if hb else None
    form = f"l{c.layout}-{'out8' if out8 else 'bf16'}"
    if not out8:
        r = _residual(s, c, fam) if hr else None
        buf, out = _buf16(c.m, c.n)
        if inplace:
            out.copy_(r)
        ops.linear_mxfp8(s["x8"], s["w8"], b, out if inplace else r, act=act, out=out)
        _sync()
        got, rf = buf.view(torch.int16), (r.float() if hr else None)
        if act:
            z = s["acc"] + b.double()
            assert z.abs().max().item() <= G.ZMAX
            ref, tol = G.gelu_ref_tol(z, rf, "round1")
            res = G.verify_gelu(got, c.m, ref, tol)
            _STATS["gelu"] = max(_STATS["gelu"], res[2])
        else:
            res = G.verify_exact(got, c.m, R.expected_bits(s["acc"], b, rf))
        dt = _note(t0, form, f"{R.case_id(c)}-{form}-{name}")
        print(f"{R.case_id(c)} {form} {name}: guards intact {res[0]}, sentinels inside {res[1]}, "
              f"{'worst err / tol' if act else 'elements != expected'} {res[2]}, {dt:.2f} s")
        assert res[0], "guard rows written"
        assert res[1] == 0, f"{res[1]} elements never written"
        assert G.passes(res), res
        return
    buf, yq, sbuf, ys = _buf8(c.m, c.n)
    _q8(s["x8"], s["w8"], b, act, yq, ys, c.m, c.n)
    _sync()
    if act:
        g = R.verify_bytes(buf, c.m, yq)
        gs = R.verify_scales(sbuf, ys)
        assert g[0] and g[1] == 0 and gs[0] and gs[1] == 0, (g, gs)
        e = ys.cpu().numpy()[mx.scale_offsets(c.m, c.n, 0)].astype(np.int32) - 127
        z = (s["acc"] + b.double()).cpu().numpy()
        assert np.abs(z).max() <= G.ZMAX
        es, away, far, share = R.out8_gelu_check(mx.e4m3_decode(yq.cpu().numpy()), e, z)
        dt = _note(t0, form, f"{R.case_id(c)}-{form}-{name}")
        _STATS["out8_gelu"] = max(_STATS["out8_gelu"], share)
        print(f"{R.case_id(c)} {form} {name}: scale bytes differing {es:.4%}, codes differing {share:.4%}, away from a "
              f"rounding boundary {away}, beyond one step {far}, {dt:.2f} s")
        assert es < 2e-3 and away == 0 and far == 0
        return
    eq, es = R.expected_out8(G.bf2f(G.rne_bits(R.pre_f32(s["acc"], b))))
    a = R.verify_bytes(buf, c.m, eq.to(DEV))
    sc = R.verify_scales(sbuf, torch.from_numpy(es).to(DEV))
    dt = _note(t0, form, f"{R.case_id(c)}-{form}-{name}")
    print(f"{R.case_id(c)} {form} {name}: bytes (guards, sentinels, != expected) {a}, scale image {sc}, {dt:.2f} s")
    for i, j in (yq != eq.to(DEV)).nonzero()[:8].tolist():
        print(f"  byte ({i}, {j}): got {int(yq[i, j]):#04x}, expected {int(eq[i, j]):#04x}")
    assert a == (True, 0, 0) and sc == (True, 0, 0)


@pytest.mark.parametrize("c", R.BIG_BF16, ids=[R.case_id(c) for c in R.BIG_BF16])
@pytest.mark.parametrize("epi", [G.EPILOGUES[0], G.EPILOGUES[3]], ids=["none", "bias_res"])
def test_big_bf16(c, epi):
    _need_256()
    t0 = time.perf_counter()
    name, act, hb, hr, _ = epi
    tn = R.TN[c.layout]
    d = R.operands(c, "exact", parts="xwb")
    x8, w8 = _mx(d["xq"], d["xe"], c.k, 0), _mx(d["wq"], d["we"], c.k, c.layout)
    b = d["b"].to(DEV) if hb else None
    r = G.to_bf16(R.operands(c, "exact", device=DEV, parts="r")["r"]) if hr else None
    buf, out = _buf16(c.m, c.n)
    ops.linear_mxfp8(x8, w8, b, r, act=act, out=out)
    _sync()
    got = buf.view(torch.int16)
    assert bool((got[:R.GUARD] == R.SENT).all() and (got[R.GUARD + c.m:] == R.SENT).all()), "guard rows written"
    assert int((got[R.GUARD:R.GUARD + c.m] == R.SENT).sum()) == 0, "elements never written"
    tiles, per = R.walk_tiles(c)
    bad = 0
    for t in tiles:
        m0, n0 = t // (c.n // tn) * 256, t % (c.n // tn) * tn
        dt_ = R.operands(c, "exact", 256, tn, m0, n0, device=DEV, parts="xw")
        exp = R.expected_bits(R.preact(dt_), b[n0:n0 + tn] if hb else None, r[m0:m0 + 256, n0:n0 + tn].float() if hr else None)
        bad += int((got[R.GUARD + m0:R.GUARD + m0 + 256, n0:n0 + tn] != exp).sum())
    dt = _note(t0, f"l{c.layout}-bf16-big", f"{R.case_id(c)}-{name}")
    print(f"{R.case_id(c)} {name}: {len(tiles)} tiles checked ({per} workgroups per XCD), elements != expected {bad}, {dt:.2f} s")
    assert bad == 0


@pytest.mark.parametrize("epi", R.EPILOGUES8[:2], ids=["none", "bias"])
def test_big_out8(epi):
    _need_256()
    t0 = time.perf_counter()
    c = R.BIG_OUT8
    name, act, hb, _, _ = epi
    d = R.operands(c, "out8", parts="xwb")
    x8, w8 = _mx(d["xq"], d["xe"], c.k, 0), _mx(d["wq"], d["we"], c.k, 2)
    b = d["b"].to(DEV) if hb else None
    buf, yq, sbuf, ys = _buf8(c.m, c.n)
    _q8(x8, w8, b, act, yq, ys, c.m, c.n)
    _sync()
    g, gs = R.verify_bytes(buf, c.m, yq), R.verify_scales(sbuf, ys)
    assert g[0] and g[1] == 0 and gs[0] and gs[1] == 0, (g, gs)        # guards intact, every byte and scale byte written
    off = torch.from_numpy(mx.scale_offsets(c.m, c.n, 0)).to(DEV)
    tiles, per = R.walk_tiles(c)
    bad = bads = 0
    for t in tiles:
        m0, n0 = t // (c.n // 256) * 256, t % (c.n // 256) * 256
        dt_ = R.operands(c, "out8", 256, 256, m0, n0, parts="xw")
        eq, es = R.expected_out8(G.bf2f(G.rne_bits(R.pre_f32(R.preact(dt_), d["b"][n0:n0 + 256] if hb else None))))
        bad += int((yq[m0:m0 + 256, n0:n0 + 256] != eq.to(DEV)).sum())
        e_t = torch.from_numpy(es[mx.scale_offsets(256, 256, 0)]).to(DEV)                 # (256 rows, 8 blocks)
        bads += int((ys[off[m0:m0 + 256, n0 // 32:n0 // 32 + 8]] != e_t).sum())
    dt = _note(t0, "l2-out8-big", f"{R.case_id(c)}-{name}")
    print(f"{R.case_id(c)} out8 {name}: {len(tiles)} tiles checked, bytes != expected {bad}, scale bytes != expected {bads}, {dt:.2f} s")
    assert bad == 0 and bads == 0


def _edge_rows(rows, k, seed):
    """bf16 rows for the quantiser: spread magnitudes, then the edges in the leading elements of the first rows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, k, generator=g) * torch.exp(torch.rand(rows, 1, generator=g) * 12 - 6)
    x[0, :] = x[0, :].clamp(-1, 1)
    x[1, :] = x[1, :].clamp(-1, 1)
    x[2, :] = x[2, :].clamp(-1, 1)
    x[0, 1], x[1, 1], x[2, 1] = 1.75, 1.75 - 2.0 ** -7, 1.75 + 2.0 ** -7              # the threshold mantissa, below, above
    x[3, :] = 0
    x[3, 0], x[3, 1], x[3, 2] = 2.0 ** -126, 2.0 ** -130, -2.0 ** -133                # smallest normal, bf16 subnormals
    x[4, :] = x[4, :].clamp(-1, 1) * 1e30
    x[4, 3] = -3.3895313892515355e38                                                    # the largest finite bf16
    x[5, :] = -0.0
    x[6, :] = 0
    x[6, :8] = torch.tensor([256.0, 17.0, 19.0, -21.0, 2.0 ** -10, 3 * 2.0 ** -10, -2.0 ** -10, 1.0625])   # e4m3 ties at e = 0
    x[7, :] = 0
    x[7, k - 1] = -3.0                                                                  # the tail chunk alone
    t = x.to(torch.bfloat16)
    return t, t.float().numpy()


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("k,kp", [(8, 256), (8, 512), (24, 256), (40, 256), (264, 512)])
def test_quantiser_edges(k, kp, layout):
    rows = 384 if layout == 1 else 512                       # two panels
    xt, xf = _edge_rows(rows, k, 100 * k + kp + layout)
    x = xt.to(DEV)
    buf, q, _, _ = _buf8(rows, kp)
    nsc = rows // (192 if layout == 1 else 256) * (kp // 128) * 1024
    sbuf = torch.full((nsc + 2 * R.GUARD_S,), R.SENT_S, dtype=torch.uint8, device=DEV)
    sc = sbuf[R.GUARD_S:R.GUARD_S + nsc]
    st = _lib.lib().mmr_quantize_mxfp8(_lib.ptr(x), rows, k, kp, layout, _lib.ptr(q), _lib.ptr(sc), _lib.stream_ptr(x.device))
    assert st == 0, _lib.lib().mmr_last_error()
    _sync()
    qo, eo = mx.quantize(xf, kp)
    a = R.verify_bytes(buf.cpu(), rows, R.e4m3_encode(torch.from_numpy(qo)))
    exp = np.full(nsc, R.SENT_S, np.uint8)                   # layout 1 leaves 256 of a K-tile's 1024 bytes unused
    exp[mx.scale_offsets(rows, kp, layout)] = (eo + 127).astype(np.uint8)
    s = sbuf.cpu()
    ok_guard = bool((s[:R.GUARD_S] == R.SENT_S).all() and (s[R.GUARD_S + nsc:] == R.SENT_S).all())
    bads = int((s[R.GUARD_S:R.GUARD_S + nsc] != torch.from_numpy(exp)).sum())
    print(f"quantiser k {k} kp {kp} layout {layout}: bytes {a}, scale guards intact {ok_guard}, scale bytes != expected {bads}")
    assert a == (True, 0, 0) and ok_guard and bads == 0
    assert bool((q[:, k:] == 0).all())                       # padding bytes zero
    assert (eo[:, -(-k // 32):] == -127).all() and eo[3, 0] == -127 and eo[5, 0] == -127   # zero blocks, the clamp, -0.0
    assert eo[0, 0] - 1 == eo[1, 0] - 1 == eo[2, 0] - 2      # above the threshold mantissa: the next exponent
    _STATS["cases"]["quantiser"] += 1


def test_refusals():
    c = R.CASES[1]
    L = _lib.lib()
    s = _shape(c, "exact")
    x8, w8 = s["x8"], s["w8"]
    w1 = _shape(R.CASES[0], "exact")["w8"]
    buf, out = _buf16(c.m, c.n)
    buf8, yq, sbuf, ys = _buf8(c.m, c.n)
    stream = _lib.stream_ptr(x8.q.device)
    p = _lib.ptr

    def untouched():
        _sync()
        assert L.mmr_last_error()
        assert bool((buf.view(torch.int16) == R.SENT).all()) and bool((buf8 == R.SENT8).all()) and bool((sbuf == R.SENT_S).all())

    def lin(xq, xs, wq, ws, wl, y, m, n, kp, act):
        assert L.mmr_linear_mxfp8(p(xq), p(xs), p(wq), p(ws), wl, None, None, p(y), m, n, kp, act, stream) != 0
        untouched()

    def q8(xq, xs, wq, ws, yq_, ys_, m, n, kp, act):
        assert L.mmr_linear_mxfp8_q8(p(xq), p(xs), p(wq), p(ws), None, p(yq_), p(ys_), m, n, kp, act, stream) != 0
        untouched()

    lin(x8.q, x8.s, w8.q, w8.s, 2, out, 128, 256, 256, 0)            # m % 256
    lin(x8.q, x8.s, w8.q, w8.s, 2, out, 256, 192, 256, 0)            # n % 256 in layout 2
    lin(x8.q, x8.s, w1.q, w1.s, 1, out, 256, 256, 256, 0)            # n % 192 in layout 1
    lin(x8.q, x8.s, w8.q, w8.s, 2, out, 256, 256, 128, 0)            # kp % 256
    lin(x8.q, x8.s, w8.q, w8.s, 2, out, 256, 256, 256, 2)            # act
    lin(x8.q, x8.s, w8.q, w8.s, 0, out, 256, 256, 256, 0)            # w_layout
    lin(x8.q, x8.s, w8.q, w8.s, 3, out, 256, 256, 256, 0)
    for hole in range(4):
        a = [x8.q, x8.s, w8.q, w8.s]
        a[hole] = None
        lin(*a, 2, out, 256, 256, 256, 0)
        q8(*a, yq, ys, 256, 256, 256, 0)
    lin(x8.q, x8.s, w8.q, w8.s, 2, None, 256, 256, 256, 0)
    q8(x8.q, x8.s, w8.q, w8.s, None, ys, 256, 256, 256, 0)
    q8(x8.q, x8.s, w8.q, w8.s, yq, None, 256, 256, 256, 0)
    q8(x8.q, x8.s, w8.q, w8.s, yq, ys, 256, 192, 256, 0)             # n % 256
    q8(x8.q, x8.s, w8.q, w8.s, yq, ys, 128, 256, 256, 0)
    q8(x8.q, x8.s, w8.q, w8.s, yq, ys, 256, 256, 128, 0)
    q8(x8.q, x8.s, w8.q, w8.s, yq, ys, 256, 256, 256, 2)


def test_zz_report():
    """Cases run per form, the worst gelu error / bound, the share of OUT8 + GELU codes at a boundary, the runtime."""
    print(json.dumps({"cases_per_form": dict(_STATS["cases"]), "worst_gelu_err_over_tol": round(_STATS["gelu"], 4),
                      "out8_gelu_codes_differing": round(_STATS["out8_gelu"], 6),
                      "runtime_s": round(time.perf_counter() - _STATS["t0"], 1),
                      "slowest": (round(_STATS["slowest"][0], 2), _STATS["slowest"][1])}))
