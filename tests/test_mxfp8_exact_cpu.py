"""CPU: the operands, the kernel model and the mutants that test_mxfp8_exact_gpu.py holds the MX-fp8 GEMM forms to
(tests/mxfp8_exact_ref.py).
  e4m3_encode    equals torch.float8_e4m3fn conversion on all 256 codes, on random values and on ties.
  operands       the families are what the docstring says: ranges, every partial sum within 22 bits, the scale images
                 read back through the offsets, adjacent blocks / K-tiles / row halves / wave columns / panels with
                 different scales, more than half of the outputs in need of rounding, any one scale changed by one
                 changes an output, the OUT8 threshold, zero and tie blocks present.
  model, mutants the model passes every check on every case, form and epilogue (on the case cut to two row panels and
                 two tile columns); wherever a mutant changes the model's output the checks fail; every mutant is
                 caught on every form it applies to.
Each printed line records the worst ratio to each derived bound."""
import functools

import numpy as np
import pytest
import torch

import gemm_routes_ref as G
import mxfp8_exact_ref as R
from oracle import mxfp8 as mx


def test_e4m3_encode_is_torchs_conversion():
    codes = np.arange(256, dtype=np.uint8)
    vals = mx.e4m3_decode(codes)
    fin = ~np.isnan(vals)
    got = R.e4m3_encode(torch.from_numpy(vals[fin]))
    assert np.array_equal(got.numpy(), codes[fin])                      # the grid encodes to itself, -0 included
    t8 = torch.from_numpy(vals[fin]).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(got, t8)
    g = torch.Generator().manual_seed(5)
    v = torch.cat([torch.randn(20000, generator=g) * 100, torch.randn(20000, generator=g) * 0.01,
                   torch.tensor([17.0, 19.0, -17.0, 0.0, -0.0, 2.0 ** -10, 3 * 2.0 ** -10, -2.0 ** -10, 2.0 ** -6 - 2.0 ** -10,
                                 448.0, -448.0, 1.0625, 1.1875])]).clamp(-448, 448)
    assert torch.equal(R.e4m3_encode(v), v.to(torch.float8_e4m3fn).view(torch.uint8))
    assert np.array_equal(mx.e4m3_decode(R.e4m3_encode(v).numpy()), mx.e4m3_round(v.numpy()))


@pytest.mark.parametrize("c", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_exact_family(c):
    rows, cols = R.cut(c)
    d = R.operands(c, "exact", rows, cols)
    assert d["xq"].abs().max() == 4 and d["wq"].abs().max() == 4 and d["b"].abs().max() <= 8 and d["r"].abs().max() == 64
    live = d["xe"] > -127
    lo, hi = (-102, 2) if c.extreme == "xlo" else ((-2, 102) if c.extreme == "xhi" else (-2, 2))
    assert d["xe"][live].min() == lo and d["xe"][live].max() == hi
    assert bool((d["xq"].view(rows, -1, 32)[~live] == 0).all()) and bool((~live[R.ZERO_ROW]).all())
    assert bool((d["xq"][:, c.k:] == 0).all()) and bool((d["xe"][:, -(-c.k // 32):] == -127).all())
    # a cut is a slice of the case; a window generated alone equals the slice
    part = R.operands(c, "exact", 64, 32, row0=128, col0=64)
    assert torch.equal(part["xq"], d["xq"][128:192]) and torch.equal(part["we"], d["we"][64:96])
    assert torch.equal(part["r"], d["r"][128:192, 64:96]) and torch.equal(part["b"], d["b"][64:96])
    # the images hold the exponents at the offsets, every byte written once (image asserts the permutation)
    xs, ws = R.image(d["xe"], 0), R.image(d["we"], c.layout)
    assert torch.equal(R._read_scales(xs, rows, c.kp, 0, None, "x"), d["xe"])
    assert torch.equal(R._read_scales(ws, cols, c.kp, c.layout, None, "w"), d["we"])
    # neighbours differ: blocks of a K-tile, K-tiles, the 128-row halves, wave columns, panels
    nb = min(c.kp, -(-c.k // 32) * 32) // 32
    xe, we, wt = d["xe"][:, :nb], d["we"][:, :nb], R.TN[c.layout] // 4
    share = (lambda a, b: (a == b).double().mean().item())
    assert share(xe[:, 1:], xe[:, :-1]) < 0.3 and share(xe[:128], xe[128:256]) < 0.3
    assert share(we[:wt], we[wt:2 * wt]) < 0.3
    if nb > 4:
        assert share(xe[:, 4:], xe[:, :-4]) < 0.3
    if rows > 256:
        assert share(xe[:256], xe[256:512]) < 0.3
    if cols > R.TN[c.layout]:
        assert share(we[:R.TN[c.layout]], we[R.TN[c.layout]:]) < 0.3
    # exactness: sum |terms| in units of 2^-4 below 2^24 (kp <= 1024: 2^22 for the dot product), and the f32 value equal to the f64
    assert c.kp * 16 * 16 * 16 + (8 + 64) * 16 < 2 ** 24
    acc = R.preact(d)
    ordi = R.ordinary(c, rows, cols)
    for b, r in ((None, None), (d["b"], None), (d["b"], d["r"])):
        ex = acc + (b.double() if b is not None else 0) + (r.double() if r is not None else 0)
        assert torch.equal(R.pre_f32(acc, b, r).double()[ordi], ex[ordi])
    # more than half of the outputs need rounding
    v = R.pre_f32(acc, d["b"], None)
    need = (G.bf2f(G.rne_bits(v)) != v)[ordi].double().mean().item()
    assert need > 0.5, need
    # any one scale changed by one changes at least one output
    base = G.rne_bits(v)
    xd, wd = R.dense(d["xq"], d["xe"]), R.dense(d["wq"], d["we"])
    for blk in range(nb):
        p = (xd[:, blk * 32:blk * 32 + 32] @ wd[:, blk * 32:blk * 32 + 32].t()).float()
        for delta in (p, -p / 2):                                     # exponent + 1 / - 1 of either operand's block
            ch = (G.rne_bits(v + delta) != base) & ordi               # (an extreme row meets only two such columns)
            zero_x = (d["xq"][:, blk * 32:blk * 32 + 32] == 0).all(1)
            assert bool((ch.any(1) | zero_x | ~ordi.any(1)).all()) and bool((ch.any(0) | ~ordi.any(0)).all()), (blk,)
    print(f"{R.case_id(c)}: {need:.1%} of the outputs need rounding")


@pytest.mark.parametrize("c", [c for c in R.CASES if c.layout == 2], ids=[R.case_id(c) for c in R.CASES if c.layout == 2])
def test_out8_family(c):
    rows, cols = R.cut(c)
    d = R.operands(c, "out8", rows, cols)
    acc = R.preact(d)
    ordi = R.ordinary(c, rows, cols)
    assert torch.equal(R.pre_f32(acc, d["b"]).double()[ordi], (acc + d["b"].double())[ordi])
    vb = G.bf2f(G.rne_bits(R.pre_f32(acc, d["b"])))
    amax = vb[R.ZERO_ROW].abs().view(-1, 32).amax(1)
    assert amax[:3].tolist() == [0.875, 1.75 - 2.0 ** -7, 3.5 + 2.0 ** -6]          # at, below and above mantissa 1.75
    _, e = mx.quantize(vb.numpy(), cols)
    assert e[R.ZERO_ROW, :3].tolist() == [-9, -8, -6]
    assert np.mean(e[:, 1:] != e[:, :-1]) > 0.5                                    # adjacent blocks, other exponents
    v0 = G.bf2f(G.rne_bits(R.pre_f32(acc, None)))
    assert bool((v0[R.ZERO_ROW] == 0).all())                                       # all-zero output blocks
    q0, e0 = mx.quantize(v0.numpy(), cols)
    assert (e0[R.ZERO_ROW] == -127).all()
    sc = v0.numpy() * np.ldexp(np.float32(1), -np.repeat(e0, 32, axis=1))
    step = np.abs(mx.e4m3_round(sc * 1.01) - mx.e4m3_round(sc * 0.99))
    ties = np.mean((np.abs(sc - q0) * 2 == step) & (step > 0))
    assert ties > 0.01, ties
    print(f"{R.case_id(c)}: {ties:.1%} of the OUT8 values on e4m3 ties")


def _checks(c, fam, epi, out8, d):
    """The check of one (case, epilogue, form) on the cut: a function buffer(s) -> pass, and the worst gelu ratio."""
    _, act, hb, hr, _ = epi
    rows, cols = d["xq"].shape[0], d["wq"].shape[0]
    acc = R.preact(d)
    b, r = (d["b"] if hb else None), (d["r"] if hr else None)
    if act:
        z = acc + b.double()
        assert z.abs().max() <= G.ZMAX and torch.equal(z * 8, (z * 8).round())
    if not out8:
        if act:
            ref, tol = G.gelu_ref_tol(z, r, "round1")
            return lambda buf: G.verify_gelu(buf, rows, ref, tol)
        exp = R.expected_bits(acc, b, r)
        return lambda buf: G.verify_exact(buf, rows, exp)
    if act:
        def chk(bufs):
            buf, sbuf = bufs
            mid = buf[R.GUARD:R.GUARD + rows]
            if not (R.verify_bytes(buf, rows, mid)[0] and R.verify_scales(sbuf, sbuf[R.GUARD_S:-R.GUARD_S])[:2] == (True, 0)):
                return (False, 0, 1)
            if int((mid == R.SENT8).sum()):
                return (True, int((mid == R.SENT8).sum()), 1)
            e = sbuf[R.GUARD_S:-R.GUARD_S].numpy()[mx.scale_offsets(rows, cols, 0)].astype(np.int32) - 127
            es, away, far, _ = R.out8_gelu_check(mx.e4m3_decode(mid.numpy()), e, z.numpy())
            return (True, 0, int(es >= 2e-3) + away + far)
        return chk
    eq, es = R.expected_out8(G.bf2f(G.rne_bits(R.pre_f32(acc, b))))
    es = torch.from_numpy(es)

    def chk(bufs):
        a, s = R.verify_bytes(bufs[0], rows, eq), R.verify_scales(bufs[1], es)
        return (a[0] and s[0], a[1] + s[1], a[2] + s[2])
    return chk


@functools.lru_cache(maxsize=None)
def _run_case(ci):
    c = R.CASES[ci]
    rows, cols = R.cut(c)
    bad, escaped, caught, worst = [], [], set(), 0.0
    forms = [("bf16", False)] + ([("out8", True)] if c.layout == 2 else [])
    for form, out8 in forms:
        for epi in (R.EPILOGUES8 if out8 else R.EPILOGUES):
            fam = "gelu" if epi[1] else ("out8" if out8 else "exact")
            d = R.operands(c, fam, rows, cols)
            xs, ws = R.image(d["xe"], 0), R.image(d["we"], c.layout)
            check = _checks(c, fam, epi, out8, d)
            base = R.model(c, d, xs, ws, epi, None, out8)
            res = check(base)
            if not G.passes(res):
                bad.append((form, epi[0], res))
            if epi[1] and not out8:
                worst = max(worst, res[2])
            for mu in R.MUTANTS:
                if (mu in R.MUTANTS8 and not out8) or (mu in R.MUTANTS16 and out8) or (mu in ("round", "f32quant") and epi[1]):
                    continue      # under GELU one bf16 rounding lies inside the bound; the exact family tells them apart
                buf = R.model(c, d, xs, ws, epi, mu, out8)
                same = all(torch.equal(a, b) for a, b in zip(buf, base)) if out8 else torch.equal(buf, base)
                if same:
                    continue
                if G.passes(check(buf)):
                    escaped.append((form, epi[0], mu))
                else:
                    caught.add((mu, f"l{c.layout}-{form}"))
    return bad, escaped, caught, worst


@pytest.mark.parametrize("ci", range(len(R.CASES)), ids=[R.case_id(c) for c in R.CASES])
def test_model_and_mutants(ci):
    bad, escaped, caught, worst = _run_case(ci)
    print(f"{R.case_id(R.CASES[ci])}: worst gelu error / bound of the model {worst:.3f}; caught {len(caught)} (mutant, form) pairs")
    assert not bad, bad
    assert not escaped, escaped
    assert worst <= 1.0


def test_every_mutant_caught_on_every_form():
    caught = set().union(*(_run_case(ci)[2] for ci in range(len(R.CASES))))
    want = [(mu, f) for mu in R.MUTANTS for f in ("l1-bf16", "l2-bf16", "l2-out8")
            if not (mu in R.MUTANTS8 and not f.endswith("out8")) and not (mu in R.MUTANTS16 and f.endswith("out8"))]
    missing = [p for p in want if p not in caught]
    assert not missing, missing


def test_walk_tiles():
    for c in R.BIG_BF16 + (R.BIG_OUT8,):
        tiles, per = R.walk_tiles(c)
        nt = (c.m // 256) * (c.n // R.TN[c.layout])
        assert per == 32 and nt > 2 * G.CUS and len(tiles) >= 32 and tiles[0] == 0 and tiles[-1] == nt - 1
        assert c.m * c.n * (2 if c is not R.BIG_OUT8 else 1) > 128 << 20           # above the non-temporal threshold
    for c in R.CASES:
        assert c.m * c.n * 2 <= 40e6
