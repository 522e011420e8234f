"""GPU: the linears outside the tiled GEMM and the f32 row kernels of the x3 mode against the f64 references,
per-element bounds and exact families of small_linear_ref.py (csrc/tower.hip linear_f32, csrc/linear_x3.hip linear_x3,
csrc/gemm_rw.hip gemm_rw, csrc/x3.hip x3_bert_embed / x3_mean_rows / x3_gather_rows).

Rules (small_linear_ref.py has the derivations): every element |got - ref| <= tol; the integer, onehot and split
families bit for bit (without GELU); a linear_rw case (one family and epilogue, its launches at every row count
pooled) has >= 99 % of its elements equal to bf16_rn(ref); launches that take the same route give the same bits
(cin = 640 pinned to 8 waves = pinned to 4; the unpinned launch = the pinned one of its NW).  Every output sits in a
buffer with 2 guard rows in front and behind (and guard columns where the row stride exceeds cout) whose bit pattern
must survive the launch; every x and residual sits between 2 NaN rows.  Rejected shapes return a status and leave
the output untouched; b = 0 returns OK and writes nothing.

Case -> route, from the dispatch code (small_linear_ref.x3_route / f32_route / rw_route restate it and
test_small_linear_cpu.py pins these rows):

  linear_x3 (one 32 x 32 tile per workgroup of NW waves, kw = cin / NW, k-steps of 32 in chunks of 3)
    cin    unpinned NW (B <= 70)  steps / wave  live steps, last chunk   pinned to the other NW
    128    4 (cin % 256)          1             1 (2 slots clamped)      pin 8 ignored
    256    8                      1             1                        NW 4: 2 steps, 2 live
    384    4 (cin % 256)          3             3                        pin 8 ignored
    512    8                      2             2                        NW 4: 4 steps, 1 live
    640    4 (cin % 256)          5             2                        pin 8 ignored: same bits as pin 4
    1536   8                      6             3                        NW 4: 12 steps, 3 live
    B = 512, cin = 256, cout = 1024: 16 * 32 = 512 tiles -> 4 waves unpinned (same bits as pin 4, not as pin 8)
    B = 1 / 31 / 32 / 33 / 70: one tile of 1 / 31 / 32 rows, two tiles with 1 row, three with 6 rows in the last
  linear_f32 (8 waves, per = ceil(cin / 16 / 8) k-steps of 16 per wave in chunks of 6)
    cin    steps  per  waves' steps
    16     1      1    1 0 0 0 0 0 0 0
    48     3      1    1 1 1 0 0 0 0 0
    112    7      1    1 x 7, wave 7 idle
    128    8      1    1 x 8
    144    9      2    2 2 2 2 1 0 0 0
    768    48     6    6 x 8 (one full chunk)
    1552   97     13   13 x 7 (chunks of 6, 6, 1), wave 7: 6
  linear_rw (8 waves per workgroup, each owning whole 32-token tiles; 256 CUs)
    (N, K)        parts  CT  tiles per wave at M <= 261
    (32, 64)      1      1   1
    (64, 64)      1      2   1
    (96, 64)      1      3   1
    (160, 192)    1      1   1 (5 passes of one tile)
    (576, 192)    2      3   1
    (1152, 192)   3      3   1
    persistent: (1152, 192), per_cu = 1, grid.x = CUs / 3 = 85, M = 2 * 85 * 8 * 32 + 3 * 32 + 5 = 43621: 1364 tiles,
    waves 0-3 of workgroup 0 own 3 tiles, every other wave 2, the last tile holds 5 rows

Measured on an MI355X against the f64 reference (worst err / tol, lowest bit-equality share; records, not thresholds):
  kernel (checks)                        err / tol   bit share
  linear_x3 (16064)                      0.491       -
  linear_f32 (2128)                      0.484       -
  linear_x3 / linear_f32 strides (80)    0.148 / 0.109
  linear_x3 / linear_f32 batched         0.145 / 0.123  (1440 / 2160 checks)
  linear_rw (528)                        0.995       0.9998
  linear_rw persistent (12)              0.992       0.99995
  x3_bert_embed (126)                    0.177       -
  x3_mean_rows (144)                     0.333       -
  x3_gather_rows                         exact
  every integer / onehot / split case bit for bit
The two linears' worst figures are the onehot family's, where the bound is nearly the two epilogue adds alone; they
equal the CPU model's to the last digit.  linear_rw's figures near 1 are the half-ulp term alone.  The file runs in
7 s (37 tests, the slowest 0.9 s).

Scratch builds, not committed, one arithmetic-only change each (no address touched), counted in failed checks of this
file's 22765:
  wave NW - 1's partial left out of linear_x3's LDS sum: 9 tests fail (every linear_x3 test, the x3 strides and the x3
    batched test; 13024 checks: 11504 of linear_x3's 16064, 80 of 80 strides, 1440 of 1440 batched), nothing else;
  the lo hi MFMA of linear_x3 removed: the same 9 tests (7810 checks: 7202, 32, 576; the integer and onehot families
    have lo(x) = 0 and cannot see it, split and the bounds do);
  gemm_rw's tile += stride sweep multiplying the first tile's rows again: test_linear_rw_persistent alone (14 checks).
The tests of test_fusion_gpu.py and test_towers_gpu.py named test_linear_x3* / test_linear_rw* also see the first two
builds (8 of their 17 fail: a whole partial or a 2^-9 term is above their global 2e-5 bar); all 17 pass on the third.
"""
import json
import math

import pytest
import torch

import rowwise_ref as R
import small_linear_ref as L
import test_rowwise_gpu as T
from mmr_amd import _lib, ops
from test_rowwise_gpu import DEV, GUARD, PAT, _guard_in, _guard_out, _vec

pytestmark = pytest.mark.gpu
SUMMARY = {}


class _Score(T._Score):
    """rowwise's collector with the comparisons on the device and a summary of this file's own."""

    def dev_tol(self, tag, got, ref, tol):
        err = (got.double() - ref).abs()
        ra = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp(min=1e-300)).max().item()
        self.worst = max(self.worst, ra) if ra == ra else float("nan")
        self.n += 1
        if not ra <= 1.0:
            self.bad.append(f"{tag}: err / tol {ra:.4g}")

    def dev_equal(self, tag, got, exp, what):
        self.n += 1
        ne = R.bits(got) != R.bits(exp)
        if bool(ne.any()):
            self.bad.append(f"{tag}: {what} ({int(ne.sum())} elements differ)")

    def dev_share(self, tag, same, total):
        sh = same / max(total, 1)
        self.share = min(self.share, sh)
        if not sh >= L.BIT_SHARE:
            self.bad.append(f"{tag}: bit-equality share {sh:.4f} < {L.BIT_SHARE}")

    def done(self):
        s = SUMMARY.setdefault(self.name, {"worst": 0.0, "share": 1.0, "checks": 0, "failed": 0})
        s["worst"] = max(s["worst"], self.worst) if self.worst == self.worst else float("nan")
        s["share"], s["checks"], s["failed"] = min(s["share"], self.share), s["checks"] + self.n, s["failed"] + len(self.bad)
        print(json.dumps({"kernel": self.name, "worst": self.worst, "share": self.share, "checks": self.n,
                          "failed": len(self.bad)}))
        assert not self.bad, f"{len(self.bad)} failed:\n" + "\n".join(self.bad[:40])


def _weights(kind, w):
    """w from the CPU -> what the op takes: the f32 rows between NaN rows, or the X3W split of them."""
    wd = _guard_in(w.reshape(-1, w.shape[-1])).view(w.shape)
    return ops.X3W(wd) if kind == "x3" else wd


def _launch(kind, x, w, bias, r, act, out):
    if kind == "x3":
        return ops.linear_x3(x, w, bias, residual=r, act=act, out=out)
    return ops.linear_f32(x, w, bias, residual=r, act=act, out=out)


def _pin(pin):
    return ops.pinned(ops.PIN_X3_WAVES, pin if pin is not None else -1)


def _refs(kind, inp, cin, nws):
    """{(act, bias, res, nw): (ref, tol) on the device} and {(bias, res): exact expectation or None}."""
    P, A = L.products(inp["x"], inp["w"])
    refs, exact = {}, {}
    for act, bias_on, res_on in L.EPILOGUES:
        for nw in nws:
            ref, tol = L.lin_ref(kind, P, A, inp["bias"] if bias_on else None, inp["r"] if res_on else None, act, cin, nw)
            refs[act, bias_on, res_on, nw] = (ref.to(DEV), tol.to(DEV))
        if not act:
            e = L.expected_exact(inp, bias_on, res_on)
            exact[bias_on, res_on] = e.to(DEV) if e is not None else None
    return refs, exact


def _linear_cases(sc, kind, cin, cout, pins, row_counts=L.LIN_B, fams=None):
    for fam in fams or L.families(kind):
        inp = L.lin_inputs(kind, fam, max(row_counts), cin, cout, 0)
        counts = (inp["rows"],) if fam == "onehot" else row_counts
        nws = sorted({L.x3_nw(cin, cout, rows, pin=p) for p in pins for rows in counts}) if kind == "x3" else [None]
        refs, exact = _refs(kind, inp, cin, nws)
        w, bias = _weights(kind, inp["w"]), _vec(inp["bias"])
        for rows in counts:
            x, r = _guard_in(inp["x"][:rows]), _guard_in(inp["r"][:rows])
            for act, bias_on, res_on in L.EPILOGUES:
                by_nw = {}
                for pin in pins:
                    nw = L.x3_nw(cin, cout, rows, pin=pin) if kind == "x3" else None
                    buf, out = _guard_out(rows, cout, torch.float32)
                    with _pin(pin):
                        _launch(kind, x, w, bias if bias_on else None, r if res_on else None, act, out)
                    tag = f"{kind} {fam} cin={cin} cout={cout} B={rows} pin={pin} nw={nw} act={act} bias={bias_on} res={res_on}"
                    sc.guard(tag, buf, rows, cout)
                    ref, tol = refs[act, bias_on, res_on, nw]
                    sc.dev_tol(tag, out, ref[:rows], tol[:rows])
                    if not act and exact[bias_on, res_on] is not None:
                        sc.dev_equal(tag, out, exact[bias_on, res_on][:rows], "exact family not bit for bit")
                    if nw in by_nw:                       # same route (an ignored pin, the unpinned choice): same bits
                        sc.dev_equal(tag, out, by_nw[nw], "differs from the other launch with this NW")
                    else:
                        by_nw[nw] = out.clone()


# ------------------------------------------------------------------------------------------ linear_x3
@pytest.mark.parametrize("cin", L.X3_CIN)
def test_linear_x3(cin):
    """Every cout, B, family and epilogue, pinned to 4 and to 8 waves and unpinned."""
    sc = _Score("linear_x3")
    for cout in L.X3_COUT:
        _linear_cases(sc, "x3", cin, cout, L.X3_PINS)
    sc.done()


def test_linear_x3_auto_four_waves():
    """>= 512 tiles take 4 waves unpinned: the bits of the launch pinned to 4, and (gauss) not those pinned to 8."""
    sc = _Score("linear_x3")
    b, cin, cout = L.X3_AUTO4
    assert L.x3_nw(cin, cout, b) == 4 and L.x3_nw(cin, cout, b, pin=8) == 8
    _linear_cases(sc, "x3", cin, cout, (None, 4), row_counts=(b,), fams=("integer", "gauss", "rowscale"))
    inp = L.lin_inputs("x3", "gauss", b, cin, cout, 0)
    x, w, outs = _guard_in(inp["x"]), _weights("x3", inp["w"]), {}
    for pin in (None, 8):
        with _pin(pin):
            outs[pin] = ops.linear_x3(x, w)
    assert not torch.equal(outs[None], outs[8]), "the unpinned launch gave the 8-wave sum"
    sc.done()


# ------------------------------------------------------------------------------------------ linear_f32
@pytest.mark.parametrize("cin", L.F32_CIN)
def test_linear_f32(cin):
    sc = _Score("linear_f32")
    for cout in L.F32_COUT:
        _linear_cases(sc, "f32", cin, cout, (None,))
    sc.done()


# ------------------------------------------------------------------------------------------ strides
@pytest.mark.parametrize("kind", ("x3", "f32"))
def test_linear_strides(kind):
    """x a column slice of a wider buffer (ldx > cin, 16-B aligned start), ldy > cout (guard columns), ldr != ldy,
    and the residual aliasing the output."""
    sc = _Score(f"linear_{kind} strides")
    for cin, cout in L.STRIDE_SHAPES[kind]:
        for fam in ("integer", "rowscale"):
            inp = L.lin_inputs(kind, fam, max(L.STRIDE_B), cin, cout, 1)
            nws = sorted({L.x3_nw(cin, cout, rows) for rows in L.STRIDE_B}) if kind == "x3" else [None]
            refs, exact = _refs(kind, inp, cin, nws)
            w, bias = _weights(kind, inp["w"]), _vec(inp["bias"])
            for rows in L.STRIDE_B:
                nw = L.x3_nw(cin, cout, rows) if kind == "x3" else None
                for name, xoff, dy, dr in L.STRIDES:
                    xbuf = torch.full((rows + 2 * GUARD, cin + 8), float("nan"), device=DEV)
                    x = xbuf[GUARD:GUARD + rows, xoff:xoff + cin]
                    x.copy_(inp["x"][:rows])
                    for act in (0, 1):
                        buf, out = _guard_out(rows, cout, torch.float32, cout + dy)
                        if dr is None:
                            out.copy_(inp["r"][:rows])
                            r = out
                        else:
                            r = _guard_in(inp["r"][:rows], cout + dr)
                        _launch(kind, x, w, bias, r, act, out)
                        tag = f"{kind} {fam} cin={cin} cout={cout} B={rows} {name} act={act}"
                        sc.guard(tag, buf, rows, cout)
                        ref, tol = refs[act, True, True, nw]
                        sc.dev_tol(tag, out, ref[:rows], tol[:rows])
                        if not act and exact[True, True] is not None:
                            sc.dev_equal(tag, out, exact[True, True][:rows], "exact family not bit for bit")
    sc.done()


# ------------------------------------------------------------------------------------------ batched forms
@pytest.mark.parametrize("kind", ("x3", "f32"))
def test_linear_batched(kind):
    """nbatch 1 / 3 / 5, contiguous and the fusion head's layout (problem i = columns i C .. of each row: ldx = nl C,
    bsx = C), bias per problem or None, residual per problem or None: every problem against its own f64 reference."""
    sc = _Score(f"linear_{kind} batched")
    fn = ops.linear_x3_batched if kind == "x3" else ops.linear_f32_batched
    for cin, cout in L.BATCH_SHAPES[kind]:
        for nb in L.BATCH_N:
            for fam in ("integer", "gauss"):
                inps = [L.lin_inputs(kind, fam, max(L.BATCH_B), cin, cout, 10 + i) for i in range(nb)]
                w = _weights(kind, torch.stack([i["w"] for i in inps]))
                bias = _guard_in(torch.stack([i["bias"] for i in inps]))
                for b in L.BATCH_B:
                    nw = L.x3_nw(cin, cout, b, nb) if kind == "x3" else None
                    xs = torch.stack([i["x"][:b] for i in inps])                                  # (nb, b, cin)
                    r = _guard_in(torch.stack([i["r"][:b] for i in inps]).view(nb * b, cout))
                    for layout in ("contiguous", "fusion"):
                        if layout == "contiguous":
                            x, kw = _guard_in(xs.view(nb * b, cin)), {}
                        else:
                            x, kw = _guard_in(xs.transpose(0, 1).reshape(b, nb * cin)), {"ldx": nb * cin, "bsx": cin}
                        for act, bias_on, res_on in L.EPILOGUES:
                            buf, out = _guard_out(nb * b, cout, torch.float32)
                            fn(x, w, bias if bias_on else None, nb, b, residual=r if res_on else None, act=act, out=out, **kw)
                            tag = (f"{kind} batched {fam} cin={cin} cout={cout} nbatch={nb} b={b} {layout} act={act} "
                                   f"bias={bias_on} res={res_on}")
                            sc.guard(tag, buf, nb * b, cout)
                            for i, inp in enumerate(inps):
                                P, A = L.products(inp["x"][:b], inp["w"])
                                ref, tol = L.lin_ref(kind, P, A, inp["bias"] if bias_on else None,
                                                     inp["r"] if res_on else None, act, cin, nw)
                                got = out[i * b:(i + 1) * b]
                                sc.dev_tol(f"{tag} problem {i}", got, ref.to(DEV), tol.to(DEV))
                                e = L.expected_exact(inp, bias_on, res_on, rows=b) if not act else None
                                if e is not None:
                                    sc.dev_equal(f"{tag} problem {i}", got, e.to(DEV), "exact family not bit for bit")
    sc.done()


# ------------------------------------------------------------------------------------------ linear_rw
@pytest.mark.parametrize("n,k", L.RW_NK)
def test_linear_rw(n, k):
    """CT 1 / 2 / 3, five passes at CT 1, two and three parts; M = 1 / 31 / 32 / 33 / 261; bias and residual present
    and absent."""
    sc = _Score("linear_rw")
    for fam in L.families("rw"):
        inp = L.lin_inputs("rw", fam, max(L.RW_M), k, n, 0)
        counts = (inp["rows"],) if fam == "onehot" else L.RW_M
        pack, bias = ops.rw_pack(_guard_in(inp["w"])), _vec(inp["bias"])
        assert pack is not None
        P, A = L.products(inp["x"], inp["w"])
        for bias_on in (False, True):
            for res_on in (False, True):
                ref, tol = L.lin_ref("rw", P, A, inp["bias"] if bias_on else None, inp["r"] if res_on else None, 0, k)
                ref, tol = ref.to(DEV), tol.to(DEV)
                e = L.expected_exact(inp, bias_on, res_on)
                e = e.to(DEV) if e is not None else None
                same = total = 0
                for m in counts:
                    x, r = _guard_in(inp["x"][:m]), _guard_in(inp["r"][:m])
                    buf, out = _guard_out(m, n, torch.bfloat16)
                    ops.linear_rw(x, pack, bias if bias_on else None, r if res_on else None, out=out)
                    tag = f"rw {fam} N={n} K={k} M={m} bias={bias_on} res={res_on}"
                    sc.guard(tag, buf, m, n)
                    sc.dev_tol(tag, out, ref[:m], tol[:m])
                    if e is not None:
                        sc.dev_equal(tag, out, e[:m], "exact family not bit for bit")
                    same += int((R.bits(out) == R.bits(R.bf16_rn(ref[:m]))).sum())
                    total += m * n
                sc.dev_share(f"rw {fam} N={n} K={k} bias={bias_on} res={res_on}", same, total)
    sc.done()


def test_linear_rw_persistent():
    """Every wave sweeps at least twice (tile += stride, the prefetch of the next tile's rows under this tile's
    MFMAs, the residual chunks of the next pass), four waves a third time, and the last tile is ragged.  M comes
    from the launcher's own formula and the device's CU count; reference and comparison on the device in f64."""
    sc = _Score("linear_rw persistent")
    n, k = L.RW_PERSISTENT
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = L.rw_persistent_m(n, k, cus)
    rt = L.rw_route(n, k, m, cus)
    assert -(-m // 32) > 2 * rt["grid_x"] * 8 and rt["tiles_per_wave"] == 3 and m % 32 == 5, rt
    assert rt["parts"] == _lib.lib().mmr_linear_rw_parts(n, k)
    for fam in ("integer", "rowscale"):
        small = L.lin_inputs("rw", fam, 1, k, n, 2)
        g_ = torch.Generator(device=DEV).manual_seed(5)
        if fam == "integer":
            x = torch.randint(-8, 9, (m, k), generator=g_, device=DEV).to(torch.bfloat16)
            r = torch.randint(-8, 9, (m, n), generator=g_, device=DEV).to(torch.bfloat16)
        else:
            sc_ = (2.0 ** (torch.arange(m, device=DEV) % 9 - 4).float())[:, None]
            x = (torch.randn(m, k, generator=g_, device=DEV) * sc_).to(torch.bfloat16)
            r = (torch.randn(m, n, generator=g_, device=DEV) * sc_).to(torch.bfloat16)
        xg = torch.full((m + 2 * GUARD, k), float("nan"), dtype=torch.bfloat16, device=DEV)
        xg[GUARD:GUARD + m] = x
        pack, bias = ops.rw_pack(_guard_in(small["w"])), _vec(small["bias"])
        wd, bd = small["w"].to(DEV).double(), small["bias"].to(DEV).double()
        buf, out = _guard_out(m, n, torch.bfloat16)
        ops.linear_rw(xg[GUARD:GUARD + m], pack, bias, r, out=out)
        sc.guard(f"rw persistent {fam}", buf, m, n)
        same = 0
        for r0 in range(0, m, 8192):
            xs, rs = x[r0:r0 + 8192].double(), r[r0:r0 + 8192].double()
            ref = xs @ wd.t() + bd + rs
            tol = 2.0 ** -8 * ref.abs() + (k + 3) * L.U24 * (xs.abs() @ wd.abs().t() + bd.abs() + rs.abs())
            got = out[r0:r0 + 8192]
            tag = f"rw persistent {fam} M={m} rows {r0}.."
            sc.dev_tol(tag, got, ref, tol)
            eq = R.bits(got) == R.bits(R.bf16_rn(ref))
            same += int(eq.sum())
            if fam == "integer" and not bool(eq.all()):
                sc.bad.append(f"{tag}: integer family not bit for bit ({int((~eq).sum())} elements differ)")
        sc.dev_share(f"rw persistent {fam}", same, m * n)
    sc.done()


# ------------------------------------------------------------------------------------------ x3 row kernels
@pytest.mark.parametrize("c", L.X3_EMBED_C)
def test_x3_bert_embed(c):
    """LN((word[id] + type) + pos) in f32 out, rowwise_ref's families under its tol_f32; b * l = 1, 15, 66."""
    sc, lib = _Score("x3_bert_embed"), _lib.lib()
    for fam in R.FAMILIES:
        for eps in ((1e-12, 1e-5) if fam == "tinyvar" else (1e-12,)):
            for b, l in L.X3_EMBED_BL:
                k = L.x3_embed_case(fam, b, l, c, c + l, eps)
                rows, tag = b * l, f"x3_bert_embed c={c} {fam} eps={eps} b={b} l={l}"
                word, pos = _guard_in(k["word"]), _guard_in(k["pos"][:l])
                typ, g, be = _vec(k["type0"]), _vec(k["g"]), _vec(k["b"])
                buf, y = _guard_out(rows, c, torch.float32)
                ids = k["ids"].to(DEV)
                _lib.check(lib.mmr_x3_bert_embed(_lib.ptr(ids), _lib.ptr(word), _lib.ptr(pos), _lib.ptr(typ), _lib.ptr(g),
                                                 _lib.ptr(be), _lib.ptr(y), b, l, c, eps, _lib.stream_ptr()),
                           "mmr_x3_bert_embed")
                sc.guard(tag, buf, rows, c)
                sc.dev_tol(tag, y, k["ref"].to(DEV), k["tol_f32"].to(DEV))
                if k["exact_beta"]:
                    sc.dev_equal(tag, y, k["b"].expand(rows, c).contiguous().to(DEV), "constant rows != beta")
    sc.done()


def test_x3_mean_rows():
    sc, lib = _Score("x3_mean_rows"), _lib.lib()
    for c in L.X3_MEAN_C:
        for l in L.X3_MEAN_L:
            for b in L.X3_MEAN_B:
                for extra in (False, True):
                    for fam in ("gauss", "integer"):
                        k = L.x3_mean_case(fam, b, l, c, c + l, extra)
                        x = _guard_in(k["x"].reshape(b * l, c))
                        e = _guard_in(k["extra"]) if extra else None
                        buf, y = _guard_out(b, c, torch.float32)
                        _lib.check(lib.mmr_x3_mean_rows(_lib.ptr(x), _lib.ptr(e), _lib.ptr(y), b, l, c, _lib.stream_ptr()),
                                   "mmr_x3_mean_rows")
                        tag = f"x3_mean_rows {fam} c={c} l={l} b={b} extra={extra}"
                        sc.guard(tag, buf, b, c)
                        sc.dev_tol(tag, y, k["ref"].to(DEV), k["tol"].to(DEV))
                        if k["exact"] is not None:
                            sc.dev_equal(tag, y, k["exact"].to(DEV), "integer family not bit for bit")
    sc.done()


@pytest.mark.parametrize("b,c,ldx", L.X3_GATHER)
def test_x3_gather_rows_exact(b, c, ldx):
    sc = _Score("x3_gather_rows")
    xc = torch.randn(b, c, generator=torch.Generator().manual_seed(b + c))
    x = _guard_in(xc, ldx)
    buf, y = _guard_out(b, c, torch.float32)
    ops.x3_gather_rows(x, b, c, ldx, out=y)
    sc.guard(f"x3_gather_rows c={c}", buf, b, c)
    sc.dev_equal(f"x3_gather_rows c={c}", y, xc.to(DEV), "y != x")
    sc.done()


# ------------------------------------------------------------------------------------------ rejections
def _untouched(buf):
    return bool((buf.view(torch.int32) == PAT[4]).all())


def test_rejected_launches_leave_the_output_untouched():
    """Through _lib (ops.linear_x3 falls back to linear_f32 for such shapes): a non-zero status, a message, and the
    output's bit pattern as it was."""
    lib, sp = _lib.lib(), _lib.stream_ptr()
    z = torch.zeros(8 * 2048 + 4, device=DEV)
    zh = torch.zeros(64 * 2048, dtype=torch.bfloat16, device=DEV)
    ids = torch.zeros(8, dtype=torch.int64, device=DEV)
    ybuf = torch.full((8 * 2048,), PAT[4], dtype=torch.int32, device=DEV).view(torch.float32)
    p = _lib.ptr

    def x3(cin=128, cout=32, ldx=128, ldy=32, ldr=32, res=True, x=z, bsx=0, bsw=0, nbatch=1, act=0, b=4):
        return lib.mmr_linear_x3(p(x), ldx, bsx, p(zh), p(zh), bsw, p(z), 0, p(z) if res else None, ldr, 0, p(ybuf), ldy, 0,
                                 nbatch, b, cin, cout, act, sp)

    def f32(cin=128, cout=32, ldx=128, ldy=32, ldr=32, res=True, x=z, act=0, b=4):
        return lib.mmr_linear_f32(p(x), ldx, p(z), p(z), p(z) if res else None, ldr, p(ybuf), ldy, b, cin, cout, act, sp)

    def f32b(cin=128, cout=32, ldx=128, ldy=32, ldr=32, x=z, bsx=0, bsw=0, nbatch=1, act=0, b=4):
        return lib.mmr_linear_f32_batched(p(x), ldx, bsx, p(z), bsw, p(z), 0, p(z), ldr, 0, p(ybuf), ldy, 0, nbatch, b, cin,
                                          cout, act, sp)

    def embed(c, b=2):
        return lib.mmr_x3_bert_embed(p(ids), p(z), p(z), p(z), p(z), p(z), p(ybuf), b, 2, c, 1e-12, sp)

    bad = []

    def rejected(what, status):
        msg = lib.mmr_last_error().decode(errors="replace")
        torch.cuda.synchronize()
        if status == 0 or not msg or not _untouched(ybuf):
            bad.append(f"{what}: status {status}, message {msg!r}, output untouched {_untouched(ybuf)}")

    one = z[1:]
    for fn, name, kcin in ((x3, "x3", 64), (f32, "f32", 24), (f32b, "f32_batched", 24)):
        for what, kw in (("cin", {"cin": kcin, "ldx": 128}), ("cout % 32", {"cout": 48, "ldy": 48, "ldr": 48}),
                         ("ldx % 4", {"ldx": 130}), ("ldx < cin", {"ldx": 124}), ("ldy < cout", {"ldy": 16}),
                         ("ldr < cout", {"ldr": 16}), ("x offset by one float", {"x": one}), ("act = 2", {"act": 2})):
            rejected(f"{name} {what}", fn(**kw))
    rejected("x3 bsx % 4", x3(bsx=130, nbatch=2))
    rejected("x3 bsw % 8", x3(bsw=4100, nbatch=2))
    rejected("f32_batched bsx % 4", f32b(bsx=130, nbatch=2))
    rejected("x3_bert_embed c = 1025", embed(1025))
    # the grid's y-dimension: a count above 65535 is a message, not a launch error (tiny l and c; nothing is launched)
    for what, status in (("x3 nbatch", x3(nbatch=L.MAX_GRID_Y + 1, b=1)), ("f32_batched nbatch", f32b(nbatch=L.MAX_GRID_Y + 1, b=1)),
                         ("x3_mean_rows b", lib.mmr_x3_mean_rows(p(z), None, p(ybuf), L.MAX_GRID_Y + 1, 1, 1, sp)),
                         ("mean_tokens b", lib.mmr_mean_tokens(p(zh), p(ybuf), L.MAX_GRID_Y + 1, 1, 1, sp))):
        msg = lib.mmr_last_error().decode(errors="replace")
        rejected(what, status)
        if str(L.MAX_GRID_Y) not in msg:
            bad.append(f"{what}: the message does not name the limit: {msg!r}")
    # b = 0: OK, nothing written
    for what, status in (("x3", x3(b=0)), ("f32", f32(b=0)), ("f32_batched", f32b(b=0)), ("x3_bert_embed", embed(8, b=0)),
                         ("x3_mean_rows", lib.mmr_x3_mean_rows(p(z), None, p(ybuf), 0, 1, 1, sp)),
                         ("mean_tokens", lib.mmr_mean_tokens(p(zh), p(ybuf), 0, 1, 1, sp)),
                         ("x3_gather_rows", lib.mmr_x3_gather_rows(p(z), 8, p(ybuf), 0, 8, sp)),
                         ("linear_rw", lib.mmr_linear_rw(p(zh), p(zh), None, None, p(ybuf), 0, 32, 64, sp))):
        torch.cuda.synchronize()
        if status != 0 or not _untouched(ybuf):
            bad.append(f"{what} b = 0: status {status}, output untouched {_untouched(ybuf)}")
    # the same argument lists with the offending value put right are taken
    for what, status in (("x3", x3()), ("f32", f32()), ("f32_batched", f32b()), ("x3_bert_embed", embed(8))):
        torch.cuda.synchronize()
        if status != 0 or _untouched(ybuf):
            bad.append(f"{what}: the valid call was not taken (status {status})")
    assert not bad, "\n".join(bad)


def test_zz_summary():
    """Prints the per-kernel figures of this run (worst err / tol, lowest bit share) in one line."""
    print("SMALL_LINEAR_SUMMARY " + json.dumps(SUMMARY))
    assert all(s["failed"] == 0 and not math.isnan(s["worst"]) for s in SUMMARY.values())
