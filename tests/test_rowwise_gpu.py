"""GPU: the bf16 / f32 row kernels against the f64 references and per-element bounds of rowwise_ref.py
(csrc/tower.hip layernorm_bf16, bert_embed, patch_merge_ln_g, patch_merge_ln, swin_head, mean_tokens,
l2_normalize_rows; csrc/fusion.hip ln_rows, ln_rows_v, ln_rows_s, add_pos_bf16, assemble_seq, assemble_seq8,
rows_to_f32).

Rules (rowwise_ref.py has the derivations): every element |got - ref| <= tol; a bf16 case (one family, width and
variant, its launches at every row count pooled) has >= 99 % of its elements equal to bf16_rn(ref) bit for bit;
`constant` rows equal beta exactly; add_pos / assemble_seq / rows_to_f32 are exact; the MX-fp8 outputs equal
quantize_mxfp8 of the bf16 output byte for byte.  Every output sits in a buffer with 2 guard rows in front and
behind (and guard columns where the row stride exceeds c) whose bit pattern must survive the launch; every input
sits between 2 NaN rows, so a read of a neighbouring row poisons the result.

Width -> form, from the dispatch code (a change there shows here which cases moved):

  layernorm_launch (nch = c / 8; LPR lanes per row, NC chunks per lane, 4 * 64 / LPR rows per block)
    c      nch  branch        LPR  NC  rows/block  clamped chunks
    8      1    fallback      8    3   32          lanes 1-7 hold only clamped duplicates
    24     3    fallback      8    3   32          lanes 3-7 idle
    96     12   fallback      8    3   32          second chunk of lanes 4-7
    160    20   fallback      16   3   16          second chunk of lanes 4-15
    192    24   even, <= 3    8    3   32          none
    384    48   even, <= 3    16   3   16          none
    320    40   even, <= 6    8    6   32          none
    640    80   even, <= 6    16   6   16          none
    768    96   even, <= 3    32   3   8           none
    1000   125  fallback      64   3   4           second chunk of lanes 61-63
    1280   160  even, <= 6    32   6   8           none
    1536   192  even, <= 3    64   3   4           none
    3072   384  even, <= 6    64   6   4           none
    3080   385  fallback      64   8   4           7th chunk of lanes 1-63, 8th of all
    4096   512  fallback      64   8   4           none
    (320, 640 and 1280 are there for the NC = 6 forms of 8, 16 and 32 lanes: with them every reachable
    LPR x NC instantiation is launched.)
    Q8: c = 160 / kp = 256 -> LPR 16 (two padding blocks per row); c = 992 / kp = 1024 -> LPR 64 fallback.
  bert_embed        c % 256 == 0 and c <= 1024: register path (256, 768, 1024); else generic (40, 520, 1280)
  patch_merge_ln    4c = 384: patch_merge_ln_g<16> (c = 96); 4c = 768: patch_merge_ln_g<32> (c = 192);
                    4c <= 2048: register form (c = 8, 104, 384, 512); else three passes (c = 520, 1024)
  swin_head         one form, c / 64 channels per lane (1, 3, 12, 16), 16 waves over t tokens
  ln_rows bf16      NI = ceil(c / 64) rounded up to {2, 3, 4, 6, 8, 12, 16}: 65 -> 2, 100 -> 2, 192 -> 3, 256 -> 4,
                    384 -> 6, 512 -> 8, 768 -> 12, 1000 -> 16, 1024 -> 16
  ln_rows f32       256, 1024: ln_rows_v<4>; 128, 384: ln_rows_v<2>; 8, 100: ln_rows_s<16, 8>; 200: ln_rows_s<32, 8>;
                    520 at row stride 521: ln_rows<float, float, 12>
  assemble_seq      c = 6: element-wise form; c = 64: assemble_seq8

Measured on an MI355X against the f64 reference (worst err / tol, lowest bit-equality share):
  kernel (cases)                                   err / tol   bit share
  layernorm_bf16 (330 cases, 990 launches)         0.995       0.9938
  layernorm_bf16 Q8 (20 launches)                  0.994       0.9965
  bert_embed (36 cases, 108 launches)              0.994       0.9982
  patch_merge_ln (32 cases, 96 launches)           0.995       0.9999
  ln_rows bf16 (198 cases, 594 launches)           0.994       0.9957
  ln_rows f32 (528 launches)                       0.207       -
  swin_head (1000 output checks)                   0.177       -
  mean_tokens                                      0.0043      -
  l2_normalize_rows (proj_head)                    0.140       -
  add_pos_bf16, assemble_seq, rows_to_f32          exact
The bf16 figures near 1 are the half-ulp term alone (an element whose reference sits next to a rounding tie); the
file runs in 4 s (70 tests, the slowest 0.36 s).  Scratch builds, not committed: with every bf16 store truncating,
47 of the 47 tests with a bf16 output fail (2256 failed checks); with the variance of layernorm_bf16 divided by
c - 1, all layernorm_launch tests fail (904 failed checks of 1096; the `constant` cases have xhat = 0 and cannot see
it) and nothing else does (both counted before the widths 320, 640 and 1280 were added).
"""
import json
import math

import pytest
import torch

import rowwise_ref as R
from mmr_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAT = {1: 0x5A, 2: 0x5A5A, 4: 0x5A5A5A5A}
ITYPE = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
GUARD = 2
SUMMARY = {}


def _guard_out(rows, c, dtype, ld=None):
    """(buffer of rows + 4 guard rows at row stride ld filled with the guard pattern, its [rows x c] interior)."""
    n = torch.empty((), dtype=dtype).element_size()
    buf = torch.full((rows + 2 * GUARD, ld or c), PAT[n], dtype=ITYPE[n], device=DEV).view(dtype)
    return buf, buf[GUARD:GUARD + rows, :c]


def _intact(buf, rows, c):
    g = buf.view(ITYPE[buf.element_size()]).clone()
    pat = g.new_full((), PAT[buf.element_size()])
    g[GUARD:GUARD + rows, :c] = pat
    return bool((g == pat).all())


def _guard_in(t, ld=None):
    """t (rows, c) from the CPU -> the interior of a device buffer with 2 NaN rows in front and behind."""
    if t is None:
        return None
    rows, c = t.shape
    buf = torch.full((rows + 2 * GUARD, ld or c), float("nan"), dtype=t.dtype, device=DEV)
    buf[GUARD:GUARD + rows, :c] = t.to(DEV)
    return buf[GUARD:GUARD + rows, :c]


def _vec(t):
    return _guard_in(t[None])[0]


class _Score:
    """Collects the worst err / tol, the lowest bit share and the failures of one kernel's cases."""

    def __init__(self, name):
        self.name, self.worst, self.share, self.bad, self.n = name, 0.0, 1.0, [], 0

    def tol(self, tag, got, ref, tol):
        ra = R.measure(got, ref, tol)
        self.worst = max(self.worst, ra) if ra == ra else float("nan")
        self.n += 1
        if not ra <= 1.0:
            self.bad.append(f"{tag}: err / tol {ra:.4g}")

    def bits(self, tag, got_list, ref_list):
        """One case: the launches' elements pooled."""
        got = torch.cat([g.reshape(-1) for g in got_list])
        ref = torch.cat([r.reshape(-1) for r in ref_list])
        sh = R.bit_share(got, ref)
        self.share = min(self.share, sh)
        if not sh >= R.BIT_SHARE:
            self.bad.append(f"{tag}: bit-equality share {sh:.4f} < {R.BIT_SHARE}")

    def equal(self, tag, got, exp, what):
        if not torch.equal(R.bits(got.cpu()), R.bits(exp.cpu())):
            n = int((R.bits(got.cpu()) != R.bits(exp.cpu())).sum())
            self.bad.append(f"{tag}: {what} ({n} elements differ)")

    def guard(self, tag, buf, rows, c):
        if not _intact(buf, rows, c):
            self.bad.append(f"{tag}: written outside its [{rows} x {c}] output")

    def done(self):
        s = SUMMARY.setdefault(self.name, {"worst": 0.0, "share": 1.0, "checks": 0, "failed": 0})
        s["worst"] = max(s["worst"], self.worst) if self.worst == self.worst else float("nan")
        s["share"], s["checks"], s["failed"] = min(s["share"], self.share), s["checks"] + self.n, s["failed"] + len(self.bad)
        print(json.dumps({"kernel": self.name, "worst": self.worst, "share": self.share, "checks": self.n,
                          "failed": len(self.bad)}))
        assert not self.bad, f"{len(self.bad)} failed:\n" + "\n".join(self.bad[:40])


def _bf16_case(sc, k, tag, launch, row_counts):
    """Launch on the leading rows of case k at every row count; launch(rows) -> (got (rows, c) bf16, guard buffer)."""
    gots, refs = [], []
    for rows in row_counts:
        got, buf = launch(rows)
        torch.cuda.synchronize()
        t = f"{tag} rows={rows}"
        sc.guard(t, buf, rows, k["c"])
        got = got.cpu()
        sc.tol(t, got, k["ref"][:rows], k["tol_bf16"][:rows])
        if k["exact_beta"]:
            sc.equal(t, got, R.bf16_rn(k["b_rows"].expand(k["rows"], k["c"])[:rows]), "constant rows != bf16_rn(beta)")
        gots.append(got)
        refs.append(k["ref"][:rows])
    sc.bits(tag, gots, refs)


# ------------------------------------------------------------------------------------------ layernorm_launch
def _ln_launch(k, x, r, g, b, alpha, rows):
    buf, out = _guard_out(rows, k["c"], torch.bfloat16)
    xs, rs = _guard_in(x[:rows]), (_guard_in(r[:rows]) if r is not None else None)
    if alpha is not None:
        ops.scaled_add_layernorm(xs, alpha, rs, g, b, k["eps"], out=out)
    elif rs is not None:
        ops.add_layernorm(xs, rs, g, b, k["eps"], out=out)
    else:
        ops.layernorm(xs, g, b, k["eps"], out=out)
    return out, buf


@pytest.mark.parametrize("c", R.LN_WIDTHS)
def test_layernorm_launch(c):
    """ops.layernorm / add_layernorm / scaled_add_layernorm: every family, alpha absent / 0.7, with and without a
    residual, rows 1 / 33 / 67 (a partial wave and a partial block at every rows-per-block value)."""
    sc = _Score("layernorm_bf16")
    for k in R.layernorm_cases(c):
        g, b = _vec(k["g"]), _vec(k["b"])
        alpha = k["alpha"].to(DEV) if k["alpha"] is not None else None
        tag = f"layernorm c={c} {k['fam']} eps={k['eps']} alpha={alpha is not None} res={k['r'] is not None}"
        _bf16_case(sc, k, tag, lambda rows: _ln_launch(k, k["x"], k["r"], g, b, alpha, rows), R.LN_ROWS)
    sc.done()


@pytest.mark.parametrize("c,kp", R.LN_Q8)
def test_layernorm_q8(c, kp):
    """The MX-fp8 form with a padded K (mmr_layernorm_bf16_q8p) at rows = 256: y under the same rules, the fp8
    and scale bytes equal to quantize_mxfp8(y), zero padding columns."""
    sc = _Score("layernorm_bf16 Q8")
    rows, L = 256, _lib.lib()
    nsc = (rows // 256) * (kp // 128) * 1024
    for fam in R.FAMILIES:
        for res in (False, True):
            k = R.ln_case(fam, rows, c, c + 5, res=res)
            tag = f"layernorm_q8 c={c} kp={kp} {fam} res={res}"
            x, r, g, b = _guard_in(k["x"]), _guard_in(k["r"]), _vec(k["g"]), _vec(k["b"])
            ybuf, y = _guard_out(rows, c, torch.bfloat16)
            qbuf, q = _guard_out(rows, kp, torch.uint8)
            sbuf = torch.full((nsc + 128,), PAT[1], dtype=torch.uint8, device=DEV)
            s = sbuf[64:64 + nsc]
            _lib.check(L.mmr_layernorm_bf16_q8p(_lib.ptr(x), _lib.ptr(r), _lib.ptr(g), _lib.ptr(b), _lib.ptr(y),
                                                _lib.ptr(q), _lib.ptr(s), rows, c, kp, k["eps"], _lib.stream_ptr()),
                       "mmr_layernorm_bf16_q8p")
            exp = ops.quantize_mxfp8(y.contiguous(), kp=kp)
            torch.cuda.synchronize()
            sc.guard(tag, ybuf, rows, c)
            sc.guard(tag + " q8", qbuf, rows, kp)
            if not bool((sbuf[:64] == PAT[1]).all() and (sbuf[64 + nsc:] == PAT[1]).all()):
                sc.bad.append(f"{tag}: scale bytes written outside the image")
            sc.tol(tag, y.cpu(), k["ref"], k["tol_bf16"])
            sc.bits(tag, [y.cpu()], [k["ref"]])
            if k["exact_beta"]:
                sc.equal(tag, y, R.bf16_rn(k["b"]).expand(rows, c), "constant rows != bf16_rn(beta)")
            sc.equal(tag, q, exp.q, "fp8 bytes != quantize_mxfp8(y)")
            sc.equal(tag, s, exp.s, "scale bytes != quantize_mxfp8(y)")
            if not bool((q[:, c:] == 0).all()):
                sc.bad.append(f"{tag}: padding columns not zero")
    sc.done()


def test_rejected_launches():
    """Shapes the API rightly rejects: a status and a message, no launch."""
    L = _lib.lib()
    z = torch.zeros(8 * 4104, dtype=torch.bfloat16, device=DEV)
    f = torch.zeros(4104, device=DEV)
    q = torch.zeros(256 * 1024, dtype=torch.uint8, device=DEV)

    def rejected(status, *words):
        msg = L.mmr_last_error().decode(errors="replace")
        assert status != 0 and all(w in msg for w in words), (status, msg)

    for c, word in ((12, "multiple of 8"), (4104, "> 4096"), (0, "multiple of 8")):
        rejected(L.mmr_layernorm_bf16(_lib.ptr(z), _lib.ptr(f), _lib.ptr(f), _lib.ptr(z), 8, c, 1e-5,
                                      _lib.stream_ptr()), "mmr_layernorm_bf16", word)
    # the issue's c = 1000 MX-fp8 case: c % 32 != 0 (992 is run instead); rows % 256 != 0; kp < c
    for rows, c, kp in ((256, 1000, 1024), (255, 992, 1024), (256, 992, 768)):
        rejected(L.mmr_layernorm_bf16_q8p(_lib.ptr(z), None, _lib.ptr(f), _lib.ptr(f), _lib.ptr(z), _lib.ptr(q),
                                          _lib.ptr(q), rows, c, kp, 1e-5, _lib.stream_ptr()), "MX-fp8", f"c={c}")
    rejected(L.mmr_swin_head(_lib.ptr(z), _lib.ptr(f), _lib.ptr(f), None, _lib.ptr(f), _lib.ptr(f), 1, 2, 100, 1e-5,
                             _lib.stream_ptr()), "mmr_swin_head", "multiple of 64")
    rejected(L.mmr_swin_head(_lib.ptr(z), _lib.ptr(f), _lib.ptr(f), None, _lib.ptr(f), _lib.ptr(f), 1, 2, 1088, 1e-5,
                             _lib.stream_ptr()), "mmr_swin_head", "<= 1024")
    rejected(L.mmr_ln_rows(_lib.ptr(f), 1032, None, None, 0, _lib.ptr(f), _lib.ptr(f), None, 0, None, _lib.ptr(f),
                           1032, 1, 1032, 1e-5, 0, 1, 1, _lib.stream_ptr()), "mmr_ln_rows", "c <= 1024")
    rejected(L.mmr_patch_merge_ln(_lib.ptr(z), _lib.ptr(f), _lib.ptr(f), _lib.ptr(z), 1, 2, 12, 1e-5,
                                  _lib.stream_ptr()), "mmr_patch_merge_ln", "c=12")
    rejected(L.mmr_add_pos_bf16(_lib.ptr(f), 1, _lib.ptr(f), _lib.ptr(z), 4, 2, 12, _lib.stream_ptr()),
             "mmr_add_pos_bf16")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ bert_embed
@pytest.mark.parametrize("c", R.EMBED_WIDTHS)
def test_bert_embed(c):
    """Register path (c % 256 == 0, c <= 1024) and generic path; b * l = 1, 15, 66 (l = 1, 5, 33); ids hold 0,
    vocab - 1 and repeats; the reference sums word + pos + type in f32 in the kernel's order."""
    sc, L = _Score("bert_embed"), _lib.lib()
    for fam in R.FAMILIES:
        for eps in ((1e-12, 1e-5) if fam == "tinyvar" else (1e-12,)):
            gots, refs = [], []
            for b, l in R.EMBED_BL:
                k = R.embed_case(fam, b, l, c, c + l, eps)
                rows, tag = b * l, f"bert_embed c={c} {fam} eps={eps} b={b} l={l}"
                word, pos = _guard_in(k["word"]), _guard_in(k["pos"][:l])
                typ, g, be = _vec(k["type0"]), _vec(k["g"]), _vec(k["b"])
                buf, y = _guard_out(rows, c, torch.bfloat16)
                ids = k["ids"].to(DEV)
                _lib.check(L.mmr_bert_embed(_lib.ptr(ids), _lib.ptr(word), _lib.ptr(pos), _lib.ptr(typ),
                                            _lib.ptr(g), _lib.ptr(be), _lib.ptr(y), b, l, c, eps, _lib.stream_ptr()),
                           "mmr_bert_embed")
                torch.cuda.synchronize()
                sc.guard(tag, buf, rows, c)
                got = y.cpu()
                sc.tol(tag, got, k["ref"], k["tol_bf16"])
                if k["exact_beta"]:
                    sc.equal(tag, got, R.bf16_rn(k["b"]).expand(rows, c), "constant rows != bf16_rn(beta)")
                gots.append(got)
                refs.append(k["ref"])
            sc.bits(f"bert_embed c={c} {fam} eps={eps}", gots, refs)
    sc.done()


# ------------------------------------------------------------------------------------------ patch_merge_ln
@pytest.mark.parametrize("c", R.MERGE_WIDTHS)
def test_patch_merge_ln(c):
    """All four forms at 1, 9 and 27 merged rows; the four source pixels carry different families (timm's
    quadrant order x[0::2,0::2], x[1::2,0::2], x[0::2,1::2], x[1::2,1::2]), and every rotation of them is run so
    that each family meets each quadrant."""
    sc, L = _Score("patch_merge_ln"), _lib.lib()
    for rot in range(4):
        quads = R.MERGE_QUADS[rot:] + R.MERGE_QUADS[:rot]
        gots, refs = [], []
        for B, H in R.MERGE_BH:
            k = R.merge_case(B, H, c, c + rot, quads=quads)
            rows, tag = k["rows"], f"patch_merge_ln c={c} B={B} H={H} quads={quads}"
            x = _guard_in(k["x"].view(B * H * H, c))
            g, b = _vec(k["g"]), _vec(k["b"])
            buf, y = _guard_out(rows, 4 * c, torch.bfloat16)
            _lib.check(L.mmr_patch_merge_ln(_lib.ptr(x), _lib.ptr(g), _lib.ptr(b), _lib.ptr(y), B, H, c, k["eps"],
                                            _lib.stream_ptr()), "mmr_patch_merge_ln")
            torch.cuda.synchronize()
            sc.guard(tag, buf, rows, 4 * c)
            got = y.cpu()
            sc.tol(tag, got, k["ref"], k["tol_bf16"])
            gots.append(got)
            refs.append(k["ref"])
        sc.bits(f"patch_merge_ln c={c} quads={quads}", gots, refs)
    sc.done()


# ------------------------------------------------------------------------------------------ swin_head
@pytest.mark.parametrize("c", R.HEAD_WIDTHS)
def test_swin_head(c):
    """t fewer than, equal to and more than the 16 waves, b = 1 / 3, with and without the patches output; all
    three f32 outputs against LN(LN(x)) and its token means in f64."""
    sc, L = _Score("swin_head"), _lib.lib()
    for fam in R.FAMILIES:
        for t in R.HEAD_T:
            for b in R.HEAD_B:
                k = R.head_case(fam, b, t, c, c + t)
                x, g, be = _guard_in(k["x"].reshape(b * t, c)), _vec(k["g"]), _vec(k["b_"])
                for want in (True, False):
                    tag = f"swin_head c={c} {fam} t={t} b={b} patches={want}"
                    pbuf, p = _guard_out(b * t, c, torch.float32)
                    gbuf, gl = _guard_out(b, c, torch.float32)
                    obuf, po = _guard_out(b, c, torch.float32)
                    _lib.check(L.mmr_swin_head(_lib.ptr(x), _lib.ptr(g), _lib.ptr(be), _lib.ptr(p) if want else None,
                                               _lib.ptr(gl), _lib.ptr(po), b, t, c, k["eps"], _lib.stream_ptr()),
                               "mmr_swin_head")
                    torch.cuda.synchronize()
                    sc.guard(tag + " patches", pbuf, b * t if want else 0, c)
                    sc.guard(tag + " global", gbuf, b, c)
                    sc.guard(tag + " pool", obuf, b, c)
                    if want:
                        sc.tol(tag + " patches", p.cpu().view(b, t, c), k["patches"], k["tol_patches"])
                    sc.tol(tag + " global", gl.cpu(), k["glob"], k["tol_glob"])
                    sc.tol(tag + " pool", po.cpu(), k["pool"], k["tol_pool"])
    sc.done()


# ------------------------------------------------------------------------------------------ mean_tokens
def test_mean_tokens():
    sc, L = _Score("mean_tokens"), _lib.lib()
    for c in R.MEAN_WIDTHS:
        for l in R.MEAN_L:
            k = R.mean_case(2, l, c, c + l)
            x = _guard_in(k["x"].reshape(2 * l, c))
            buf, y = _guard_out(2, c, torch.float32)
            _lib.check(L.mmr_mean_tokens(_lib.ptr(x), _lib.ptr(y), 2, l, c, _lib.stream_ptr()), "mmr_mean_tokens")
            torch.cuda.synchronize()
            tag = f"mean_tokens c={c} l={l}"
            sc.guard(tag, buf, 2, c)
            sc.tol(tag, y.cpu(), k["ref"], k["tol"])
    sc.done()


# ------------------------------------------------------------------------------------------ ln_rows
def _lnrows_launch(k, dev, rows, ld_x, ld_y):
    c, dt = k["c"], k["x"].dtype
    buf, out = _guard_out(rows, c, dt, ld_y)
    x = _guard_in(k["x"][:rows], ld_x)
    r = _guard_in(k["r"][:rows]) if k["r"] is not None else None
    post = _guard_in(k["post"][:rows]) if k["post"] is not None else None
    ops.ln_rows(x, dev["g"], dev["b"], k["eps"], alpha=dev["alpha"], residual=r, post=post, post_scale=dev["ps"],
                out=out, groups=k["groups"], group_div=k["group_div"])
    return out, buf


def _lnrows_dev(k):
    two = (lambda t: t if t.dim() == 2 else t[None])
    return {"g": _guard_in(two(k["g"])), "b": _guard_in(two(k["b"])),
            "alpha": k["alpha"].to(DEV) if k["alpha"] is not None else None,
            "ps": k["post_scale"].to(DEV) if k["post_scale"] is not None else None}


def _lnrows_tag(k):
    return (f"ln_rows {str(k['x'].dtype)[6:]} c={k['c']} {k['fam']} eps={k['eps']} groups={k['groups']} "
            f"div={k['group_div']} alpha={k['alpha'] is not None} res={k['r'] is not None} post={k['post'] is not None}")


@pytest.mark.parametrize("c", R.LNROWS_BF16)
def test_ln_rows_bf16(c):
    """One width per NI instantiation plus ragged widths; rows 1 / 9 / 13; groups = 3 with group_div 1 / 2 (gamma,
    beta, alpha and post-scale differ per group); residual and post present and absent; output row stride c + 1."""
    sc = _Score("ln_rows bf16")
    for k in R.lnrows_cases(c, torch.bfloat16):
        dev = _lnrows_dev(k)
        _bf16_case(sc, k, _lnrows_tag(k), lambda rows: _lnrows_launch(k, dev, rows, c, c + 1), R.LNROWS_ROWS)
    sc.done()


@pytest.mark.parametrize("c,extra", R.LNROWS_F32)
def test_ln_rows_f32(c, extra):
    """f32 I/O: the 4-wide, 2-wide, 16-lane short, 32-lane short and scalar (odd row stride) forms."""
    sc = _Score("ln_rows f32")
    for k in R.lnrows_cases(c, torch.float32):
        dev, tag = _lnrows_dev(k), _lnrows_tag(k)
        for rows in R.LNROWS_ROWS:
            out, buf = _lnrows_launch(k, dev, rows, c + extra, c + extra)
            torch.cuda.synchronize()
            t = f"{tag} rows={rows}"
            sc.guard(t, buf, rows, c)
            sc.tol(t, out.cpu(), k["ref"][:rows], k["tol_f32"][:rows])
            if k["exact_beta"]:
                sc.equal(t, out, k["b_rows"].float().expand(k["rows"], c)[:rows], "constant rows != beta")
    sc.done()


# ------------------------------------------------------------------------------------------ exact kernels
@pytest.mark.parametrize("c", (8, 96, 1000))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("f32", "bf16"))
def test_add_pos_exact(dtype, c):
    """y = bf16_rn(fl32(x + pos[row % l])) bit for bit; l divides neither row count."""
    sc, L = _Score("add_pos_bf16"), _lib.lib()
    for rows, l in ((13, 5), (67, 7)):
        g_ = torch.Generator().manual_seed(rows + c)
        xc = (torch.randn(rows, c, generator=g_) * 3).to(dtype)
        pc = torch.randn(l, c, generator=g_)
        exp = (xc.float() + pc[torch.arange(rows) % l]).to(torch.bfloat16)
        x, pos = _guard_in(xc), _guard_in(pc)
        buf, y = _guard_out(rows, c, torch.bfloat16)
        _lib.check(L.mmr_add_pos_bf16(_lib.ptr(x), int(dtype == torch.float32), _lib.ptr(pos), _lib.ptr(y), rows, l, c,
                                      _lib.stream_ptr()), "mmr_add_pos_bf16")
        torch.cuda.synchronize()
        tag = f"add_pos {dtype} c={c} rows={rows} l={l}"
        sc.guard(tag, buf, rows, c)
        sc.equal(tag, y, exp, "y != bf16_rn(fl32(x + pos))")
        sc.n += 1
    sc.done()


@pytest.mark.parametrize("c", (6, 64))
@pytest.mark.parametrize("np_", (1, 5))
def test_assemble_seq_exact(np_, c):
    """seq = bf16_rn(fl32([x1; pf; x2] + pe)) bit for bit: the element-wise form (c = 6) and assemble_seq8 (c = 64)."""
    sc, L, B = _Score("assemble_seq"), _lib.lib(), 3
    g_ = torch.Generator().manual_seed(np_ + c)
    x1, x2 = torch.randn(B, c, generator=g_), torch.randn(B, c, generator=g_) * 5
    pf = torch.randn(B * np_, c, generator=g_).to(torch.bfloat16)
    pe = torch.randn(np_ + 2, c, generator=g_)
    exp = (torch.cat([x1[:, None], pf.float().view(B, np_, c), x2[:, None]], 1) + pe).to(torch.bfloat16)
    rows = B * (np_ + 2)
    buf, y = _guard_out(rows, c, torch.bfloat16)
    dx1, dpf, dx2, dpe = _guard_in(x1), _guard_in(pf), _guard_in(x2), _guard_in(pe)
    _lib.check(L.mmr_assemble_seq(_lib.ptr(dx1), _lib.ptr(dpf), _lib.ptr(dx2), _lib.ptr(dpe), _lib.ptr(y), B, np_, c,
                                  _lib.stream_ptr()), "mmr_assemble_seq")
    torch.cuda.synchronize()
    sc.guard(f"assemble_seq c={c} np={np_}", buf, rows, c)
    sc.equal(f"assemble_seq c={c} np={np_}", y, exp.view(rows, c), "seq != bf16_rn(fl32(cat + pe))")
    sc.n += 1
    sc.done()


@pytest.mark.parametrize("b,c,ldx", ((5, 96, 200), (3, 7, 9), (2, 300, 301)))
def test_rows_to_f32_exact(b, c, ldx):
    """Strided bf16 rows widened to f32: exact; row stride above c."""
    sc = _Score("rows_to_f32")
    xc = torch.randn(b, c, generator=torch.Generator().manual_seed(b + c)).to(torch.bfloat16)
    x = _guard_in(xc, ldx)
    buf, y = _guard_out(b, c, torch.float32)
    ops.rows_to_f32(x, b, c, ldx, out=y)
    torch.cuda.synchronize()
    sc.guard(f"rows_to_f32 c={c}", buf, b, c)
    sc.equal(f"rows_to_f32 c={c}", y, xc.float(), "y != f32(x)")
    sc.n += 1
    sc.done()


# ------------------------------------------------------------------------------------------ proj_head l2norm
@pytest.mark.parametrize("b", (1, 5))
def test_proj_head_l2norm(b):
    """l2_normalize_rows behind proj_head(l2norm=True), d = 32, cin = 16: every element within the f32 bound of
    y / |y| (y the same launch without the normalisation, the norm in f64), every row of unit norm, and an
    all-zero input with zero biases gives zeros, not NaN.
    Bound: |y|^2 is 32 products and a 6-level tree (<= 8 roundings, half of that in the root), rsqrtf <= 2 ulp,
    one product: <= 16 * 2^-24 relative, plus 2^-23 |ref|."""
    sc, L, d, cin = _Score("l2_normalize_rows"), _lib.lib(), 32, 16
    g_ = torch.Generator().manual_seed(b)
    xc, wc, bc = torch.randn(b, cin, generator=g_), torch.randn(d, cin, generator=g_), torch.randn(d, generator=g_)

    def run(x, w, bias, l2):
        buf, y = _guard_out(b, d, torch.float32)
        _lib.check(L.mmr_proj_head(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), None, None, None, None, _lib.ptr(y), b, cin,
                                   d, l2, _lib.stream_ptr()), "mmr_proj_head")
        torch.cuda.synchronize()
        sc.guard(f"proj_head b={b} l2norm={l2}", buf, b, d)
        return y.cpu()

    x, w, bias = _guard_in(xc), _guard_in(wc), _vec(bc)
    raw, got = run(x, w, bias, 0).double(), run(x, w, bias, 1)
    ref = raw / raw.norm(dim=1, keepdim=True)
    sc.tol(f"proj_head b={b}", got, ref, (2.0 ** -23 + 16 * R.U24) * ref.abs())
    norm = got.double().norm(dim=1)
    sc.tol(f"proj_head b={b} unit norm", norm, torch.ones(b, dtype=torch.float64), torch.full((b,), 16 * R.U24,
                                                                                              dtype=torch.float64))
    zero = run(_guard_in(torch.zeros(b, cin)), w, _vec(torch.zeros(d)), 1)
    sc.equal(f"proj_head b={b} zero input", zero, torch.zeros(b, d), "zero rows must stay zero")
    sc.done()


def test_zz_summary():
    """Prints the per-kernel figures of this run (worst err / tol, lowest bit share) in one line."""
    print("ROWWISE_SUMMARY " + json.dumps(SUMMARY))
    assert all(s["failed"] == 0 and not math.isnan(s["worst"]) for s in SUMMARY.values())
