"""Exact references, operands built by the test, a kernel model and its mutants for the MX-fp8 forms of the 8-phase GEMM
(csrc/gemm.hip gemm_bf16_tn_p8<FP8>: mmr_linear_mxfp8 on 256 x 192 tiles, weight layout 1, and 256 x 256 tiles, layout 2;
mmr_linear_mxfp8_q8, the OUT8 form whose epilogue requantises the output), shared by test_mxfp8_exact_cpu.py and
test_mxfp8_exact_gpu.py.  The helpers (bits, rne_bits, verify_exact, verify_gelu, gelu_ref_tol, GUARD, SENT, _hash) are
gemm_routes_ref's.

Operands are built here, not by the quantiser under test: element values on the e4m3 grid encoded by e4m3_encode
(pinned to torch.float8_e4m3fn on the CPU), one exponent per (row, 32-block) written as an E8M0 byte (e + 127) through
oracle.mxfp8.scale_offsets into the GEMM's image order, wrapped in ops.MXFP8.

Families (a hash of the indices, so any row / column range of a case is generated alone):
  exact   act = 0.  Elements integers in [-4, 4]; the x exponent of (row, k-block) and the w exponent of (column,
          k-block) hashed in [-2, 2], so every (row, block) has its own scale and adjacent blocks, adjacent K-tiles,
          the two 128-row halves, the wave columns and adjacent panels all differ; bias multiples of 1/4 in [-8, 8],
          residual integers in [-64, 64].  Every product is a multiple of 2^-4 below 2^8 and every partial sum up to
          kp = 1024 below 2^18: 22 bits, so the f32 dot product is exact in any order (at most 12 bits between its
          smallest and largest product, inside what tools/mfma_fp8_probe.hip found exact) and so are the two epilogue
          adds: the output is expected BIT FOR BIT, rne_bits of the exact value (round1: the 8-phase kernel adds the
          residual in f32 and rounds once).
          Specials: ~1.6 % of the x blocks and the whole of row ZERO_ROW are zero with scale byte 0; blocks past k
          (kp > k) are zero with scale byte 0 (what the quantiser writes for a zero block).  Extreme scales, a case's
          flavour: "xlo" gives the x rows EXT_ROWS exponent -100 + h and the w columns EXT_COLS +100 + h, "xhi" the
          reverse (both at once would overflow where +100 meets +100).  Extreme against extreme the sums stay in the
          narrow range; extreme against ordinary the accumulator is ~2^-100 or ~2^+100, still exact, and the epilogue
          adds round once each exactly as the f32 reference below does (acc + b, then + r, the kernel's order).
  out8    the exact family with every w column's exponents moved by g(column / 32) hashed in [-3, 3] and its bias
          times 2^g: adjacent 32-column blocks of an output row take different output exponents.  Bias entries of the
          first three 32-column blocks are replaced so that, on the all-zero row (output = bias), the block amax is
          1.75 (the 0x600000 threshold mantissa), the bf16 value below it and the one above it.  Without a bias the
          zero row gives all-zero output blocks.  e4m3 ties occur by themselves (integers against a step of 2 or
          more) and are counted on the CPU.  Expected: oracle.mxfp8.quantize of bf16_rn of the exact pre-activation,
          bytes and scale image bit for bit.
  gelu    act = 1.  Elements in {-1, 0, 1} with density sqrt(6 / k), exponents in {-1, 0, 1}, bias and residual
          multiples of 1/8: z = acc + b is an exact multiple of 1/8, |z| <= ZMAX asserted; per element
          gemm_routes_ref.gelu_ref_tol with the 8-phase entries (gelu_fast2, round1).  For OUT8 + GELU the existing
          boundary-aware check of test_mxfp8_gpu.py on this exact z (no accumulation term in its slack).

model() restates the kernel: accumulation K-tile by K-tile with the scales read from the images through the offsets,
the epilogue in f32, round1, the OUT8 requantiser (integer restatement of the 32-block amax, exponent and e4m3
rounding, independent of the oracle's), written into sentinel-filled buffers with guards.  Mutants (wherever one
changes the model's output, the checks fail): see MUTANTS."""
import collections

import numpy as np
import torch

import gemm_routes_ref as G
from oracle import mxfp8 as mx

GUARD, SENT = G.GUARD, G.SENT
SENT8 = 0x7F                    # e4m3 NaN: no finite value converts to it
SENT_S = 0xFF                   # E8M0 NaN: the exponent clamp ends at byte 253
GUARD_S = 64                    # guard bytes on each side of a scale image
ZERO_ROW = 5
EXT_ROWS, EXT_COLS = (3, 130), (2, 100)       # both 128-row halves; two wave columns
TN = {1: 192, 2: 256}

Case = collections.namedtuple("Case", "layout m n k kp extreme note")
CASES = (
    Case(1, 256, 192, 256, 256, "xlo", "one tile, seven idle workgroups, two K-tiles"),
    Case(2, 256, 256, 256, 256, "xhi", "one tile, seven idle workgroups, two K-tiles"),
    Case(1, 768, 576, 768, 768, "xhi", "nine tiles, uneven XCD shares, six K-tiles"),
    Case(2, 768, 768, 768, 768, "xlo", "nine tiles, uneven XCD shares, six K-tiles"),
    Case(1, 4096, 4416, 256, 256, None, "368 tiles, 1-2 per workgroup"),
    Case(2, 4096, 4352, 256, 256, None, "272 tiles, 1-2 per workgroup"),
    Case(1, 256, 192, 264, 512, None, "kp = 512 operand with k = 264: zero-padded tail blocks"),
    Case(2, 256, 256, 264, 512, None, "kp = 512 operand with k = 264: zero-padded tail blocks"),
)
BIG_BF16 = (Case(1, 8192, 8448, 256, 256, None, "138 MB of bf16: non-temporal LDS-staged stores"),
            Case(2, 8192, 8448, 256, 256, None, "138 MB of bf16: non-temporal LDS-staged stores"))
BIG_OUT8 = Case(2, 8192, 16640, 256, 256, None, "136 MB of bytes: non-temporal OUT8 stores")
EPILOGUES = G.EPILOGUES                                     # bf16 out
EPILOGUES8 = tuple(e for e in G.EPILOGUES if not e[3])      # OUT8: none, bias, bias + GELU
MUTANTS = ("kperm", "nextkt", "half", "wavecol", "panel", "mask7", "lastkt", "tileswap", "skiptile", "trunc",
           "biascol", "round", "actlate", "amax16", "rdrr", "f32quant")
MUTANTS8 = ("amax16", "rdrr", "f32quant")                   # OUT8 only
MUTANTS16 = ("trunc", "round", "actlate")                   # bf16 out only (OUT8 takes no residual)


def case_id(c):
    return f"l{c.layout}-{c.m}x{c.n}x{c.k}" + (f"p{c.kp}" if c.kp != c.k else "")


def cut(c):
    """(rows, cols) of a case as the CPU tests run it: at most two row panels and two tile columns."""
    return min(c.m, 512), min(c.n, 2 * TN[c.layout])


# ---------------------------------------------------------------------------------------------- e4m3
def e4m3_encode(v):
    """f32 tensor, |v| <= 448 -> OCP e4m3fn bytes (uint8), round to nearest even, in integer arithmetic on the f32
    bits (values on the grid encode exactly; the sign of a zero is kept)."""
    v = v.float().contiguous()
    b = v.view(torch.int32)
    sign = (b >> 24) & 0x80
    ab = b & 0x7FFFFFFF
    normal = ((ab + 0x7FFFF + ((ab >> 20) & 1)) >> 20) - (120 << 3)           # exponent rebias 127 -> 7
    sub = torch.round(v.abs() * 512.0).to(torch.int32)                          # step 2^-9; 8 = the smallest normal
    return (sign | torch.where(ab >= 0x3C800000, normal, sub)).to(torch.uint8)  # 0x3C800000 = 2^-6


# ---------------------------------------------------------------------------------------------- data
def density(k):
    return min(1.0, (6.0 / k) ** 0.5)


def _pow2(e):
    """2^e in f64 from the exponent field (-1022 <= e <= 1023): exact on every device (a device's ldexp / pow is not:
    it returned 2^e off by an ulp for some e, which showed as -1e-13 where a sum cancels)."""
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def gcol(c, cols, device="cpu"):
    """out8 family: the exponent shift of each column's 32-column block, in [-3, 3]."""
    j = torch.arange(cols, dtype=torch.int64, device=device)
    return (G._hash(j // 32, 0, _salt(c, "out8") + 7) % 7 - 3)


def _salt(c, fam):
    return (c.m * 31 + c.n * 17 + c.kp * 7 + c.k * 3 + {"exact": 0, "out8": 0, "gelu": 5}[fam]) % 1000003


def operands(c, fam, rows=None, cols=None, row0=0, col0=0, device="cpu", parts="xwbr"):
    """Rows row0 .. row0 + rows and columns col0 .. col0 + cols of a case's operands: xq (rows, kp) f32 element values,
    xe (rows, kp / 32) int64 exponents (-127: scale byte 0), wq / we the same for the columns, b (cols,) f32, r (rows,
    cols) f32."""
    rows, cols = c.m if rows is None else rows, c.n if cols is None else cols
    s = _salt(c, fam)
    ar = (lambda a, cnt: torch.arange(a, a + cnt, dtype=torch.int64, device=device))
    i, j = ar(row0, rows)[:, None], ar(col0, cols)[:, None]
    kk, blk = ar(0, c.kp)[None, :], ar(0, c.kp // 32)[None, :]
    live_k, live_b = kk < c.k, blk * 32 < c.k
    out = {}
    if fam == "gelu":
        thr = int(density(c.k) * 4096)

        def elem(h):
            return torch.where((h & 4095) < thr, 1 - 2 * ((h >> 12) & 1), torch.zeros_like(h))

        def expo(h):
            return h % 3 - 1
    else:
        def elem(h):
            return h % 9 - 4

        def expo(h):
            return h % 5 - 2
    if "x" in parts:
        xq, xe = elem(G._hash(i, kk, s + 1)) * live_k, expo(G._hash(i, blk, s + 5))
        if fam != "gelu":
            zero = (G._hash(i, blk, s + 8) % 61 == 0) | (i == ZERO_ROW)
            if c.extreme:
                ext = sum(i == t for t in EXT_ROWS).bool()
                xe = xe + ext * (-100 if c.extreme == "xlo" else 100)
            xq = xq * ~zero.repeat_interleave(32, dim=1)
            xe = torch.where(zero, torch.full_like(xe, -127), xe)
        out["xq"], out["xe"] = xq.float(), torch.where(live_b, xe, torch.full_like(xe, -127))
    if "w" in parts:
        wq, we = elem(G._hash(j, kk, s + 2)) * live_k, expo(G._hash(j, blk, s + 6))
        if fam != "gelu" and c.extreme:
            ext = sum(j == t for t in EXT_COLS).bool()
            we = we + ext * (100 if c.extreme == "xlo" else -100)
        if fam == "out8":
            we = we + (G._hash(j // 32, 0, s + 7) % 7 - 3)
        out["wq"], out["we"] = wq.float(), torch.where(live_b, we, torch.full_like(we, -127))
    if "b" in parts:
        jj = j[:, 0]
        b = (G._hash(jj, 0, s + 3) % 65 - 32).double() / (8 if fam == "gelu" else 4)
        if fam == "out8":
            b = b * _pow2(G._hash(jj // 32, 0, s + 7) % 7 - 3)
            # the zero row's output is the bias: block amax at the threshold mantissa 1.75, one bf16 ulp below, one above
            for blk32, top in ((0, 1.75), (1, 1.75 - 2.0 ** -7), (2, 1.75 + 2.0 ** -7)):
                inb = (jj // 32 == blk32)
                b = torch.where(inb, b.clamp(-1, 1) * 0.25, b)
                b = torch.where(jj == blk32 * 32 + 9, torch.full_like(b, top * 2.0 ** (blk32 - 1)), b)
        out["b"] = b.float()
    if "r" in parts:
        out["r"] = (G._hash(i, ar(col0, cols)[None, :], s + 4) % 129 - 64).float() / (8 if fam == "gelu" else 1)
    return out


def image(e, layout):
    """Exponents (rows, kp / 32) -> the scale image (uint8 numpy), bytes e + 127 at oracle.mxfp8.scale_offsets."""
    e = e.cpu().numpy()
    rows, kp = e.shape[0], e.shape[1] * 32
    pr = 192 if layout == 1 else 256
    assert rows % pr == 0 and kp % 128 == 0
    img = np.zeros(rows // pr * (kp // 128) * 1024, np.uint8)
    off = mx.scale_offsets(rows, kp, layout)
    assert np.unique(off).size == off.size and off.max() < img.size      # layout 1 uses 768 of a K-tile's 1024 bytes
    img[off] = (e + 127).astype(np.uint8)
    return img


def dense(q, e):
    """Element values and block exponents -> the operand in f64 (exact)."""
    return q.double() * _pow2(e.clamp(min=-1000)).repeat_interleave(32, dim=1)


def exact_acc(xd, wd):
    """x w^T of dense f64 operands (every partial sum an integer multiple of one power of two within 53 bits: exact in
    any order)."""
    return xd @ wd.t()


def preact(d):
    """The exact accumulator of a set of operands in f64."""
    return exact_acc(dense(d["xq"], d["xe"]), dense(d["wq"], d["we"]))


def ordinary(c, rows, cols, row0=0, col0=0, device="cpu"):
    """(rows, cols) mask of the outputs that meet no extreme scale."""
    i = torch.arange(row0, row0 + rows, device=device)[:, None]
    j = torch.arange(col0, col0 + cols, device=device)[None, :]
    if not c.extreme:
        return torch.ones(rows, cols, dtype=torch.bool, device=device)
    return ~(sum(i == t for t in EXT_ROWS).bool() | sum(j == t for t in EXT_COLS).bool())


# ---------------------------------------------------------------------------------------------- expectations
def pre_f32(acc, b, r=None):
    """f32 value before the output rounding, in the kernel's order: (acc + b) + r.  Exact on ordinary outputs
    (asserted by the tests: equal to the f64 sum); one correctly rounded add each where an extreme scale is met."""
    v = acc.float()
    if b is not None:
        v = v + b
    return v if r is None else v + r


def expected_bits(acc, b, r=None):
    return G.rne_bits(pre_f32(acc, b, r))


def expected_out8(vb):
    """bf16-rounded outputs (m, n) f32 -> (bytes (m, n) uint8, scale image uint8 numpy) by the oracle."""
    m, n = vb.shape
    q, e = mx.quantize(vb.cpu().numpy(), n)
    img = np.zeros(m // 256 * (n // 128) * 1024, np.uint8)
    img[mx.scale_offsets(m, n, 0)] = (e + 127).astype(np.uint8)
    return e4m3_encode(torch.from_numpy(q)), img


def verify_bytes(buf, m, exp):
    """OUT8 bytes: buf (m + 2 GUARD, n) uint8 -> (guards intact, sentinels inside, bytes != expected)."""
    mid = buf[GUARD:GUARD + m]
    return (bool((buf[:GUARD] == SENT8).all() and (buf[GUARD + m:] == SENT8).all()), int((mid == SENT8).sum()),
            int((mid != exp).sum()))


def verify_scales(sbuf, exp):
    """Scale image between GUARD_S guard bytes (uint8 tensor) -> (guards intact, bytes never written, bytes != exp)."""
    mid = sbuf[GUARD_S:sbuf.numel() - GUARD_S]
    return (bool((sbuf[:GUARD_S] == SENT_S).all() and (sbuf[sbuf.numel() - GUARD_S:] == SENT_S).all()),
            int((mid == SENT_S).sum()), int((mid != exp).sum()))


# ---------------------------------------------------------------------------------------------- kernel model
def _read_scales(img, rows, kp, layout, mutant, side):
    """The exponents the kernel applies to (row, block), read from the image through the offsets."""
    pr = 192 if layout == 1 else 256
    r = np.arange(rows)[:, None]
    blk = np.arange(kp // 32)[None, :]
    kt, fq = blk // 4, blk % 4
    if mutant == "kperm" and side == "x":
        fq = 3 - fq
    if mutant == "nextkt":
        kt = (kt + 1) % (kp // 128)
    if mutant == "half" and side == "x":
        r = r ^ 128
    if mutant == "wavecol" and side == "w":
        r = r // pr * pr + (r % pr + pr // 4) % pr
    if mutant == "panel":
        r = np.where(r // pr == 1, r - pr, r)
    off = mx.scale_offsets(rows, kp, layout)[np.broadcast_to(r, (rows, kp // 32)), np.broadcast_to(kt * 4 + fq, (rows, kp // 32))]
    by = img[off].astype(np.int64)
    if mutant == "mask7":
        by = by & 0x7F
    return torch.from_numpy(by - 127)


def requantise(v, mutant=None):
    """The OUT8 epilogue on staged values v (m, n) f32 -> (bytes (m, n) uint8, scale image with SENT_S where nothing was
    written): amax over a row's 32 columns, e = exponent(amax) - 8 (+ 1 above mantissa 1.75), clamped, v 2^-e rounded
    to e4m3."""
    m, n = v.shape
    grp = 16 if mutant == "amax16" else 32
    ab = v.abs().view(m, n // grp, grp).amax(-1).contiguous().view(torch.int32)
    ex = (((ab >> 23) & 255) - 127 - 8 + ((ab & 0x7FFFFF) > 0x600000).int()).clamp(-127, 126)
    q = e4m3_encode(torch.ldexp(v, -ex.repeat_interleave(grp, dim=1)))
    if mutant == "amax16":
        ex = ex[:, ::2]
    off = mx.scale_offsets(m, n, 0)
    if mutant == "rdrr":            # i (the round) and fr (the row of the round) exchanged
        r = np.arange(m)[:, None]
        blk = np.arange(n // 32)[None, :]
        rr = r % 256
        off = (r // 256 * (n // 128) + blk // 4) * 1024 + (((rr // 128) * 4 + blk % 4) * 16 + (rr % 128) // 16) * 8 + rr % 16
    img = np.full(m // 256 * (n // 128) * 1024, SENT_S, np.uint8)
    img[off] = (ex + 127).numpy().astype(np.uint8)
    return q, img


def model(c, d, xs, ws, epi, mutant=None, out8=False):
    """The kernel on the CPU.  d: operands (cut), xs / ws: their scale images.  -> bf16 out: the (rows + 2 GUARD, cols)
    int16 buffer; OUT8: (the uint8 byte buffer with guard rows, the scale image between GUARD_S guard bytes)."""
    _, act, hb, hr, inplace = epi
    rows, cols, tn = d["xq"].shape[0], d["wq"].shape[0], TN[c.layout]
    xe = _read_scales(xs, rows, c.kp, 0, mutant, "x")
    we = _read_scales(ws, cols, c.kp, c.layout, mutant, "w")
    xd, wd = dense(d["xq"], xe), dense(d["wq"], we)
    acc = torch.zeros(rows, cols, dtype=torch.float64)
    for kt in range(c.kp // 128 - (1 if mutant == "lastkt" else 0)):
        acc += xd[:, kt * 128:(kt + 1) * 128] @ wd[:, kt * 128:(kt + 1) * 128].t()
    b = d["b"] if hb else None
    if hb and mutant == "biascol":
        b = b[(torch.arange(cols) + tn) % cols]
    r = d["r"] if hr else None

    def gelu(v):
        if out8:
            return torch.from_numpy(mx.gelu_q8(v.numpy()))
        return torch.from_numpy(G.gelu_fast_np(v.numpy(), "fast2", np.float32))

    v = acc.float()
    if b is not None:
        v = v + b
    if act and mutant != "actlate":
        v = gelu(v)
    if r is not None:
        v = (G.bf2f(G.rne_bits(v)) if mutant == "round" else v) + r
    if act and mutant == "actlate":
        v = gelu(v)
    tiles = [(i, i + 256, j, j + tn) for i in range(0, rows, 256) for j in range(0, cols, tn)]

    def walk(out, start):
        if mutant == "tileswap" and len(tiles) > 1:
            (a0, a1, b0, b1), (c0, c1, d0, d1) = tiles[0], tiles[-1]
            t = out[a0:a1, b0:b1].clone()
            out[a0:a1, b0:b1] = out[c0:c1, d0:d1]
            out[c0:c1, d0:d1] = t
        if mutant == "skiptile":
            r0, r1, c0, c1 = tiles[-1]
            out[r0:r1, c0:c1] = start[r0:r1, c0:c1]
        return out

    if not out8:
        out = G.trunc_bits(v) if mutant == "trunc" else G.rne_bits(v)
        start = G.rne_bits(r) if inplace else torch.full((rows, cols), SENT, dtype=torch.int16)
        buf = torch.full((rows + 2 * GUARD, cols), SENT, dtype=torch.int16)
        buf[GUARD:GUARD + rows] = walk(out, start)
        return buf
    q, img = requantise(v if mutant == "f32quant" else G.bf2f(G.rne_bits(v)), mutant)
    q = walk(q, torch.full((rows, cols), SENT8, dtype=torch.uint8))
    if mutant == "skiptile":
        r0, r1, c0, c1 = tiles[-1]
        rr, bb = np.arange(r0, r1)[:, None], np.arange(c0 // 32, c1 // 32)[None, :]
        img[mx.scale_offsets(rows, cols, 0)[rr, bb]] = SENT_S
    buf = torch.full((rows + 2 * GUARD, cols), SENT8, dtype=torch.uint8)
    buf[GUARD:GUARD + rows] = q
    sbuf = torch.full((img.size + 2 * GUARD_S,), SENT_S, dtype=torch.uint8)
    sbuf[GUARD_S:GUARD_S + img.size] = torch.from_numpy(img)
    return buf, sbuf


# ---------------------------------------------------------------------------------------------- OUT8 + GELU
def out8_gelu_check(q, e, z):
    """The boundary-aware check of test_mxfp8_gpu.py on an exact pre-activation z (f64 numpy): q the decoded e4m3
    values, e the block exponents the kernel wrote.  The accumulator is exact, so the slack holds only the GELU form's
    distance from erf and one bf16 ulp.  -> (share of scale bytes that differ, codes differing away from a rounding
    boundary, codes further than one step plus the slack, share of differing codes)."""
    ref = G.gelu_f64(torch.from_numpy(z)).numpy()
    refb = torch.from_numpy(ref).float().to(torch.bfloat16).float().numpy()
    qo, eo = mx.quantize(refb, z.shape[1])
    same = np.repeat(e == eo, 32, axis=1)
    er = np.ldexp(1.0, -np.repeat(e, 32, axis=1))
    ulp16 = np.ldexp(1.0, np.floor(np.log2(np.maximum(np.abs(ref), 1e-30))).astype(int) - 7)
    slack = (np.abs(mx.gelu_q8(z).astype(np.float64) - ref) + ulp16) * er
    diff = (q != qo) & same
    near = np.abs(refb * er - (q.astype(np.float64) + qo) / 2) <= slack * 1.0001
    a = np.maximum(np.abs(q), np.abs(qo))
    ex = np.floor(np.log2(np.maximum(a, 2.0 ** -30)))
    step = np.where(ex >= -6, 2.0 ** (ex - 3), 2.0 ** -9)
    far = np.abs(q - qo) > (step + 2 * slack) * 1.0001
    return float(np.mean(e != eo)), int(np.count_nonzero(diff & ~near)), int(np.count_nonzero(diff & far)), float(diff.mean())


# ---------------------------------------------------------------------------------------------- the walk
def walk_tiles(c, cus=G.CUS):
    """Tile indices (row-major over (m / 256, n / tile width)) worth checking on a large case, >= 32: the first and
    last tile of the walk, of every XCD's share, each workgroup slot's second tile in two shares, and one of every
    residue mod 8."""
    tm, tn = c.m // 256, c.n // TN[c.layout]
    nt = tm * tn
    grid = max(8, min(cus // 8 * 8, nt) // 8 * 8)
    per = grid // 8
    pick = {0, nt - 1}
    for xcd in range(8):
        lo, hi = nt * xcd // 8, nt * (xcd + 1) // 8
        pick |= {lo, hi - 1}
        if xcd in (0, 5) and lo + per < hi:
            pick |= {lo + per, min(lo + per + 3, hi - 1), hi - 1 - ((hi - 1 - lo) % per)}      # second tiles
    pick |= {nt // 2 + i for i in range(8)} | {nt // 3 + 2 * i for i in range(8)}
    assert {t % 8 for t in pick} == set(range(8)) and len(pick) >= 32
    return sorted(pick), per
