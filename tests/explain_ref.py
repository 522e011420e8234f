"""f64 numpy restatement of the attention explanations (csrc/explain.hip) and of the map alignment
(csrc/map_align.hip), with the tolerances the tests hold the kernels to.  Tests-only; no scipy.

Explanations, per sample (the reference's ExplanationEngine.explain, explain.py:825-947):
  p_txt = column mean of txt2img, t_img = column mean of img2txt
  p_comb: Lc == Np column mean; Lc > Np the window of Np consecutive columns with the largest column-sum mass (ties:
          lowest offset), zeros when max / (total + 1e-12) < 0.06, else the chosen columns' means; Lc < Np absent
  t_comb: Lc == T column mean; Lc > T the same search over row sums (ratio 0.0), the chosen rows' means; Lc < T the
          row means min-max normalised to [0, 1], uniform 1 / Lc when |max - min| < 1e-8
  final_patch = minmax(0.6 p_txt + 0.4 p_comb) or of the one that exists; final_token likewise, trimmed
  heat map = bilinear(minmax(v) as G x G -> (H, W)), align_corners=False
Everything here is f64; the kernel rounds each mean to f32 once and goes on in f32.

Tolerances (eps = 2^-24 = the f32 unit roundoff; c = max / (max - min) of the vector being normalised):
  raw vectors                2 eps relative (one rounding of the f64 mean, a factor 2 of slack)
  normalised vectors         (4 c + 4) eps absolute: x, min, max each carry eps relative, the subtraction
                             amplifies that by c, the division and the + 1e-8 add a few eps on a result <= 1
  against f32-recorded       the reference sums n terms in f32: (4 c + 2 n) eps
  heat-map pixels            the vector bound of the map's source (a twice-normalised source adds (4 + 4) eps:
                             c = 1) + (2 G + 1) 2^-22: the f32 source coordinate is off by <= G 2^-22 per axis
                             (values in [0, 1], so a pixel moves by at most that much per axis), 4 products
  pearson                    HW 2^-50 (f64 sums of HW terms);  HW eps against an f32 record
  spearman                   2^-50: the sums are exact integers, one sqrt and one division
  integers, IoU              equal"""
import math

import numpy as np

EPS = 2.0 ** -24
W_A, W_B = float(np.float32(0.6)), float(np.float32(0.4))  # the weights as the f32 arithmetic holds them


def minmax(v):
    v = np.asarray(v, np.float64)
    return (v - v.min()) / ((v.max() - v.min()) + 1e-8)


def cond(v):
    """c = max |.| / (max - min) of a vector about to be normalised (inf for a constant one)"""
    v = np.asarray(v, np.float64)
    r = v.max() - v.min()
    return float(np.abs(v).max() / r) if r > 0 else math.inf


def tol_raw(v):
    return 2 * EPS * np.abs(np.asarray(v, np.float64))


def tol_norm(src, n_f32_terms=None):
    return (4 * cond(src) + (4 if n_f32_terms is None else 2 * n_f32_terms)) * EPS


def tol_pixel(vec_tol, g, renormalised=False):
    return vec_tol + (8 * EPS if renormalised else 0.0) + (2 * g + 1) * 2.0 ** -22


def window(sums, n, ratio):
    """-> (offset, below, gap): argmax over the windows of n consecutive entries (lowest offset on ties), whether
    max / (total + 1e-12) < ratio, and best - second best window sum (inf with one window)"""
    sums = np.asarray(sums, np.float64)
    w = np.array([sums[o:o + n].sum() for o in range(len(sums) - n + 1)])
    off = int(np.argmax(w))
    rest = np.delete(w, off)
    gap = float(w[off] - rest.max()) if len(rest) else math.inf
    return off, bool(w[off] / (sums.sum() + 1e-12) < ratio), gap


def explain_sample(txt2img, img2txt, comb, T):
    """One sample's vectors (f64; None where the reference has none) + offsets, gaps and the sources of every
    normalisation (for the tolerances)."""
    r = {k: None for k in ("p_txt", "t_img", "p_comb", "t_comb", "final_patch", "final_token", "final_patch_src",
                           "final_token_src", "t_comb_src")}
    r["off_p"] = r["off_t"] = -1
    r["gap_p"] = r["gap_t"] = math.inf
    r["below_p"] = False
    if txt2img is not None:
        a = np.asarray(txt2img, np.float64)
        r["p_txt"] = a.mean(0)
        npatch = a.shape[1]
    if img2txt is not None:
        a = np.asarray(img2txt, np.float64)
        r["t_img"] = a.mean(0)
        npatch = a.shape[0]
    if comb is not None:
        c = np.asarray(comb, np.float64)
        lc = c.shape[0]
        if lc == npatch:
            r["p_comb"], r["off_p"] = c.mean(0), 0
        elif lc > npatch:
            off, below, gap = window(c.sum(0), npatch, 0.06)
            r["off_p"], r["gap_p"], r["below_p"] = off, gap, below
            r["p_comb"] = np.zeros(npatch) if below else c[:, off:off + npatch].mean(0)
        if lc == T:
            r["t_comb"], r["off_t"] = c.mean(0), 0
        elif lc > T:
            off, below, gap = window(c.sum(1), T, 0.0)
            r["off_t"], r["gap_t"] = off, gap
            r["t_comb"] = np.zeros(T) if below else c[off:off + T, :].mean(1)
        else:
            v = c.mean(1)
            r["t_comb_src"] = v
            rng = v.max() - v.min()
            r["t_comb"] = np.full(lc, 1.0 / lc) if abs(rng) < 1e-8 else np.clip((v - v.min()) / (rng + 1e-8), 0, 1)
    for out, x, y in (("final_patch", r["p_txt"], r["p_comb"]), ("final_token", r["t_img"], r["t_comb"])):
        if x is not None and y is not None:
            n = min(len(x), len(y))
            src = W_A * x[:n] + W_B * y[:n]
        else:
            src = x if x is not None else y
        if src is not None:
            r[out + "_src"], r[out] = src, minmax(src)
    return r


def fixture_conditions(r, name="", row_search=True, token_cond=64.0):
    """The conditions a fixture sample (r = explain_sample(...)) must meet for the comparisons to be decided above
    rounding: the best and second-best window sums >= 1e-3 apart (row_search=False: the row search is not used —
    a row-stochastic comb with Lc > T has all row sums 1 and t_comb = 1 / Lc whichever row wins); every vector
    that is normalised has max / (max - min) <= 64 (token_cond for the token vector); every constant test
    |range| < 1e-8 is decided with f32 means on either side: each mean is off by <= eps max|v|, so the range by
    <= 2 eps max|v|, and the range must be <= 1e-8 - 4 eps max|v| or >= 1e-7."""
    gaps = [r["gap_p"]] + ([r["gap_t"]] if row_search else [])
    assert min(gaps) >= 1e-3 or r["below_p"], (name, gaps)
    for k, lim in (("final_patch_src", 64.0), ("final_token_src", token_cond), ("t_comb_src", None), ("p_txt", 64.0),
                   ("p_comb", 64.0)):
        v = r.get(k)
        if v is None or len(v) < 2 or not np.any(v):
            continue
        rng = float(v.max() - v.min())
        if k == "t_comb_src":
            assert rng <= 1e-8 - 4 * EPS * float(np.abs(v).max()) or rng >= 1e-7, (name, k, rng)
        else:
            assert cond(v) <= lim, (name, k, cond(v))


def heat_map(v, size):
    """compute_attention_map (explain.py:87-102) in f64: minmax, G x G, bilinear align_corners=False"""
    v = minmax(v)
    g = math.isqrt(len(v))
    assert g * g == len(v)
    grid = v.reshape(g, g)
    H, W = size

    def axis(out):
        s = np.maximum((np.arange(out) + 0.5) * (g / out) - 0.5, 0.0)
        i0 = np.minimum(np.floor(s).astype(np.int64), g - 1)
        i1 = np.minimum(i0 + 1, g - 1)
        return i0, i1, s - i0
    y0, y1, ly = axis(H)
    x0, x1, lx = axis(W)
    top = grid[y0][:, x0] * (1 - lx)[None, :] + grid[y0][:, x1] * lx[None, :]
    bot = grid[y1][:, x0] * (1 - lx)[None, :] + grid[y1][:, x1] * lx[None, :]
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def topk_count(n, frac):
    return max(1, int(n * frac))


def ranks2(a):
    """2 x scipy.stats.rankdata(a, 'average') as exact integers (-0 == +0)"""
    a = np.asarray(a).ravel()
    _, inv, cnt = np.unique(a, return_inverse=True, return_counts=True)
    end = np.cumsum(cnt)
    return (2 * end - cnt + 1)[inv].astype(np.int64)  # start + end + 1, start = end - cnt


def map_stats(a, ks):
    a = np.asarray(a).ravel()
    s = np.sort(a)
    a64 = a.astype(np.float64)
    mu = a64.mean()
    return {"ranks2": ranks2(a), "thresholds": np.array([s[len(a) - k] for k in ks], a.dtype),
            "constant": bool(np.all(a == a[0])), "mean": mu, "ssd": float(((a64 - mu) ** 2).sum())}


def compare_pair(a, b, ks):
    """compare_maps (helper.py:173-209) of one pair from exact integer ranks -> dict"""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    sa, sb = map_stats(a, ks), map_stats(b, ks)
    n = len(a)
    ca, cb = sa["ranks2"] - (n + 1), sb["ranks2"] - (n + 1)
    sab, saa, sbb = int((ca * cb).sum()), int((ca * ca).sum()), int((cb * cb).sum())
    flat = sa["constant"] or sb["constant"]
    da, db = a.astype(np.float64) - sa["mean"], b.astype(np.float64) - sb["mean"]
    pearson = 0.0 if flat else float((da * db).sum() / math.sqrt(sa["ssd"] * sb["ssd"]))
    spearman = 0.0 if flat else sab / math.sqrt(float(saa) * float(sbb))
    iu = []
    for ta, tb in zip(sa["thresholds"], sb["thresholds"]):
        at, bt = a >= ta, b >= tb
        iu.append((int((at & bt).sum()), int((at | bt).sum())))
    return {"pearson": pearson, "spearman": spearman, "rank_sums": (sab, saa, sbb), "inter_union": iu,
            "iou": [i / (u + 1e-8) for i, u in iu]}


def iou_key(topk_frac):
    return f"iou_top{int(topk_frac * 100)}pct"


# ---- the recorded reference values (tests/golden/explain_mini.npz, make_golden_explain.py)
def record_names(g):
    return sorted(k[:-5] for k in g.files if k.endswith(":keys"))


def record_inputs(g, a, name):
    """-> txt2img, img2txt, comb (one sample each), T, image size"""
    if name.startswith("syn_"):
        return tuple(g[f"{name}:in_{k}"] for k in ("txt2img", "img2txt", "comb")) + (int(name.split("_")[3]), (8, 8))
    tag, b = name.split("_")
    return tuple(a[f"{tag}_layer_1_{k}"][int(b)] for k in ("txt2img", "img2txt", "comb")) + (
        128 if tag == "text" else 1, (28, 28))


def check_against_record(g, name, vec, size, maps=None):
    """vec: the restatement's explain_sample of the record's inputs (tolerances and the expected values for the
    restatement's own check) — or, with maps, the values under test: maps[key] -> array."""
    keys = bytes(g[f"{name}:keys"]).decode().split("|")
    want_keys = ["txt2img", "img2txt"] + (["comb_img"] if np.any(vec["p_comb"]) else []) + [
        "comb_txt", "final_patch_map", "final_token_map"]
    assert keys == want_keys, (name, keys)
    npatch, lt, lc = len(vec["p_txt"]), len(vec["t_img"]), vec["lc"]
    G = math.isqrt(npatch)
    tp = tol_norm(vec["p_txt"], lt)
    tc = tol_norm(vec["p_comb"], lc) if np.any(vec["p_comb"]) else 0.0
    tf = tol_norm(vec["final_patch_src"], max(lt, lc))
    expect = {"txt2img": (heat_map(vec["p_txt"], size), tol_pixel(tp, G)),
              "img2txt": (vec["t_img"], (npatch + 2) * EPS * np.abs(vec["t_img"])),
              "comb_img": (heat_map(vec["p_comb"], size) if np.any(vec["p_comb"]) else None, tol_pixel(tc, G)),
              "comb_txt": (vec["t_comb"], (lc + 2) * EPS * np.abs(vec["t_comb"]) if vec["t_comb_src"] is None
                           else tol_norm(vec["t_comb_src"], lc)),
              "final_patch_map": (heat_map(vec["final_patch"], size), tol_pixel(tf, G, True)),
              "final_token_map": (vec["final_token"], tol_norm(vec["final_token_src"], max(npatch, lc))
                                  if len(vec["final_token"]) > 1 else 0.0)}
    worst = {}
    for k in keys:
        ref = g[f"{name}:{k}"].astype(np.float64)
        val, tol = expect[k]
        got = val if maps is None else np.asarray(maps[k], np.float64)
        assert got.shape == ref.shape, (name, k, got.shape, ref.shape)
        worst[k] = float((np.abs(got - ref) - tol).max())
        if k == "comb_txt" and vec["t_comb_src"] is not None and np.ptp(vec["t_comb_src"]) < 1e-8:
            assert np.array_equal(got.astype(np.float32), ref.astype(np.float32)), (name, k)  # uniform 1 / Lc, exactly
    assert all(v <= 0.0 for v in worst.values()), (name, worst)
    return worst


def sample_with_lc(t2i, i2t, comb, T):
    r = explain_sample(t2i, i2t, comb, T)
    r["lc"] = comb.shape[0]
    return r
