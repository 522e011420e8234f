"""GPU: the list kernels behind the kNN scan (csrc/knn.hip knn_merge, knn_link_filter, knn_rerank, knn_rerank_comp,
knn_rerank_mix) and their entry points, against the f64 references, input families and bounds of
retrieval_lists_ref.py (test_retrieval_lists_cpu.py checks those first).

Rules.  Merge: every output bit for bit (indices, f32 and f64 scores, payload, (-1, -inf, 0.0) padding), the separate
arrays and the packed buffer alike.  Link graph: neighbour lists, counts and -1 tails equal to oracle.dls.link_graph in
every scan mode and for a native fp16 index.  Rerank: order, indices, -1 / 0.0 padding exact; raw components within
4 ulp, scaled within the per-query bound, finals within 4 * 2^-53 (a + b + g); fused = components + mix, f32 index =
native fp16 index and one index = two shards + merge + mix with torch.equal.  Outputs that go through the C ABI are
pre-filled with a sentinel, so a slot the kernel leaves unwritten cannot pass; a rejected call must leave them
untouched.

Before the two fixes that came with this file, 119 of the 365 tests failed on an MI355X:
  rerank_mix_out left out_final / out_emb / out_lab / out_kg past the valid candidates unwritten (107): all 47 `-short`
    cases each of test_rerank_fused and test_rerank_components_then_mix, the 8 of test_rerank_outside_the_shard
    (`-full` too: the other shard's rows are empty slots), the 4 `-short` of test_sharded_identity,
    test_rerank_wrappers[short];
  knn_merge ranked the same (score, index) from two lists onto one output slot (12): test_merge[duplicates_*] (4) and
    test_merge_abi[duplicates_*-separate / -packed] (8).
With the fixes: 365 passed in 4.1 s (slowest test 0.24 s, the first launch); raw and scaled components came out bit
for bit equal to the numpy reference (0 ulp), finals within 0.25 of their bound, and one index = two shards + merge +
mix held with torch.equal without touching the mix arithmetic.  Scratch builds, not committed: knn_merge breaking equal
scores by the higher index fails 88 tests (test_merge 29, test_merge_abi 58, test_merge_packed_without_payload_output);
the min-max taken over all kc lanes instead of the valid ones fails 98 (test_rerank_fused 43,
test_rerank_components_then_mix 43, test_rerank_outside_the_shard 7, test_sharded_identity 4, test_rerank_wrappers 1).
"""

import numpy as np
import pytest
import torch

import retrieval_lists_ref as R
from mmr_amd import _lib, parallel, retrieval
from mmr_amd.retrieval import GalleryIndex

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT, SENT_I = 777.25, -12345
WORST = {"raw_ulp": 0.0, "scaled/tol": 0.0, "final/tol": 0.0}


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(DEV)


def host(t):
    return t.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def assert_bits(got, ref, what):
    got = host(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    bad = np.argwhere(bits(got) != bits(ref))
    assert len(bad) == 0, f"{what}: {len(bad)} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r}, " \
                          f"ref {ref[tuple(bad[0])]!r}"


def stream():
    return _lib.stream_ptr(torch.device(DEV))

# ------------------------------------------------------------------------------------------------ merge

def _merge_inputs(c):
    return dev(c["s"]), dev(c["i"]), None if c["pay"] is None else dev(c["pay"])


def _pack(s, i, pay):
    return torch.stack([parallel.pack_lists(i[li], s[li], None if pay is None else pay[li]) for li in range(i.shape[0])])


@pytest.mark.parametrize("name", R.MERGE_NAMES)
def test_merge(name):
    """retrieval.merge_topk (separate arrays) and pack_lists + retrieval.merge_topk_packed against merge_ref"""
    c = R.merge_case(name)
    ref = R.merge_ref(c["s"], c["i"], c["k_out"], c["pay"], c["q0"], c["nq"])
    s, i, pay = _merge_inputs(c)
    P = 0 if pay is None else pay.shape[-1]
    got = retrieval.merge_topk(s, i, c["k_out"], payload=pay, q0=c["q0"], nq=c["nq"])
    for g, r, what in zip(got, ref, ("idx", "f32", "f64", "payload")):
        assert_bits(g, r, f"{name}: {what}")
    packed = _pack(s, i, pay)   # [L][B + 1][k_in][2 + P]: the status row makes nq_total = B + 1
    assert_bits(packed[:, :-1, :, 1].contiguous().view(torch.int64), c["i"], f"{name}: index bits through pack_lists")
    gotp = retrieval.merge_topk_packed(packed, c["k_out"], P, q0=c["q0"], nq=c["nq"])
    assert len(gotp) == len(got)
    for g, r, what in zip(gotp, ref, ("idx", "f32", "f64", "payload")):
        assert_bits(g, r, f"{name}: packed {what}")


def _merge_abi(c, packed, f32=True, f64=True, k_in=None, n_lists=None, nq_total=None, width=None, out_pay=True,
               q0=None, nq=None):
    """mmr_merge_topk_payload / _packed through ctypes with sentinel-filled outputs -> (status, outputs)."""
    s, i, pay = _merge_inputs(c)
    L_, B, K = i.shape
    P = 0 if pay is None else pay.shape[-1]
    q0 = c["q0"] if q0 is None else q0
    nq = c["nq"] if nq is None else nq
    k_out = c["k_out"]
    oi = torch.full((nq, k_out), SENT_I, dtype=torch.int64, device=DEV)
    o32 = torch.full((nq, k_out), SENT, dtype=torch.float32, device=DEV) if f32 else None
    o64 = torch.full((nq, k_out), SENT, dtype=torch.float64, device=DEV) if f64 else None
    op = torch.full((nq, k_out, max(P, 1)), SENT, dtype=torch.float64, device=DEV) if (P and out_pay) else None
    width = P if width is None else width
    n_lists = L_ if n_lists is None else n_lists
    k_in = K if k_in is None else k_in
    if packed:
        buf = _pack(s, i, pay)
        st = _lib.lib().mmr_merge_topk_packed(_lib.ptr(buf), width, n_lists, B + 1 if nq_total is None else nq_total, q0,
                                              nq, k_in, k_out, _lib.ptr(oi), _lib.ptr(o32), _lib.ptr(o64), _lib.ptr(op),
                                              stream())
    else:
        st = _lib.lib().mmr_merge_topk_payload(_lib.ptr(s), _lib.ptr(i), _lib.ptr(pay), width, n_lists,
                                               B if nq_total is None else nq_total, q0, nq, k_in, k_out, _lib.ptr(oi),
                                               _lib.ptr(o32), _lib.ptr(o64), _lib.ptr(op), stream())
    torch.cuda.synchronize()
    return st, (oi, o32, o64, op)


@pytest.mark.parametrize("packed", [False, True], ids=["separate", "packed"])
@pytest.mark.parametrize("n,name", list(enumerate(R.MERGE_NAMES)), ids=R.MERGE_NAMES)
def test_merge_abi(n, name, packed):
    """sentinel-filled outputs (an unwritten slot shows), out_score / out_score64 NULL in turn"""
    c = R.merge_case(name)
    ref = R.merge_ref(c["s"], c["i"], c["k_out"], c["pay"], c["q0"], c["nq"])
    f32, f64 = [(True, True), (False, True), (True, False), (False, False)][n % 4]
    st, got = _merge_abi(c, packed, f32=f32, f64=f64)
    assert st == 0, _lib.lib().mmr_last_error()
    for g, r, what in zip(got, ref, ("idx", "f32", "f64", "payload")):
        if g is not None:
            assert_bits(g, r, f"{name}: {what}")
    if not packed and c["q0"] == 0 and c["nq"] == c["i"].shape[1]:   # the plain entry point: no payload, no window
        s, i, _ = _merge_inputs(c)
        oi = torch.full((c["nq"], c["k_out"]), SENT_I, dtype=torch.int64, device=DEV)
        o32 = torch.full((c["nq"], c["k_out"]), SENT, dtype=torch.float32, device=DEV) if f32 else None
        o64 = torch.full((c["nq"], c["k_out"]), SENT, dtype=torch.float64, device=DEV) if f64 else None
        st = _lib.lib().mmr_merge_topk(_lib.ptr(s), _lib.ptr(i), i.shape[0], c["nq"], i.shape[2], c["k_out"],
                                       _lib.ptr(oi), _lib.ptr(o32), _lib.ptr(o64), stream())
        torch.cuda.synchronize()
        assert st == 0
        for g, r, what in zip((oi, o32, o64), ref, ("idx", "f32", "f64")):
            if g is not None:
                assert_bits(g, r, f"{name}: mmr_merge_topk {what}")


def test_merge_packed_without_payload_output():
    """the packed form accepts a payload in the buffer with out_payload NULL (the payload form does not)"""
    c = R.merge_case("width_p3")
    ref = R.merge_ref(c["s"], c["i"], c["k_out"], c["pay"])
    st, got = _merge_abi(c, True, out_pay=False)
    assert st == 0
    for g, r, what in zip(got[:3], ref, ("idx", "f32", "f64")):
        assert_bits(g, r, what)


def _untouched(outs):
    oi, o32, o64, op = outs
    return bool((oi == SENT_I).all()) and all(o is None or bool((o == SENT).all()) for o in (o32, o64, op))


@pytest.mark.parametrize("packed", [False, True], ids=["separate", "packed"])
def test_merge_rejections(packed):
    """non-zero status and nothing launched.  The buffers are as large as the rejected sizes claim."""
    big = R._mcase("too_many", *R._merge_random(17, 2, 241, 1, 900), 5)     # 17 * 241 = 4097 entries
    st, outs = _merge_abi(big, packed)
    assert st != 0 and _untouched(outs)
    wide = R._mcase("too_wide", *R._merge_random(3, 7, 5, 17, 901), 9)
    st, outs = _merge_abi(wide, packed)
    assert st != 0 and _untouched(outs)
    c = R.merge_case("width_p3")     # 7 queries (+ the status row when packed): claim 6 in total, ask for 2..7
    st, outs = _merge_abi(c, packed, nq_total=6, q0=2, nq=5)
    assert st != 0 and _untouched(outs)
    st, outs = _merge_abi(c, packed, q0=-1, nq=3)
    assert st != 0 and _untouched(outs)
    if not packed:
        st, outs = _merge_abi(c, False, out_pay=False)   # payload set, out_payload NULL
        assert st != 0 and _untouched(outs)
    assert b"merge" in _lib.lib().mmr_last_error()

# ------------------------------------------------------------------------------------------------ link graph

@pytest.mark.parametrize("mode", ["x3", "f32", "f16", "native16"])
@pytest.mark.parametrize("name", list(R.LINK_CASES))
def test_link_graph(name, mode):
    kind, thr, ml, batch, base = R.LINK_CASES[name]
    G = R.link_gallery(kind)
    ix = GalleryIndex(G.astype(np.float16), idx_base=base) if mode == "native16" else GalleryIndex(G, idx_base=base,
                                                                                                   mode=mode)
    try:
        nbr, cnt = ix.link_graph(thr, ml, batch=batch)
        nbr, cnt = host(nbr), host(cnt)
    finally:
        ix.close()
    want = R.link_expected(name)
    assert cnt.tolist() == [len(w) for w in want]
    assert (nbr[np.arange(ml)[None, :] >= cnt[:, None]] == -1).all()
    got = [nbr[r, :cnt[r]].tolist() for r in range(len(G))]
    bad = [r for r in range(len(G)) if got[r] != want[r]]
    assert not bad, f"{len(bad)} rows differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"
    assert all(r not in got[r] for r in range(len(G)))

# ------------------------------------------------------------------------------------------------ rerank

_INDEX = {}


def index(d, dk, half=False, row0=0, nrows=None, base=0):
    """cached (GalleryIndex of gallery rows [row0, row0 + nrows) at idx_base, its label and KG tables on device)"""
    key = (d, dk, half, row0, nrows, base)
    if key not in _INDEX:
        gal = R.rerank_gallery(d, dk)
        sl = slice(row0, R.N_GAL if nrows is None else row0 + nrows)
        rows = gal["G"][sl]
        _INDEX[key] = (GalleryIndex(rows.astype(np.float16) if half else rows, idx_base=base),
                       dev(gal["lab"][sl]), dev(gal["kg"][sl]))
    return _INDEX[key]


def _qdev(qs, cand=None):
    return dev(qs["q_emb"]), dev(qs["cand"] if cand is None else cand), dev(qs["q_lab"]), dev(qs["q_kg"])


def _outs(nq, topk, want):
    return (torch.full((nq, topk), SENT_I, dtype=torch.int64, device=DEV),
            [torch.full((nq, topk), SENT, dtype=torch.float64, device=DEV) if want else None for _ in range(4)])


def rerank_abi(ixt, q_emb, cand, q_lab, q_kg, topk, w, want=True, kc=None, dk=None):
    ix, g_lab, g_kg = ixt
    nq = cand.shape[0]
    oi, outs = _outs(nq, max(topk, 1), want)
    st = _lib.lib().mmr_index_rerank(ix._h, _lib.ptr(q_emb), nq, _lib.ptr(cand), cand.shape[1] if kc is None else kc,
                                     _lib.ptr(q_lab), _lib.ptr(g_lab), _lib.ptr(q_kg), _lib.ptr(g_kg),
                                     q_kg.shape[1] if dk is None else dk, *map(float, w), topk, _lib.ptr(oi),
                                     *(_lib.ptr(o) for o in outs), stream())
    torch.cuda.synchronize()
    return st, (oi, *outs)


def mix_abi(cand, comp, topk, w, want=True, kc=None):
    nq = cand.shape[0]
    oi, outs = _outs(nq, max(topk, 1), want)
    st = _lib.lib().mmr_rerank_mix(_lib.ptr(cand), _lib.ptr(comp), nq, cand.shape[1] if kc is None else kc,
                                   *map(float, w), topk, _lib.ptr(oi), *(_lib.ptr(o) for o in outs), stream())
    torch.cuda.synchronize()
    return st, (oi, *outs)


def check_rerank(got, ref, w, what):
    oi, fin, e, l, k = (host(t) for t in got)
    assert np.array_equal(oi, ref["idx"]), f"{what}: order / indices / -1 padding"
    topk = oi.shape[1]
    past = np.arange(topk)[None, :] >= ref["valid"].sum(1)[:, None]
    for name, g in (("final", fin), ("e", e), ("l", l), ("k", k)):
        assert (bits(g[past]) == 0).all(), f"{what}: {name} past the valid candidates is not +0.0"
    for p, (name, g) in enumerate((("e", e), ("l", l), ("k", k))):
        err, tol = np.abs(g - ref[name]), ref["tol"][:, p:p + 1]
        print(f"{what}: scaled {name} worst err {err.max():.3e}, bound {tol.max():.3e}")
        assert (err <= tol).all(), f"{what}: scaled {name} err {err.max():.3e}"
        if (tol > 0).any():
            WORST["scaled/tol"] = max(WORST["scaled/tol"], float((err / np.where(tol > 0, tol, np.inf)).max()))
    err = np.abs(fin - ref["final"])
    print(f"{what}: final worst err {err.max():.3e}, bound {R.final_tol(w):.3e}")
    assert (err <= R.final_tol(w)).all(), f"{what}: final err {err.max():.3e} > {R.final_tol(w):.3e}"
    if sum(w):
        WORST["final/tol"] = max(WORST["final/tol"], float(err.max() / R.final_tol(w)))


def check_raw(comp, ref, what):
    comp = host(comp)
    zero = ref["raw"] == 0
    assert comp.shape == ref["raw"].shape and (comp[zero] == 0).all(), f"{what}: raw not exactly 0.0 for an empty slot / a zero norm / an empty union"
    ulps = np.abs(comp - ref["raw"]) / np.spacing(np.abs(ref["raw"]))
    print(f"{what}: raw worst {ulps.max():.2f} ulp")
    WORST["raw_ulp"] = max(WORST["raw_ulp"], float(ulps.max()))
    assert (np.abs(comp - ref["raw"]) <= R.raw_tol(ref["raw"])).all(), f"{what}: raw {ulps.max():.2f} ulp"


def _case_id(c):
    return "kc{}_top{}_w{}_d{}_dk{}".format(*c)


@pytest.mark.parametrize("part", ["full", "short"])
@pytest.mark.parametrize("case", R.RERANK_CASES, ids=_case_id)
def test_rerank_fused(case, part):
    """mmr_index_rerank (all outputs, sentinel-filled) and GalleryIndex.rerank(want_components=False)"""
    kc, topk, wi, d, dk = case
    w = R.WEIGHTS[wi]
    qs = R.rerank_queries(d, dk, kc, part)
    ref = R.rerank_ref(qs["q_emb"], qs["cand"], qs["q_lab"], qs["q_kg"], qs["gal"], topk, w)
    ixt = index(d, dk)
    q = _qdev(qs)
    st, got = rerank_abi(ixt, *q, topk, w)
    assert st == 0
    check_rerank(got, ref, w, "fused")
    st, lean = rerank_abi(ixt, *q, topk, w, want=False)      # NULL component outputs
    assert st == 0 and torch.equal(lean[0], got[0])


@pytest.mark.parametrize("part", ["full", "short"])
@pytest.mark.parametrize("case", R.RERANK_CASES, ids=_case_id)
def test_rerank_components_then_mix(case, part):
    """rerank_components within 4 ulp of the raw reference; mmr_rerank_mix of them = the fused call, bit for bit"""
    kc, topk, wi, d, dk = case
    w = R.WEIGHTS[wi]
    qs = R.rerank_queries(d, dk, kc, part)
    ref = R.rerank_ref(qs["q_emb"], qs["cand"], qs["q_lab"], qs["q_kg"], qs["gal"], topk, w)
    ix, g_lab, g_kg = ixt = index(d, dk)
    q_emb, cand, q_lab, q_kg = _qdev(qs)
    comp = torch.full((cand.shape[0], kc, 3), SENT, dtype=torch.float64, device=DEV)
    st = _lib.lib().mmr_index_rerank_components(ix._h, _lib.ptr(q_emb), cand.shape[0], _lib.ptr(cand), kc,
                                                _lib.ptr(q_lab), _lib.ptr(g_lab), _lib.ptr(q_kg), _lib.ptr(g_kg), dk,
                                                _lib.ptr(comp), stream())
    assert st == 0
    check_raw(comp, ref, "components")
    assert torch.equal(comp, ix.rerank_components(q_emb, cand, q_lab, g_lab, q_kg, g_kg))
    st, mixed = mix_abi(cand, comp, topk, w)
    assert st == 0
    check_rerank(mixed, ref, w, "mix")
    st, fused = rerank_abi(ixt, q_emb, cand, q_lab, q_kg, topk, w)
    assert st == 0
    for a, b, what in zip(mixed, fused, ("idx", "final", "e", "l", "k")):
        assert torch.equal(a, b), f"mix != fused: {what}"
    st, lean = mix_abi(cand, comp, topk, w, want=False)
    assert st == 0 and torch.equal(lean[0], mixed[0])


@pytest.mark.parametrize("part", ["full", "short"])
def test_rerank_wrappers(part):
    """GalleryIndex.rerank / retrieval.rerank_mix (outputs from torch.empty) return what the C ABI wrote"""
    kc, topk, d, dk = 15, 15, 100, 3
    w = R.WEIGHTS[0]
    qs = R.rerank_queries(d, dk, kc, part)
    ref = R.rerank_ref(qs["q_emb"], qs["cand"], qs["q_lab"], qs["q_kg"], qs["gal"], topk, w)
    ix, g_lab, g_kg = index(d, dk)
    q_emb, cand, q_lab, q_kg = _qdev(qs)
    got = ix.rerank(q_emb, cand, q_lab, g_lab, q_kg, g_kg, topk, *w)
    check_rerank(got, ref, w, "GalleryIndex.rerank")
    lean = ix.rerank(q_emb, cand, q_lab, g_lab, q_kg, g_kg, topk, *w, want_components=False)
    assert torch.equal(lean[0], got[0]) and all(o is None for o in lean[1:])
    comp = ix.rerank_components(q_emb, cand, q_lab, g_lab, q_kg, g_kg)
    mixed = retrieval.rerank_mix(cand, comp, topk, *w)
    check_rerank(mixed, ref, w, "retrieval.rerank_mix")
    lean = retrieval.rerank_mix(cand, comp, topk, *w, want_components=False)
    assert torch.equal(lean[0], mixed[0]) and all(o is None for o in lean[1:])


@pytest.mark.parametrize("part", ["full", "short"])
@pytest.mark.parametrize("kc,d,dk", [(15, 100, 3), (64, 192, 64), (2, 8, 1), (63, 8, 100)])
def test_rerank_native_fp16_index(kc, d, dk, part):
    """a native fp16 index of the (fp16-exact) rows = the f32 index of the upcast rows, bit for bit"""
    qs = R.rerank_queries(d, dk, kc, part)
    q = _qdev(qs)
    for w in R.WEIGHTS[:2]:
        st, a = rerank_abi(index(d, dk), *q, kc, w)
        st2, b = rerank_abi(index(d, dk, half=True), *q, kc, w)
        assert st == 0 and st2 == 0
        for x, y, what in zip(a, b, ("idx", "final", "e", "l", "k")):
            assert torch.equal(x, y), what
    ca = index(d, dk)[0].rerank_components(q[0], q[1], q[2], index(d, dk)[1], q[3], index(d, dk)[2])
    cb = index(d, dk, half=True)[0].rerank_components(q[0], q[1], q[2], index(d, dk, half=True)[1], q[3],
                                                      index(d, dk, half=True)[2])
    assert torch.equal(ca, cb)


@pytest.mark.parametrize("part", ["full", "short"])
@pytest.mark.parametrize("kc,d,dk", R.SHARDED_CASES)
def test_rerank_outside_the_shard(kc, d, dk, part):
    """a shard index given the whole (global) candidate list: rows of the other shard are empty slots for the
    fused call and zero components for rerank_components"""
    sc = R.sharded_case(d, dk, kc, part)
    qs = sc["qs"]
    q_emb, cand, q_lab, q_kg = _qdev(qs, sc["cand"])
    for s, (row0, nrows) in enumerate(sc["shards"]):
        base = R.SHARD_BASE + row0
        ixt = index(d, dk, row0=row0, nrows=nrows, base=base)
        for w in R.SHARD_WEIGHTS:
            ref = R.rerank_ref(qs["q_emb"], sc["cand"], qs["q_lab"], qs["q_kg"], qs["gal"], kc, w, idx_base=base,
                               row0=row0, nrows=nrows)
            st, got = rerank_abi(ixt, q_emb, cand, q_lab, q_kg, kc, w)
            assert st == 0
            check_rerank(got, ref, w, f"shard {s}")
        comp = ixt[0].rerank_components(q_emb, cand, q_lab, ixt[1], q_kg, ixt[2])
        check_raw(comp, dict(raw=sc["comps"][s]), f"shard {s} components")
        assert (bits(host(comp)[sc["lists"][s] < 0]) == 0).all()


@pytest.mark.parametrize("part", ["full", "short"])
@pytest.mark.parametrize("kc,d,dk", R.SHARDED_CASES)
def test_sharded_identity(kc, d, dk, part):
    """two shard indices: rerank_components on each -> merge_topk with the components as payload -> rerank_mix
    = rerank on one index of the whole gallery, torch.equal on all five outputs"""
    sc = R.sharded_case(d, dk, kc, part)
    qs = sc["qs"]
    q_emb, cand, q_lab, q_kg = _qdev(qs, sc["cand"])
    whole = index(d, dk, base=R.SHARD_BASE)
    comps = []
    for row0, nrows in sc["shards"]:
        ix, g_lab, g_kg = index(d, dk, row0=row0, nrows=nrows, base=R.SHARD_BASE + row0)
        comps.append(ix.rerank_components(q_emb, cand, q_lab, g_lab, q_kg, g_kg))
    scores = dev(np.stack([sc["scores"], sc["scores"]]))
    mi, _, _, mc = retrieval.merge_topk(scores, dev(sc["lists"]), kc, payload=torch.stack(comps))
    assert_bits(mi, sc["merged_idx"], "merged candidates")
    check_raw(mc, dict(raw=sc["merged_comp"]), "merged components")
    for w in R.WEIGHTS:
        for topk in sorted({1, kc}):
            st, mixed = mix_abi(mi, mc, topk, w)
            st2, one = rerank_abi(whole, q_emb, mi, q_lab, q_kg, topk, w)
            st3, holes = rerank_abi(whole, q_emb, cand, q_lab, q_kg, topk, w)   # the unmerged list, -1 slots inside
            assert st == 0 and st2 == 0 and st3 == 0
            for a, b, c, what in zip(mixed, one, holes, ("idx", "final", "e", "l", "k")):
                assert torch.equal(a, b), f"sharded != single index: {what} (weights {w}, topk {topk})"
                assert torch.equal(a, c), f"sharded != single index on the list with holes: {what}"
            ref = R.rerank_ref(qs["q_emb"], sc["cand"], qs["q_lab"], qs["q_kg"], qs["gal"], topk, w,
                               idx_base=R.SHARD_BASE)
            check_rerank(mixed, ref, w, "sharded")


def test_rerank_rejections():
    """kc = 0, kc = 65, topk > kc, dk = 0: non-zero status, outputs untouched.  Buffers sized for kc = 65."""
    d, dk = 100, 3
    qs = R.rerank_queries(d, dk, 64, "full")
    q_emb, _, q_lab, q_kg = _qdev(qs)
    nq = q_emb.shape[0]
    cand = torch.zeros((nq, 65), dtype=torch.int64, device=DEV)
    comp = torch.zeros((nq, 65, 3), dtype=torch.float64, device=DEV)
    ixt = index(d, dk)

    def untouched(outs):
        return bool((outs[0] == SENT_I).all()) and all(bool((o == SENT).all()) for o in outs[1:])
    for kc, topk, dk_arg in ((0, 1, dk), (65, 65, dk), (65, 1, dk), (15, 16, dk), (15, 0, dk), (15, 15, 0)):
        st, outs = rerank_abi(ixt, q_emb, cand, q_lab, q_kg, topk, R.WEIGHTS[0], kc=kc, dk=dk_arg)
        assert st != 0 and untouched(outs), (kc, topk, dk_arg)
        assert b"rerank" in _lib.lib().mmr_last_error()
        if dk_arg == dk:
            st, outs = mix_abi(cand, comp, topk, R.WEIGHTS[0], kc=kc)
            assert st != 0 and untouched(outs), (kc, topk)
        out = torch.full((nq, 65, 3), SENT, dtype=torch.float64, device=DEV)
        if not (1 <= kc <= 64 and dk_arg >= 1):
            st = _lib.lib().mmr_index_rerank_components(ixt[0]._h, _lib.ptr(q_emb), nq, _lib.ptr(cand), kc,
                                                        _lib.ptr(q_lab), _lib.ptr(ixt[1]), _lib.ptr(q_kg),
                                                        _lib.ptr(ixt[2]), dk_arg, _lib.ptr(out), stream())
            torch.cuda.synchronize()
            assert st != 0 and bool((out == SENT).all()), (kc, dk_arg)


def test_zz_report():
    """not a check: the worst figures of this run against their bounds (pytest -s shows them)"""
    print("retrieval lists, worst over the run:", {k: round(v, 4) for k, v in WORST.items()})
    for ix, _, _ in _INDEX.values():
        ix.close()
    _INDEX.clear()
