"""CPU: the references, builders and bounds of retrieval_lists_ref.py, before the GPU file relies on them.

(a) parallel.merge_topk_host / merge_gathered and parallel.rerank_mix_host equal the references on every case the
    GPU file launches (merge outputs bit for bit; rerank orders, indices, padding and scaled values exactly, finals
    within the final bound: the host form mixes in plain f64, the reference in extended precision).
(b) every input family meets the conditions its name states, and the stated separations hold: adjacent reference
    finals bit-equal or > 1e-9 apart, link-graph scores exactly on the threshold or > 1e-9 from it.
(c) each mutant of the references changes an asserted output on a named family.
"""
import numpy as np
import pytest
import torch

import retrieval_lists_ref as R
from mmr_amd import parallel
from oracle import dls as odls


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def assert_bits(got, ref, what):
    got = got.numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    assert np.array_equal(bits(got), bits(ref)), what


# ------------------------------------------------------------------------------------------------ (a) host forms

@pytest.mark.parametrize("name", R.MERGE_NAMES)
def test_merge_host_equals_ref(name):
    c = R.merge_case(name)
    ref = R.merge_ref(c["s"], c["i"], c["k_out"], c["pay"], c["q0"], c["nq"])
    w = slice(c["q0"], c["q0"] + c["nq"])
    s, i = torch.from_numpy(c["s"][:, w].copy()), torch.from_numpy(c["i"][:, w].copy())
    pay = None if c["pay"] is None else torch.from_numpy(c["pay"][:, w].copy())
    got = parallel.merge_topk_host(s, i, c["k_out"], payload=pay)
    for g, r, what in zip(got, ref, ("idx", "f32", "f64", "payload")):
        assert_bits(g, r, f"{name}: {what}")
    # the packed route: pack_lists per list (status row appended), merge_gathered on the host buffer
    P = 0 if c["pay"] is None else c["pay"].shape[-1]
    packed = torch.stack([parallel.pack_lists(torch.from_numpy(c["i"][li]), torch.from_numpy(c["s"][li]),
                                              None if P == 0 else torch.from_numpy(c["pay"][li]))
                          for li in range(c["i"].shape[0])])
    assert_bits(packed[:, :-1, :, 1].contiguous().numpy().view(np.int64), c["i"], f"{name}: pack_lists index bits")
    got = parallel.merge_gathered(packed, c["q0"], c["nq"], c["k_out"], payload_width=P)
    for g, r, what in zip(got, ref, ("idx", "f32", "f64", "payload")):
        assert_bits(g, r, f"{name}: packed {what}")


def _ref(case, part, mutant=None, **kw):
    kc, topk, wi, d, dk = case
    qs = R.rerank_queries(d, dk, kc, part)
    return qs, R.rerank_ref(qs["q_emb"], qs["cand"], qs["q_lab"], qs["q_kg"], qs["gal"], topk, R.WEIGHTS[wi],
                            mutant=mutant, **kw)


def _assert_mix_host(cand, comp, topk, w, ref):
    got = parallel.rerank_mix_host(torch.from_numpy(cand), torch.from_numpy(comp), topk, *w)
    oi, fin, e, l, k = (t.numpy() for t in got)
    assert np.array_equal(oi, ref["idx"])
    for g, key in ((e, "e"), (l, "l"), (k, "k")):
        assert np.array_equal(g, ref[key]), key
    assert np.abs(fin - ref["final"]).max() <= R.final_tol(w)
    past = np.arange(topk)[None, :] >= (cand >= 0).sum(1)[:, None]
    assert (oi[past] == -1).all() and all((x[past] == 0).all() for x in (fin, e, l, k))


@pytest.mark.parametrize("part", ["full", "short"])
@pytest.mark.parametrize("case", R.RERANK_CASES, ids=lambda c: "kc{}_top{}_w{}_d{}_dk{}".format(*c))
def test_rerank_mix_host_equals_ref(case, part):
    qs, ref = _ref(case, part)
    _assert_mix_host(qs["cand"], ref["raw"], case[1], R.WEIGHTS[case[2]], ref)


@pytest.mark.parametrize("part", ["full", "short"])
@pytest.mark.parametrize("kc,d,dk", R.SHARDED_CASES)
def test_sharded_host_equals_ref(kc, d, dk, part):
    """components per shard -> merge with payload -> mix, in the host forms, against the whole-index reference"""
    sc = R.sharded_case(d, dk, kc, part)
    qs = sc["qs"]
    s2 = torch.from_numpy(np.stack([sc["scores"], sc["scores"]]))
    mi, _, _, mc = parallel.merge_topk_host(s2, torch.from_numpy(sc["lists"]), kc, payload=torch.from_numpy(sc["comps"]))
    assert_bits(mi, sc["merged_idx"], "merged idx")
    assert_bits(mc, sc["merged_comp"], "merged components")
    for row0, nrows in sc["shards"]:   # one shard alone (the other's rows are empty slots): the order is defined too
        for w in R.SHARD_WEIGHTS:
            one = R.rerank_ref(qs["q_emb"], sc["cand"], qs["q_lab"], qs["q_kg"], qs["gal"], kc, w,
                               idx_base=R.SHARD_BASE + row0, row0=row0, nrows=nrows)
            assert R.finals_separated(one["finals"])
    for w in R.WEIGHTS:
        whole = R.rerank_ref(qs["q_emb"], sc["cand"], qs["q_lab"], qs["q_kg"], qs["gal"], kc, w, idx_base=R.SHARD_BASE)
        mixed = R.rerank_ref(None, sc["merged_idx"], None, None, None, kc, w, comp=sc["merged_comp"])
        for key in ("idx", "final", "e", "l", "k"):
            assert np.array_equal(whole[key], mixed[key]), key   # holes removed, order kept: the same result
        _assert_mix_host(sc["merged_idx"], sc["merged_comp"], kc, w, whole)


def test_link_ref_is_the_oracle_graph():
    """link_ref's own implementation (the one the mutants run on) with no mutant = oracle.dls.link_graph"""
    for name, (kind, thr, ml, _, _) in R.LINK_CASES.items():
        assert R.link_ref(R.link_gallery(kind), thr, ml, mutant="none") == R.link_expected(name), name
        assert R.link_expected(name) == odls.link_graph(R.link_gallery(kind), thr, ml)

# ------------------------------------------------------------------------------------------------ (b) conditions

def test_merge_families_meet_their_conditions():
    names = set(R.MERGE_NAMES)
    sizes = {c["i"].shape[0] * c["i"].shape[2] for c in R.merge_cases()}
    assert {1, 7, 15, 512, 4096} <= sizes
    for L, k_in, _ in R.MERGE_SIZES:   # k_out below, at and above n_lists * k_in at every size
        m = L * k_in
        ks = {c["k_out"] for c in R.merge_cases() if c["name"].startswith(f"rand_{L}x{k_in}_")}
        assert {m, m + 3} <= ks and (m == 1 or min(ks) < m)
    assert {f"width_p{p}" for p in (0, 1, 3, 16)} <= names
    c = R.merge_case("valid_counts")
    assert ((c["i"] >= 0).sum((0, 2)) == R.VALID_COUNTS).all() and c["k_out"] == 8
    assert {0, 1, 7} & set(R.VALID_COUNTS) and 8 in R.VALID_COUNTS and {9, 15} & set(R.VALID_COUNTS)
    for q in (1, 2, 3, 4):   # head of list 0 and middle of list 1 empty, valid entries after them
        assert c["i"][0, q, 0] == -1 and c["i"][1, q, 2] == -1 and (c["i"][1:, q] >= 0).any()
    assert (c["s"][c["i"] < 0] == 1e300).all()   # an empty slot's score must be ignored
    assert (R.merge_case("all_empty")["i"] == -1).all()
    c = R.merge_case("equal_scores")
    assert (c["s"] == 1.5).all() and (c["i"] >= 0).all()
    assert all(len(set(c["i"][:, q].ravel())) == 15 for q in range(7))
    c = R.merge_case("signed_zero")
    assert (c["s"] == 0).all() and np.signbit(c["s"]).any() and not np.signbit(c["s"]).all()
    c = R.merge_case("neginf_valid")
    v = c["i"] >= 0
    assert np.isneginf(c["s"][v]).any() and (v.sum((0, 2)) < c["k_out"]).any()
    for name in ("duplicates_p3_k15", "duplicates_p3_k4", "duplicates_p16_k18"):
        c = R.merge_case(name)
        for a, b in (((0, 0, 3), (1, 0, 4)), ((1, 0, 4), (2, 0, 1))):   # query 0: one entry in three lists
            assert c["i"][a] == c["i"][b] >= 0 and c["s"][a] == c["s"][b]
            assert not np.array_equal(c["pay"][a], c["pay"][b])
        assert (c["s"][:, 0][c["i"][:, 0] >= 0] <= 5.0).all()   # it ranks first: k_out = 4 cuts behind it
    c = R.merge_case("window")
    assert (c["q0"], c["nq"], c["i"].shape[1]) == (2, 5, 7)
    c = R.merge_case("big_idx")
    for q in range(7):
        assert set(np.array(R.BIG_IDX, np.uint64).astype(np.int64)) <= set(c["i"][:, q].ravel())
    big = np.array(R.BIG_IDX, np.uint64).astype(np.int64)
    assert (big > 2 ** 53).sum() >= 2 and np.isnan(big.view(np.float64)).any() and np.isinf(big.view(np.float64)).any()
    assert float(2 ** 53 + 1) == float(2 ** 53 + 2) or float(2 ** 53 + 1) == float(2 ** 53)  # f64 cannot order them
    assert (R.merge_case("big_idx_equal")["s"] == -0.5).all()


def test_link_families_meet_their_conditions():
    for name, (kind, thr, ml, batch, base) in R.LINK_CASES.items():
        G = R.link_gallery(kind)
        s = R.exact_cos(G, G)
        # thr_above sits one ulp above the score 3 / (1 * 5), which is one division of exact operands: the score is
        # the double 0.6 on any correctly rounding machine, so that case too is measured from 0.6
        gap = np.abs(s - (R.ON if name == "thr_above" else thr))
        assert not ((gap != 0) & (gap <= 1e-9)).any(), f"{name}: a score within 1e-9 of the threshold, not on it"
        assert np.abs(G).max() <= 8 and (G == np.round(G)).all()
        assert (G.astype(np.float16).astype(np.float32) == G).all()   # the native fp16 index holds the same rows
    s = R.exact_cos(R.link_gallery("e1_345"), R.link_gallery("e1_345"))
    assert s[0, 1] == 0.6 == R.ON and R.ABOVE > 0.6
    assert R.link_expected("thr_on") == [[1], [0], []] and R.link_expected("thr_above") == [[], [], []]
    G = R.link_gallery("zeros")
    assert ((G == 0).all(1).sum()) == 4
    assert R.link_expected("zeros_t0")[17] == list(range(0, 13))[:17][:12]   # a zero row: every score 0, index order
    for name in ("dups_m1", "dups_m12", "dups_m255"):
        kind, thr, ml, _, _ = R.LINK_CASES[name]
        G = R.link_gallery(kind)
        last = 20 + ml + 2
        assert (G[20:last + 1] == G[20]).all()
        row = R.exact_cos(G[last:last + 1], G)[0]
        top = np.lexsort((np.arange(len(G)), -row))[:ml + 1]
        assert last not in top, f"{name}: the last copy is in its own top-(max_links + 1)"
        got = R.link_expected(name)[last]
        assert len(got) == ml and last not in got
    assert {R.LINK_CASES[n][2] for n in R.LINK_CASES} >= {1, 12, 255}
    assert {len(R.link_gallery(v[0])) for v in R.LINK_CASES.values()} >= {1, 3, 300, 2500}
    assert any(len(R.link_gallery(v[0])) < v[2] + 1 for v in R.LINK_CASES.values())
    assert {R.link_gallery(v[0]).shape[1] for v in R.LINK_CASES.values()} >= {8, 96, 100, 128}
    assert any(v[4] != 0 for v in R.LINK_CASES.values())
    for edge in (64, 256):   # a batch that starts before the boundary and ends behind it, not on it
        assert any(r0 < edge < min(r0 + v[3], len(R.link_gallery(v[0]))) for v in R.LINK_CASES.values()
                   for r0 in range(0, len(R.link_gallery(v[0])), v[3]))


def test_rerank_cases_cover_the_issue():
    assert {c[0] for c in R.RERANK_CASES} == set(R.KCS)
    for kc in R.KCS:
        assert {c[1] for c in R.RERANK_CASES if c[0] == kc} == {1, kc}
        assert {c[2] for c in R.RERANK_CASES if c[0] == kc} == {0, 1, 2, 3}
    assert {(c[3], c[4]) for c in R.RERANK_CASES} == set(R.DDK)


@pytest.mark.parametrize("part", ["full", "short"])
@pytest.mark.parametrize("case", R.RERANK_CASES, ids=lambda c: "kc{}_top{}_w{}_d{}_dk{}".format(*c))
def test_rerank_families_meet_their_conditions(case, part):
    kc, topk, wi, d, dk = case
    qs, ref = _ref(case, part)
    assert R.finals_separated(ref["finals"])
    gal, cand, raw, valid = qs["gal"], qs["cand"], ref["raw"], ref["valid"]
    for a in (gal["G"], gal["kg"], qs["q_emb"], qs["q_kg"]):
        assert np.abs(a).max() <= 8 and (a == np.round(a)).all()
    q = {n: i for i, n in enumerate(qs["names"])}
    nv = valid.sum(1)
    if part == "full":
        assert (nv == kc).all()
        assert (qs["q_emb"][q["zero_qemb"]] == 0).all() and (raw[q["zero_qemb"], :, 0] == 0).all()
        assert (qs["q_kg"][q["zero_qkg"]] == 0).all() and (raw[q["zero_qkg"], :, 2] == 0).all()
        z = cand[q["zero_grow"]]
        assert (gal["G"][z] == 0).all(1).sum() == min(2, kc) and (raw[q["zero_grow"]][(gal["G"][z] == 0).all(1), 0] == 0).all()
        assert (gal["kg"][cand[q["zero_gkg"]]] == 0).all() and (raw[q["zero_gkg"], :, 2] == 0).all()
        assert qs["q_lab"][q["empty_labels"]] == 0 and (gal["lab"][cand[q["empty_labels"]]] == 0).any()
        assert (raw[q["empty_labels"], :, 1] == 0).all()
        b63 = np.uint64(1 << 63)
        assert qs["q_lab"][q["bit63"]] & b63 and (gal["lab"][cand[q["bit63"]]] & b63).any()
        for name, comp in (("const_emb", [0]), ("const_lab", [1]), ("const_kg", [2]), ("const_all", [0, 1, 2])):
            r = raw[q[name]]
            for p in range(3):
                const = (r[:, p] == r[0, p]).all()
                assert const if p in comp else (kc < 15 or not const), (name, p)
            if kc > 1:
                assert all(key in ("final",) or (ref[key][q[name]] == 0).all()
                           for key, p in (("e", 0), ("l", 1), ("k", 2)) if p in comp)
        if kc > 1:
            assert len(set(cand[q["const_all"]])) == kc      # distinct rows, identical in all three tables
            assert (ref["finals"][q["const_all"]] == 0).all()
            assert ref["idx"][q["const_all"]][0] == cand[q["const_all"]][kc - 1]   # later candidate first
            assert cand[q["dup_cand"]][0] == cand[q["dup_cand"]][kc - 1]
            t = cand[q["twin_rows"]]
            lo, hi = R.GRP["same_all"]
            assert ((t >= lo) & (t < hi)).sum() == 2
    else:
        assert nv[q["all_empty"]] == 0 and nv[q["one_valid"]] == 1
        assert (nv < kc).sum() >= len(nv) - 1 and (topk == 1 or (nv < topk).any())
        if kc >= 3:
            assert cand[q["hole_head"]][0] == -1 and (cand[q["hole_head"]][1:] >= 0).all()
            m = cand[q["hole_mid"]]
            assert m[kc // 2] == -1 and m[0] >= 0 and m[-1] >= 0
            assert cand[q["hole_tail"]][-1] == -1 and (cand[q["hole_tail"]][:-1] >= 0).all()
        if kc >= 4:
            h = cand[q["holes_dup"]]
            on = h[h >= 0]
            assert len(on) >= 2 and on[0] == on[-1]
    # equal adjacent finals come out later candidate first
    for qi in range(len(nv)):
        pos = {}
        for j in np.nonzero(valid[qi])[0]:
            pos.setdefault(int(cand[qi, j]), []).append(j)
        f, ids = ref["final"][qi], ref["idx"][qi]
        for r in range(min(topk, nv[qi]) - 1):
            if f[r] == f[r + 1] and ids[r] != ids[r + 1]:
                assert max(pos[int(ids[r])]) > min(pos[int(ids[r + 1])])

# ------------------------------------------------------------------------------------------------ (c) mutants

def test_merge_mutants_change_named_families():
    for name, mutant, out in (("equal_scores", "tie_high", 0), ("big_idx_equal", "tie_high", 0),
                              ("signed_zero", "tie_high", 2), ("duplicates_p3_k15", "payload_first", 3),
                              ("duplicates_p3_k4", "payload_first", 3), ("duplicates_p16_k18", "payload_first", 3)):
        c = R.merge_case(name)
        ref = R.merge_ref(c["s"], c["i"], c["k_out"], c["pay"], c["q0"], c["nq"])
        mut = R.merge_ref(c["s"], c["i"], c["k_out"], c["pay"], c["q0"], c["nq"], mutant=mutant)
        assert not np.array_equal(bits(ref[out]), bits(mut[out])), (name, mutant)


def test_link_mutants_change_named_families():
    kind, thr, ml, _, _ = R.LINK_CASES["thr_on"]
    assert R.link_ref(R.link_gallery(kind), thr, ml, mutant="gt") != R.link_expected("thr_on")
    kind, thr, ml, _, _ = R.LINK_CASES["zeros_t0"]   # orthogonal integer rows score exactly 0.0 = the threshold
    assert R.link_ref(R.link_gallery(kind), thr, ml, mutant="gt") != R.link_expected("zeros_t0")
    for name in ("thr_on", "dups_m1", "dups_m12", "dups_m255", "n2500", "n3_m12"):
        kind, thr, ml, _, _ = R.LINK_CASES[name]
        assert R.link_ref(R.link_gallery(kind), thr, ml, mutant="keep_self") != R.link_expected(name), name


def test_rerank_mutants_change_named_families():
    case = (15, 15, 0, 100, 3)
    assert case in R.RERANK_CASES
    qs, ref = _ref(case, "full")
    _, mut = _ref(case, "full", mutant="earlier_first")
    q = {n: i for i, n in enumerate(qs["names"])}
    for name in ("const_all", "twin_rows"):   # (the same candidate twice reads the same either way)
        assert not np.array_equal(ref["idx"][q[name]], mut["idx"][q[name]]), name
    assert np.array_equal(ref["idx"][q["plain"]], mut["idx"][q["plain"]])
    qs, ref = _ref(case, "short")
    _, mut = _ref(case, "short", mutant="minmax_all")
    q = {n: i for i, n in enumerate(qs["names"])}
    for name in ("hole_head", "hole_mid", "hole_tail", "holes_many", "one_valid"):
        assert not np.array_equal(ref["l"][q[name]], mut["l"][q[name]]), name   # Jaccard > 0: the 0.0 of an empty slot is a new minimum
        assert not np.array_equal(ref["final"][q[name]], mut["final"][q[name]]), name
