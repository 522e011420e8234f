"""CPU: the set-algorithm restatement of the DLS walk (tests/dls_walk_ref.py, the reference the device walk is
tested against) returns what the reference's heap walk returns: the same index lists as oracle.dls.walk_retrieve
for five parameter sets, and the golden's recorded walks (tests/golden/dls_rerank.npz: walk_idx / walk_score,
K = 5 on the reference's graph t50_m10) with scores within 1e-6 (the existing host-walk tolerance; the f64
expression differs from the recorded f32 scores by 1.4e-7 at most)."""
import os

import numpy as np
import pytest

from mmr_amd import synthetic
from oracle import dls as odls

from conftest import GOLDEN
from dls_walk_ref import walk
from test_oracle_dls import graph_from

# (K, seed_size, max_steps, candidate_multiplier)
PARAMS = [(5, 5, 100, 10), (3, 2, 4, 1), (10, 7, 100, 2), (1, 1, 100, 1), (50, 5, 100, 10)]


@pytest.fixture(scope="module")
def fx():
    f = np.load(os.path.join(GOLDEN, "dls_rerank.npz"), allow_pickle=False)
    G, _ = synthetic.dls_gallery()
    Qm, _ = synthetic.labelled_gallery(synthetic.DLS_Q, synthetic.DLS_D, synthetic.SEED + 12)
    return f, G, graph_from(f, "t50_m10"), Qm


def ref_seeds(n, seed_size, s):
    return np.random.RandomState(s).choice(n, size=min(seed_size, n), replace=False)


@pytest.mark.parametrize("K,seed_size,max_steps,cm", PARAMS)
def test_restatement_matches_heap_walk(fx, K, seed_size, max_steps, cm):
    f, G, graph, Qm = fx
    for qi in range(synthetic.DLS_Q):
        ref_i, ref_s = odls.walk_retrieve(G, graph, Qm[qi], K=K, seed_size=seed_size, max_steps=max_steps,
                                          candidate_multiplier=cm, seed=synthetic.SEED + qi)
        got_i, got_s, _, _ = walk(G, graph, Qm[qi], ref_seeds(len(G), seed_size, synthetic.SEED + qi), K, max_steps,
                                  r=max(cm * K, seed_size))
        assert got_i == ref_i, (qi, got_i, ref_i)
        np.testing.assert_allclose(got_s, ref_s, rtol=0, atol=1e-6)


def test_restatement_matches_golden(fx):
    f, G, graph, Qm = fx
    for qi in range(synthetic.DLS_Q):
        got_i, got_s, steps, visited = walk(G, graph, Qm[qi], ref_seeds(len(G), 5, synthetic.SEED + qi), 5)
        n = len(got_i)
        assert n == min(5, len(f["walk_idx"][qi]))
        assert got_i == f["walk_idx"][qi][:n].tolist()
        np.testing.assert_allclose(got_s, f["walk_score"][qi][:n], rtol=0, atol=1e-6)
        assert 0 <= steps <= 100 and visited >= n


def test_seed_stream_is_the_global_one():
    """RandomState(s).choice is np.random.seed(s); np.random.choice, and leaves the global state alone."""
    state = np.random.get_state()
    a = ref_seeds(1200, 5, 2709)
    assert all(np.array_equal(x, y) for x, y in zip(state, np.random.get_state()) if isinstance(x, np.ndarray))
    np.random.seed(2709)
    assert a.tolist() == np.random.choice(1200, size=5, replace=False).tolist()
    np.random.set_state(state)
