"""Test infrastructure (numpy only): the DLS walk of src/Retrieval/retrieval.py:198-244 restated as the set
algorithm include/mmr.h states for mmr_index_dls_walk, scored in f64.

score(i) = <g_i, q> / (|g_i| * (|q| + 1e-6) + 1e-12) from the f32 rows in f64; order (score desc, index asc);
the set and `visited` start as the seeds (invalid or repeated ones skipped); a step removes the best row, adds its
unvisited valid neighbours, keeps the best r, stops uncounted when nothing was added; the output is the best
min(k, |set|) in (score desc, index DESC) order."""
import numpy as np


def walk(embs, graph, q, seeds, k, max_steps=100, r=None):
    """graph: neighbour lists or an (n, max_links) table (-1 padded).  -> (idx list, score list (f64), steps,
    visited count); r defaults to max(10 k, len(seeds))."""
    E = np.asarray(embs, np.float32).astype(np.float64)
    qv = np.asarray(q, np.float32).astype(np.float64).reshape(-1)
    n = E.shape[0]
    r = max(10 * k, len(seeds)) if r is None else r
    qn = np.sqrt(qv @ qv) + 1e-6

    def score(i):
        return float((E[i] @ qv) / (np.sqrt(E[i] @ E[i]) * qn + 1e-12))

    visited, cand = set(), {}
    for s in seeds:
        s = int(s)
        if 0 <= s < n and s not in visited:
            visited.add(s)
            cand[s] = score(s)
    steps = 0
    while steps < max_steps and cand:
        best = min(cand, key=lambda i: (-cand[i], i))
        del cand[best]
        added = False
        for v in graph[best]:
            v = int(v)
            if v < 0 or v >= n or v in visited:
                continue
            visited.add(v)
            cand[v] = score(v)
            added = True
        if len(cand) > r:
            keep = sorted(cand, key=lambda i: (-cand[i], i))[:r]
            cand = {i: cand[i] for i in keep}
        if not added:
            break
        steps += 1
    top = sorted(cand, key=lambda i: (-cand[i], i))[:k]
    top = sorted(top, key=lambda i: (cand[i], i), reverse=True)
    return top, [cand[i] for i in top], steps, len(visited)


def walk_batch(embs, graph, Q, seeds, k, max_steps=100, r=None):
    """-> idx (B, k) int64 (-1 padded), score (B, k) f64 (-inf padded), steps (B,), visited (B,)."""
    B = len(Q)
    idx = np.full((B, k), -1, np.int64)
    sc = np.full((B, k), -np.inf, np.float64)
    st, vis = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        i, s, st[b], vis[b] = walk(embs, graph, Q[b], seeds[b], k, max_steps, r)
        idx[b, :len(i)] = i
        sc[b, :len(i)] = s
    return idx, sc, st, vis
