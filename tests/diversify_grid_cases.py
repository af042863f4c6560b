"""Host restatement and cases for the diversity grid (qrlsh.diversify_grid / evaluate_diversity; test infrastructure
only).

grid_ref restates qrlsh_diversify_grid from diversify_cases.greedy_ref (the rule), diversify_cases.redundancy_ref (the
in-list pairs) and a plain-Python scoring of the picks -- never from the project's device code.  Per (setting, request)
12 int64 words: listed, hits, known, the 1-based rank of the first hit, dcg, relevant test cells, test cells, avail, the
in-list pairs with sim > 0, their sim sum, the largest sim, the sum of red.  Per setting 24 totals: 0-7 the column sums
over the requests served, 8 requests served, 9 requests with a relevant test cell, 10 requests with a hit, 11 the ideal
DCG, 12 / 13 the sums of words 8 / 9, 14 the maximum of word 10, 15 the sum of word 11, 16 requests whose list is not the
plain prefix of their pool, 17 requests that ended before min(k, n), 18-23 zero."""
import numpy as np

import diversify_cases as DC
import rank_eval_cases as RC

LINE, TOTALS = 12, 24
RELEVANT = 60

_greedy = {}


def greedy_of(case, penalty, max_sim):
    """greedy_ref of a Case under one setting, computed once per (case, setting)"""
    key = (case.name, case.N, case.k, len(case.rows), penalty, max_sim)
    if key not in _greedy:
        _greedy[key] = DC.greedy_ref(*case.arrays(), case.lists, case.k, penalty, max_sim)
    return _greedy[key]


def grid_ref(arrays, lists, k, settings, truth=None, users=None, relevant=None, gains=None, request_counts=None,
             greedy=None, redundancy=None):
    """arrays: (cand_idx, cand_val, avail) of a call; lists: {q: (ids, milli)}; settings: (penalty, max_sim) pairs.
    truth: None or int [nu][nq], then users (None: request x is row x), relevant, gains (k integers) and
    request_counts (None or [m][2]).  greedy / redundancy: callables that replace greedy_ref(penalty, max_sim) and
    redundancy_ref(idx) (a cache, or the dense brute form).
    -> (per int64 [S][m][12], totals int64 [S][24], (idx, val, red int32 [S][m][k], count int32 [S][m]))"""
    ci, cv, av = (np.asarray(a) for a in arrays)
    m, N = ci.shape
    S = len(settings)
    per = np.zeros((S, m, LINE), dtype=np.int64)
    totals = np.zeros((S, TOTALS), dtype=np.int64)
    out = (np.full((S, m, k), -1, dtype=np.int32), np.zeros((S, m, k), dtype=np.int32),
           np.zeros((S, m, k), dtype=np.int32), np.zeros((S, m), dtype=np.int32))
    if truth is not None:
        truth = np.asarray(truth)
        gains = [int(g) for g in gains]
        assert len(gains) == k and relevant >= 1
    for s, (penalty, max_sim) in enumerate(settings):
        idx, val, red, count = greedy(penalty, max_sim) if greedy else DC.greedy_ref(ci, cv, av, lists, k, penalty,
                                                                                   max_sim)
        words, _ = redundancy(idx) if redundancy else DC.redundancy_ref(idx, lists)
        for x in range(m):
            user = x if users is None else int(users[x])
            served = int(av[x]) >= 0 and (truth is None or 0 <= user < truth.shape[0])
            per[s, x, 7] = int(av[x])
            if not served:
                continue
            out[0][s, x], out[1][s, x], out[2][s, x], out[3][s, x] = idx[x], val[x], red[x], count[x]
            t, n = int(count[x]), min(N, int(av[x]))
            hits = known = first = dcg = rel_cells = test_cells = 0
            if truth is not None:
                for p in range(t):
                    tv = int(truth[user, int(idx[x, p])])
                    if tv != 0:
                        known += 1
                    if tv >= relevant:
                        hits += 1
                        dcg += gains[p]
                        if first == 0:
                            first = p + 1
                if request_counts is not None:
                    rel_cells, test_cells = int(request_counts[x][0]), int(request_counts[x][1])
            line = [t, hits, known, first, dcg, rel_cells, test_cells, int(av[x]), int(words[x, 1]), int(words[x, 2]),
                    int(words[x, 3]), int(red[x, :t].sum())]
            assert words[x, 0] == t
            per[s, x] = line
            early = t < min(k, n)
            moved = early or any(int(idx[x, p]) != int(ci[x, p]) for p in range(t))
            tot = totals[s]
            tot[:8] += line[:8]
            tot[8] += 1
            if truth is not None:
                tot[9] += rel_cells > 0
                tot[10] += hits > 0
                tot[11] += sum(gains[:min(k, max(rel_cells, 0))])
            tot[12] += line[8]
            tot[13] += line[9]
            tot[14] = max(tot[14], line[10])
            tot[15] += line[11]
            tot[16] += moved
            tot[17] += early
    return per, totals, out


def truth_case(nu=37, seed=91):
    """-> (truth int32 [nu][NQ], relevant): ratings 1 .. 100 at about 0.6 of the cells, 0 elsewhere"""
    rng = np.random.default_rng(seed)
    truth = rng.integers(1, 101, (nu, DC.NQ)) * (rng.random((nu, DC.NQ)) < 0.6)
    return truth.astype(np.int32), RELEVANT


def users_of(m, nu=37):
    """request x is user (5 x) % nu: repeated and unordered"""
    return np.array([(5 * x) % nu for x in range(m)], dtype=np.int32)


def counts_of(arrays, truth, users, relevant):
    """request_counts for a planted call, int64 [m][2]: the relevant cells and the rated cells of the user's truth among
    the pool's columns (what a held-out split would call the relevant test cells and the test cells; 0 for an empty
    pool, so some requests have no relevant test cell)"""
    ci, _, av = arrays
    out = np.zeros((len(av), 2), dtype=np.int64)
    for x in range(len(av)):
        n = min(ci.shape[1], max(int(av[x]), 0))
        row = truth[int(users[x]), ci[x, :n].astype(np.int64)]
        out[x] = int((row >= relevant).sum()), int((row != 0).sum())
    return out


def scored(case, settings=DC.SETTINGS):
    """a Case under `settings` with truth_case's truth: -> (kwargs of the scoring, grid_ref's triple); computed once"""
    key = (case.name, case.N, case.k, len(case.rows), tuple(settings))
    if key not in _scored:
        truth, relevant = truth_case()
        arrays = case.arrays()
        users = users_of(len(arrays[2]))
        kw = dict(truth=truth, users=users, relevant=relevant, gains=RC.dcg_gains_ref(case.k),
                  request_counts=counts_of(arrays, truth, users, relevant))
        _scored[key] = (kw, grid_ref(arrays, case.lists, case.k, settings,
                                     greedy=lambda p, ms: greedy_of(case, p, ms), **kw))
    return _scored[key]


_scored = {}
