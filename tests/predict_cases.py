"""Seeded prediction cases whose cells sit on a rounding knife edge (test infrastructure only).

N1 (csrc/predict.hip, recommender.py:36-47 and 301-331) promises bit-exact float64: both orders of
weighted_average's two sums, the blend in the reference's operand order without FMA contraction, and Python's
half-to-even round.  On random data a wrong order or rounding almost never shows.  Here most zero cells are
built so that the REAL value of the blend is exactly k + 1/2:

* a cell's rated neighbours hold two ratings, c (group L) and c + 1 (group H), and the weights are split so that
  W(H) / (W(H) + W(L)) is a chosen fraction: the weighted average is then exactly c + p/q in real arithmetic;
* per branch of the blend (recommender.py:324-331, weights 0.6 / 0.4, mean 60) the denominators are
    query-only  0.8 qp + 12          eighths on the query side,
    user-only   0.7 up + 18          sevenths on the user side,
    both        0.6 qp + 0.4 up      sixths on both sides,
  and c (and the other side's base) is chosen so that the blend is k + 1/2;
* the similarities are milli values / 1000, as the hot path and the reference produce them, so the float64
  result lies a few ulps from k + 1/2 -- or on it -- and which side it lands on depends on the summation order,
  the rounding mode and contraction.

Layout: users [0, tu) and queries [0, tq) are the targets; every target (user i, query j) cell is 0.  Each target
query owns a private block of neighbour queries and each target user a private block of neighbour users, so that
row i over query j's block (the query side of cell (i, j)) and column j over user i's block (its user side) can be
set per cell.  Unrated neighbours are interleaved with the rated ones.  Everything else -- the remaining users,
queries and their lists -- is ordinary random data.  The last query is referenced by no query list ("spare"): a
test may change its column without moving any prediction outside it."""
from fractions import Fraction

import numpy as np

QW, UW, DM = Fraction(3, 5), Fraction(2, 5), 60     # recommender.py:32-34, exact
DENOM = {"q": (8, None), "u": (None, 7), "b": (6, 6)}   # branch -> (query-side, user-side) denominator
BRANCHES = ("q", "u", "b")


def sequential_sum(a):
    """numba's nopython np.sum: one accumulator, index order (the drop-in Recommender's default order)"""
    r = 0.0
    for v in a:
        r += float(v)
    return r


def blend_real(branch, qp, up):
    """the blend of recommender.py:324-331 in exact arithmetic"""
    if branch == "q":
        return qp * (QW + UW / 2) + DM * (UW / 2)
    if branch == "u":
        return up * (UW + QW / 2) + DM * (QW / 2)
    return qp * QW + up * UW


def list_length(rng, longest):
    """a neighbour-list length: 1-7, 8-32 with n % 8 != 0 and == 0, 33-64 (capped at `longest`)"""
    while True:
        kind = rng.integers(0, 4)
        if kind == 0:
            n = int(rng.integers(1, 8))
        elif kind == 1:
            n = int(rng.choice([8, 16, 24, 32]))
        elif kind == 2:
            n = int(rng.choice([k for k in range(9, 32) if k % 8]))
        else:
            n = int(rng.integers(33, 65))
        if n <= longest:
            return n


def _subset_sum(rng, vals, target):
    """indexes (into vals) of a random subset summing to target, or None (bitset DP, random item order)"""
    order = rng.permutation(len(vals))
    mask = (1 << (target + 1)) - 1
    reach = [1]
    for k in order:
        reach.append((reach[-1] | (reach[-1] << int(vals[k]))) & mask)
    if not (reach[-1] >> target) & 1:
        return None
    pick, t = [], target
    for s in range(len(order) - 1, -1, -1):
        if (reach[s] >> t) & 1:
            continue
        pick.append(int(order[s]))
        t -= int(vals[order[s]])
    return pick


def _split(rng, w, q):
    """(H, L, fraction) with W(H) / W(H + L) = fraction, a multiple of 1/q in (0, 1) -- or, when q is None or no
    split is found, fraction 0: H empty, L a random non-empty subset"""
    n = len(w)
    if q is not None and n >= 2:
        for _ in range(12):
            h = int(rng.integers(1, min(3, n - 1) + 1))
            H = [int(x) for x in rng.choice(n, size=h, replace=False)]
            wh = int(sum(w[k] for k in H))
            rest = [k for k in range(n) if k not in H]
            room = int(sum(w[k] for k in rest))
            ps = [p for p in range(1, q) if (wh * (q - p)) % p == 0 and wh * (q - p) // p <= room]
            if not ps:
                continue
            p = int(rng.choice(ps))
            pick = _subset_sum(rng, [w[k] for k in rest], wh * (q - p) // p)
            if pick is not None:
                return H, [rest[k] for k in pick], Fraction(p, q)
    m = int(rng.integers(1, n + 1))
    return [], [int(x) for x in rng.choice(n, size=m, replace=False)], Fraction(0)


def _bases(rng, branch, fq, fu, hq, hu):
    """(c_q, c_u): the ratings of group L on each side, with blend_real(c_q + fq, c_u + fu) = k + 1/2, or None"""
    top_q, top_u = 100 - (1 if hq else 0), 100 - (1 if hu else 0)
    sols = []
    for a in range(1, 11) if branch != "u" else [1]:
        for b in range(1, 11) if branch != "q" else [1]:
            v = blend_real(branch, a + fq, b + fu)
            if v - (v.numerator // v.denominator) == Fraction(1, 2):
                sols.append((a, b))
    if not sols:
        return None
    a, b = sols[int(rng.integers(0, len(sols)))]
    a += 10 * int(rng.integers(0, (top_q - a) // 10 + 1))
    b += 10 * int(rng.integers(0, (top_u - b) // 10 + 1))
    return a, b


class PredictCase:
    """ratings int32 [nu][nq]; qs / us: {id: {'indexes', 'values'}} (the oracle's form, lists in stored order);
    knife: int64 [n][2] knife-edge cells; branch: their branch ('q' / 'u' / 'b'); spare: the unreferenced query"""

    def __init__(self, ratings, qs, us, knife, branch, spare):
        self.ratings, self.qs, self.us, self.knife, self.branch, self.spare = ratings, qs, us, knife, branch, spare
        self.nu, self.nq = ratings.shape

    def coo(self):
        """(q_src, q_dst, q_milli) int32 torch tensors sorted by source: what fill_predictions takes"""
        import torch
        src, dst, mil = [], [], []
        for j in sorted(self.qs):
            idx = self.qs[j]["indexes"]
            src += [j] * len(idx)
            dst += idx.tolist()
            mil += np.rint(self.qs[j]["values"] * 1000).astype(np.int64).tolist()
        return tuple(torch.tensor(x, dtype=torch.int32) for x in (src, dst, mil))

    def csr(self):
        """(q_off int64 [nq + 1], q_idx int32, q_val float64) as qrlsh_predict takes them"""
        deg = np.zeros(self.nq, dtype=np.int64)
        for j, v in self.qs.items():
            deg[j] = len(v["indexes"])
        q_off = np.concatenate(([0], np.cumsum(deg))).astype(np.int64)
        q_idx = np.zeros(int(q_off[-1]), dtype=np.int32)
        q_val = np.zeros(int(q_off[-1]), dtype=np.float64)
        for j, v in self.qs.items():
            q_idx[q_off[j]:q_off[j + 1]] = v["indexes"]
            q_val[q_off[j]:q_off[j + 1]] = v["values"]
        return q_off, q_idx, q_val

    def user_lists(self, ku=None):
        """(u_idx int32 [nu][ku], u_val float64 [nu][ku]) padded with -1 / 0 to ku (default: the longest list)"""
        longest = max(len(v["indexes"]) for v in self.us.values())
        ku = max(longest, 1) if ku is None else ku
        assert ku >= longest
        ui = np.full((self.nu, ku), -1, dtype=np.int32)
        uv = np.zeros((self.nu, ku), dtype=np.float64)
        for u, v in self.us.items():
            ui[u, :len(v["indexes"])] = v["indexes"]
            uv[u, :len(v["indexes"])] = v["values"]
        return ui, uv

    def longest_query_list(self):
        return max((len(v["indexes"]) for v in self.qs.values()), default=0)


def _milli_list(rng, n, positive):
    return np.sort(rng.integers(1 if positive else 0, 1001, size=n))[::-1]


def _knife_milli_list(rng, n):
    """a target's similarities: half of the lists random milli values, half small multiples of one unit (ties
    and common factors, as rounded cosines have them), which admit far more exact splits on short lists"""
    if rng.random() < 0.5:
        return _milli_list(rng, n, True)
    unit = int(rng.integers(1, 126))
    return np.sort(unit * rng.integers(1, 9, size=n))[::-1]


def build_case(seed, nu, nq, tu, tq, user_longest=64, query_longest=64, fill=0.5, ordinary_query_longest=28,
               ordinary_user_longest=19):
    """A seeded case: tu x tq knife-edge cells (fewer where a list's weights admit no exact split), the rest of
    the matrix random with `fill` rated, every user with a list (user lists up to `user_longest`), about 80 %
    of the non-target queries with one.  Private blocks are drawn while the pools last; a target whose block
    cannot be had gets a short list from what is left."""
    rng = np.random.default_rng(seed)
    spare = nq - 1
    ratings = (rng.integers(1, 101, size=(nu, nq)) * (rng.random((nu, nq)) < fill)).astype(np.int32)
    qs, us = {}, {}
    # private blocks
    qpool = list(rng.permutation(np.arange(tq, spare)))
    upool = list(rng.permutation(np.arange(tu, nu)))
    for j in range(tq):
        n = min(list_length(rng, query_longest), len(qpool))
        if n == 0:
            continue
        idx = np.array([qpool.pop() for _ in range(n)], dtype=np.int64)
        qs[j] = {"indexes": idx, "values": _knife_milli_list(rng, n) / 1000.0}
    for i in range(tu):
        n = min(list_length(rng, user_longest), len(upool))
        idx = np.array([upool.pop() for _ in range(n)], dtype=np.int64)
        us[i] = {"indexes": idx, "values": _knife_milli_list(rng, n) / 1000.0}
    # ordinary lists: never the spare query, never a duplicate inside a list
    for j in range(tq, nq):
        if rng.random() < 0.8:
            n = int(rng.integers(1, min(ordinary_query_longest, query_longest, spare) + 1))
            idx = rng.choice(spare, size=n, replace=False).astype(np.int64)
            qs[j] = {"indexes": idx, "values": _milli_list(rng, n, False) / 1000.0}
    for u in range(tu, nu):
        n = int(rng.integers(1, min(ordinary_user_longest, user_longest, nu) + 1))
        idx = rng.choice(nu, size=n, replace=False).astype(np.int64)
        us[u] = {"indexes": idx, "values": _milli_list(rng, n, False) / 1000.0}
    # the target block: every cell 0, its two neighbourhoods set per cell
    ratings[:tu, :tq] = 0
    knife, branch = [], []
    for i in range(tu):
        ul = us[i]
        wu = np.rint(ul["values"] * 1000).astype(np.int64)
        for j in range(tq):
            ql = qs.get(j)
            choices = [b for b in BRANCHES if (b != "q" or ql is not None) and (b != "u" or len(wu))
                       and (b != "b" or (ql is not None and len(wu)))]
            row_q = np.zeros(0 if ql is None else len(ql["indexes"]), dtype=np.int32)
            col_u = np.zeros(len(wu), dtype=np.int32)
            # the first branch whose weights split; user-only last (it also takes an unsplit list: 0.7 c + 18)
            order = [str(b) for b in rng.permutation([b for b in choices if b != "u"])] + [b for b in choices if b == "u"]
            for b in order:
                dq, du = DENOM[b]
                hq = lq = hu = lu = []
                fq = fu = Fraction(0)
                if b in ("q", "b"):
                    hq, lq, fq = _split(rng, np.rint(ql["values"] * 1000).astype(np.int64), dq)
                if b in ("u", "b"):
                    hu, lu, fu = _split(rng, wu, du)
                base = _bases(rng, b, fq, fu, len(hq), len(hu))
                if base is not None:
                    row_q[lq] = base[0]
                    row_q[hq] = base[0] + 1
                    col_u[lu] = base[1]
                    col_u[hu] = base[1] + 1
                    knife.append((i, j))
                    branch.append(str(b))
                    break
            if ql is not None:
                ratings[i, ql["indexes"]] = row_q
            ratings[ul["indexes"], j] = col_u
    return PredictCase(ratings, qs, us, np.array(knife, dtype=np.int64).reshape(-1, 2), np.array(branch), spare)
