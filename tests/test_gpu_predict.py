"""N1 on the device (csrc/predict.hip) held to oracle.predict_cells on knife-edge cells (tests/predict_cases.py):
cells whose real blend is exactly k + 1/2, so that the float64 result depends on the summation order, on
half-to-even rounding and on the absence of FMA contraction.  qrlsh_predict has five forms:

  F1  one thread per cell over the CSR lists                 kq = 0 (no workspace)
  F2  tile, 64 users x 16 queries over a byte copy            ku <= 32 and every rating in 0 .. 255
  F3  row, the user's row staged in LDS                       otherwise, nq <= 131072, the row's ratings in 0 .. 255
  F4  row, the row read from memory                           as F3, for a row holding a rating outside 0 .. 255
  F5  one thread per cell over the transposed lists           otherwise, nq > 131072

Each form is reached through the C ABI with legal inputs only: user lists padded with -1 beyond 32 columns
(F3, F5), a rating of 300 in some rows of the spare column -- a query no list references, so only that column's
predictions move (F4, F5) -- and nq on both sides of 131072."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import oracle as O
import predict_cases as PC

pytestmark = pytest.mark.gpu

from qrlsh import _lib, predict  # noqa: E402

DEV = "cuda"
SAMPLE = 20_000
ORDERS = {"pairwise": (_lib.SUM_PAIRWISE, O.np_sum_order), "sequential": (_lib.SUM_SEQUENTIAL, PC.sequential_sum)}
PAD_KU = 40       # a user-list stride beyond the tile form's 32
WIDE = 300        # a rating that does not fit a byte


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def form_of(nq, ku, kq, wide):
    """the form qrlsh_predict runs (the dispatch of predict.hip restated, grid limits aside)"""
    if kq == 0:
        return "F1"
    if ku <= 32 and not wide:
        return "F2"
    if nq <= 131072:
        return "F4" if wide else "F3"
    return "F5"


class DeviceLists:
    """one case's lists on the device: CSR query lists, user lists padded to any stride"""

    def __init__(self, q_off, q_idx, q_val, ui, uv):
        self.q = [_dev(x) for x in (q_off, q_idx, q_val)]
        self.kq = int(np.diff(q_off).max()) if len(q_off) > 1 else 0
        self.ku = int((ui >= 0).sum(1).max())
        self.ui, self.uv = ui, uv
        self.users = {}

    @classmethod
    def of(cls, case):
        return cls(*case.csr(), *case.user_lists())

    def user(self, ku):
        """(u_idx, u_val) on the device with row stride ku (-1 / 0 padded)"""
        if ku not in self.users:
            nu = self.ui.shape[0]
            ui = np.full((nu, ku), -1, dtype=np.int32)
            uv = np.zeros((nu, ku), dtype=np.float64)
            w = min(ku, self.ui.shape[1])
            assert (self.ui[:, w:] < 0).all()
            ui[:, :w], uv[:, :w] = self.ui[:, :w], self.uv[:, :w]
            self.users[ku] = (_dev(ui), _dev(uv))
        return self.users[ku]


def c_predict(lists, ratings, order, ku, kq, weights=(0.6, 0.4, 60.0), out=None, ws=None):
    """qrlsh_predict through the C ABI; a fresh output (filled with -7) and workspace unless given"""
    lib = _lib.load()
    nu, nq = ratings.shape
    if out is None:
        out = torch.full((nu, nq), -7, dtype=torch.int32, device=DEV)
    if kq and ws is None:
        ws = torch.empty((int(lib.qrlsh_predict_workspace_bytes(nu, nq, kq)),), dtype=torch.uint8, device=DEV)
    flag = torch.zeros((1,), dtype=torch.int32, device=DEV)
    u_idx, u_val = lists.user(ku)
    rc = lib.qrlsh_predict(_vp(ratings), nu, nq, *map(_vp, lists.q), _vp(u_idx), _vp(u_val), ku, *map(float, weights),
                           ORDERS[order][0], _vp(out), _vp(flag), kq, _vp(ws) if kq else None,
                           ws.numel() if kq else 0, None)
    assert rc == 0, lib.qrlsh_last_error()
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    return out


def sample_cells(seed, nu, nq, n, exclude_col=None):
    rng = np.random.default_rng(seed)
    i = rng.integers(0, nu, size=2 * n)
    j = rng.integers(0, nq - (1 if exclude_col == nq - 1 else 0), size=2 * n)
    flat = np.unique(i * nq + j)
    flat = flat[rng.permutation(len(flat))[:n]]
    return np.stack([flat // nq, flat % nq], axis=1)


def at(out, cells):
    return out[torch.from_numpy(cells[:, 0]).to(DEV), torch.from_numpy(cells[:, 1]).to(DEV)].cpu().numpy()


def assert_cells(out, ratings, qs, us, cells, order, want=None, **weights):
    if want is None:
        want = O.predict_cells(ratings, qs, us, cells, summation=ORDERS[order][1], **weights)
    got = at(out, cells)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%d of %d cells differ, first %s: device %d, oracle %d" % (
        len(bad), len(cells), cells[bad[0]].tolist(), got[bad[0]], want[bad[0]])


# ---------------------------------------------------------------------------- orders and rounding, fill_predictions
@pytest.fixture(scope="module", params=[32, 64], ids=["user_lists_to_32", "user_lists_to_64"])
def knife_case(request):
    return PC.build_case(300 + request.param, nu=1500, nq=6000, tu=24, tq=120, user_longest=request.param)


def test_fill_predictions_summation_orders_and_rounding_on_knife_cells(knife_case):
    """fill_predictions in both sum_orders and both transpose_lists (user lists to 32: tile form or cells; to 64:
    row form or cells) equals predict_cells in the same order on every knife cell and a sample of the rest; and
    on the cells where the two orders round differently, the two device results differ -- the flag reaches the
    kernel, through predict.py's mapping"""
    c = knife_case
    coo = c.coo()
    cells = np.concatenate([c.knife, sample_cells(1, c.nu, c.nq, SAMPLE)])
    want = {o: O.predict_cells(c.ratings, c.qs, c.us, cells, summation=ORDERS[o][1]) for o in ORDERS}
    flips = cells[want["pairwise"] != want["sequential"]]
    assert len(flips) >= 20
    for tl in (True, False):
        got = {}
        for o in ORDERS:
            out = predict.fill_predictions(c.ratings, *coo, c.us, device=DEV, sum_order=o, transpose_lists=tl)
            got[o] = at(out, cells)
            bad = np.flatnonzero(got[o] != want[o])
            assert len(bad) == 0, "%s, transpose_lists=%s: %d of %d cells differ, first %s" % (
                o, tl, len(bad), len(cells), cells[bad[0]].tolist())
        differ = got["pairwise"] != got["sequential"]
        assert np.array_equal(cells[differ], flips), "transpose_lists=%s" % tl


# ---------------------------------------------------------------------------- every form through the C ABI
SHAPES = {   # name -> (builder arguments, forms reached)
    # F3 / F4 at the largest row the LDS holds
    "nq131072": (dict(seed=11, nu=220, nq=131072, tu=8, tq=160, user_longest=32), ["F1", "F2", "F3", "F4", "F4_padded"]),
    # one query more: the cell form over the transposed lists instead
    "nq131073": (dict(seed=12, nu=220, nq=131073, tu=8, tq=160, user_longest=32), ["F1", "F2", "F5", "F5_wide"]),
    # 3 users: 49 row slices of 1021 cells
    "nu3": (dict(seed=13, nu=3, nq=50001, tu=1, tq=200, user_longest=2), ["F1", "F2", "F3", "F4", "F4_padded"]),
    # partial tiles both ways (333 % 64, 5003 % 16)
    "nu333_nq5003": (dict(seed=14, nu=333, nq=5003, tu=10, tq=100, user_longest=32),
                     ["F1", "F2", "F3", "F4", "F4_padded"]),
    # user lists of 33-64: no tile form
    "user_lists_to_64": (dict(seed=15, nu=1200, nq=6000, tu=20, tq=100, user_longest=64), ["F1", "F3", "F4"]),
}
FORM_RUNS = {   # form -> (the wide matrix, user lists padded beyond 32, workspace)
    "F1": (False, False, False), "F2": (False, False, True), "F3": (False, True, True), "F4": (True, False, True),
    "F4_padded": (True, True, True), "F5": (False, True, True), "F5_wide": (True, False, True)}


class ShapeCase:
    """one shape's case on the device, the oracle's values on its knife cells + sample (base matrix) and on the
    spare column (wide matrix), and F1 on the base matrix per order -- built once for all of its forms"""

    def __init__(self, shape):
        kw = dict(SHAPES[shape][0])
        c = self.c = PC.build_case(kw.pop("seed"), **kw)
        self.L = DeviceLists.of(c)
        self.wide = c.ratings.copy()
        self.wide[np.arange(c.nu) % 3 == 1, c.spare] = WIDE          # some rows only: LDS and memory rows mix
        self.base_t, self.wide_t = _dev(c.ratings), _dev(self.wide)
        self.cells = np.concatenate([c.knife, sample_cells(2, c.nu, c.nq, SAMPLE, exclude_col=c.spare)])
        self.col = np.stack([np.arange(c.nu), np.full(c.nu, c.spare)], axis=1)
        self.f1, self.want = {}, {}

    def want_cells(self, order):
        if order not in self.want:
            self.want[order] = O.predict_cells(self.c.ratings, self.c.qs, self.c.us, self.cells,
                                               summation=ORDERS[order][1])
        return self.want[order]

    def f1_out(self, order):
        if order not in self.f1:
            self.f1[order] = c_predict(self.L, self.base_t, order, self.L.ku, 0)
        return self.f1[order]


_CASE = {}


def shape_case(shape):
    if shape not in _CASE:
        _CASE.clear()      # one shape's device buffers at a time
        _CASE[shape] = ShapeCase(shape)
    return _CASE[shape]


@pytest.mark.parametrize("shape,form", [(s, f) for s in SHAPES for f in SHAPES[s][1]])
def test_every_form_is_bit_equal_to_the_cell_form_and_the_oracle(shape, form):
    """per case and form, both orders: the form is bit-equal to F1 on the whole matrix (on the wide matrix: outside
    the spare column, and the whole spare column equals predict_cells); the knife cells and a sample of 20 000
    others equal predict_cells"""
    s = shape_case(shape)
    c, L = s.c, s.L
    wide, padded, ws = FORM_RUNS[form]
    ku = max(PAD_KU, L.ku) if padded else L.ku
    kq = L.kq if ws else 0
    assert form_of(c.nq, ku, kq, wide) == form[:2], (form, ku, kq)
    if shape == "user_lists_to_64":
        assert L.ku > 32
    for order in ORDERS:
        ref = s.f1_out(order)
        out = ref if form == "F1" else c_predict(L, s.wide_t if wide else s.base_t, order, ku, kq)
        if wide:
            assert torch.equal(out[:, :-1], ref[:, :-1]), order
            assert_cells(out, s.wide, c.qs, c.us, s.col, order)
        else:
            assert torch.equal(out, ref), order
        assert_cells(out, c.ratings, c.qs, c.us, s.cells, order, want=s.want_cells(order))


# ---------------------------------------------------------------------------- the bench shape
def test_bench_shape_forms_and_sample():
    """bench.py's N1 workload, restated: 2000 users x 100 000 queries, ratings 1..100 with 75 % of the cells
    unrated, 0..28 query neighbours (milli similarities, sorted descending over the whole list array), 19 user
    neighbours (random users, similarities rounded to 3 decimals).  F2 (what bench.py runs), F1 and F3 (user
    lists padded to 40) are bit-equal on the whole matrix; a sample of 20 000 cells and every cell of 4 columns
    equal predict_cells, in both orders"""
    nu, nq = 2000, 100_000
    kq_max, ku = round(math.log(nq, 1.5)), round(math.log(nu, 1.5))
    rng = np.random.default_rng(2000)
    ratings = rng.integers(1, 101, size=(nu, nq), dtype=np.int32)
    for r0 in range(0, nu, 250):
        ratings[r0:r0 + 250][rng.random((min(250, nu - r0), nq), dtype=np.float32) < 0.75] = 0
    deg = rng.integers(0, kq_max + 1, size=nq)
    q_off = np.concatenate(([0], np.cumsum(deg))).astype(np.int64)
    q_idx = rng.integers(0, nq, size=int(q_off[-1])).astype(np.int32)
    q_val = np.sort(rng.integers(0, 1001, size=int(q_off[-1])))[::-1] / 1000.0
    ui = rng.integers(0, nu, size=(nu, ku)).astype(np.int32)
    uv = np.round(rng.random((nu, ku)), 3)
    qs = {j: {"indexes": q_idx[q_off[j]:q_off[j + 1]].astype(np.int64), "values": q_val[q_off[j]:q_off[j + 1]]}
          for j in np.flatnonzero(deg).tolist()}
    us = {u: {"indexes": ui[u].astype(np.int64), "values": uv[u]} for u in range(nu)}
    L = DeviceLists(q_off, q_idx, q_val, ui, uv)
    assert L.kq == kq_max and L.ku == ku
    r = _dev(ratings)
    cols = rng.choice(nq, size=4, replace=False)
    cells = np.concatenate([sample_cells(3, nu, nq, SAMPLE)] +
                           [np.stack([np.arange(nu), np.full(nu, j)], axis=1) for j in cols])
    for order in ORDERS:
        f2 = c_predict(L, r, order, ku, L.kq)
        assert torch.equal(c_predict(L, r, order, ku, 0), f2)
        assert torch.equal(c_predict(L, r, order, PAD_KU, L.kq), f2)
        assert_cells(f2, ratings, qs, us, cells, order)


# ---------------------------------------------------------------------------- parameters, workspace reuse
@pytest.fixture(scope="module")
def small_case():
    c = PC.build_case(16, nu=333, nq=5003, tu=10, tq=100, user_longest=32)
    wide = c.ratings.copy()
    wide[np.arange(c.nu) % 3 == 1, c.spare] = WIDE
    return c, wide, DeviceLists.of(c)


def test_non_default_weights_and_mean_reach_the_kernel(small_case):
    """query_weight 0.7, user_weight 0.3, default_mean 55 through the C ABI (F1, F2, F3) against predict_cells
    with the same values, in both orders"""
    c, _, L = small_case
    r = _dev(c.ratings)
    cells = np.concatenate([c.knife, sample_cells(4, c.nu, c.nq, SAMPLE)])
    w = dict(query_weight=0.7, user_weight=0.3, default_mean=55)
    for order in ORDERS:
        outs = [c_predict(L, r, order, ku, kq, weights=(0.7, 0.3, 55.0))
                for ku, kq in ((L.ku, 0), (L.ku, L.kq), (PAD_KU, L.kq))]
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        assert_cells(outs[0], c.ratings, c.qs, c.us, cells, order, **w)
        assert not torch.equal(outs[0], c_predict(L, r, order, L.ku, 0))


def test_one_workspace_and_output_across_wide_and_byte_calls(small_case):
    """back-to-back calls sharing one workspace and one output, alternating a wide and a byte-range matrix and
    the two orders (tile and row forms taking turns over the same flag word and output): each result equals a
    fresh call with a new workspace and a -7-filled output"""
    c, wide, L = small_case
    lib = _lib.load()
    mats = [_dev(c.ratings), _dev(wide)]
    ws = torch.empty((int(lib.qrlsh_predict_workspace_bytes(c.nu, c.nq, L.kq)),), dtype=torch.uint8, device=DEV)
    out = torch.full((c.nu, c.nq), -7, dtype=torch.int32, device=DEV)
    seq = [(1, "pairwise", L.ku), (0, "sequential", L.ku), (1, "sequential", L.ku), (0, "pairwise", L.ku),
           (1, "pairwise", PAD_KU), (0, "sequential", PAD_KU), (0, "pairwise", L.ku), (1, "sequential", L.ku)]
    for m, order, ku in seq:
        got = c_predict(L, mats[m], order, ku, L.kq, out=out, ws=ws)
        assert torch.equal(got, c_predict(L, mats[m], order, ku, L.kq)), (m, order, ku)
