"""A dataset whose rows come and go under a served QueryIndex (csrc/tablerows.hip).

A dataset row lives in a slot: slot s owns row s of the permutation table and bit s of every value bitmap.  A table
drawn for capacity >= D rows (ops.legacy_permutations(P, capacity)) has the free slots D .. capacity-1; an added row takes
the lowest slot never used, a removed row's slot is dead and is not used again.  The contract: after any sequence of row
operations the index's signatures, norms, band arrays and lists are those of answer_sets + ops.minhash + a fresh
QueryIndex / pipeline.query_similarities (at the held K) over the edited table in slot numbering with the same
permutation table.  (The rule is this project's: the reference draws permutation(drows) and never edits its dataset.)

MinHash makes both directions local.  An added row lowers sig[q][p] to min(sig[q][p], perm_p[slot]) for exactly the
queries it satisfies: one sweep over the served queries marks those a value really drops for, a second kernel writes
their new rows, QueryIndex.replace puts them in.  A removed row leaves a position stale only where sig[q][p] ==
perm_p[slot]: those queries are marked, their answer sets are taken again over the shrunk table, QueryIndex.set puts them
in.  Queries that match a row but keep their signature are not touched at all."""
import numpy as np
import torch

from . import _lib, answers, ops

LIVE_ROW = 0                       # bitmap row 0: the slots in use
MAX_FEAT = _lib.TABLE_ROWS_MAX_FEAT


def _values(x):
    a = np.asarray(x.to_numpy() if hasattr(x, "to_numpy") else x, dtype=object)
    return a


class TableDictionary:
    """host side: per feature, value (compared as str, as the reference compares cells) -> bitmap row.  Row 0 is the live
    row; values get rows in the order they are first seen, from the table's cells and from the queries alike: a value a
    query names that no row holds has a row of its own (all zero until a row brings the value), never a shared one."""

    def __init__(self, nfeat):
        if not 1 <= nfeat <= MAX_FEAT:
            raise ValueError("a live table takes 1..%d features (the live row is the 64th column of an answer-set "
                             "query), got %d" % (MAX_FEAT, nfeat))
        self.nfeat = nfeat
        self.maps = [dict() for _ in range(nfeat)]
        self.nrows = 1

    def _column(self, f, col, add):
        """value ids of one feature's values; unknown values get new rows (add) or -2"""
        vals, inv = np.unique(np.asarray([str(v) for v in col], dtype=object).astype(str), return_inverse=True)
        ids = np.empty(len(vals), dtype=np.int32)
        mp = self.maps[f]
        for k, v in enumerate(vals.tolist()):
            r = mp.get(v)
            if r is None:
                if add:
                    r = mp[v] = self.nrows
                    self.nrows += 1
                else:
                    r = -2
            ids[k] = r
        return ids[inv.reshape(-1)]

    def encode_cells(self, rows, add=True):
        """rows [m, nfeat] values -> int32 [m, nfeat] value ids"""
        rows = _values(rows)
        if rows.ndim != 2 or rows.shape[1] != self.nfeat:
            raise ValueError("rows must have one column per feature (%d)" % self.nfeat)
        out = np.empty(rows.shape, dtype=np.int32)
        for f in range(self.nfeat):
            out[:, f] = self._column(f, rows[:, f], add) if rows.shape[0] else 0
        return out

    def encode_queries(self, queries, add=True):
        """queries [k, nfeat] values, "" = unconstrained -> int32 [k, nfeat] value ids, -1 = unconstrained"""
        q = _values(queries)
        if q.ndim != 2 or q.shape[1] != self.nfeat:
            raise ValueError("queries must have one column per feature (%d)" % self.nfeat)
        out = np.full(q.shape, -1, dtype=np.int32)
        for f in range(self.nfeat):
            col = np.asarray([str(v) for v in q[:, f]], dtype=object)
            want = col != ""
            if want.any():
                out[want, f] = self._column(f, col[want], add)
        return out


def with_live_column(qrows):
    """qrows [k, nfeat] -> [k, nfeat + 1]: the live row as one more constrained column, so that no query -- an
    all-unconstrained one included -- matches a dead slot (answer_sets_kernel starts from "every row below D")"""
    if isinstance(qrows, torch.Tensor):
        live = torch.full((qrows.shape[0], 1), LIVE_ROW, dtype=torch.int32, device=qrows.device)
        return torch.cat((qrows, live), dim=1).contiguous()
    qrows = np.asarray(qrows, dtype=np.int32)
    return np.ascontiguousarray(np.concatenate((qrows, np.full((qrows.shape[0], 1), LIVE_ROW, dtype=np.int32)), axis=1))


class _Bitmaps:
    """what answers.answer_sets reads of an AnswerIndex"""

    def __init__(self, bitmaps, wpr, D):
        self.bitmaps, self.wpr, self.D = bitmaps, wpr, D


class LiveTable:
    """On the device: .bitmaps int32 [row capacity, wpr] (AnswerIndex's layout: one bitmap over the slots per (feature,
    value), wpr sized for .capacity and a multiple of 4; row 0 = the slots in use), .cells int32 [capacity, nfeat] (the
    value id of every slot's cell, -1 for a slot that is free or dead), .qrows int32 [n, nfeat] of the served queries (-1
    = unconstrained).  On the host: .dictionary (TableDictionary), .D the high-water slot, .live bool [capacity].
    .last_matched / .last_changed: the queries the last add_rows / remove_rows matched and rewrote (a batch beyond 65536
    rows runs as successive batches: the counts are summed over them)."""

    def __init__(self, nfeat, capacity, device):
        self.dictionary = TableDictionary(nfeat)
        self.nfeat = nfeat
        self.capacity = int(capacity)
        if not 1 <= self.capacity < 2**31:
            raise ValueError("capacity must lie in [1, 2^31)")
        self.device = device
        self.wpr = max(4, ((self.capacity + 31) // 32 + 3) // 4 * 4)
        self.D = 0
        self.live = np.zeros(self.capacity, dtype=bool)
        self._cells = np.full((self.capacity, nfeat), -1, dtype=np.int32)
        self.cells = torch.full((self.capacity, nfeat), -1, dtype=torch.int32, device=device)
        self.bitmaps = torch.zeros((64, self.wpr), dtype=torch.int32, device=device)
        self.qrows = torch.empty((0, nfeat), dtype=torch.int32, device=device)
        self.last_matched = self.last_changed = None

    @property
    def n(self):
        return self.qrows.shape[0]

    @classmethod
    def build(cls, columns, queries, capacity=None, device="cuda"):
        """columns: one 1-D array of cells per feature (the dataset's columns); queries [n, nfeat] values, "" =
        unconstrained: the served queries, in the index's order; capacity: slots (default: the rows given)"""
        columns = [_values(c).reshape(-1) for c in columns]
        D = len(columns[0]) if columns else 0
        if any(len(c) != D for c in columns):
            raise ValueError("columns must have one length")
        capacity = max(D, 1) if capacity is None else int(capacity)
        if capacity < D:
            raise ValueError("capacity %d is below the table's %d rows" % (capacity, D))
        t = cls(len(columns), capacity, device)
        rows = np.stack(columns, axis=1) if D else np.empty((0, len(columns)), dtype=object)
        cells = t.dictionary.encode_cells(rows)
        q = t.encode(queries)
        t.qrows = torch.from_numpy(q).to(device)
        t._place(cells, np.arange(D, dtype=np.int64))
        return t

    # ---- internals ---------------------------------------------------------------------------------------------------
    def _reserve_rows(self):
        need, have = self.dictionary.nrows, self.bitmaps.shape[0]
        if need > have:
            grown = torch.zeros((max(need, 2 * have), self.wpr), dtype=torch.int32, device=self.device)
            grown[:have].copy_(self.bitmaps)
            self.bitmaps = grown

    def _place(self, cells, slots):
        """cells into slots: the mirrors, the device cells, the bits.  -> the RowBatch"""
        self._reserve_rows()
        batch = ops.RowBatch(cells, slots, self.device)
        if batch.m:
            self._cells[slots] = cells
            self.live[slots] = True
            self.cells[batch.slots.to(torch.int64)] = batch.cells
            ops.bitmaps_set_rows(self.bitmaps, batch, LIVE_ROW, True)
            self.D = max(self.D, batch.slot_hi)
        return batch

    def _check_index(self, index, update_lists, slot_hi):
        if index.n != self.n:
            raise ValueError("the index holds %d queries, the table's qrows %d" % (index.n, self.n))
        if index.table is None:
            raise ValueError("the index holds no permutation table")
        if slot_hi > index.table.D:
            raise ValueError("no free slot: the permutation table was drawn for %d rows (capacity)" % index.table.D)
        if update_lists and index.lists is None:
            raise ValueError("this index holds no lists to update (none were given, or a call without "
                             "update_lists=True dropped them)")

    # ---- queries -----------------------------------------------------------------------------------------------------
    def encode(self, queries):
        """queries [k, nfeat] values ("" = unconstrained) -> int32 numpy qrows; values new to the dictionary get
        (all-zero) bitmap rows"""
        q = self.dictionary.encode_queries(queries)
        self._reserve_rows()
        return q

    def answer_sets(self, qrows=None):
        """-> (offsets int64 [k + 1], rows int32) on the device: the live slots every query matches, ascending; default:
        the served queries"""
        q = self.qrows if qrows is None else qrows
        if not isinstance(q, torch.Tensor):
            q = torch.from_numpy(np.ascontiguousarray(q, dtype=np.int32)).to(self.device)
        if q.dim() != 2 or q.shape[1] != self.nfeat:
            raise ValueError("qrows must be [k, %d]" % self.nfeat)
        if self.D == 0:
            return (torch.zeros((q.shape[0] + 1,), dtype=torch.int64, device=self.device),
                    torch.empty((0,), dtype=torch.int32, device=self.device))
        return answers.answer_sets(_Bitmaps(self.bitmaps, self.wpr, self.D), with_live_column(q.to(torch.int32)))

    def _as_qrows(self, qrows):
        if not isinstance(qrows, torch.Tensor):
            qrows = torch.from_numpy(np.ascontiguousarray(qrows, dtype=np.int32))
        qrows = qrows.to(self.device, torch.int32)
        if qrows.dim() != 2 or qrows.shape[1] != self.nfeat:
            raise ValueError("qrows must be [k, %d]" % self.nfeat)
        return qrows

    def add_queries(self, qrows):
        """after QueryIndex.append: the appended queries' qrows"""
        self.qrows = torch.cat((self.qrows, self._as_qrows(qrows)), dim=0).contiguous()

    def remove_queries(self, new_pos):
        """after QueryIndex.remove: its new_pos (-1 = removed)"""
        keep = torch.as_tensor(np.asarray(new_pos.cpu() if isinstance(new_pos, torch.Tensor) else new_pos) >= 0)
        if keep.numel() != self.n:
            raise ValueError("new_pos must hold one entry per served query (%d)" % self.n)
        self.qrows = self.qrows[keep.to(self.device)].contiguous()

    def set_queries(self, ids, qrows):
        """after QueryIndex.replace: row x of qrows is now query ids[x]"""
        ids = torch.as_tensor(np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids).reshape(-1).astype(np.int64))
        qrows = self._as_qrows(qrows)
        if ids.numel() != qrows.shape[0] or (ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.n)):
            raise ValueError("ids must name one served query per row")
        self.qrows[ids.to(self.device)] = qrows

    # ---- rows --------------------------------------------------------------------------------------------------------
    def add_rows(self, rows, index, update_lists=False):
        """rows [m, nfeat] values (the dataset's form) take the slots D .. D + m - 1; index (the QueryIndex over the
        served queries, drawn with a table of >= D + m rows) gets the changed queries' new rows through
        QueryIndex.replace(update_lists=...).  With no changed query neither the index nor its lists are touched
        (update_lists=False then does not drop the lists).  ValueError, nothing changed, for a wrong shape, fewer than m
        free slots, an index out of step or update_lists=True without lists.  -> int64 array [m], the slots taken"""
        rows = _values(rows)
        if rows.ndim != 2 or rows.shape[1] != self.nfeat:
            raise ValueError("rows must be [m, %d]: one column per feature" % self.nfeat)
        m = rows.shape[0]
        if self.D + m > self.capacity:
            raise ValueError("%d rows for %d free slots (capacity %d)" % (m, self.capacity - self.D, self.capacity))
        self._check_index(index, update_lists, self.D + m)
        slots = np.arange(self.D, self.D + m, dtype=np.int64)
        cells = self.dictionary.encode_cells(rows)
        self.last_matched = self.last_changed = 0
        for j0 in range(0, m, _lib.TABLE_ROWS_MAX_M):
            j1 = min(m, j0 + _lib.TABLE_ROWS_MAX_M)
            batch = self._place(cells[j0:j1], slots[j0:j1])
            changed, matched = ops.table_rows_mark(self.qrows, batch, index.table, index.sig)
            self.last_matched += matched
            self.last_changed += changed.count
            if changed.count:
                ids = changed.members()
                sig, norm2 = ops.table_rows_fill(self.qrows, batch, index.table, index.sig, ids)
                index.replace(ids.to(torch.int64) & 0xFFFFFFFF, sig, norm2, update_lists=update_lists)
        return slots

    def remove_rows(self, slots, index, update_lists=False):
        """slots: distinct live slots (ValueError otherwise, nothing changed).  The queries whose minimum sat on one of them
        are marked against the index's rows, the bits are cleared, and their answer sets over the shrunk table go through
        QueryIndex.set(update_lists=...); a query that loses its last row becomes the all -1 row this way.  With no changed
        query neither the index nor its lists are touched."""
        s = np.asarray(slots.cpu() if isinstance(slots, torch.Tensor) else slots).reshape(-1)
        if s.size and not np.issubdtype(s.dtype, np.integer):
            raise ValueError("slots must be integers")
        s = s.astype(np.int64)
        if s.size and (s.min() < 0 or s.max() >= self.D or np.unique(s).size != s.size or not self.live[s].all()):
            raise ValueError("slots must be distinct live slots below %d" % self.D)
        self._check_index(index, update_lists, 0)
        self.last_matched = self.last_changed = 0
        for j0 in range(0, s.size, _lib.TABLE_ROWS_MAX_M):
            part = s[j0:j0 + _lib.TABLE_ROWS_MAX_M]
            batch = ops.RowBatch(self._cells[part], part, self.device)
            changed, matched = ops.table_rows_mark(self.qrows, batch, index.table, index.sig, remove=True)
            ops.bitmaps_set_rows(self.bitmaps, batch, LIVE_ROW, False)
            self.live[part] = False
            self._cells[part] = -1
            self.cells[batch.slots.to(torch.int64)] = -1
            self.last_matched += matched
            self.last_changed += changed.count
            if changed.count:
                ids = changed.members()
                off, rws = self.answer_sets(self.qrows[ids.to(torch.int64) & 0xFFFFFFFF])
                index.set(ids.to(torch.int64) & 0xFFFFFFFF, off, rws, update_lists=update_lists)
