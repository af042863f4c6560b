"""User-similarity lists that stay exact when users rate queries (csrc/userlists.hip).

UserLists.build() takes the lists of users.user_similarities once; .rate() applies a batch of cell edits to the device
matrix and brings the lists of the touched clusters up to date: afterwards they are element for element what
users.user_similarities(new_ratings, labels, K) gives, with the labels and K of the build.  The changed rows R and the
full rows that name one of them (picked) are scored against their clusters from the raw ratings (qrlsh_user_pairs_score:
no centred copy of the matrix); every other row of a touched cluster merges R's new scores into what it holds.  One
read-back per batch (the number of picked rows).

.add_columns(), .remove_columns() and .set_columns() follow queries that are appended, removed or re-rated
(csrc/usercolumns.hip): the rows whose values in the affected columns differ are found on the device, the matrix moves
out of place to its new column space, and the same update runs over it with those rows as R.  Two read-backs per batch
(R's count with its pair count, then the picked rows)."""
import numpy as np
import torch

from . import _lib, ops, users as _users
from .ops import _ptr, _stream

MAX_K = _lib.USER_LISTS_MAX_K


def pairs_score(ratings, mean, norm2, pairs):
    """milli int32 [n] of pairs (int64 [n] = a << 32 | b) from the raw int32 ratings and their rows' mean / norm2
    (rows_stats): ops.score_pairs(users.center_rows(ratings), ops.row_norms(.), pairs)[0], bit for bit"""
    lib = _lib.load()
    nu, nq = ratings.shape
    n = pairs.numel()
    milli = torch.empty((n,), dtype=torch.int32, device=ratings.device)
    ws = ops._ws(lib.qrlsh_user_pairs_score_workspace_bytes(nq, n), ratings.device)
    _lib.check(lib.qrlsh_user_pairs_score(_ptr(ratings), nu, nq, _ptr(mean), _ptr(norm2), _ptr(pairs), n, _ptr(milli),
                                          _ptr(ws), ws.numel(), _stream()))
    return milli


def rows_stats(ratings, rows=None, mean=None, norm2=None):
    """(mean float64 [nu], norm2 int64 [nu]) of the truncated centred rows; rows (int32 device ids) = only those,
    written at their own index into the mean / norm2 given"""
    lib = _lib.load()
    nu, nq = ratings.shape
    dev = ratings.device
    if mean is None:
        mean = torch.zeros((nu,), dtype=torch.float64, device=dev)
        norm2 = torch.zeros((nu,), dtype=torch.int64, device=dev)
    m = nu if rows is None else rows.numel()
    _lib.check(lib.qrlsh_user_rows_stats(_ptr(ratings), nu, nq, _ptr(rows), m, _ptr(mean), _ptr(norm2), _stream()))
    return mean, norm2


class UserLists:
    """The live user lists of one utility matrix.  Fields (device tensors): ratings int32 [nu][nq] (edited in place by
    rate(); a column operation binds a new tensor and leaves the old one as it was),
    idx / milli int32 [nu][K] (-1 / 0 past a row's end), len int32 [nu], mean float64 [nu], norm2 int64 [nu], label
    int32 [nu] (dense), c_off int64 [nc + 1], c_mem / c_pos int32 [nu]."""

    @classmethod
    def build(cls, ratings, labels, K=None, device="cuda"):
        """ratings (nu, nq) integers (0 = unrated): uploaded as int32; an int32 device tensor is used where it is and
        edited in place by rate().  labels (nu,) cluster ids, any integers (relabelled densely).  K: list length
        (default users.max_candidates(nu)); ValueError outside 1..64."""
        r = ratings if isinstance(ratings, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(np.asarray(ratings), dtype=np.int32))
        if r.dim() != 2:
            raise ValueError("ratings must be 2-D, got shape %s" % (tuple(r.shape),))
        nu, nq = (int(d) for d in r.shape)
        if nu < 1 or nu >= 2**31 or nq >= 2**31:
            raise ValueError("ratings must have 1 .. 2^31 - 1 rows and fewer than 2^31 columns")
        if K is None:
            K = _users.max_candidates(nu)
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= int(K) <= MAX_K:
            raise ValueError("K must be an integer in 1..%d, got %r" % (MAX_K, K))
        lab = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).reshape(-1)
        if lab.size != nu or not np.issubdtype(lab.dtype, np.integer):
            raise ValueError("labels must hold one integer per user (%d)" % nu)
        r = r.to(device=device, dtype=torch.int32).contiguous()
        if r.data_ptr() % 16:
            r = r.clone()
        self = cls()
        self.ratings, self.nu, self.nq, self.K = r, nu, nq, int(K)
        dev = r.device
        # dense labels and the cluster structure (plumbing: torch)
        dense = torch.unique(torch.from_numpy(lab.astype(np.int64)).to(dev), return_inverse=True)[1]
        self.nc = int(dense.max().item()) + 1
        order = torch.sort(dense, stable=True)[1]            # members ascending within a cluster
        counts = torch.bincount(dense, minlength=self.nc)
        self.c_off = torch.zeros((self.nc + 1,), dtype=torch.int64, device=dev)
        torch.cumsum(counts, dim=0, out=self.c_off[1:])
        self.c_mem = order.to(torch.int32).contiguous()
        pos = torch.empty((nu,), dtype=torch.int64, device=dev)
        pos[order] = torch.arange(nu, device=dev) - self.c_off[:-1][dense[order]]
        self.c_pos = pos.to(torch.int32).contiguous()
        self.label = dense.to(torch.int32).contiguous()
        self._counts = counts                                 # cluster sizes, int64 [nc]
        self._sizes = counts.cpu().numpy()                    # host copies: the pair count of rate()'s R needs no read-back
        self._dense_host = dense.cpu().numpy()
        # the first lists, in the dense form
        src, dst, val = _users.user_similarities(r, lab, self.K, device=dev)
        self.idx = torch.full((nu, self.K), -1, dtype=torch.int32, device=dev)
        self.milli = torch.zeros((nu, self.K), dtype=torch.int32, device=dev)
        cnt = torch.bincount(src.to(torch.int64), minlength=nu)
        self.len = cnt.to(torch.int32).contiguous()
        if src.numel():
            first = torch.cumsum(cnt, dim=0) - cnt
            s64 = src.to(torch.int64)
            k = torch.arange(src.numel(), device=dev) - first[s64]
            self.idx[s64, k] = dst
            self.milli[s64, k] = val
        self.mean, self.norm2 = rows_stats(r)
        self.last_picked = None
        return self

    def rate(self, users, queries, values):
        """Cell edits ratings[users[i]][queries[i]] = values[i] (0 = unrate); repeats of one cell keep the last value.
        ValueError for an id outside range or a negative value (nothing changed).  -> the number of rows rewritten
        (the changed rows and the full rows that named one of them); .last_picked = the latter."""
        u = np.asarray(users.cpu() if isinstance(users, torch.Tensor) else users).reshape(-1)
        q = np.asarray(queries.cpu() if isinstance(queries, torch.Tensor) else queries).reshape(-1)
        v = np.asarray(values.cpu() if isinstance(values, torch.Tensor) else values).reshape(-1)
        if not (u.size == q.size == v.size):
            raise ValueError("users, queries and values differ in length")
        if u.size == 0:
            return 0
        for name, a in (("users", u), ("queries", q), ("values", v)):
            if not np.issubdtype(a.dtype, np.integer):
                raise ValueError("%s must be integers" % name)
        u, q, v = u.astype(np.int64), q.astype(np.int64), v.astype(np.int64)
        if u.min() < 0 or u.max() >= self.nu:
            raise ValueError("user id outside [0, %d)" % self.nu)
        if q.min() < 0 or q.max() >= self.nq:
            raise ValueError("query id outside [0, %d)" % self.nq)
        if v.min() < 0 or v.max() >= 2**31:
            raise ValueError("values must lie in [0, 2^31)")
        cell = u * self.nq + q
        _, last = np.unique(cell[::-1], return_index=True)   # the last occurrence of every cell
        keep = np.sort(cell.size - 1 - last)
        u, q, v = u[keep], q[keep], v[keep]
        R = np.unique(u)

        lib, st, dev = _lib.load(), _stream(), self.ratings.device
        nu, nq = self.nu, self.nq
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        ud, qd, vd, Rd = up(u), up(q), up(v), up(R)
        flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        _lib.check(lib.qrlsh_ratings_set(_ptr(self.ratings), nu, nq, _ptr(ud), _ptr(qd), _ptr(vd), u.size, _ptr(flag), st))
        return self._refresh(Rd, int(R.size), int((self._sizes[self._dense_host[R]] - 1).sum()))

    def _refresh(self, Rd, r, r_pairs, rmap=None):
        """The lists after the rows R (Rd: int32 device ids ascending, r of them, r_pairs = the sum of their clusters'
        sizes - 1) changed in self.ratings: their statistics, mark, S = R + picked scored against their clusters, apply.
        rmap: the id map over R where the caller holds it.  -> len(S); sets .last_picked"""
        lib, st, dev = _lib.load(), _stream(), self.ratings.device
        nu, K, nc = self.nu, self.K, self.nc
        rows_stats(self.ratings, Rd, self.mean, self.norm2)
        map_bytes = lib.qrlsh_idmap_workspace_bytes(nu)
        pmap = ops._ws(map_bytes, dev)
        out3 = torch.zeros((3,), dtype=torch.int64, device=dev)
        if rmap is None:
            rmap = ops._ws(map_bytes, dev)
            out2 = torch.zeros((2,), dtype=torch.int64, device=dev)
            _lib.check(lib.qrlsh_idmap_build(_ptr(Rd), r, nu, _ptr(rmap), rmap.numel(), _ptr(out2), st))
        _lib.check(lib.qrlsh_user_lists_mark(_ptr(self.idx), _ptr(self.len), nu, K, _ptr(rmap), _ptr(self.label),
                                             _ptr(self.c_off), nc, _ptr(pmap), _ptr(out3), st))
        n_pick, broken, pick_pairs = out3.tolist()            # the one read-back of the shared tail
        if broken:
            raise ValueError("the stored user lists break their contract (an index outside [0, %d) or a length outside "
                             "[0, %d])" % (nu, K))
        if n_pick:
            picked = torch.empty((n_pick,), dtype=torch.int32, device=dev)
            _lib.check(lib.qrlsh_idmap_list(_ptr(pmap), nu, _ptr(picked), st))
            S = torch.sort(torch.cat((Rd, picked)))[0].contiguous()
        else:
            S = Rd
        s = int(S.numel())
        n_pairs = int(r_pairs) + int(pick_pairs)
        off = torch.empty((s + 1,), dtype=torch.int64, device=dev)
        pairs = torch.empty((max(n_pairs, 1),), dtype=torch.int64, device=dev)
        _lib.check(lib.qrlsh_user_cluster_pairs_count(_ptr(S), s, _ptr(self.label), _ptr(self.c_off), nu, nc, _ptr(off), st))
        _lib.check(lib.qrlsh_user_cluster_pairs_fill(_ptr(S), s, _ptr(self.label), _ptr(self.c_off), _ptr(self.c_mem),
                                                     _ptr(self.c_pos), nu, nc, _ptr(off), _ptr(pairs), st))
        pm = pairs_score(self.ratings, self.mean, self.norm2, pairs[:n_pairs])
        _lib.check(lib.qrlsh_user_lists_apply(_ptr(self.idx), _ptr(self.milli), _ptr(self.len), nu, K, _ptr(rmap),
                                              _ptr(pmap), s, _ptr(self.label), _ptr(self.c_off), _ptr(self.c_mem),
                                              _ptr(self.c_pos), nc, _ptr(off), _ptr(pm), n_pairs, st))
        self.last_picked = int(n_pick)
        return s

    # ---- queries appended, removed, re-rated: the matrix moves to its new column space (csrc/usercolumns.hip) ----------
    def _block(self, block, m=None):
        """a batch's incoming values -> (int32 device tensor [nu][m] or None for all zero, m).  A host array is checked
        (integers in [0, 2^31), shape [nu][m]) and uploaded; an int32 device tensor is taken as it is."""
        if isinstance(block, torch.Tensor) and block.device.type != "cpu":
            if block.dtype != torch.int32 or block.dim() != 2 or block.shape[0] != self.nu or (m is not None and block.shape[1] != m):
                raise ValueError("a device block must be int32 [%d][%s], got %s %s"
                                 % (self.nu, "m" if m is None else m, block.dtype, tuple(block.shape)))
            if block.device != self.ratings.device:
                raise ValueError("the block is on %s, the matrix on %s" % (block.device, self.ratings.device))
            return block.contiguous(), int(block.shape[1])
        b = np.asarray(block.numpy() if isinstance(block, torch.Tensor) else block)
        if b.ndim != 2 or b.shape[0] != self.nu or (m is not None and b.shape[1] != m) or not np.issubdtype(b.dtype, np.integer):
            raise ValueError("the block must be an integer [%d][%s] array, got %s %s"
                             % (self.nu, "m" if m is None else m, b.dtype, b.shape))
        if b.size and (b.min() < 0 or b.max() >= 2**31):
            raise ValueError("values must lie in [0, 2^31)")
        return torch.from_numpy(np.ascontiguousarray(b, dtype=np.int32)).to(self.ratings.device), int(b.shape[1])

    def _columns(self, name, cols, m=None):
        c = np.asarray(cols.cpu() if isinstance(cols, torch.Tensor) else cols).reshape(-1)
        if c.size and not np.issubdtype(c.dtype, np.integer):
            raise ValueError("%s: the columns must be integers" % name)
        c = c.astype(np.int64)
        if m is not None and c.size != m:
            raise ValueError("%s: %d columns for a block of %d" % (name, c.size, m))
        if c.size and (c.min() < 0 or c.max() >= self.nq):
            raise ValueError("%s: column outside [0, %d)" % (name, self.nq))
        return c

    def _move(self, cols, block, m, src):
        """cols: the affected old columns (host int64 [m], -1 = none), block: device int32 [nu][m] or None (zeros),
        src: host int64 [nq2] -- what the matrix holds afterwards (usercolumns.hip).  The rows whose values differ are
        found against the old matrix, the matrix moves out of place, then the lists follow."""
        lib, st, dev = _lib.load(), _stream(), self.ratings.device
        nu, nq, nq2 = self.nu, self.nq, int(src.size)
        if nq2 >= 2**31:
            raise ValueError("the matrix would have %d columns: fewer than 2^31 are served" % nq2)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        rmap = ops._ws(lib.qrlsh_idmap_workspace_bytes(nu), dev)
        head = torch.zeros((4,), dtype=torch.int64, device=dev)     # R's count, a refused column, R's pairs, a refused src
        flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        _lib.check(lib.qrlsh_ratings_columns_changed(_ptr(self.ratings), nu, nq, _ptr(up(cols)), _ptr(block), m, _ptr(rmap),
                                                     _ptr(head), st))
        new = torch.empty((nu, nq2), dtype=torch.int32, device=dev)
        _lib.check(lib.qrlsh_ratings_columns_move(_ptr(self.ratings), nu, nq, _ptr(up(src)), nq2, _ptr(block), m, _ptr(new),
                                                  _ptr(flag), st))
        Rbuf = torch.full((nu,), -1, dtype=torch.int32, device=dev)
        _lib.check(lib.qrlsh_idmap_list(_ptr(rmap), nu, _ptr(Rbuf), st))
        member = Rbuf >= 0
        head[2] = ((self._counts[self.label.to(torch.int64)[Rbuf.clamp(min=0).to(torch.int64)]] - 1) * member).sum()
        head[3] = flag[0]
        r, bad_col, r_pairs, bad_src = head.tolist()          # the first read-back; the tail's mark is the second
        if bad_col or bad_src:
            raise RuntimeError("a column outside range reached the device (%d, %d)" % (bad_col, bad_src))
        self.ratings, self.nq = new, nq2
        self.last_picked = 0
        if r == 0:
            return 0
        return self._refresh(Rbuf[:r].contiguous(), r, r_pairs, rmap)

    def add_columns(self, block):
        """Append columns to the matrix: block = integer [nu][m] host array (values in [0, 2^31)), int32 device tensor
        [nu][m], or an int m = m unrated columns.  The lists follow exactly: the rows that rated one of the new columns
        are the changed rows.  ValueError for a wrong shape or value (nothing changed).  -> the number of rows
        rewritten; .last_picked as after rate().  The matrix is rebuilt out of place (.ratings is a new tensor)."""
        if isinstance(block, (int, np.integer)) and not isinstance(block, bool):
            m, bd = int(block), None
            if m < 0:
                raise ValueError("cannot append %d columns" % m)
        else:
            bd, m = self._block(block)
        if m == 0:
            self.last_picked = 0
            return 0
        src = np.concatenate((np.arange(self.nq, dtype=np.int64), -1 - np.arange(m, dtype=np.int64)))
        return self._move(np.full(m, -1, dtype=np.int64), bd, m, src)

    def remove_columns(self, cols):
        """Take columns out of the matrix (integers in any order, duplicates allowed; ValueError for one outside
        [0, nq), nothing changed); the columns left keep their order.  The rows that had rated one of them are the
        changed rows.  Removing every column is legal (nq == 0: every list is empty then).  -> rows rewritten"""
        c = np.unique(self._columns("remove_columns", cols))
        if c.size == 0:
            self.last_picked = 0
            return 0
        keep = np.ones(self.nq, dtype=bool)
        keep[c] = False
        return self._move(c, None, int(c.size), np.flatnonzero(keep))

    def set_columns(self, cols, block):
        """Overwrite whole columns: block[:, k] becomes column cols[k] (cols distinct; block as add_columns takes it,
        but not an int).  The rows whose values in these columns differ from the block are the changed rows.
        ValueError for a duplicate or a column outside [0, nq), a wrong shape or value (nothing changed).
        -> rows rewritten"""
        c = self._columns("set_columns", cols)
        if np.unique(c).size != c.size:
            raise ValueError("set_columns: the columns must be distinct")
        bd, m = self._block(block, int(c.size))
        if m == 0:
            self.last_picked = 0
            return 0
        src = np.arange(self.nq, dtype=np.int64)
        src[c] = -1 - np.arange(m, dtype=np.int64)
        return self._move(c, bd, m, src)

    def coo(self):
        """(src, dst, milli) int32 device tensors, the form users.user_similarities returns"""
        keep = torch.arange(self.K, device=self.idx.device).unsqueeze(0) < self.len.unsqueeze(1)
        src = torch.arange(self.nu, dtype=torch.int32, device=self.idx.device).unsqueeze(1).expand(-1, self.K)
        return src[keep].contiguous(), self.idx[keep].contiguous(), self.milli[keep].contiguous()

    def as_user_sims(self):
        """(u_idx int32 [nu][K], u_val float64 = milli / 1000.0, ku) -- predict.user_lists' tuple, taken wherever
        `user_sims` is"""
        # through a table divided on the host: the values are those of users.sims_to_dict (milli / 1000.0 in IEEE
        # division), which a device-side division by a scalar -- a multiplication by its reciprocal -- does not give
        table = torch.from_numpy(np.arange(1001, dtype=np.float64) / 1000.0).to(self.idx.device)
        return self.idx, table[self.milli.to(torch.int64)], self.K
