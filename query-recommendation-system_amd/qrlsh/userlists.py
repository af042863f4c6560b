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
(R's count with its pair count, then the picked rows).

.add_users(), .remove_users() and .nearest() let users join and leave (csrc/userrows.hip): new rows are R of the same
update over grown arrays (nothing is picked: no stored entry names a new id); removed rows are R with mean and norm2
zeroed, so every score against them is 0 and the positive-only lists drop them, after which the survivors are renumbered
by rank.  Labels stay those of the build, and so does K unless .set_list_length() changes it (a prefix for a smaller K;
for a larger one the full rows are rescored as the changed rows of the same update); the original label values are
kept beside the dense ones (.user_labels()).  One read-back per batch of new users (add_users(labels=None) adds one, for the assignment), two per
removal (the picked rows, then the renumbering's flags)."""
import numpy as np
import torch

from . import _lib, ops, users as _users
from ._args import _int_in
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
    int32 [nu] (dense), c_off int64 [nc + 1], c_mem / c_pos int32 [nu].  A row operation (add_users, remove_users) binds new
    tensors throughout and leaves the old ones as they were."""

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
        K = _int_in(K, "K", 1, MAX_K)
        lab = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).reshape(-1)
        if lab.size != nu or not np.issubdtype(lab.dtype, np.integer):
            raise ValueError("labels must hold one integer per user (%d)" % nu)
        r = r.to(device=device, dtype=torch.int32).contiguous()
        if r.data_ptr() % 16:
            r = r.clone()
        self = cls()
        self.ratings, self.nu, self.nq, self.K = r, nu, nq, K
        dev = r.device
        self._set_clusters(lab.astype(np.int64))
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

    def _set_clusters(self, lab):
        """dense labels and the cluster structure of lab (host int64 [nu], the label values as the caller gave them:
        kept for user_labels()) -- plumbing: torch"""
        dev, nu = self.ratings.device, int(lab.size)
        self._labels_host = lab
        dense = torch.unique(torch.from_numpy(lab).to(dev), return_inverse=True)[1]
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

    def user_labels(self):
        """int64 host [nu]: every user's label in the label space given to build (add_users extends it)"""
        return self._labels_host.copy()

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

    def _refresh(self, Rd, r, r_pairs, rmap=None, stats=True, flag=None):
        """The lists after the rows R (Rd: int32 device ids ascending, r of them, r_pairs = the sum of their clusters'
        sizes - 1) changed in self.ratings: their statistics, mark, S = R + picked scored against their clusters, apply.
        rmap: the id map over R where the caller holds it.  stats=False: mean / norm2 of R are what the caller put there
        (remove_users: zeros).  flag: a device int32 [1] of the caller's that rides on the read-back (RuntimeError when it is
        set).  -> len(S); sets .last_picked"""
        lib, st, dev = _lib.load(), _stream(), self.ratings.device
        nu, K, nc = self.nu, self.K, self.nc
        if stats:
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
        if flag is None:
            n_pick, broken, pick_pairs = out3.tolist()        # the one read-back of the shared tail
        else:
            n_pick, broken, pick_pairs, refused = torch.cat((out3, flag.to(torch.int64))).tolist()
            if refused:
                raise RuntimeError("a row outside range reached the device")
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

    # ---- users join and leave: the matrix moves to its new row space (csrc/userrows.hip) -------------------------------
    def _rows(self, rows):
        """a batch of new rows -> (int32 device tensor [m][nq], contiguous and 16-byte aligned, m), checked the way
        _block checks a column block"""
        dev = self.ratings.device
        if isinstance(rows, torch.Tensor) and rows.device.type != "cpu":
            if rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[1] != self.nq:
                raise ValueError("device rows must be int32 [m][%d], got %s %s" % (self.nq, rows.dtype, tuple(rows.shape)))
            if rows.device != dev:
                raise ValueError("the rows are on %s, the matrix on %s" % (rows.device, dev))
            rd = rows.contiguous()
        else:
            b = np.asarray(rows.numpy() if isinstance(rows, torch.Tensor) else rows)
            if b.ndim != 2 or b.shape[1] != self.nq or not np.issubdtype(b.dtype, np.integer):
                raise ValueError("the rows must be an integer [m][%d] array, got %s %s" % (self.nq, b.dtype, b.shape))
            if self.nu + b.shape[0] >= 2**31:
                raise ValueError("%d rows beside %d users: fewer than 2^31 are served" % (b.shape[0], self.nu))
            if b.size and (b.min() < 0 or b.max() >= 2**31):
                raise ValueError("values must lie in [0, 2^31)")
            rd = torch.from_numpy(np.ascontiguousarray(b, dtype=np.int32)).to(dev)
        if rd.data_ptr() % 16:
            rd = rd.clone()
        return rd, int(rd.shape[0])

    def _nearest(self, rd, m, want_all=False):
        """(best_user, best_milli[, milli [m][nu]]) of the device rows rd against the nu users held now"""
        lib, st, dev = _lib.load(), _stream(), self.ratings.device
        nu, nq = self.nu, self.nq
        user = torch.empty((m,), dtype=torch.int32, device=dev)
        milli = torch.empty((m,), dtype=torch.int32, device=dev)
        every = torch.empty((m, nu), dtype=torch.int32, device=dev) if want_all else None
        rmean, rnorm2 = rows_stats(rd)
        step = max(1, min(m, (2**28) // nu))              # m * nu < 2^32 per call, and a workspace of 2 GiB at most
        for k0 in range(0, m, step):
            k1 = min(m, k0 + step)
            ws = ops._ws(lib.qrlsh_user_rows_nearest_workspace_bytes(nu, k1 - k0), dev)
            _lib.check(lib.qrlsh_user_rows_nearest(_ptr(self.ratings), nu, nq, _ptr(self.mean), _ptr(self.norm2),
                                                   ops._vp(rd.data_ptr() + 4 * k0 * nq), k1 - k0,
                                                   ops._vp(rmean.data_ptr() + 8 * k0), ops._vp(rnorm2.data_ptr() + 8 * k0),
                                                   ops._vp(user.data_ptr() + 4 * k0), ops._vp(milli.data_ptr() + 4 * k0),
                                                   None if every is None else ops._vp(every.data_ptr() + 4 * k0 * nu),
                                                   _ptr(ws), ws.numel(), st))
        return (user, milli, every) if want_all else (user, milli)

    def nearest(self, rows):
        """The most similar existing user of every row of `rows` (integer [m][nq] host array or int32 device tensor), by
        the lists' own score: -> (user int32 [m], milli int32 [m]) device tensors, ties to the lowest user id, (-1, 0)
        where no score is positive.  Nothing is inserted; add_users(labels=None) assigns by this answer."""
        rd, m = self._rows(rows)
        if m == 0:
            dev = self.ratings.device
            return torch.empty((0,), dtype=torch.int32, device=dev), torch.empty((0,), dtype=torch.int32, device=dev)
        return self._nearest(rd, m)

    _STATE = ("ratings", "nu", "nq", "idx", "milli", "len", "mean", "norm2", "label", "c_off", "c_mem", "c_pos", "nc",
              "_counts", "_sizes", "_dense_host", "_labels_host", "last_picked")

    def _rebound(self, work):
        """run work(); a row operation only ever binds new tensors, so when it fails every field is bound back"""
        held = {k: getattr(self, k) for k in self._STATE}
        try:
            return work()
        except BaseException:
            for k, v in held.items():
                setattr(self, k, v)
            raise

    def _move_rows(self, src, block, m):
        """src: host int64 [nu2] -> the matrix with row u2 = src[u2] >= 0 ? ratings[src[u2]] : block[~src[u2]], a new
        tensor (the old one is not written)"""
        lib, dev = _lib.load(), self.ratings.device
        nu2 = int(src.size)
        sd = torch.from_numpy(np.ascontiguousarray(src, dtype=np.int32)).to(dev)
        new = torch.empty((nu2, self.nq), dtype=torch.int32, device=dev)
        flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        _lib.check(lib.qrlsh_ratings_rows_move(_ptr(self.ratings), self.nu, self.nq, _ptr(sd), nu2, _ptr(block), m,
                                               _ptr(new), _ptr(flag), _stream()))
        return new, sd, flag

    def add_users(self, rows, labels=None):
        """Append users: rows = integer [m][nq] host array (values in [0, 2^31)) or int32 device tensor; they take the
        ids nu .. nu+m-1.  labels: one integer per new user in the label space given to build -- a value some user holds
        joins that cluster, any other opens a new one (shared by the new users that give it).  labels=None: each new
        user joins the cluster of the existing user it is most similar to (nearest(): the lists' score, ties to the
        lowest id; only users of the matrix before the batch count), or, where no score is positive, gets a cluster of
        its own labelled one more than the largest label in use, counting up in row order.  The lists follow exactly
        (the new rows are the changed rows; nothing is picked).  ValueError for a wrong shape, value or label count, or
        2^31 users and more (nothing changed).  -> int64 host [m], the labels the new users hold."""
        rd, m = self._rows(rows)
        lab = None
        if labels is not None:
            lab = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).reshape(-1)
            if lab.size != m or (m and not np.issubdtype(lab.dtype, np.integer)):
                raise ValueError("labels must hold one integer per new user (%d)" % m)
            lab = lab.astype(np.int64)
        if m == 0:
            return np.zeros(0, dtype=np.int64)
        nu, nu2 = self.nu, self.nu + m
        if nu2 >= 2**31:
            raise ValueError("the matrix would have %d rows: fewer than 2^31 are served" % nu2)
        dev = self.ratings.device
        if lab is None:
            user, milli = self._nearest(rd, m)
            near = torch.stack((user, milli)).cpu().numpy()  # the assignment's read-back
            lab = np.empty(m, dtype=np.int64)
            top = int(self._labels_host.max())
            for k in range(m):
                if near[1, k] >= 1:
                    lab[k] = self._labels_host[near[0, k]]
                else:
                    top += 1
                    lab[k] = top
        src = np.concatenate((np.arange(nu, dtype=np.int64), -1 - np.arange(m, dtype=np.int64)))
        grow = lambda t, fill: torch.cat((t, torch.full((m,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=dev)))

        def work():
            new, _, flag = self._move_rows(src, rd, m)
            self.ratings, self.nu = new, nu2
            self.idx, self.milli, self.len = grow(self.idx, -1), grow(self.milli, 0), grow(self.len, 0)
            self.mean, self.norm2 = grow(self.mean, 0), grow(self.norm2, 0)
            self._set_clusters(np.concatenate((self._labels_host, lab)))
            Rd = torch.arange(nu, nu2, dtype=torch.int32, device=dev)
            self._refresh(Rd, m, int((self._sizes[self._dense_host[nu:]] - 1).sum()), flag=flag)
        self._rebound(work)
        return lab.copy()

    def remove_users(self, users):
        """Take users out (integers in any order, duplicates allowed; ValueError for one outside [0, nu) or when nobody
        would be left, nothing changed); the users left are renumbered by rank and clusters left empty disappear.  The
        full rows that named a removed user are scored again against the surviving members of their cluster
        (.last_picked of them); every other row keeps its entries.  -> int64 host [old nu]: the new id of every old
        user, -1 for a removed one."""
        g = np.asarray(users.cpu() if isinstance(users, torch.Tensor) else users).reshape(-1)
        if g.size and not np.issubdtype(g.dtype, np.integer):
            raise ValueError("remove_users: the users must be integers")
        g = np.unique(g.astype(np.int64))
        nu, K = self.nu, self.K
        if g.size and (g[0] < 0 or g[-1] >= nu):
            raise ValueError("remove_users: user outside [0, %d)" % nu)
        if g.size >= nu:
            raise ValueError("remove_users: no user would be left")
        new_pos = np.arange(nu, dtype=np.int64)
        if g.size == 0:
            self.last_picked = 0
            return new_pos
        keep = np.ones(nu, dtype=bool)
        keep[g] = False
        new_pos = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)
        src = np.flatnonzero(keep)
        lib, st, dev = _lib.load(), _stream(), self.ratings.device
        # the removed rows score 0 against everybody: the update drops them from every list and picks the full rows
        # that named one of them
        gd = torch.from_numpy(g.astype(np.int32)).to(dev)
        g64 = gd.to(torch.int64)

        def work():
            self.mean, self.norm2 = self.mean.clone(), self.norm2.clone()
            self.idx, self.milli, self.len = self.idx.clone(), self.milli.clone(), self.len.clone()
            self.mean[g64] = 0
            self.norm2[g64] = 0
            self._refresh(gd, int(g.size), int((self._sizes[self._dense_host[g]] - 1).sum()), stats=False)
            new, sd, flag = self._move_rows(src, None, 0)
            nu2 = int(src.size)
            idx = torch.empty((nu2, K), dtype=torch.int32, device=dev)
            milli = torch.empty((nu2, K), dtype=torch.int32, device=dev)
            ln = torch.empty((nu2,), dtype=torch.int32, device=dev)
            flag2 = torch.zeros((1,), dtype=torch.int32, device=dev)
            pd = torch.from_numpy(new_pos.astype(np.int32)).to(dev)
            _lib.check(lib.qrlsh_user_lists_renumber(_ptr(self.idx), _ptr(self.milli), _ptr(self.len), nu, K, _ptr(sd), nu2,
                                                     _ptr(pd), _ptr(idx), _ptr(milli), _ptr(ln), _ptr(flag2), st))
            refused, broken = torch.cat((flag, flag2)).tolist()       # the second read-back of a removal
            if refused:
                raise RuntimeError("a row outside range reached the device")
            if broken:
                raise ValueError("the stored user lists break their contract (an entry names a removed user, an index "
                                 "outside [0, %d) or a length outside [0, %d])" % (nu, K))
            s64 = sd.to(torch.int64)
            self.ratings, self.nu = new, nu2
            self.idx, self.milli, self.len = idx, milli, ln
            self.mean, self.norm2 = self.mean[s64].contiguous(), self.norm2[s64].contiguous()
            self._set_clusters(self._labels_host[keep])
        self._rebound(work)
        return new_pos

    # ---- changing the list length ------------------------------------------------------------------------------------
    def set_list_length(self, K2):
        """give the lists the list length K2 (1..64) without a rebuild: afterwards idx / milli / len are element for
        element what build() over the same matrix and labels gives with K = K2, .K = K2, and every later operation keeps
        them exact at K2.  New tensors are bound throughout; the old ones are not written.
        K2 < K: the first K2 columns (lists are ordered value descending, id ascending: a prefix is the shorter list).
        K2 > K: the arrays are restrided to [nu][K2]; a row with fewer than K entries was never cut and stays; the rows
        of exactly K entries are the changed rows of the ordinary update (_refresh): each is scored against its whole
        cluster and takes its K2 best positive scores.  Every other row of a touched cluster merges scores that did not
        change and ends as it was, and nothing else is picked -- no row is full at the new stride.  One read-back (the
        full rows) beside the update's own.
        -> the number of rows rescored (0 for a cut), also in .last_picked.  ValueError for K2 outside 1..64 (nothing
        changed)."""
        K1, K2 = self.K, _int_in(K2, "K2", 1, MAX_K)
        if K2 == K1:
            self.last_picked = 0
            return 0
        if K2 < K1:
            idx, milli = self.idx[:, :K2].contiguous(), self.milli[:, :K2].contiguous()
            self.idx, self.milli, self.len, self.K = idx, milli, self.len.clamp(max=K2), K2
            self.last_picked = 0
            return 0
        dev, nu = self.ratings.device, self.nu
        Rd = torch.nonzero(self.len == K1).reshape(-1).to(torch.int32).contiguous()
        R = Rd.cpu().numpy().astype(np.int64)                 # the read-back: the rows the cut can have shortened
        idx = torch.full((nu, K2), -1, dtype=torch.int32, device=dev)
        milli = torch.zeros((nu, K2), dtype=torch.int32, device=dev)
        idx[:, :K1], milli[:, :K1] = self.idx, self.milli

        def work():
            self.idx, self.milli, self.len, self.K = idx, milli, self.len.clone(), K2
            if R.size:
                self._refresh(Rd, int(R.size), int((self._sizes[self._dense_host[R]] - 1).sum()), stats=False)
            self.last_picked = int(R.size)
        try:
            self._rebound(work)
        except BaseException:
            self.K = K1
            raise
        return int(R.size)

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
