"""Serving new queries: a band-key index of a finished hot-path run, probed many times (csrc/index.hip).

The hot path (pipeline.query_similarities) answers a closed set of queries.  A QueryIndex keeps what a new query needs
from such a run -- the permutation table, the signature rows, their norms, b and r = P / b, and the indexed band keys
sorted per band with a directory -- and answers, for a batch of new queries:

    neighbours       the K best indexed queries sharing a non-empty band (lsh.py:40-55, recommender.py:187-214 for
                     the query appended alone, K held fixed; milli descending, then id ascending)
    predict_columns  the hybrid prediction of every user's cell of each new query (recommender.py:313-331 with a
                     zero column: the user side is 0)
    top_users        the users with the largest non-zero predictions (qrlsh_recommend_topk on those rows)

New queries enter the index with append / add (qrlsh_index_append: the batch is sorted and merged into the sorted
band keys, byte for byte what a fresh build of all n + m rows gives, without sorting the n indexed records again);
afterwards they are indexed queries like the others, with the ids n .. n + m - 1.  An index that holds the run's
top-K lists (lists=...) keeps them current on the way (update_lists=True, csrc/lists.hip): after the append the batch
is probed against the grown index and every list, old and new, becomes what a run over all rows with the same K gives.
Queries leave with remove (csrc/remove.hip): the survivors are renumbered by rank, the band arrays are compacted into
what a fresh build of the surviving rows gives, and held lists are kept exact on the way (update_lists=True).
Queries change with replace / set (csrc/replace.hip): chosen ids take new rows and keep their ids; the band arrays lose
their old records and gain the new ones where (mix bits, id) puts them, and held lists are kept exact on the way.

Everything runs on the device; the indexed data never leaves it."""
import torch

from . import _lib, ops
from ._args import _int_in
from ._inputs import int_array, matrix, on_device, sum_order_code
from .pipeline import max_candidates
from .predict import QUERY_WEIGHT, USER_WEIGHT, DEFAULT_MEAN
from .recommend import top_k

MAX_K = _lib.INDEX_MAX_K


def _ids_arg(ids, dev):
    """the ids of remove() / replace(): a tensor or array of integers (floats and bools: ValueError) -> flat int64
    tensor on dev"""
    return int_array(ids, None, "ids").reshape(-1).to(dev, torch.int64)


def _u32_bits(t):
    """int64 values in [0, 2^32) -> int32 tensor of their uint32 bit patterns, as the library takes ids"""
    return ((t + 2**31) % 2**32 - 2**31).to(torch.int32)


class QueryIndex:
    """sig: the indexed signature rows (int32 [n, P], or compact uint16 rows carried as torch.int16) on the device;
    norm2: int64 [n] (None: computed); b: bands (P % b == 0); table: the ops.PermTable the rows were drawn with
    (needed only by .signatures); keys: int64 [b, n] band keys (default: qrlsh_band_keys of sig; caller keys only
    filter -- every candidate is checked against the rows); K: default list length (round(log_1.5 n); a defaulted K
    follows n when queries are appended, a given K stays); lists: the run's top-K lists (src, dst, val) int32 COO as
    pipeline.query_similarities returns them (by src, value descending, dst ascending), held in .lists by reference --
    never written: an update puts new tensors there.  Their list length (.lists_K) starts as the K of the constructor and
    does not follow n: stored rows were cut at it, so appends with update_lists=True keep .lists equal to a run over
    all rows WITH THAT K, not with the K a fresh run of the grown set would default to.  set_list_length(K2) changes it
    on purpose: a smaller K2 cuts every row to its first K2 entries, a larger one probes the rows of exactly lists_K
    entries again against the index (the only rows the cut can have shortened) and keeps the rest as stored.

    .sig and .norm2 are contiguous views of the first n rows of capacity buffers: append copies the m new rows behind
    them and the buffers grow geometrically (reserve pre-sizes them).  The tensors given to the constructor are never
    written: the first append or reserve moves the rows into a buffer of the index's own."""

    def __init__(self, sig, norm2, b, table=None, keys=None, K=None, lists=None):
        if not isinstance(sig, torch.Tensor) or sig.dtype not in (torch.int32, torch.int16) or sig.dim() != 2:
            raise TypeError("sig must be a 2-D int32 or int16 (compact) tensor")
        ops._need(sig, sig.dtype, "sig", 2)
        n, P = sig.shape
        b = _int_in(b, "b", 1, 65535)
        if P % b != 0:
            raise ValueError("signature length %d not divisible by b=%d" % (P, b))
        if n >= 2**32 - 1:
            raise ValueError("at most 2^32 - 2 indexed queries")
        if norm2 is not None:
            ops._need(norm2, torch.int64, "norm2", 1)
            if norm2.numel() != n or norm2.device != sig.device:
                raise ValueError("norm2 must hold one int64 per signature row, on the rows' device")
        if keys is not None:
            ops._need(keys, torch.int64, "keys", 2)
            if tuple(keys.shape) != (b, n) or keys.device != sig.device:
                raise ValueError("keys must be int64 [b, n] = [%d, %d] on the rows' device" % (b, n))
        if table is not None and (table.P != P or (sig.dtype == torch.int16 and not ops.can_compact(table))):
            raise ValueError("the permutation table does not match the signature rows")
        self._default_K = K is None
        if K is None:
            K = self._K_rule(n)
        self.K = _int_in(K, "K", 1, MAX_K)
        self.sig, self.n, self.P, self.b, self.r = sig, n, P, b, P // b
        self.table = table
        self.norm2 = norm2 if norm2 is not None else ops.row_norms(ops.sig_to_int32(sig))
        self._sig_buf, self._norm2_buf = self.sig, self.norm2      # capacity buffers; .sig / .norm2 = their first n rows
        self._own_rows = False      # the buffers are still the constructor's tensors: copied before the first write
        keys = ops.band_keys(ops.sig_to_int32(sig), b) if keys is None else keys.clone()
        self.keys, self.ids, self.dir = ops.index_build(keys)
        self.lists, self.lists_K = None, None
        self.last_picked = None
        if lists is not None:
            self.lists, self.lists_K = self._check_lists(lists), self.K

    def _check_lists(self, lists):
        if not isinstance(lists, (tuple, list)) or len(lists) != 3:
            raise ValueError("lists must be the (src, dst, val) of a run")
        for t, name in zip(lists, ("src", "dst", "val")):
            ops._need(t, torch.int32, "lists " + name, 1)
            if t.device != self.sig.device or t.numel() != lists[0].numel():
                raise ValueError("the lists must be three int32 tensors of one length on the rows' device")
        src, dst, _ = lists
        if src.numel():
            ok = bool(((src[1:] >= src[:-1]).all() & (src[0] >= 0) & (src[-1] < self.n) & (dst.min() >= 0)
                       & (dst.max() < self.n)).item())
            if not ok:
                raise ValueError("the lists must be ordered by src and name queries in [0, %d)" % self.n)
        return tuple(lists)

    @property
    def _probe_step(self):
        """the queries of one probe call: the library takes m * b < 2^32 words per call"""
        return max(1, (2**32 - 1) // self.b)

    def _empty_lists(self, parts=3):
        """the CSR lists of no probe row: zeros [1] int64 and `parts` empty int32 tensors"""
        dev = self.sig.device
        return (torch.zeros((1,), dtype=torch.int64, device=dev),) + tuple(
            torch.empty((0,), dtype=torch.int32, device=dev) for _ in range(parts))

    @staticmethod
    def _K_rule(n):
        return min(max(max_candidates(n) if n > 1 else 1, 1), MAX_K)

    @classmethod
    def from_result(cls, res, table, lists=False):
        """the index of a finished run: pipeline.query_similarities' HotPathResult and the table it was drawn with;
        lists=True: with the run's top-K lists in .lists (references to res.src / dst / val), list length res.K"""
        return cls(res.sig, res.norm2, res.b, table=table, K=res.K if res.K else None,
                   lists=(res.src, res.dst, res.val) if lists else None)

    # ---- new queries -----------------------------------------------------------------------------------------------
    def signatures(self, offsets, rows):
        """MinHash rows of new queries (CSR answer sets) under the held table, in the index's row dtype:
        -> (sig, norm2, keys [b, m])"""
        if self.table is None:
            raise ValueError("this index holds no permutation table; pass signatures to neighbours()")
        return ops.minhash(offsets, rows, self.table, b=self.b, want_norm=True, compact=self.sig.dtype == torch.int16)

    def _probe_rows(self, sig, norm2, keys):
        if not isinstance(sig, torch.Tensor) or sig.dtype not in (torch.int32, torch.int16) or sig.dim() != 2:
            raise TypeError("sig must be a 2-D int32 or int16 (compact) tensor")
        if sig.shape[1] != self.P:
            raise ValueError("new signatures have %d values, the index %d" % (sig.shape[1], self.P))
        sig = sig.to(self.sig.device).contiguous()
        if sig.dtype != self.sig.dtype:     # same values, the index's row format
            sig = ops.sig_to_int32(sig) if self.sig.dtype == torch.int32 else \
                sig.to(torch.int32).bitwise_and(0xFFFF).to(torch.int16)
        m = sig.shape[0]
        if norm2 is not None:
            ops._need(norm2, torch.int64, "norm2", 1)
            if norm2.numel() != m:
                raise ValueError("norm2 must hold one int64 per new signature")
        if keys is not None:
            ops._need(keys, torch.int64, "keys", 2)
            if tuple(keys.shape) != (self.b, m):
                raise ValueError("keys must be int64 [b, m] = [%d, %d]" % (self.b, m))
        if norm2 is None:
            norm2 = ops.row_norms(ops.sig_to_int32(sig))
        if keys is None:
            keys = ops.band_keys(ops.sig_to_int32(sig), self.b)
        return sig, norm2, keys

    # ---- growing the index -----------------------------------------------------------------------------------------
    def reserve(self, total):
        """room for `total` indexed queries in the row and norm buffers (no effect when they already hold as many)"""
        total = _int_in(total, "total", 0, 2**32 - 2)
        if total <= self._sig_buf.shape[0]:
            return
        dev = self.sig.device
        sig_buf = torch.empty((total, self.P), dtype=self.sig.dtype, device=dev)
        norm2_buf = torch.empty((total,), dtype=torch.int64, device=dev)
        sig_buf[:self.n].copy_(self.sig)
        norm2_buf[:self.n].copy_(self.norm2)
        self._sig_buf, self._norm2_buf = sig_buf, norm2_buf
        self.sig, self.norm2 = sig_buf[:self.n], norm2_buf[:self.n]
        self._own_rows = True

    def append(self, sig, norm2=None, keys=None, update_lists=False):
        """index m more queries: sig as in neighbours() (int32 or compact int16 rows, converted to the index's format);
        norm2 / keys [b, m]: theirs, or None (computed; caller keys only filter, as in the constructor).
        -> (first_id, m): the new queries are the indexed queries first_id .. first_id + m - 1.  Afterwards .n, .sig,
        .norm2, .keys, .ids and .dir describe the grown index -- the arrays a fresh QueryIndex over all rows holds --
        and a defaulted K is round(log_1.5 n) of the new n.
        update_lists=True (an index that holds lists; ValueError otherwise): the batch is then probed against the grown
        index (every new query kept out of its own list) and .lists is replaced by the lists of all n + m queries at
        the lists' own K (.lists_K, the run's -- not a defaulted K that follows n); any split of a batch into
        successive appends gives the same lists.  update_lists=False: held lists would go stale, so .lists becomes None
        (and a later update_lists=True raises)."""
        if update_lists and self.lists is None:
            raise ValueError("this index holds no lists to update (none were given, or an append without "
                             "update_lists=True dropped them)")
        given = keys is not None
        sig, norm2, keys = self._probe_rows(sig, norm2, keys)
        n, m = self.n, sig.shape[0]
        if n + m >= 2**32 - 1:
            raise ValueError("at most 2^32 - 2 indexed queries")
        if update_lists and n + m >= 2**31:
            raise ValueError("lists are kept for fewer than 2^31 queries")
        if m == 0:
            return n, 0
        step = self._probe_step
        if update_lists and m > step:
            for q0 in range(0, m, step):
                q1 = min(m, q0 + step)
                self.append(sig[q0:q1], norm2[q0:q1].contiguous(), keys[:, q0:q1].contiguous(), update_lists=True)
            return n, m
        grown = ops.index_append(self.keys, self.ids, self.dir, keys.clone() if given or update_lists else keys)
        if n + m > self._sig_buf.shape[0]:
            self.reserve(max(n + m, 2 * self._sig_buf.shape[0]))
        self._sig_buf[n:n + m].copy_(sig)
        self._norm2_buf[n:n + m].copy_(norm2)
        self.keys, self.ids, self.dir = grown
        self.n = n + m
        self.sig, self.norm2 = self._sig_buf[:self.n], self._norm2_buf[:self.n]
        if self._default_K:
            self.K = self._K_rule(self.n)
        if update_lists:
            K = self.lists_K
            raw, pws = ops.index_probe(self.keys, self.ids, self.dir, self.r, keys)
            off, idx, milli, _, skeys = ops.index_finish(self.sig, self.norm2, sig, norm2, self.b, pws, raw, K, first_id=n)
            self.lists = ops.lists_update(*self.lists, n, m, self.b, K, raw, skeys, off, idx, milli)
        else:
            self.lists = None
        return n, m

    def add(self, offsets, rows, update_lists=False):
        """signatures() of CSR answer sets, then append(): -> (first_id, m)"""
        return self.append(*self.signatures(offsets, rows), update_lists=update_lists)

    # ---- shrinking the index ---------------------------------------------------------------------------------------
    def remove(self, ids, update_lists=False):
        """take queries out of the index: ids = their positions (array or tensor of integers, any order, duplicates
        allowed; ValueError for one outside [0, n), the index unchanged).  The survivors are renumbered by rank, so ids
        stay dense.  -> new_pos, int64 device tensor [old n]: the new id of every old id, -1 for a removed one.
        Afterwards .n, .sig, .norm2, .keys, .ids and .dir are the arrays a fresh QueryIndex over the surviving rows holds
        (built with the surviving keys: one stable compaction per band, no sort), and a defaulted K follows the new n.
        update_lists=True (an index that holds lists; ValueError otherwise): .lists becomes the lists of a run over the
        survivors at .lists_K.  Stored rows shorter than K only lose their removed entries; a row of exactly K entries
        that loses one is probed again against the shrunk index, with the keys it is indexed under.
        update_lists=False: held lists would go stale, so .lists becomes None.  No ids: nothing happens.
        .last_picked: how many rows the last remove(update_lists=True) probed again (None after one without)."""
        if update_lists and self.lists is None:
            raise ValueError("this index holds no lists to update (none were given, or an append or remove without "
                             "update_lists=True dropped them)")
        dev = self.sig.device
        t = _ids_arg(ids, dev)
        n = self.n
        if update_lists and n >= 2**31:
            raise ValueError("lists are kept for fewer than 2^31 queries")
        if t.numel() == 0:
            return torch.arange(n, dtype=torch.int64, device=dev)
        # ids beyond uint32 all become 2^32 - 1, which no index holds (n < 2^32 - 1): the map build flags them
        t = torch.where((t < 0) | (t > 0xFFFFFFFF), torch.full_like(t, 0xFFFFFFFF), t)
        removed = ops.idmap_build(_u32_bits(t), n)
        new_pos = removed.positions()
        left = n - removed.count
        pick = None
        if update_lists:
            K = self.lists_K
            pick = ops.lists_remove_mark(self.lists[0], self.lists[1], n, K, removed)
        keys, ids_, dirw, pick_keys = ops.index_remove(self.keys, self.ids, removed, pick)
        sig, norm2 = ops.rows_remove(self.sig, self.norm2, removed)
        if update_lists:
            self_ids = new_pos[pick.members().to(torch.int64) & 0xFFFFFFFF].to(torch.int32)
            lists = ops.lists_remove(*self.lists, n, K, removed, pick,
                                     *self._probe_indexed((keys, ids_, dirw), sig, norm2, self_ids, pick_keys, K), self_ids)
        self.keys, self.ids, self.dir = keys, ids_, dirw
        self.n = left
        self.sig, self.norm2 = sig, norm2
        self._sig_buf, self._norm2_buf = sig, norm2
        self._own_rows = True
        if self._default_K:
            self.K = self._K_rule(self.n)
        self.lists = lists if update_lists else None
        self.last_picked = pick.count if update_lists else None
        return new_pos

    # ---- replacing queries in place -------------------------------------------------------------------------------
    def replace(self, ids, sig, norm2=None, keys=None, update_lists=False):
        """give indexed queries new rows: ids = their positions (array or tensor of m distinct integers in [0, n), any
        order; ValueError for a duplicate or an id outside, the index unchanged), sig / norm2 / keys [b, m] as append()
        takes them, row x for ids[x].  n, b and every other id stay.  Afterwards .sig, .norm2, .keys, .ids and .dir are
        the arrays a fresh QueryIndex over the rows with those overwritten holds (with caller keys: over the key matrix
        with those columns overwritten); a new record goes among the records of equal mix bits by its id.
        update_lists=True (an index that holds lists; ValueError otherwise): .lists becomes the lists of a run over the
        new rows at .lists_K.  A row outside ids drops its entries that name a replaced query and merges with the
        replaced queries that now name it, ties by id both ways; a row of exactly K entries that loses one is probed
        again with the keys it is indexed under (.last_picked counts them); a replaced query is probed with its new row.
        Any split of a batch into successive replacements gives the same result.  update_lists=False: .lists becomes
        None.  No ids: nothing happens.  The tensors given to the constructor are never written."""
        if update_lists and self.lists is None:
            raise ValueError("this index holds no lists to update (none were given, or a call without update_lists=True "
                             "dropped them)")
        t = _ids_arg(ids, self.sig.device)
        sig, norm2, keys = self._probe_rows(sig, norm2, keys)     # the sort below leaves copies: consumed freely
        n, m = self.n, sig.shape[0]
        if t.numel() != m:
            raise ValueError("%d ids for %d rows" % (t.numel(), m))
        if update_lists and n >= 2**31:
            raise ValueError("lists are kept for fewer than 2^31 queries")
        if m == 0:
            return
        t, order = torch.sort(t)
        if bool(((t[0] < 0) | (t[-1] >= n) | (t[1:] == t[:-1]).any()).item()):
            raise ValueError("ids must be distinct and lie in [0, %d)" % n)
        sig, norm2, keys = sig[order].contiguous(), norm2[order].contiguous(), keys[:, order].contiguous()
        step = self._probe_step
        if update_lists and m > step:             # successive replacements give the same lists
            self._replace_check_lists(t)
            picked = 0
            for q0 in range(0, m, step):
                q1 = min(m, q0 + step)
                self.replace(t[q0:q1], sig[q0:q1], norm2[q0:q1], keys[:, q0:q1].contiguous(), update_lists=True)
                picked += self.last_picked
            self.last_picked = picked
            return
        rids = _u32_bits(t)
        replaced = ops.idmap_build(rids, n)
        pick = None
        if update_lists:
            K = self.lists_K
            pick = ops.lists_remove_mark(self.lists[0], self.lists[1], n, K, replaced)     # raises before any write
        nkeys, nids, ndir, pick_keys = ops.index_replace(self.keys, self.ids, self.dir, replaced, rids,
                                                         keys.clone() if update_lists else keys, pick)
        if not self._own_rows:      # copy on first write: the constructor's tensors stay as they were given
            self._sig_buf, self._norm2_buf = self._sig_buf.clone(), self._norm2_buf.clone()
            self.sig, self.norm2 = self._sig_buf[:n], self._norm2_buf[:n]
            self._own_rows = True
        ops.rows_replace(self.sig, self.norm2, rids, sig, norm2)
        self.keys, self.ids, self.dir = nkeys, nids, ndir
        if not update_lists:
            self.lists, self.last_picked = None, None
            return
        raw, pws = ops.index_probe(nkeys, nids, ndir, self.r, keys)
        r_off, r_idx, r_milli, _, skeys = ops.index_finish_rows(self.sig, self.norm2, sig, norm2, self.b, pws, raw, K, rids,
                                                                want_keys=True)
        pick_ids = pick.members()
        self.lists = ops.lists_replace(*self.lists, n, self.b, K, replaced, rids, pick, pick_ids, raw, skeys, r_off, r_idx,
                                       r_milli, *self._probe_indexed((nkeys, nids, ndir), self.sig, self.norm2, pick_ids,
                                                                     pick_keys, K))
        self.last_picked = pick.count

    def _replace_check_lists(self, t):
        """the stored lists' contract, checked before the first of several successive replacements writes anything"""
        ops.lists_remove_mark(self.lists[0], self.lists[1], self.n, self.lists_K,
                              ops.idmap_build(_u32_bits(t[:1]), self.n))

    def _chunked(self, m, probe):
        """probe(q0, q1) -> (off, idx, milli, ...) of probe rows q0 .. q1-1, called for chunks of m * b < 2^32 words (what
        the library takes per call; the results do not depend on the split) -> the same for all m rows, offsets stitched.
        m = 0 gives the empty (off, idx, milli) of _probe_indexed; neighbours() answers m = 0 itself"""
        step = self._probe_step
        parts = [probe(q0, min(m, q0 + step)) for q0 in range(0, m, step)]
        if len(parts) == 1:
            return parts[0]
        if not parts:
            return self._empty_lists(2)
        offs, base = [torch.zeros((1,), dtype=torch.int64, device=self.sig.device)], 0
        for p in parts:
            offs.append(p[0][1:] + base)
            base += p[1].numel()
        return (torch.cat(offs),) + tuple(torch.cat([p[k] for p in parts]) for k in range(1, len(parts[0])))

    def _probe_indexed(self, index, sig, norm2, self_ids, keys, K):
        """the lists of chosen indexed rows: self_ids int32 [count] (uint32 bit patterns) = their ids in sig / norm2, keys
        [b, count] = the keys they are indexed under, index = (keys, ids, dir) to probe -> (off, idx, milli), every row
        kept out of its own list"""
        rows = self_ids.to(torch.int64) & 0xFFFFFFFF
        psig, pnorm2 = sig[rows], norm2[rows]

        def probe(q0, q1):
            raw, pws = ops.index_probe(*index, self.r, keys[:, q0:q1].contiguous())
            return ops.index_finish_rows(sig, norm2, psig[q0:q1], pnorm2[q0:q1].contiguous(), self.b, pws, raw, K,
                                         self_ids[q0:q1].contiguous())[:3]
        return self._chunked(self_ids.numel(), probe)

    # ---- changing the list length of the held lists ---------------------------------------------------------------
    def set_list_length(self, K2):
        """give the held lists the list length K2 (1..MAX_K) without a run: afterwards .lists is element for element
        the lists of a full run over the indexed rows with K = K2, .lists_K = K2, and every later update_lists=True keeps
        them exact at K2.  .K (the default probe length), the index arrays and the rows are not touched; .lists gets new
        tensors, the old ones are never written.
        K2 < lists_K: a cut (csrc/listcut.hip) -- the first K2 entries of every stored row are the row a run with K2
        would have stored; one read-back.  K2 > lists_K: a regrow -- a stored row with fewer than lists_K entries was
        never cut and stays; the rows of exactly lists_K entries are probed again against the index with K2, under the
        keys they are indexed under (so caller keys behave the same); two read-backs beside the probe's own (the picked
        rows, the new total).
        K2 == lists_K: nothing happens (.lists stays the same object).
        -> the number of rows probed again (0 for a cut), also in .last_picked.  ValueError, nothing changed: K2 outside
        1..MAX_K, an index without lists, n >= 2^31, or stored lists that break their contract (src not ascending, an id
        outside [0, n), a row longer than lists_K)."""
        K2 = _int_in(K2, "K2", 1, MAX_K)
        if self.lists is None:
            raise ValueError("this index holds no lists (none were given, or a call without update_lists=True dropped them)")
        if self.n >= 2**31:
            raise ValueError("lists are kept for fewer than 2^31 queries")
        K1 = self.lists_K
        src, dst, val = self.lists
        if K2 == K1:
            self.last_picked = 0
            return 0
        if K2 < K1:
            lists = ops.lists_cut(src, dst, val, self.n, K1, K2)        # raises before anything is bound
            self.lists, self.lists_K, self.last_picked = lists, K2, 0
            return 0
        pick = ops.lists_regrow_mark(src, self.n, K1)                   # raises before anything is bound
        if pick.count:
            pick_ids = pick.members()
            pick_keys = ops.index_pick_keys(self.keys, self.ids, pick)
            probed = self._probe_indexed((self.keys, self.ids, self.dir), self.sig, self.norm2, pick_ids, pick_keys, K2)
            lists = ops.lists_remove(src, dst, val, self.n, K2, ops.idmap_empty(self.n, src.device), pick, *probed,
                                     pick_ids)
        else:
            lists = (src, dst, val)       # no row was cut: the lists at K2 are the lists held
        self.lists, self.lists_K, self.last_picked = lists, K2, pick.count
        return pick.count

    def set(self, ids, offsets, rows, update_lists=False):
        """signatures() of CSR answer sets, then replace(): answer set x becomes that of indexed query ids[x]"""
        return self.replace(ids, *self.signatures(offsets, rows), update_lists=update_lists)

    def neighbours_of(self, first_id, m, K=None, keys=None):
        """the lists of the indexed queries first_id .. first_id + m - 1 recomputed from the index: each query's K best
        among ALL other indexed queries (itself excluded; rows with the same signature and another id stay in, at
        1000).  keys [b, m]: the band keys these queries were indexed under when they were the caller's (default:
        computed from the rows, as the constructor does).  -> (off, idx, milli, avail) as neighbours()."""
        K = self.K if K is None else _int_in(K, "K", 1, MAX_K)
        first_id = _int_in(first_id, "first_id", 0, max(self.n, 0))
        m = _int_in(m, "m", 0, self.n - first_id)
        if m == 0:
            return self._empty_lists()
        if m * self.b >= 2**32:
            raise ValueError("at most %d queries per call" % ((2**32 - 1) // self.b))
        sig, norm2, keys = self._probe_rows(self.sig[first_id:first_id + m], self.norm2[first_id:first_id + m].contiguous(),
                                            keys)
        raw, pws = ops.index_probe(self.keys, self.ids, self.dir, self.r, keys)
        off, idx, milli, avail, _ = ops.index_finish(self.sig, self.norm2, sig, norm2, self.b, pws, raw, K,
                                                     first_id=first_id)
        return off, idx, milli, avail

    def _run(self, sig, norm2, keys, K):
        raw, pws = ops.index_probe(self.keys, self.ids, self.dir, self.r, keys)
        return ops.index_finish(self.sig, self.norm2, sig, norm2, self.b, pws, raw, K), raw

    def neighbours(self, sig, norm2=None, keys=None, K=None):
        """sig: signature rows of m new queries (int32 or compact int16; converted to the index's format); norm2 /
        keys: theirs, or None (computed).  K: list length, default the index's (1..256).
        -> (off int64 [m + 1], idx int32, milli int32, avail int32 [m]) device tensors: CSR lists of indexed ids by
        milli descending, then id ascending; avail = distinct candidates before the cut."""
        K = self.K if K is None else _int_in(K, "K", 1, MAX_K)
        sig, norm2, keys = self._probe_rows(sig, norm2, keys)
        m = sig.shape[0]
        if m == 0:
            return self._empty_lists()
        return self._chunked(m, lambda q0, q1: self._run(sig[q0:q1], norm2[q0:q1], keys[:, q0:q1].contiguous(), K)[0][:4])

    def candidates(self, sig, norm2=None, keys=None):
        """every candidate of every new query, uncut: -> (query int64, id int64) device tensors, ordered by query,
        then the band that first brought the id"""
        sig, norm2, keys = self._probe_rows(sig, norm2, keys)
        m = sig.shape[0]
        dev = self.sig.device
        if m == 0:
            e = torch.empty((0,), dtype=torch.int64, device=dev)
            return e, e.clone()
        if m * self.b >= 2**32:
            raise ValueError("at most %d new queries per call" % ((2**32 - 1) // self.b))
        (_, _, _, _, skeys), raw = self._run(sig, norm2, keys, 1)
        kept = skeys != -1
        q = torch.div((raw[kept] >> 32) & 0xFFFFFFFF, self.b, rounding_mode="floor")
        return q, raw[kept] & 0xFFFFFFFF

    def predict_columns(self, ratings, off, idx, milli, sum_order="pairwise", query_weight=QUERY_WEIGHT,
                        user_weight=USER_WEIGHT, default_mean=DEFAULT_MEAN):
        """ratings: (nu, n) utility matrix of the indexed queries (0 = missing; array or tensor); (off, idx, milli):
        neighbours()' lists.  -> int32 device tensor [m, nu]: every user's predicted cell of each new query."""
        sum_order = sum_order_code(sum_order)
        r = matrix(ratings, "ratings")
        if r.shape[1] != self.n:
            raise ValueError("ratings have %d columns, the index %d queries" % (r.shape[1], self.n))
        if r.shape[0] > 65535 * 256:
            raise ValueError("at most %d users" % (65535 * 256))
        for t, name in ((off, "off"), (idx, "idx"), (milli, "milli")):
            if not isinstance(t, torch.Tensor) or t.dim() != 1:
                raise ValueError("%s must be a 1-D device tensor (neighbours()' output)" % name)
        dev = self.sig.device
        return ops.predict_columns(on_device(r, dev), off.to(dev, torch.int64).contiguous(),
                                   idx.to(dev, torch.int32).contiguous(), milli.to(dev, torch.int32).contiguous(),
                                   query_weight, user_weight, default_mean, sum_order)

    @staticmethod
    def top_users(columns, k):
        """columns: predict_columns' [m, nu] output.  -> (users int32 [m, k], values int32 [m, k], avail int32 [m]): per
        new query the users with the largest non-zero predictions, value descending then user ascending (-1 / 0
        padding), and how many users have one (qrlsh_recommend_topk over the rows, nothing rated)."""
        if not isinstance(columns, torch.Tensor) or columns.dim() != 2:
            raise ValueError("columns must be predict_columns' 2-D device tensor")
        zeros = torch.zeros_like(columns, dtype=torch.int32)
        return top_k(zeros, columns, k, device=columns.device)
