"""Device-resident passage-embedding bank of the interaction rerankers (rr_bank_*, include/rerank_mi355.h).

The interaction families rerank from the frozen retriever's token embeddings, which the reference hands over in fp16
(`D = D.half()`, src/models/flmr/models/flmr/modeling_flmr.py:1554-1555 of the reference).  A `PassageBank` keeps them on the
device in that form, every passage at its own length, under the caller's passage ids; a forward then names passages
(RerankEngine.forward_interaction_bank, InteractionRerankModel.forward_passages, pipeline.InteractionStages) instead of
uploading and packing a padded float32 [N, Lc, D] tensor per query.

A bank created with a `PlaidCodec` is a COMPRESSED one: it holds the rows as a ColBERTv2 / PLAID index stores them (one int32
centroid code and D * nbits / 8 residual bytes per token; third_party/ColBERT/colbert/indexing/codecs/residual.py of the reference)
and decodes them on the device inside the forward's gather, bit for bit the fp16 bank of the decoded rows (the decoded row:
include/rerank_mi355.h, rr_bank_create_plaid).  `read_plaid_index` reads such an index from disk with torch.load and json alone.

`PassageBank.maxsim` / RerankEngine.bank_li_scores give the retriever's own score of (query, passage) pairs (MaxSim and the score
matrix, rr_bank_li_scores) from either kind of bank, without a padded context tensor.

`PassageBank.search` / RerankEngine.bank_search give the k best passages of the bank (or of a range of it) per query by that
score, exactly (rr_bank_search): every passage is scored, nothing is pruned.  With a `PlaidSearch` the same calls run PLAID's
staged search over a compressed bank (rr_bank_search_plaid, RerankEngine.bank_search_plaid): candidates by centroid, two
centroid-only pruning passes, exact MaxSim on the survivors.  `PassageBank.build_ivf` builds the bank's inverted file on the
device (rr_bank_build_ivf: per centroid the sorted unique passages holding a token of that code, the reference's ivf.pid.pt;
`extend_ivf` takes it over passages added later, rr_bank_extend_ivf; `ivf` / `save_ivf` read and write it), and
`PlaidSearch(..., ivf=True)` takes the candidates from it (rr_bank_search_plaid_ivf): the same result, with work that follows the lists of the query's cells instead of the rows of the bank.  `PassageBank.filter`
makes a candidate filter (a `BankFilter`: a device bitmap over the bank's passages, one set for every query or one per query,
rr_bank_filter_fill) and `search(..., filter=)` restricts any of the three searches to it (rr_bank_search_filtered,
rr_bank_search_plaid_filtered, rr_bank_search_plaid_ivf_filtered): the reference's filter_fn.

`PassageBank.add_compress` fills a compressed bank from embeddings that are on the device (rr_bank_add_compress): nearest centroid
on the matrix core and residual bucketising in two kernels, the codec's cutoffs given as `PlaidCodec(bucket_cutoffs=...)`.

`PlaidCodec.train` makes the codec itself from embeddings on the device (rr_plaid_kmeans, rr_plaid_residuals): k-means centroids by
Lloyd's iteration with an exact fixed-point sum, bucket cutoffs and weights from held-out residuals; `PlaidCodec.save` writes it as an
index stores it.  With it a compressed bank is built from a retriever's embeddings with nothing but this library.

`PassageBank.save_plaid_index` writes a compressed bank as the index directory the reference's indexer writes and its Searcher opens
(`write_plaid_index`: chunk files, codec, metadata.json, ivf.pid.pt), the rows taken off the device by rr_bank_export_plaid
(`export_compressed`: the unmasked rows of a range back to back, compacted by a kernel); `load_plaid_index(..., ivf=True)` brings the
directory back with its inverted file (`load_ivf`, rr_bank_load_ivf) instead of rebuilding it.

An fp16 bank WITH A CENTROID TABLE (`create_bank(..., centroids=)`, `PassageBank.set_centroids`; rr_bank_set_centroids) keeps its fp16
rows and holds one centroid code per row beside them, assigned on the device by every `add`: the pruned searches, the inverted file,
the filters, `remove` and the sharded search take it as they take a compressed bank, with the exact stage on the fp16 rows; there
are no residuals, so `save_plaid_index` / `export_compressed` refuse it.  `PassageBank.codes` reads a passage's codes.

`search_banks` searches several banks of one process as one (every bank searched, the k-lists merged on the device over global
indices by rr_bank_merge_topk); a bank split over RANKS is sharding.ShardedBank.

`BankTable`, `plan_bank_batch`, `plan_bank_scores`, `PlaidCodec`, `read_plaid_index` and `write_plaid_index` are the host side: pure Python /
numpy / torch on the CPU, usable and tested without a device.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

from .pair_inputs import group_pairs_by_length


class PlaidSearch:
    """The parameters of PLAID's pruned search (rr_bank_search_plaid): `ncells` centroids per query token open the candidate set,
    centroids whose best score is below `centroid_score_threshold` do not count in the first pruning pass, `ndocs` candidates
    survive it and ndocs // 4 the second; `coarse_tokens`: the leading query tokens the approximate stages use (None: all).
    `ivf`: take the candidates from the bank's inverted file (rr_bank_search_plaid_ivf; PassageBank.build_ivf first): the same
    result, bit for bit, with work that follows the lists of the query's cells instead of the rows of the bank."""

    def __init__(self, ncells: int, centroid_score_threshold: float, ndocs: int, coarse_tokens: Optional[int] = None, ivf: bool = False):
        self.ncells, self.centroid_score_threshold, self.ndocs = int(ncells), float(centroid_score_threshold), int(ndocs)
        self.coarse_tokens = None if coarse_tokens is None else int(coarse_tokens)
        self.ivf = bool(ivf)

    @classmethod
    def defaults(cls, k: int, coarse_tokens: Optional[int] = None, ivf: bool = False) -> "PlaidSearch":
        """The reference's parameters by k (third_party/ColBERT/colbert/searcher.py:97-122): k <= 100: ncells 2, threshold 0.45,
        ndocs 1024 (its k <= 10 branch sets the same three).  Its k > 100 defaults need ndocs = max(4 k, 4096), above what the
        search takes: NotImplementedError."""
        k = int(k)
        if k < 1:
            raise ValueError(f"PlaidSearch.defaults: k = {k}")
        if k <= 100:
            return cls(2, 0.45, 1024, coarse_tokens, ivf)
        raise NotImplementedError(f"PlaidSearch.defaults: k = {k}: the reference's defaults above k = 100 (ncells 4, threshold 0.4, "
                                  f"ndocs {max(4 * k, 4096)}) need ndocs above 1024, the most the pruned search takes")

    def __repr__(self) -> str:
        return (f"PlaidSearch(ncells={self.ncells}, centroid_score_threshold={self.centroid_score_threshold}, ndocs={self.ndocs}, "
                f"coarse_tokens={self.coarse_tokens}" + (", ivf=True)" if self.ivf else ")"))


def f16_default_slack(query_norm_sum: float, li_dim: int, Lq: int) -> float:
    """The bound on |A - E| that rr_bank_search_f16's certificate stands on (include/rerank_mi355.h, SLACK), for unit rows stored as
    fp16 (R = 1 + 2^-10) and |E| <= S R: S R (2^-11 + D 2^-22) + Lq 2^-22 S R + Lq sqrt(D) 2^-25 R, S = `query_norm_sum`, the sum
    over a query's tokens of their 2-norms (the largest over the queries of a call).  The last term: below fp16's normal range
    (2^-14) an element's rounding error is absolute, at most 2^-25, not 2^-11 of the element.  For query elements below
    F16_QUERY_LIMIT in magnitude only: one at or above it rounds to infinity, and no finite slack bounds that (F16Search.slack_for)."""
    r = 1.0 + 2.0 ** -10
    sr = float(query_norm_sum) * r
    return sr * (2.0 ** -11 + int(li_dim) * 2.0 ** -22) + int(Lq) * 2.0 ** -22 * sr + int(Lq) * float(li_dim) ** 0.5 * 2.0 ** -25 * r


F16_QUERY_LIMIT = 65520.0          # the least magnitude that round-to-nearest-even takes to fp16's infinity


class F16Search:
    """The parameters of the exhaustive search whose first pass runs on the fp16 matrix core (rr_bank_search_f16): the `ndocs`
    (1 .. 1024) approximately best passages per query are rescored exactly; `slack`: the bound on |approximate - exact| its
    certificate uses, None: f16_default_slack on the call's queries."""

    def __init__(self, ndocs: int, slack: Optional[float] = None):
        self.ndocs = int(ndocs)
        if self.ndocs < 1:
            raise ValueError(f"F16Search: ndocs = {ndocs}")
        if self.ndocs > 1024:
            raise NotImplementedError(f"F16Search: ndocs = {ndocs} (at most 1024, the selection kernel's limit)")
        self.slack = None if slack is None else float(slack)
        if self.slack is not None and not self.slack >= 0.0:
            raise ValueError(f"F16Search: slack = {slack} (>= 0, not NaN)")

    def slack_for(self, query_li) -> float:
        """`slack`, or the default bound for `query_li` [n_queries, Lq, D] (two reductions on its device, one read-back): +inf
        when an element is infinite or rounds to infinity in fp16 (the query is then certified only if every passage is
        rescored), NaN for a NaN query (the entries refuse it)."""
        if self.slack is not None:
            return self.slack
        import torch
        q = query_li.double()
        s, top = torch.stack([q.norm(dim=-1).sum(dim=-1).max(), q.abs().max()]).tolist()
        d = f16_default_slack(s, int(query_li.shape[-1]), int(query_li.shape[-2]))
        if d == d and top >= F16_QUERY_LIMIT:
            return float("inf")
        return d

    def __repr__(self) -> str:
        return f"F16Search(ndocs={self.ndocs}, slack={self.slack})"


def _f16_entry(engine, bank):
    """The entry `fast=` names for `bank`: a compressed bank (one with a codec) takes engine.bank_search_f16_plaid, whose first pass
    decodes the rows it multiplies; an fp16 bank, plain or coded, engine.bank_search_f16.  The same arguments, the same dict."""
    return engine.bank_search_f16_plaid if getattr(bank, "codec", None) is not None else engine.bank_search_f16


def _fast_check(name: str, fast, plaid, filter, sparse) -> None:
    """`fast` names the unfiltered exhaustive search: with `plaid`, a filter or `sparse` there is no such entry."""
    if fast is not None and (plaid is not None or filter is not None or sparse):
        raise ValueError(f"{name}: fast= with plaid=, filter= or sparse= (the fp16 first pass scores every passage of the range)")


class BankFilter:
    """A candidate filter of the bank searches (PassageBank.filter; "CANDIDATE FILTERS", include/rerank_mi355.h): `bits`, the device
    bitmap int32 [rows, ld] (bit i & 31 of word i >> 5 of a row: dense bank index i), `rows` (1: one set for every query; else one
    row per query) and `passages`, the passage count of the bank when it was built: passages added later are not allowed by it;
    `generation`, the bank's generation then: a removal renumbers the passages and a `clear` forgets them (a refill puts other
    passages under the old numbers), so a filter from before either names passages the bank no longer holds there."""

    def __init__(self, bits, rows: int, passages: int, generation: int = 0):
        self.bits, self.rows, self.passages, self.generation = bits, int(rows), int(passages), int(generation)

    def __repr__(self) -> str:
        return f"BankFilter(rows={self.rows}, passages={self.passages})"


class BankTable:
    """The host table of a bank: passage id -> dense index, dense index -> passage id (`ids`), and every passage's length in rows."""

    def __init__(self):
        self.index_of: dict = {}
        self.lengths: list = []
        self.ids: list = []

    def __len__(self) -> int:
        return len(self.lengths)

    def __contains__(self, passage_id) -> bool:
        return passage_id in self.index_of

    def check_new(self, passage_ids: Sequence) -> None:
        """ValueError when an id is in the table already or appears twice in `passage_ids`; nothing is changed."""
        seen = set()
        for pid in passage_ids:
            if pid in self.index_of or pid in seen:
                raise ValueError(f"passage id {pid!r} is in the bank already: an id is added once")
            seen.add(pid)

    def append(self, passage_ids: Sequence, lengths: Sequence[int], first_index: Optional[int] = None) -> int:
        """Register ids with their lengths under the next dense indices; returns the first of them."""
        assert len(passage_ids) == len(lengths), "one length per passage id"
        self.check_new(passage_ids)
        first = len(self.lengths)
        assert first_index is None or first_index == first, f"the bank's indices continue at {first_index}, the table's at {first}"
        for pid, ln in zip(passage_ids, lengths):
            assert int(ln) >= 1, f"passage {pid!r}: length {ln}"
            self.index_of[pid] = len(self.lengths)
            self.lengths.append(int(ln))
            self.ids.append(pid)
        return first

    def lookup(self, passage_ids: Sequence):
        """(indices, lengths) of `passage_ids` as int64 numpy arrays; an id the table does not hold raises a KeyError naming it."""
        import numpy as np
        idx = np.empty(len(passage_ids), dtype=np.int64)
        lens = np.empty(len(passage_ids), dtype=np.int64)
        for i, pid in enumerate(passage_ids):
            try:
                j = self.index_of[pid]
            except KeyError:
                raise KeyError(f"passage id {pid!r} is not in the bank") from None
            idx[i], lens[i] = j, self.lengths[j]
        return idx, lens

    def check_remove(self, passage_ids: Sequence):
        """The dense indices of `passage_ids` as a list; KeyError names an id the table does not hold, ValueError one given
        twice; nothing is changed."""
        idx = self.lookup(passage_ids)[0].tolist()
        if len(set(idx)) != len(idx):
            seen = set()
            for pid in passage_ids:
                if pid in seen:
                    raise ValueError(f"passage id {pid!r} is given twice: an id is removed once")
                seen.add(pid)
        return idx

    def remove(self, indices: Sequence[int]) -> list:
        """Drop the passages at the dense `indices` (distinct, inside the table: IndexError / ValueError, nothing changed): the
        others keep their order and are renumbered from 0; `index_of`, `ids` and `lengths` are rebuilt.  Returns the map old
        dense index -> new dense index, -1 for a removed passage."""
        n = len(self.lengths)
        gone = set()
        for i in indices:
            i = int(i)
            if not 0 <= i < n:
                raise IndexError(f"index {i} lies outside the table's {n} passages")
            if i in gone:
                raise ValueError(f"index {i} is given twice")
            gone.add(i)
        new_index, ids, lengths = [], [], []
        for i in range(n):
            if i in gone:
                new_index.append(-1)
            else:
                new_index.append(len(ids))
                ids.append(self.ids[i])
                lengths.append(self.lengths[i])
        self.ids, self.lengths = ids, lengths
        self.index_of = {pid: j for j, pid in enumerate(ids)}
        return new_index

    def clear(self) -> None:
        self.index_of.clear()
        self.lengths.clear()
        self.ids.clear()


def plan_bank_batch(table: BankTable, passage_ids: Sequence, K: Optional[int], list_sizes: Optional[Sequence[int]], padded_len: int,
                    granule: int = 16, segment_cost_rows: int = 0) -> dict:
    """Host side of one rr_forward_interaction_bank call.  `passage_ids`: the candidates in pair order, K per query, or
    `list_sizes[q]` for query q (K is None then).  Returns
      indices, lengths : bank index and length of every pair, pair order
      owner            : the query of every pair, pair order
      order, seg_n, seg_len : the packed pair order and the segment table (pair_inputs.group_pairs_by_length over the lengths)
      pair_passage, pair_query : int32, `indices` / `owner` in packed order — what the C call takes.
    Every pair appears once in `order` and every passage fits its segment; an unknown id raises KeyError naming it."""
    import numpy as np
    idx, lens = table.lookup(passage_ids)
    N = int(idx.size)
    assert N >= 1, "no passages"
    if list_sizes is None:
        assert K is not None and K >= 1 and N % K == 0, f"{N} passages are not lists of {K}"
        owner = np.arange(N, dtype=np.int64) // K
    else:
        sizes = np.asarray(list_sizes, dtype=np.int64).reshape(-1)
        assert sizes.size > 0 and int(sizes.min()) >= 1 and int(sizes.sum()) == N, \
            f"list_sizes {sizes.tolist()} do not partition {N} passages into non-empty lists"
        owner = np.repeat(np.arange(sizes.size, dtype=np.int64), sizes)
    assert int(lens.max()) <= padded_len, f"a passage of {int(lens.max())} rows exceeds the padded context length {padded_len}"
    order, seg_n, seg_len = group_pairs_by_length(lens, int(padded_len), int(granule), 1, int(segment_cost_rows))
    return dict(indices=idx, lengths=lens, owner=owner, order=order, seg_n=seg_n, seg_len=seg_len,
                pair_passage=idx[order].astype(np.int32), pair_query=owner[order].astype(np.int32))


def plan_bank_scores(table: BankTable, passage_ids: Sequence, n_queries: int, pair_query=None, K: Optional[int] = None,
                     list_sizes: Optional[Sequence[int]] = None, padded_len: Optional[int] = None) -> dict:
    """Host side of one rr_bank_li_scores call.  `passage_ids`: the passages in pair order (any passage any number of times).
    The query of every pair: `pair_query` explicitly (any order), or K pairs per query, or `list_sizes[q]` pairs for query q, as
    plan_bank_batch lays pairs out; exactly one of the three.  `padded_len`: the context rows per pair of the score block,
    default: the longest passage of the call.  Returns
      indices, lengths         : bank index and length of every pair (int64)
      pair_passage, pair_query : int32, pair order — what the C call takes
      padded_len               : int.
    The pairs are not reordered: the outputs come back in the caller's order.  An unknown id raises KeyError naming it."""
    import numpy as np
    idx, lens = table.lookup(passage_ids)
    N = int(idx.size)
    assert N >= 1, "no passages"
    assert (pair_query is not None) + (K is not None) + (list_sizes is not None) == 1, "one of pair_query, K and list_sizes"
    if pair_query is not None:
        owner = np.asarray(pair_query, dtype=np.int64).reshape(-1)
        assert owner.size == N, f"{owner.size} query indices for {N} passages"
    elif list_sizes is not None:
        sizes = np.asarray(list_sizes, dtype=np.int64).reshape(-1)
        assert sizes.size > 0 and int(sizes.min()) >= 1 and int(sizes.sum()) == N, \
            f"list_sizes {sizes.tolist()} do not partition {N} passages into non-empty lists"
        owner = np.repeat(np.arange(sizes.size, dtype=np.int64), sizes)
    else:
        assert K >= 1 and N % K == 0, f"{N} passages are not lists of {K}"
        owner = np.arange(N, dtype=np.int64) // K
    assert int(owner.min()) >= 0 and int(owner.max()) < n_queries, \
        f"the pairs name queries {int(owner.min())} .. {int(owner.max())}, query_li holds {n_queries}"
    longest = int(lens.max())
    Lc = longest if padded_len is None else int(padded_len)
    assert longest <= Lc, f"a passage of {longest} rows exceeds the padded context length {Lc}"
    return dict(indices=idx, lengths=lens, pair_passage=idx.astype(np.int32), pair_query=owner.astype(np.int32), padded_len=Lc)


PLAID_NBITS = (1, 2, 4, 8)


def plaid_shape_ok(nbits: int, dim: int) -> bool:
    """What a compressed bank takes: nbits 1, 2, 4 or 8; dim a power of two in [8, 512] and a multiple of 8 * nbits."""
    return nbits in PLAID_NBITS and 8 <= dim <= 512 and dim & (dim - 1) == 0 and dim % (8 * nbits) == 0


class PlaidCodec:
    """The tables of a ColBERTv2 / PLAID residual codec, as an index stores them: `centroids` [C, D] (kept as fp16: the index
    saves them with .half(), codecs/residual.py:161), `bucket_weights` [2^nbits] (kept as float32) and `nbits`; optionally
    `bucket_cutoffs` [2^nbits - 1] (the first tensor of buckets.pt, kept as float32), which compressing needs and decoding does
    not.  It validates shapes, dtypes and the cutoffs (ValueError: wrong count, a NaN, a decreasing sequence); `decode` and
    `compress` run the host definitions of the library."""

    def __init__(self, centroids, bucket_weights, nbits: int, *, bucket_cutoffs=None):
        import torch
        if not isinstance(nbits, int) or isinstance(nbits, bool) or nbits not in PLAID_NBITS:
            raise ValueError(f"nbits {nbits!r}: 1, 2, 4 or 8")
        centroids, bucket_weights = torch.as_tensor(centroids), torch.as_tensor(bucket_weights)
        if centroids.dim() != 2 or centroids.shape[0] < 1 or not centroids.is_floating_point():
            raise ValueError(f"centroids must be a floating-point [C, D] tensor, got {centroids.dtype} {tuple(centroids.shape)}")
        dim = int(centroids.shape[1])
        if not plaid_shape_ok(nbits, dim):
            raise ValueError(f"dim {dim} at nbits {nbits}: a power of two in [8, 512] and a multiple of {8 * nbits}")
        if not bucket_weights.is_floating_point() or tuple(bucket_weights.shape) != (1 << nbits,):
            raise ValueError(f"bucket_weights must be {1 << nbits} floating-point values at nbits {nbits}, got {bucket_weights.dtype} "
                             f"{tuple(bucket_weights.shape)}")
        self.nbits, self.dim = nbits, dim
        self.centroids = centroids.detach().to(device="cpu", dtype=torch.float16).contiguous()
        self.bucket_weights = bucket_weights.detach().to(device="cpu", dtype=torch.float32).contiguous()
        self.bucket_cutoffs = None
        self.avg_residual = None             # PlaidCodec.train: the mean absolute held-out residual, and how the training went
        self.train_stats = None
        if bucket_cutoffs is not None:
            cut = torch.as_tensor(bucket_cutoffs)
            if not cut.is_floating_point() or tuple(cut.shape) != ((1 << nbits) - 1,):
                raise ValueError(f"bucket_cutoffs must be {(1 << nbits) - 1} floating-point values at nbits {nbits}, got {cut.dtype} "
                                 f"{tuple(cut.shape)}")
            cut = cut.detach().to(device="cpu", dtype=torch.float32).contiguous()
            if bool(torch.isnan(cut).any()):
                raise ValueError("bucket_cutoffs hold a NaN")
            if cut.numel() > 1 and bool((cut[1:] < cut[:-1]).any()):
                raise ValueError("bucket_cutoffs decrease: a bucket is the number of cutoffs below a residual")
            self.bucket_cutoffs = cut

    @property
    def n_centroids(self) -> int:
        return int(self.centroids.shape[0])

    @property
    def residual_bytes(self) -> int:
        """Bytes of packed residual per row."""
        return self.dim // 8 * self.nbits

    def decode(self, codes, residuals):
        """The decoded rows [R, D] float16 of `codes` [R] / `residuals` [R, residual_bytes] in host code
        (rr_util_plaid_decode_rows: the bit-level definition the device is held to; no GPU needed)."""
        import numpy as np
        import torch
        from . import _lib as L
        lib = L.load()
        codes = np.ascontiguousarray(np.asarray(codes).reshape(-1), dtype=np.int32)
        res = np.ascontiguousarray(np.asarray(residuals), dtype=np.uint8).reshape(codes.size, self.residual_bytes)
        out = torch.empty((codes.size, self.dim), dtype=torch.float16)
        rc = lib.rr_util_plaid_decode_rows(self.centroids.data_ptr(), self.n_centroids, self.bucket_weights.data_ptr(), self.nbits,
                                           self.dim, codes.ctypes.data, res.ctypes.data, codes.size, out.data_ptr())
        if rc == L.RR_ERR_BAD_SHAPE:
            raise ValueError(f"a centroid code lies outside [0, {self.n_centroids})")
        L.check(rc, None, "rr_util_plaid_decode_rows")
        return out

    def compress(self, rows):
        """(codes int32 [R], residuals uint8 [R, residual_bytes]) of `rows` [R, D] (float32 or float16; anything else goes through
        float32) in host code (rr_util_plaid_compress_rows: the compressed row of include/rerank_mi355.h, the definition the
        device is held to; no GPU needed).  Needs `bucket_cutoffs`; dim must be a multiple of 16."""
        import torch
        from . import _lib as L
        lib = L.load()
        if self.bucket_cutoffs is None:
            raise ValueError("compress needs the codec's bucket_cutoffs (PlaidCodec(..., bucket_cutoffs=...))")
        rows = torch.as_tensor(rows)
        if rows.dim() != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [R, {self.dim}], got {tuple(rows.shape)}")
        dt = rows.dtype if rows.dtype in (torch.float32, torch.float16) else torch.float32
        rows = rows.detach().to(device="cpu", dtype=dt).contiguous()
        R = int(rows.shape[0])
        codes = torch.empty(R, dtype=torch.int32)
        res = torch.empty((R, self.residual_bytes), dtype=torch.uint8)
        L.check(lib.rr_util_plaid_compress_rows(rows.data_ptr(), L.RR_F16 if dt == torch.float16 else L.RR_F32, R, self.dim,
                                                self.centroids.data_ptr(), self.n_centroids, self.bucket_cutoffs.data_ptr(), self.nbits,
                                                codes.data_ptr(), res.data_ptr()), None, "rr_util_plaid_compress_rows")
        return codes, res

    QUANTILE_MAX_ELEMENTS = 1 << 24          # what torch.quantile takes

    @staticmethod
    def bucket_statistics(residuals, nbits: int):
        """(bucket_cutoffs [2^nbits - 1], bucket_weights [2^nbits], avg_residual scalar) of held-out `residuals` [H, D] float32, on
        the device the tensor lives on: the mean absolute residual and the two `quantile` calls of the reference's
        _compute_avg_residual (third_party/ColBERT/colbert/indexing/collection_indexer.py:305-319), operation for operation.
        ValueError for an empty block and for more elements than torch.quantile takes."""
        import torch
        if residuals.dim() != 2 or residuals.numel() == 0:
            raise ValueError(f"the held-out block is empty: {tuple(residuals.shape)}")
        if residuals.numel() > PlaidCodec.QUANTILE_MAX_ELEMENTS:
            raise ValueError(f"the held-out block holds {residuals.numel()} elements, torch.quantile takes at most "
                             f"{PlaidCodec.QUANTILE_MAX_ELEMENTS}: lower heldout_max")
        avg_residual = torch.abs(residuals).mean(dim=0).cpu()
        num_options = 2 ** nbits
        quantiles = torch.arange(0, num_options, device=residuals.device) * (1 / num_options)
        cutoffs_q, weights_q = quantiles[1:], quantiles + (0.5 / num_options)
        cutoffs = residuals.float().quantile(cutoffs_q)
        weights = residuals.float().quantile(weights_q)
        return cutoffs.cpu(), weights.cpu(), avg_residual.mean()

    @classmethod
    def train(cls, engine, embeddings, nbits: int, n_centroids: Optional[int] = None, *, niters: int = 20, seed: int = 123,
              max_points_per_centroid: int = 256, heldout_fraction: float = 0.05, heldout_max: int = 50_000) -> "PlaidCodec":
        """Train a codec from `embeddings` [N, D] (a device tensor, float32 or float16; D the engine's li_dim) with nothing but this
        library: what the reference's indexer does with faiss k-means and _compute_avg_residual (collection_indexer.py:211-319,
        452-465).  The rows are shuffled with a CPU torch.randperm seeded with `seed`; the last int(min(heldout_fraction * N,
        heldout_max)) of them are held out, as the reference splits them; at most max_points_per_centroid * C of the rest train
        (faiss's default); the first C training rows are the initial centroids of rr_plaid_kmeans (THE TRAINED CENTROIDS,
        include/rerank_mi355.h; `niters` Lloyd iterations, empty clusters re-seeded from `seed`).  The held-out rows' residuals
        (rr_plaid_residuals) give avg_residual and the bucket cutoffs and weights by `bucket_statistics`, on the device.
        n_centroids None: plaid_num_partitions(N).
        The residuals are taken against the fp16 table, the one the index stores and add_compress uses; the reference's CPU branch
        subtracts the unrounded float32 table (its GPU branch the .half() one, as here).
        Returns a PlaidCodec with cutoffs; `.avg_residual` (float) and `.train_stats` (dict: n_train, n_heldout, counts int32 [C],
        stats int32 [niters, 2] = (rows that changed code, clusters re-seeded) per iteration).  ValueError when the held-out block
        is empty or holds more elements than torch.quantile takes."""
        import torch
        from . import _lib as L
        if embeddings.dim() != 2 or not embeddings.is_cuda:
            raise ValueError(f"embeddings must be a device tensor [N, D], got {embeddings.device} {tuple(embeddings.shape)}")
        N, D = int(embeddings.shape[0]), int(embeddings.shape[1])
        if D != int(engine.arch["li_dim"]):
            raise ValueError(f"embeddings hold rows of {D}, the engine's li_dim is {int(engine.arch['li_dim'])}")
        if not isinstance(nbits, int) or isinstance(nbits, bool) or nbits not in PLAID_NBITS:
            raise ValueError(f"nbits {nbits!r}: 1, 2, 4 or 8")
        Cn = plaid_num_partitions(N) if n_centroids is None else int(n_centroids)
        n_held = int(min(heldout_fraction * N, heldout_max))
        if n_held < 1:
            raise ValueError(f"the held-out block is empty: {N} rows at heldout_fraction {heldout_fraction}, heldout_max {heldout_max}")
        if n_held * D > cls.QUANTILE_MAX_ELEMENTS:
            raise ValueError(f"the held-out block holds {n_held * D} elements, torch.quantile takes at most {cls.QUANTILE_MAX_ELEMENTS}: "
                             "lower heldout_max")
        n_train = min(N - n_held, int(max_points_per_centroid) * Cn)
        if Cn < 1 or Cn > n_train:
            raise ValueError(f"{Cn} centroids of {n_train} training rows")
        dt = embeddings.dtype if embeddings.dtype in (torch.float32, torch.float16) else torch.float32
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(int(seed))).to(embeddings.device)
        shuffled = embeddings.to(dt)[perm]
        train = shuffled[:n_train].contiguous()
        held = shuffled[N - n_held:].contiguous()
        del shuffled
        lib, dev = engine.lib, embeddings.device
        rdt = L.RR_F16 if dt == torch.float16 else L.RR_F32
        st = torch.cuda.current_stream(dev).cuda_stream
        init = torch.arange(Cn, dtype=torch.int32)
        cen = torch.empty((Cn, D), dtype=torch.float16, device=dev)
        counts = torch.empty(Cn, dtype=torch.int32, device=dev)
        stats = torch.zeros((max(int(niters), 1), 2), dtype=torch.int32, device=dev)
        L.check(lib.rr_plaid_kmeans(engine.h, L.ptr(train), rdt, n_train, init.data_ptr(), Cn, int(niters), int(seed) & ((1 << 64) - 1),
                                    L.ptr(cen), L.ptr(counts), L.ptr(stats), st), engine.h, "rr_plaid_kmeans")
        codes = torch.empty(n_held, dtype=torch.int32, device=dev)
        resid = torch.empty((n_held, D), dtype=torch.float32, device=dev)
        L.check(lib.rr_plaid_residuals(engine.h, L.ptr(held), rdt, n_held, L.ptr(cen), Cn, L.ptr(codes), L.ptr(resid), st), engine.h,
                "rr_plaid_residuals")
        cutoffs, weights, avg = cls.bucket_statistics(resid, nbits)
        codec = cls(cen.cpu(), weights, nbits, bucket_cutoffs=cutoffs)
        codec.avg_residual = float(avg)
        codec.train_stats = dict(n_train=n_train, n_heldout=n_held, counts=counts.cpu(), stats=stats[:int(niters)].cpu())
        return codec

    def save(self, path: str) -> None:
        """Write the codec into the directory `path` as the reference's indexer does (codecs/residual.py:154-167): `centroids.pt`
        (fp16) and `buckets.pt` = (cutoffs, weights), the files read_plaid_index reads, and `avg_residual.pt` (the scalar a trained
        codec carries, 0 otherwise), which it does not read.  Needs `bucket_cutoffs`."""
        import os

        import torch
        if self.bucket_cutoffs is None:
            raise ValueError("save needs the codec's bucket_cutoffs: buckets.pt holds (cutoffs, weights)")
        os.makedirs(path, exist_ok=True)
        torch.save(self.centroids, os.path.join(path, "centroids.pt"))
        torch.save((self.bucket_cutoffs, self.bucket_weights), os.path.join(path, "buckets.pt"))
        torch.save(torch.tensor(float(self.avg_residual or 0.0)), os.path.join(path, "avg_residual.pt"))


def plaid_num_partitions(n_embeddings) -> int:
    """The number of centroids the reference's indexer picks for n_embeddings token embeddings: 2^floor(log2(16 sqrt(n)))
    (third_party/ColBERT/colbert/indexing/collection_indexer.py:98)."""
    import numpy as np
    if not n_embeddings >= 1:
        raise ValueError(f"n_embeddings = {n_embeddings}")
    return int(2 ** np.floor(np.log2(16 * np.sqrt(n_embeddings))))


def read_plaid_index(index_path: str):
    """Read a ColBERTv2 / PLAID index directory as the reference's indexer writes it
    (third_party/ColBERT/colbert/indexing/index_saver.py:33-46, collection_indexer.py): `metadata.json` (config.nbits, config.dim,
    num_chunks), `centroids.pt`, `buckets.pt` = (cutoffs, weights), and per chunk i `{i}.codes.pt`, `{i}.residuals.pt`,
    `doclens.{i}.json`.  torch.load and json only; nothing of colbert is imported.  Returns (PlaidCodec, chunks); `chunks` is a
    generator of (first passage number, codes int32 [R], residuals uint8 [R, D * nbits / 8], doclens list) that loads one chunk at a
    time.  The passage numbers run through the chunks in order, as the index numbers them.  The codec keeps the index's cutoffs, so a
    bank created with it can also compress new embeddings (PassageBank.add_compress)."""
    import json
    import os

    import torch

    def load(name):
        path = os.path.join(index_path, name)
        try:
            return torch.load(path, map_location="cpu", weights_only=True)
        except TypeError:                                   # a torch without weights_only
            return torch.load(path, map_location="cpu")

    with open(os.path.join(index_path, "metadata.json")) as f:
        meta = json.load(f)
    nbits, dim, n_chunks = int(meta["config"]["nbits"]), int(meta["config"]["dim"]), int(meta["num_chunks"])
    buckets = load("buckets.pt")
    codec = PlaidCodec(load("centroids.pt"), buckets[1], nbits, bucket_cutoffs=buckets[0])
    if codec.dim != dim:
        raise ValueError(f"{index_path}: metadata.json says dim {dim}, centroids.pt holds rows of {codec.dim}")

    def chunks():
        first = 0
        for i in range(n_chunks):
            with open(os.path.join(index_path, f"doclens.{i}.json")) as f:
                doclens = [int(x) for x in json.load(f)]
            codes = load(f"{i}.codes.pt").to(torch.int32).reshape(-1).contiguous()
            res = load(f"{i}.residuals.pt").to(torch.uint8).reshape(codes.numel(), codec.residual_bytes).contiguous()
            if sum(doclens) != codes.numel():
                raise ValueError(f"{index_path}: chunk {i} holds {codes.numel()} rows, its doclens sum to {sum(doclens)}")
            yield first, codes, res, doclens
            first += len(doclens)
    return codec, chunks()


def write_ivf(path: str, ivf) -> str:
    """Write `ivf` = (pids int32 [postings], lengths int64 [n_centroids]) as `path`/ivf.pid.pt, torch.save((ivf, ivf_lengths)) as the
    reference's indexer does (optimize_ivf, colbert/indexing/utils.py:8-48).  Returns the file's path."""
    import os

    import torch
    pids, lengths = ivf
    pids = torch.as_tensor(pids).detach().to(device="cpu", dtype=torch.int32).reshape(-1).contiguous()
    lengths = torch.as_tensor(lengths).detach().to(device="cpu", dtype=torch.int64).reshape(-1).contiguous()
    if int(lengths.sum()) != pids.numel() or (lengths.numel() and int(lengths.min()) < 0):
        raise ValueError(f"write_ivf: {pids.numel()} pids for lists of {int(lengths.sum())} entries in all")
    os.makedirs(path, exist_ok=True)
    out = os.path.join(path, "ivf.pid.pt")
    torch.save((pids, lengths), out)
    return out


def write_plaid_index(index_path: str, codec: "PlaidCodec", chunks, *, ivf=None, config: Optional[dict] = None, passage_ids=None) -> dict:
    """Write a ColBERTv2 / PLAID index directory: what the reference's indexer writes and what its loader reads
    (third_party/ColBERT/colbert/indexing/index_saver.py:79-90, collection_indexer.py:366-449, search/index_loader.py,
    indexing/codecs/residual_embeddings.py:26-95), and what read_plaid_index reads.  torch and json only; nothing of colbert is
    imported.  `chunks` yields (codes int32 [R_i], residuals uint8 [R_i, D * nbits / 8], doclens) per chunk, passages in index order.
    Written: per chunk i `{i}.codes.pt`, `{i}.residuals.pt`, `doclens.{i}.json` (a list of ints) and `{i}.metadata.json`
    ({"passage_offset", "num_passages", "num_embeddings", "embedding_offset"}); the codec's three files (PlaidCodec.save);
    `metadata.json` = {"config": {"dim", "nbits", **config}, "num_chunks", "num_partitions" (the centroid count), "num_embeddings",
    "avg_doclen"}; `ivf.pid.pt` (write_ivf) when `ivf` = (pids, lengths) is given; `passage_ids.json` when `passage_ids` is given and
    every id is an int or a str (anything else does not survive json: the file is left out).  No plan.json: only a resumed indexing
    run reads it.  Returns metadata.json's dict.
    ValueError, before anything is written: a codec without cutoffs (PlaidCodec.save's).  ValueError at the chunk it concerns: doclens
    that do not sum to the chunk's rows or hold a value below 1, residuals that are not [R_i, the codec's residual_bytes], an empty
    chunk; no chunk at all; `passage_ids` of another count than the passages."""
    import json
    import os

    import torch
    if not isinstance(codec, PlaidCodec):
        raise TypeError(f"codec must be a PlaidCodec, got {type(codec).__name__}")
    if codec.bucket_cutoffs is None:
        raise ValueError("save needs the codec's bucket_cutoffs: buckets.pt holds (cutoffs, weights)")
    os.makedirs(index_path, exist_ok=True)
    codec.save(index_path)
    n_chunks = passages = embeddings = 0
    for codes, res, doclens in chunks:
        i = n_chunks
        codes = torch.as_tensor(codes).detach().to(device="cpu", dtype=torch.int32).reshape(-1).contiguous()
        res = torch.as_tensor(res).detach().to(device="cpu")
        doclens = [int(x) for x in doclens]
        R = int(codes.numel())
        if not doclens or min(doclens) < 1 or sum(doclens) != R:
            raise ValueError(f"write_plaid_index: chunk {i} holds {R} rows, its {len(doclens)} doclens (each at least 1) sum to {sum(doclens)}")
        if res.dtype != torch.uint8 or tuple(res.shape) != (R, codec.residual_bytes):
            raise ValueError(f"write_plaid_index: chunk {i}: residuals must be uint8 [{R}, {codec.residual_bytes}], got {res.dtype} "
                             f"{tuple(res.shape)}")
        torch.save(codes, os.path.join(index_path, f"{i}.codes.pt"))
        torch.save(res.contiguous(), os.path.join(index_path, f"{i}.residuals.pt"))
        with open(os.path.join(index_path, f"doclens.{i}.json"), "w") as f:
            json.dump(doclens, f)
        with open(os.path.join(index_path, f"{i}.metadata.json"), "w") as f:
            f.write(json.dumps({"passage_offset": passages, "num_passages": len(doclens), "num_embeddings": R,
                                "embedding_offset": embeddings}, indent=4) + "\n")
        n_chunks, passages, embeddings = n_chunks + 1, passages + len(doclens), embeddings + R
    if n_chunks == 0:
        raise ValueError("write_plaid_index: no chunk")
    if passage_ids is not None:
        ids = list(passage_ids)
        if len(ids) != passages:
            raise ValueError(f"write_plaid_index: {len(ids)} passage ids for {passages} passages")
        if all(isinstance(x, (int, str)) and not isinstance(x, bool) for x in ids):
            with open(os.path.join(index_path, "passage_ids.json"), "w") as f:
                json.dump(ids, f)
    if ivf is not None:
        write_ivf(index_path, ivf)
    meta = {"config": {"dim": codec.dim, "nbits": codec.nbits, **(config or {})}, "num_chunks": n_chunks,
            "num_partitions": codec.n_centroids, "num_embeddings": embeddings, "avg_doclen": embeddings / passages}
    with open(os.path.join(index_path, "metadata.json"), "w") as f:
        f.write(json.dumps(meta, indent=4) + "\n")
    return meta


class PassageBank:
    """A device store of passage token embeddings under the caller's ids (`add`, `remove`): fp16 rows, or with a `codec` (PlaidCodec)
    the residual codes of a ColBERTv2 / PLAID index, decoded on the device in every forward; one mask byte per row either way.
    With `centroids` (no codec): fp16 rows and a centroid code per row beside them (`set_centroids`).
    Created by RerankEngine.create_bank; usable by every interaction engine of the same device and li_dim."""

    generation = 0                           # incremented by `remove` and by `clear`: dense indices from before (a BankFilter's) are stale

    def __init__(self, engine, capacity_rows: int, max_passages: int, codec: Optional[PlaidCodec] = None, centroids=None):
        from . import _lib as L
        if codec is not None and centroids is not None:
            raise ValueError("give a codec (a compressed bank) or centroids (an fp16 bank with a centroid table), not both")
        self._L, self.lib = L, engine.lib
        self.device, self.li_dim = engine.device, int(engine.arch["li_dim"])
        self.table = BankTable()
        self.padded_len = 0                  # the longest Lc (compressed: passage) an add has seen, a high-water mark that `remove`
                                             # and `clear` never lower: a forward's default padded length
        self.codec = codec
        self._centroids = None               # an fp16 bank's centroid table (set_centroids), host fp16 [C, D]
        h = C.c_void_p()
        if codec is None:
            L.check(self.lib.rr_bank_create(engine.h, int(capacity_rows), int(max_passages), C.byref(h)), engine.h, "rr_bank_create")
        else:
            if not isinstance(codec, PlaidCodec):
                raise TypeError(f"codec must be a PlaidCodec, got {type(codec).__name__}")
            if codec.dim != self.li_dim:
                raise ValueError(f"the codec's rows hold {codec.dim} values, the engine's li_dim is {self.li_dim}")
            L.check(self.lib.rr_bank_create_plaid(engine.h, int(capacity_rows), int(max_passages), codec.nbits, codec.n_centroids,
                                                  codec.centroids.data_ptr(), codec.bucket_weights.data_ptr(), C.byref(h)),
                    engine.h, "rr_bank_create_plaid")
        self.h = h
        if codec is not None and codec.bucket_cutoffs is not None:
            self._check(self.lib.rr_bank_set_plaid_cutoffs(h, codec.bucket_cutoffs.data_ptr()), "rr_bank_set_plaid_cutoffs",
                        bad_shape=ValueError)
        if centroids is not None:
            self.set_centroids(centroids)

    @property
    def centroids(self):
        """The centroid table the bank's codes index, host fp16 [C, D]: the codec's of a compressed bank, the one `set_centroids`
        gave an fp16 bank; None for an fp16 bank without one."""
        return self.codec.centroids if self.codec is not None else getattr(self, "_centroids", None)

    @property
    def n_centroids(self) -> int:
        """The rows of `centroids`; 0 for an fp16 bank without a table (which the pruned searches and the inverted file refuse)."""
        c = self.centroids
        return 0 if c is None else int(c.shape[0])

    def set_centroids(self, centroids) -> None:
        """Give an fp16 bank a centroid table (rr_bank_set_centroids): `centroids` [C, li_dim], 1 <= C <= 262144 (kept as fp16;
        PlaidCodec.train(...).centroids fits).  Every row the bank holds is assigned its code on the device now (the code of the
        compressed row, include/rerank_mi355.h: for equal rows the codes `add_compress` writes), and every later `add` assigns
        the codes of its rows behind the ingest.  Called again it replaces the table, assigns every row anew and drops the
        inverted file.  A load-time call: it allocates and synchronises the current stream.  A compressed bank and an li_dim
        that is no multiple of 16 raise NotImplementedError, a table of another shape or size ValueError, a failed allocation
        MemoryError; the bank is unchanged then."""
        import torch
        if self.codec is not None:
            raise NotImplementedError("set_centroids on a compressed bank: its codes belong to its residuals (the codec holds the table)")
        cen = torch.as_tensor(centroids).detach().to(device="cpu", dtype=torch.float16).contiguous()
        if cen.dim() != 2 or cen.shape[1] != self.li_dim:
            raise ValueError(f"centroids must be [C, {self.li_dim}], got {tuple(cen.shape)}")
        self._check(self.lib.rr_bank_set_centroids(self.h, cen.data_ptr(), int(cen.shape[0]), self._stream()), "rr_bank_set_centroids",
                    bad_shape=ValueError)
        self._centroids = cen

    def codes(self, passage_id):
        """The centroid codes of one passage on the host, int32 [len] (rr_bank_read_codes; synchronises the current stream), of a
        compressed bank or an fp16 bank with a centroid table; NotImplementedError for an fp16 bank without one."""
        import torch
        if not self.n_centroids:
            raise NotImplementedError("codes on an fp16 bank without a centroid table: it holds no codes (set_centroids)")
        return self._read("rr_bank_read_codes", passage_id, ((), torch.int32))[0]

    def __del__(self):
        self.close()

    def close(self) -> None:
        h = getattr(self, "h", None)
        if h:
            try:
                self.lib.rr_bank_destroy(h)
            except Exception:
                pass
            self.h = None

    def __len__(self) -> int:
        return len(self.table)

    def __contains__(self, passage_id) -> bool:
        return passage_id in self.table

    def _check(self, rc: int, what: str, bad_shape=AssertionError) -> None:
        if rc >= 0:
            return
        L = self._L
        exc = bad_shape if rc == L.RR_ERR_BAD_SHAPE else L._EXC.get(rc, RuntimeError)
        raise exc(f"{what}: {self.lib.rr_status_string(rc).decode()}: {self.lib.rr_bank_last_error(self.h).decode()}")

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def info(self) -> dict:
        """rr_bank_info: passages held, rows used, row capacity.  A compressed bank adds `nbits` and `bytes_per_row` (format());
        an fp16 bank's dict is those three keys alone."""
        p, r, c = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        self._check(self.lib.rr_bank_info(self.h, C.byref(p), C.byref(r), C.byref(c)), "rr_bank_info")
        out = dict(passages=int(p.value), rows_used=int(r.value), capacity_rows=int(c.value))
        if self.codec is not None:
            f = self.format()
            out.update(nbits=f["nbits"], bytes_per_row=f["bytes_per_row"])
        return out

    def format(self) -> dict:
        """rr_bank_format, either kind of bank: nbits (0: an fp16 bank), the codec's centroids (0) and the device bytes one row
        takes, mask byte included."""
        nb, nc, bpr = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        self._check(self.lib.rr_bank_format(self.h, C.byref(nb), C.byref(nc), C.byref(bpr)), "rr_bank_format")
        return dict(nbits=int(nb.value), n_centroids=int(nc.value), bytes_per_row=int(bpr.value))

    def add(self, passage_ids: Sequence, context_li, context_mask, lengths: Optional[Sequence[int]] = None) -> int:
        """Append the passages `passage_ids` from the padded tensors a retriever produces: `context_li` [n, Lc, D] (host or
        device; float32 or float16, anything else goes through float32) and the 0/1 `context_mask` [n, Lc].  Values are kept as
        `context_li.half()`, the mask as (mask != 0), positions unchanged.  `lengths`: the rows each passage keeps (1 + index of
        its last unmasked token, at least 1) as the host knows them; without it they are derived on the device and copied once.
        Returns the first of the n dense indices.  An id added twice raises ValueError, a length outside [1, Lc] ValueError,
        rows or passage slots that do not suffice MemoryError; the bank is unchanged then."""
        if self.codec is not None:
            raise NotImplementedError("a compressed bank takes residual codes (add_compressed): nothing here compresses embeddings")
        return self._add_padded("rr_bank_add", passage_ids, context_li, context_mask, lengths)

    def add_compress(self, passage_ids: Sequence, context_li, context_mask, lengths: Optional[Sequence[int]] = None,
                     extend_ivf: bool = False) -> int:
        """`add` for a compressed bank (rr_bank_add_compress): the padded tensors a retriever produces are compressed on the
        device against the codec's centroids and cutoffs and appended as codes and residual bytes — the compressed row of
        include/rerank_mi355.h, what the reference's indexer computes from `context_li.half()`.  Arguments, return value and
        errors as `add`; an fp16 bank, a codec without cutoffs and an li_dim that is no multiple of 16 raise NotImplementedError.
        `extend_ivf`: after a successful add, take the inverted file over the new passages (extend_ivf(): a load-time call)."""
        if self.codec is None:
            raise NotImplementedError("add_compress on an fp16 bank: it keeps embeddings as they are (add)")
        first = self._add_padded("rr_bank_add_compress", passage_ids, context_li, context_mask, lengths)
        if extend_ivf:
            self.extend_ivf()
        return first

    def _add_padded(self, entry_name: str, passage_ids, context_li, context_mask, lengths) -> int:
        """`add` and `add_compress` behind their own refusals: the padded tensors brought to the device as the entry point
        `entry_name` (rr_bank_add / rr_bank_add_compress) takes them, the call, the ids appended to the table."""
        import numpy as np
        import torch
        from .pair_inputs import pair_lengths
        L = self._L
        ids = list(passage_ids)
        n = len(ids)
        if context_li.dim() != 3 or context_li.shape[0] != n or context_li.shape[2] != self.li_dim:
            raise ValueError(f"context_li must be [{n}, Lc, {self.li_dim}], got {tuple(context_li.shape)}")
        Lc = int(context_li.shape[1])
        self.table.check_new(ids)
        dt = context_li.dtype if context_li.dtype in (torch.float32, torch.float16) else torch.float32
        li = context_li.to(device=self.device, dtype=dt).contiguous()
        cm = context_mask.reshape(n, Lc).to(device=self.device, dtype=torch.float32).contiguous()
        if lengths is None:
            lengths = pair_lengths(cm).cpu().numpy()
        ln = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1), dtype=np.int32)
        if ln.size != n:
            raise ValueError(f"{ln.size} lengths for {n} passages")
        first = C.c_int32(-1)
        self._check(getattr(self.lib, entry_name)(self.h, L.ptr(li), L.RR_F16 if dt == torch.float16 else L.RR_F32, L.ptr(cm), ln.ctypes.data,
                                                  n, Lc, C.byref(first), self._stream()), entry_name, bad_shape=ValueError)
        self.table.append(ids, ln.tolist(), int(first.value))
        self.padded_len = max(self.padded_len, Lc)
        return int(first.value)

    def add_compressed(self, passage_ids: Sequence, codes, residuals, doclens: Sequence[int], mask=None, extend_ivf: bool = False) -> int:
        """Append the passages `passage_ids` of a compressed bank from an index's own arrays (rr_bank_add_plaid): `codes` [R]
        integer centroid codes and `residuals` [R, D * nbits / 8] uint8, the rows of the passages one after the other, R =
        sum(doclens); `doclens` the rows of each passage; `mask` [R] (non-zero = a token that counts) or None = all ones — the
        ColBERT indexer has dropped the skiplist tokens already.  Host tensors / arrays (a device tensor is copied back).  A
        load-time call: it synchronises the current stream.  Returns the first of the dense indices.  An id added twice, a code
        outside the codec's centroids, a length below 1 or arrays that do not fit the lengths raise ValueError, rows or passage
        slots that do not suffice MemoryError, an fp16 bank NotImplementedError; the bank is unchanged then.
        `extend_ivf`: after a successful add, take the inverted file over the new passages (extend_ivf())."""
        import numpy as np
        import torch

        def host(x, dtype):
            if torch.is_tensor(x):
                x = x.detach().cpu().numpy()
            return np.ascontiguousarray(np.asarray(x), dtype=dtype)
        if self.codec is None:
            raise NotImplementedError("add_compressed on an fp16 bank: create the bank with a codec (create_bank(..., codec=PlaidCodec(...)))")
        ids = list(passage_ids)
        n = len(ids)
        ln = host(doclens, np.int64).reshape(-1)
        if ln.size != n or n == 0:
            raise ValueError(f"{ln.size} doclens for {n} passages")
        if int(ln.min()) < 1 or int(ln.max()) > 2 ** 31 - 1:
            raise ValueError(f"a passage of {int(ln.min() if ln.min() < 1 else ln.max())} rows")
        R = int(ln.sum())
        cd = host(codes, np.int64).reshape(-1)
        if cd.size != R:
            raise ValueError(f"{cd.size} codes for {R} rows (sum of doclens)")
        if cd.size and (int(cd.min()) < 0 or int(cd.max()) >= self.codec.n_centroids):
            raise ValueError(f"centroid codes span [{int(cd.min())}, {int(cd.max())}], the codec holds {self.codec.n_centroids} centroids")
        rs = host(residuals, np.uint8)
        if rs.shape != (R, self.codec.residual_bytes):
            raise ValueError(f"residuals must be [{R}, {self.codec.residual_bytes}] uint8, got {rs.shape}")
        mk = None
        if mask is not None:
            mk = (host(mask, np.float32).reshape(-1) != 0).astype(np.uint8)
            if mk.size != R:
                raise ValueError(f"{mk.size} mask values for {R} rows")
        self.table.check_new(ids)
        cd32, ln32 = cd.astype(np.int32), ln.astype(np.int32)
        first = C.c_int32(-1)
        self._check(self.lib.rr_bank_add_plaid(self.h, cd32.ctypes.data, rs.ctypes.data, mk.ctypes.data if mk is not None else None,
                                               ln32.ctypes.data, n, C.byref(first), self._stream()), "rr_bank_add_plaid",
                    bad_shape=ValueError)
        self.table.append(ids, ln32.tolist(), int(first.value))
        self.padded_len = max(self.padded_len, int(ln.max()))
        if extend_ivf:
            self.extend_ivf()
        return int(first.value)

    def load_plaid_index(self, index_path: str, passage_ids: Optional[Sequence] = None, ivf: bool = False, extend_ivf: bool = False) -> int:
        """Fill a compressed bank from a ColBERTv2 / PLAID index directory (read_plaid_index), chunk by chunk through
        add_compressed.  The bank's codec must hold the index's tables (create the bank with the codec read_plaid_index returns).
        `passage_ids`: the caller's id of passage number i of the index at position i; default: the ids of the directory's
        passage_ids.json when it has one (save_plaid_index writes it), else the passage numbers themselves.
        `ivf`: also load the directory's ivf.pid.pt (load_ivf, verified against the bank) instead of leaving the inverted file to a
        build_ivf; the file numbers passages as the index does, so the bank must be empty before the call (ValueError).
        `extend_ivf`: after the last chunk, take the bank's inverted file over the passages added (extend_ivf(): once, not per chunk;
        a bank that held passages and a file before the load keeps that file's lists and gains the new entries).
        Returns the number of passages added."""
        import json
        import os

        import torch
        codec, chunks = read_plaid_index(index_path)
        mine = self.codec
        if mine is None:
            raise NotImplementedError("load_plaid_index on an fp16 bank: create the bank with the index's codec")
        if (mine.nbits, mine.dim) != (codec.nbits, codec.dim) or not torch.equal(mine.centroids, codec.centroids) \
                or not torch.equal(mine.bucket_weights, codec.bucket_weights):
            raise ValueError(f"{index_path}: the index's codec (nbits {codec.nbits}, dim {codec.dim}, {codec.n_centroids} centroids) is "
                             "not the bank's")
        if ivf and len(self.table):
            raise ValueError(f"load_plaid_index(ivf=True): the bank holds {len(self.table)} passages already; ivf.pid.pt numbers "
                             "passages from 0 (build_ivf after the load instead)")
        ids_file = os.path.join(index_path, "passage_ids.json")
        if passage_ids is None and os.path.exists(ids_file):
            with open(ids_file) as f:
                passage_ids = json.load(f)
        added = 0
        for first, codes, res, doclens in chunks:
            ids = list(range(first, first + len(doclens))) if passage_ids is None else list(passage_ids[first:first + len(doclens)])
            if len(ids) != len(doclens):
                raise ValueError(f"{len(passage_ids)} passage ids for an index of more than {first + len(ids)} passages")
            self.add_compressed(ids, codes, res, doclens)
            added += len(doclens)
        if ivf:
            self.load_ivf(index_path)
        if extend_ivf:
            self.extend_ivf()
        return added

    def export_compressed(self, first: int = 0, count: Optional[int] = None):
        """The passages first .. first + count - 1 (dense indices; None: through the last) as an index stores them, on the device
        (rr_bank_export_plaid): (codes int32 [R], residuals uint8 [R, D * nbits / 8], doclens list): the UNMASKED rows of every
        passage back to back, doclens[i] of passage first + i (0 for a passage with no unmasked row).  Masked rows do not travel:
        a bank filled from the result scores and searches like this one, but it is no snapshot of the masked rows.  One sizing
        call, an allocation of exactly R rows, one export call; it synchronises the current stream.  An fp16 bank raises
        NotImplementedError, a range outside the bank ValueError."""
        first, n = int(first), (len(self.table) - int(first) if count is None else int(count))
        doclens, R = self._export_sizes(first, n)
        codes, res = self._export_rows(first, n, R)
        return codes, res, doclens

    def _export_sizes(self, first: int, n: int):
        """The sizing call of rr_bank_export_plaid: (doclens list, R)."""
        import numpy as np
        if self.codec is None and self.n_centroids:
            raise NotImplementedError("export_compressed on an fp16 bank with a centroid table: it holds codes but no residuals; "
                                      "add_compress into a compressed bank (create_bank(codec=...)) writes them")
        if self.codec is None:
            raise NotImplementedError("export_compressed on an fp16 bank: it holds no codes")
        doclens = np.empty(max(n, 1), dtype=np.int32)
        R = C.c_int64(-1)
        self._check(self.lib.rr_bank_export_plaid(self.h, first, n, doclens.ctypes.data, None, None, 0, C.byref(R), self._stream()),
                    "rr_bank_export_plaid", bad_shape=ValueError)
        return doclens[:n].tolist(), int(R.value)

    def _export_rows(self, first: int, n: int, R: int):
        """The export call of rr_bank_export_plaid into tensors of exactly R rows (from _export_sizes): (codes, residuals)."""
        import numpy as np
        import torch
        codes = torch.empty(R, device=self.device, dtype=torch.int32)
        res = torch.empty((R, self.codec.residual_bytes), device=self.device, dtype=torch.uint8)
        if R:
            doclens = np.empty(n, dtype=np.int32)
            got = C.c_int64(-1)
            self._check(self.lib.rr_bank_export_plaid(self.h, first, n, doclens.ctypes.data, codes.data_ptr(), res.data_ptr(), R, C.byref(got),
                                                      self._stream()), "rr_bank_export_plaid", bad_shape=ValueError)
            assert int(got.value) == R, f"the export moved {int(got.value)} rows, the sizing call counted {R}"
        return codes, res

    def save_plaid_index(self, index_path: str, chunk_passages: int = 25000, ivf: bool = True, config: Optional[dict] = None) -> dict:
        """Write the bank as a ColBERTv2 / PLAID index directory (write_plaid_index) that read_plaid_index / load_plaid_index and the
        reference's loader open: the bank walked in chunks of `chunk_passages` passages (the reference's chunk size:
        collection_indexer.py's min(25000, ...)), each exported on the device (rr_bank_export_plaid) and copied to the host; the
        codec; metadata.json ({"dim", "nbits", **config} as its config); the passage ids as passage_ids.json when they are ints or
        strs; with `ivf` the bank's inverted file as ivf.pid.pt, extended first (extend_ivf: the bytes of a fresh build) when the bank
        has none or it covers fewer passages than the bank holds.  The index holds the unmasked rows only, as the reference's indexer would have stored the passages.
        Every sizing call runs before the first file is written: a bank with a passage that has no unmasked row cannot be
        represented (an index's doclens are at least 1) and raises ValueError naming up to eight ids, with nothing written.  An
        fp16 bank raises NotImplementedError, a codec without cutoffs PlaidCodec.save's ValueError, an empty bank ValueError.
        Returns metadata.json's dict."""
        if self.codec is None and self.n_centroids:
            raise NotImplementedError("save_plaid_index on an fp16 bank with a centroid table: an index stores residuals, which it does "
                                      "not hold; add_compress into a compressed bank (create_bank(codec=...)) and save that one")
        if self.codec is None:
            raise NotImplementedError("save_plaid_index on an fp16 bank: it holds no codes")
        if self.codec.bucket_cutoffs is None:
            raise ValueError("save needs the codec's bucket_cutoffs: buckets.pt holds (cutoffs, weights)")
        P, step = len(self.table), int(chunk_passages)
        if P < 1 or step < 1:
            raise ValueError(f"save_plaid_index: {P} passages in chunks of {step}")
        plan, empty = [], []
        for first in range(0, P, step):
            n = min(step, P - first)
            doclens, R = self._export_sizes(first, n)
            empty += [self.table.ids[first + i] for i, d in enumerate(doclens) if d < 1]
            plan.append((first, n, doclens, R))
        if empty:
            raise ValueError(f"save_plaid_index: {len(empty)} passages have no unmasked row, which an index cannot hold (doclens are at "
                             f"least 1): {', '.join(repr(x) for x in empty[:8])}{' ...' if len(empty) > 8 else ''}")
        pair = None
        if ivf:
            if self.ivf_info()["passages_covered"] < P:
                self.extend_ivf()
            pair = self.ivf()

        def chunks():
            for first, n, doclens, R in plan:
                codes, res = self._export_rows(first, n, R)
                yield codes.cpu(), res.cpu(), doclens
        return write_plaid_index(index_path, self.codec, chunks(), ivf=pair, config=config, passage_ids=self.table.ids)

    def lookup(self, passage_ids: Sequence):
        """(indices, lengths) of `passage_ids`; KeyError names an id the bank does not hold."""
        return self.table.lookup(passage_ids)

    def read(self, passage_id):
        """One passage back on the host (rr_bank_read; synchronises the current stream): (rows [len, D] float16, mask [len]
        uint8).  A compressed bank returns the decoded rows: what its forwards use."""
        import torch
        return self._read("rr_bank_read", passage_id, ((self.li_dim,), torch.float16), ((), torch.uint8))

    def read_compressed(self, passage_id):
        """One passage of a compressed bank back on the host as it is stored (rr_bank_read_plaid; synchronises the current
        stream): (codes int32 [len], residuals uint8 [len, D * nbits / 8], mask uint8 [len])."""
        import torch
        if self.codec is None:
            raise NotImplementedError("read_compressed on an fp16 bank: it holds no codes (read)")
        return self._read("rr_bank_read_plaid", passage_id, ((), torch.int32), ((self.codec.residual_bytes,), torch.uint8), ((), torch.uint8))

    def _read(self, entry_name: str, passage_id, *outputs):
        """`read` and `read_compressed`: host tensors [len, *shape] of `outputs` = (shape, dtype), ..., filled by `entry_name`."""
        import torch
        idx, lens = self.table.lookup([passage_id])
        n = int(lens[0])
        outs = tuple(torch.empty((n, *shape), dtype=dt) for shape, dt in outputs)
        got = getattr(self.lib, entry_name)(self.h, int(idx[0]), *(o.data_ptr() for o in outs), n, self._stream())
        self._check(got, entry_name)
        assert got == n, f"the bank holds {got} rows for passage {passage_id!r}, the table {n}"
        return outs

    def maxsim(self, engine, query_li, passage_ids, **kw):
        """The retriever's MaxSim [n_pairs] of the pairs (query, passage id) from this bank: engine.bank_li_scores(...)["maxsim"]."""
        return engine.bank_li_scores(self, query_li, passage_ids, **kw)["maxsim"]

    def filter_lists(self, allowed=None, excluded=None):
        """The host half of `filter`: (indices int32 [total], offsets int64 [rows + 1], exclude) as rr_bank_filter_fill takes them.
        Exactly one of `allowed` / `excluded` is given (ValueError).  A flat sequence of passage ids is one row; a sequence whose
        elements are all lists (or arrays) is one row per query (a tuple is an id, never a row).  Ids go through the table: a
        KeyError names an id the bank does not hold."""
        import numpy as np
        if (allowed is None) == (excluded is None):
            raise ValueError("filter: give exactly one of allowed / excluded")
        given = allowed if allowed is not None else excluded
        given = given.tolist() if hasattr(given, "tolist") else list(given)
        nested = len(given) > 0 and all(isinstance(r, list) or (hasattr(r, "tolist") and getattr(r, "ndim", 0) > 0) for r in given)
        rows = [r.tolist() if hasattr(r, "tolist") else list(r) for r in given] if nested else [given]
        offsets = np.zeros(len(rows) + 1, dtype=np.int64)
        for i, r in enumerate(rows):
            offsets[i + 1] = offsets[i] + len(r)
        flat = [pid for r in rows for pid in r]
        indices = self.table.lookup(flat)[0].astype(np.int32) if flat else np.zeros(0, dtype=np.int32)
        return np.ascontiguousarray(indices), offsets, excluded is not None

    def filter(self, allowed=None, excluded=None) -> BankFilter:
        """A candidate filter for `search` over the passages the bank holds now: the passages `allowed`, or every passage but
        those `excluded` (exactly one of the two; passage ids, as filter_lists takes them: a flat sequence is one set for every
        query, a list of lists one set per query).  The bitmap is written on the device (rr_bank_filter_fill) on the current
        stream.  Build it again after an add: a filter knows the passage count it was built for."""
        import torch
        indices, offsets, exclude = self.filter_lists(allowed, excluded)
        passages, rows = len(self.table), len(offsets) - 1
        if passages < 1:
            raise ValueError("filter: the bank holds no passage")
        ld = (passages + 31) // 32
        bits = torch.empty((rows, ld), device=self.device, dtype=torch.int32)
        self._check(self.lib.rr_bank_filter_fill(self.h, indices.ctypes.data if indices.size else None, offsets.ctypes.data, rows, int(exclude),
                                                 bits.data_ptr(), ld, self._stream()), "rr_bank_filter_fill", bad_shape=ValueError)
        return BankFilter(bits, rows, passages, self.generation)

    def search(self, engine, query_li, k: int, first: int = 0, count: Optional[int] = None, plaid: Optional[PlaidSearch] = None,
               filter: Optional[BankFilter] = None, sparse: bool = False, fast: Optional[F16Search] = None):
        """The k best passages per query by the retriever's MaxSim, every passage of the bank scored (engine.bank_search;
        `first` / `count`: a range of dense indices).  Returns (passage_ids, scores): passage_ids[q] the ids of query q best
        first, scores float32 [n_queries, k] on the device.  Copies the indices to the host (synchronises).
        With `plaid` (a PlaidSearch; compressed banks and fp16 banks with a centroid table) the pruned search runs instead (engine.bank_search_plaid): passage_ids[q]
        has its true length, at most k (a query may find fewer candidates, or none), and scores holds -inf behind it.  A
        PlaidSearch with ivf=True takes the candidates from the inverted file (build_ivf first): the same result.
        With `filter` (a BankFilter, `filter`) only the passages it allows compete, in the exact and in the pruned search
        (engine.bank_search_filtered / bank_search_plaid_filtered / bank_search_plaid_ivf_filtered): passage_ids[q] has its true
        length on the exact path too.  A filter built for fewer passages than the range ends at raises ValueError.
        `sparse` (with `filter`, exact search only; ValueError otherwise): the list-driven form of the filtered exact search
        (engine.bank_search_filtered_sparse): the same result, with work that follows the allowed passages, not the range.
        `fast` (an F16Search; with `plaid`, `filter` or `sparse`: ValueError): the exhaustive search whose first pass runs
        on the fp16 matrix core (engine.bank_search_f16; on a compressed bank engine.bank_search_f16_plaid).  Returns its dict instead, on the device, nothing copied: {"indices" int32
        [n_queries, k] dense indices, "scores" float32 [n_queries, k] exact, "certified" int32 [n_queries]}."""
        _fast_check("search", fast, plaid, filter, sparse)
        _sparse_check("search", sparse, filter, plaid)
        if fast is not None:
            return _f16_entry(engine, self)(self, query_li, k, fast.ndocs, fast.slack, first=first, count=count)
        ids = self.table.ids
        if filter is not None:
            if getattr(filter, "generation", self.generation) != self.generation:
                raise ValueError(f"search: the filter was built at generation {filter.generation} of the bank, a removal has renumbered "
                                 f"its passages since (generation {self.generation}): build it again (PassageBank.filter)")
            end = len(self.table) if count is None else int(first) + int(count)
            if filter.passages < end:
                raise ValueError(f"search: the filter was built for {filter.passages} passages, the range ends at {end}: build it again "
                                 "(PassageBank.filter)")
            if plaid is None:
                entry = engine.bank_search_filtered_sparse if sparse else engine.bank_search_filtered
                r = entry(self, query_li, k, filter, first=first, count=count)
            else:
                entry = engine.bank_search_plaid_ivf_filtered if getattr(plaid, "ivf", False) else engine.bank_search_plaid_filtered
                r = entry(self, query_li, k, filter, ncells=plaid.ncells, centroid_score_threshold=plaid.centroid_score_threshold,
                          ndocs=plaid.ndocs, coarse_tokens=plaid.coarse_tokens, first=first, count=count)
            counts = r["counts"].tolist()
            return [[ids[j] for j in row[:c]] for row, c in zip(r["indices"].tolist(), counts)], r["scores"]
        if plaid is None:
            r = engine.bank_search(self, query_li, k, first=first, count=count)
            return [[ids[j] for j in row] for row in r["indices"].tolist()], r["scores"]
        entry = engine.bank_search_plaid_ivf if getattr(plaid, "ivf", False) else engine.bank_search_plaid
        r = entry(self, query_li, k, ncells=plaid.ncells, centroid_score_threshold=plaid.centroid_score_threshold, ndocs=plaid.ndocs,
                  coarse_tokens=plaid.coarse_tokens, first=first, count=count)
        counts = r["counts"].tolist()
        return [[ids[j] for j in row[:c]] for row, c in zip(r["indices"].tolist(), counts)], r["scores"]

    def build_ivf(self) -> dict:
        """Build, or rebuild, the inverted file over every passage the bank holds now (rr_bank_build_ivf): per centroid the sorted
        unique passages (dense indices) with an unmasked token of that code.  On the device; a load-time call that allocates and
        synchronises the current stream.  Passages added later are not covered until the next build; `clear` drops the file.
        Returns ivf_info().  An fp16 bank raises NotImplementedError, a failed allocation MemoryError with the previous file kept."""
        if not self.n_centroids:
            raise NotImplementedError("build_ivf on an fp16 bank: it holds no centroid codes")
        self._check(self.lib.rr_bank_build_ivf(self.h, self._stream()), "rr_bank_build_ivf", bad_shape=ValueError)
        return self.ivf_info()

    def extend_ivf(self) -> dict:
        """Take the inverted file over the passages added since it was built (rr_bank_extend_ivf): afterwards the bank holds, byte for
        byte, the file build_ivf would build now.  Only the new passages are walked; the old postings are copied to their new places
        and the new entries of every list sorted behind them.  A file that covers every passage is left untouched (nothing is
        allocated or synchronised); without a file the call is build_ivf.  A load-time call otherwise: it allocates the new file
        beside the old one and synchronises the current stream.  tools/bench_bank_ivf_extend.py times it against build_ivf.
        Returns ivf_info().  An fp16 bank raises NotImplementedError, a failed allocation MemoryError with the previous file kept."""
        if not self.n_centroids:
            raise NotImplementedError("extend_ivf on an fp16 bank: it holds no centroid codes")
        self._check(self.lib.rr_bank_extend_ivf(self.h, self._stream()), "rr_bank_extend_ivf", bad_shape=ValueError)
        return self.ivf_info()

    def ivf_info(self) -> dict:
        """rr_bank_ivf_info: passages_covered (0: no inverted file), postings (entries of all lists), longest_list."""
        p, n, m = C.c_int32(0), C.c_int64(0), C.c_int32(0)
        self._check(self.lib.rr_bank_ivf_info(self.h, C.byref(p), C.byref(n), C.byref(m)), "rr_bank_ivf_info")
        return dict(passages_covered=int(p.value), postings=int(n.value), longest_list=int(m.value))

    def ivf(self):
        """The inverted file on the host (rr_bank_ivf_read; synchronises the current stream) as the reference's ivf.pid.pt holds
        it: (pids int32 [postings], lengths int64 [n_centroids]); list c is pids[sum(lengths[:c]) : sum(lengths[:c + 1])], dense
        bank indices in ascending order.  ValueError without a file (build_ivf)."""
        import torch
        info = self.ivf_info()
        if not info["passages_covered"]:
            raise ValueError("ivf: the bank has no inverted file (build_ivf)")
        offsets = torch.empty(self.n_centroids + 1, dtype=torch.int64)
        pids = torch.empty(info["postings"], dtype=torch.int32)
        self._check(self.lib.rr_bank_ivf_read(self.h, offsets.data_ptr(), pids.data_ptr() if pids.numel() else None, self._stream()),
                    "rr_bank_ivf_read")
        return pids, offsets[1:] - offsets[:-1]

    def save_ivf(self, path: str) -> str:
        """Write the inverted file as `path`/ivf.pid.pt, torch.save((ivf, ivf_lengths)) as the reference's indexer does
        (optimize_ivf, colbert/indexing/utils.py:8-48), beside what PlaidCodec.save writes.  The pids are dense bank indices: they
        are the reference's passage numbers when the bank was filled in the index's order.  Returns the file's path."""
        return write_ivf(path, self.ivf())

    def load_ivf(self, path_or_pair, verify: bool = True) -> dict:
        """Take the inverted file from an ivf.pid.pt instead of building it (rr_bank_load_ivf): `path_or_pair` is the file, the
        index directory that holds it, or the pair (pids int32 [postings], lengths [n_centroids]) itself; the lengths are summed
        into offsets here.  The file must cover every passage the bank holds now under its dense indices (an index loaded into an
        empty bank in the index's order).  The library checks it on the host (offsets from 0 that do not decrease, pids inside
        the bank, every list strictly ascending) and, with `verify`, compares it with a fresh build over the bank, which is what
        catches the file of another index; verify=False trusts the caller and costs the upload alone.  ValueError for a file that
        fails a check or the comparison, with the previous file kept; an fp16 bank raises NotImplementedError.  A load-time call:
        it allocates and synchronises the current stream.  Returns ivf_info()."""
        import os

        import torch
        if not self.n_centroids:
            raise NotImplementedError("load_ivf on an fp16 bank: it holds no centroid codes")
        pair = path_or_pair
        if isinstance(pair, (str, os.PathLike)):
            path = os.path.join(pair, "ivf.pid.pt") if os.path.isdir(pair) else os.fspath(pair)
            try:
                pair = torch.load(path, map_location="cpu", weights_only=True)
            except TypeError:                                   # a torch without weights_only
                pair = torch.load(path, map_location="cpu")
        pids, lengths = pair
        pids = torch.as_tensor(pids).detach().to(device="cpu", dtype=torch.int32).reshape(-1).contiguous()
        lengths = torch.as_tensor(lengths).detach().to(device="cpu", dtype=torch.int64).reshape(-1)
        if lengths.numel() != self.n_centroids:
            raise ValueError(f"load_ivf: {lengths.numel()} lists, the codec holds {self.n_centroids} centroids")
        offsets = torch.zeros(lengths.numel() + 1, dtype=torch.int64)
        offsets[1:] = torch.cumsum(lengths, 0)
        if int(offsets[-1]) != pids.numel():
            raise ValueError(f"load_ivf: {pids.numel()} pids for lists of {int(offsets[-1])} entries in all")
        self._check(self.lib.rr_bank_load_ivf(self.h, offsets.data_ptr(), pids.data_ptr() if pids.numel() else None, int(bool(verify)),
                                              self._stream()), "rr_bank_load_ivf", bad_shape=ValueError)
        return self.ivf_info()

    def remove(self, passage_ids: Sequence) -> dict:
        """Remove the passages `passage_ids` and compact the rest on the device (rr_bank_remove): afterwards the bank is what a
        fresh bank filled with the survivors in their order would be, bit for bit; their dense indices are renumbered from 0,
        and the freed rows and passage slots serve later adds (a removed id may be added again).  An inverted file stays, rebuilt
        over the survivors of the passages it covered (passages behind them stay uncovered: extend_ivf).  Returns {"passages": held now, "rows_freed", "new_index": int32 numpy
        array, old dense index -> new, -1 for a removed passage}.  A load-time call: it allocates its staging block and
        synchronises the current stream; work on other streams that reads the bank must have completed.  An id the bank does not
        hold raises KeyError, an id given twice ValueError, a staging block that cannot be allocated MemoryError, each with the
        bank unchanged.  `generation` goes up by one (as `clear` raises it): filters built before (PassageBank.filter) and a
        ShardedBank's refresh() are stale.  If only the rebuild of the inverted file fails, the passages are removed, the file is
        gone (build_ivf) and the library's error is raised.
        `padded_len` stays: it is the high-water mark of the adds (the longest Lc, or compressed passage, an add has seen), not a
        function of the contents, and it is the default padded context length of the bank forwards, whose fusion normalisers run
        over the padded axis.  A bank after a removal and a fresh bank of the survivors can therefore differ in their DEFAULT
        logits; pass `padded_len` to the forward where the two must agree."""
        import numpy as np
        ids = list(passage_ids)
        idx = np.ascontiguousarray(self.table.check_remove(ids), dtype=np.int32)
        held = len(self.table)
        before = self.info()["rows_used"]
        new_index = np.empty(held, dtype=np.int32)
        rc = self.lib.rr_bank_remove(self.h, idx.ctypes.data if idx.size else None, int(idx.size), new_index.ctypes.data if held else None,
                                     self._stream())
        now = self.info()
        if rc < 0 and now["passages"] == held:                   # refused, or failed before anything changed
            self._check(rc, "rr_bank_remove", bad_shape=ValueError)
        if idx.size:
            self.table.remove(idx.tolist())
            self.generation += 1
        self._check(rc, "rr_bank_remove", bad_shape=ValueError)   # the passages went, the inverted file's rebuild failed
        return dict(passages=now["passages"], rows_freed=before - now["rows_used"], new_index=new_index)

    def clear(self) -> None:
        """Forget every passage (rr_bank_clear; the capacity stays; the inverted file goes).  Forwards that read the bank must have
        completed.  `generation` goes up by one, as after `remove`: a refill puts other passages under the old dense indices, so
        filters built before (PassageBank.filter) and a ShardedBank's refresh() are stale.  `padded_len` stays, as after `remove`:
        the high-water mark of the adds, not a function of the contents."""
        self._check(self.lib.rr_bank_clear(self.h), "rr_bank_clear")
        self.table.clear()
        self.generation += 1


def _sparse_check(name: str, sparse: bool, filter, plaid) -> None:
    """`sparse` names the list-driven form of the FILTERED EXACT search: without a filter, or with `plaid`, there is none."""
    if sparse and filter is None:
        raise ValueError(f"{name}: sparse=True needs a filter (the list-driven form walks the passages a filter allows)")
    if sparse and plaid is not None:
        raise ValueError(f"{name}: sparse=True with plaid (the pruned searches touch candidates only already)")


def search_bank_part(engine, bank, query_li, k: int, plaid: Optional[PlaidSearch] = None, filter: Optional[BankFilter] = None,
                     sparse: bool = False, fast: Optional[F16Search] = None) -> dict:
    """One part's list for RerankEngine.bank_merge_topk: the search of `bank` (the exact one, or with `plaid` / `filter` what
    PassageBank.search runs for them) with k_local = min(k, len(bank)), as {"indices": int32 [n_queries, k] dense indices of
    THIS bank, "scores": float32 [n_queries, k], "counts": int32 [n_queries]} on the device.  Behind k_local the rows hold -1 /
    -inf; an exact search, which returns no counts, gets k_local as its count; an empty bank contributes count 0 and no search
    call.  `sparse`: as PassageBank.search takes it.  `fast` (an F16Search): engine.bank_search_f16 (a compressed bank: bank_search_f16_plaid) with ndocs = max(fast.ndocs,
    k_local) capped at 1024, and one more entry, "certified" int32 [n_queries] (an empty bank: all 1)."""
    import torch
    _fast_check("search_bank_part", fast, plaid, filter, sparse)
    _sparse_check("search_bank_part", sparse, filter, plaid)
    nq, k, dev = int(query_li.shape[0]), int(k), engine.device
    k_local = min(k, len(bank))
    out = dict(indices=torch.full((nq, k), -1, device=dev, dtype=torch.int32),
               scores=torch.full((nq, k), float("-inf"), device=dev, dtype=torch.float32),
               counts=torch.zeros((nq,), device=dev, dtype=torch.int32))
    if fast is not None:
        out["certified"] = torch.ones((nq,), device=dev, dtype=torch.int32)
    if k_local < 1:
        return out
    if fast is not None:
        r = _f16_entry(engine, bank)(bank, query_li, k_local, min(max(fast.ndocs, k_local), 1024), fast.slack)
        out["certified"] = r["certified"]
    elif plaid is not None:
        kw = dict(ncells=plaid.ncells, centroid_score_threshold=plaid.centroid_score_threshold, ndocs=plaid.ndocs,
                  coarse_tokens=plaid.coarse_tokens)
        ivf = getattr(plaid, "ivf", False)
        if filter is None:
            r = (engine.bank_search_plaid_ivf if ivf else engine.bank_search_plaid)(bank, query_li, k_local, **kw)
        else:
            r = (engine.bank_search_plaid_ivf_filtered if ivf else engine.bank_search_plaid_filtered)(bank, query_li, k_local, filter, **kw)
    elif filter is not None:
        r = (engine.bank_search_filtered_sparse if sparse else engine.bank_search_filtered)(bank, query_li, k_local, filter)
    else:
        r = engine.bank_search(bank, query_li, k_local)
    if k_local == k and "counts" in r:
        return r
    out["indices"][:, :k_local] = r["indices"]
    out["scores"][:, :k_local] = r["scores"]
    if "counts" in r:
        out["counts"] = r["counts"]
    else:
        out["counts"].fill_(k_local)
    return out


def search_banks(engine, banks: Sequence, query_li, k: int, plaid: Optional[PlaidSearch] = None, filters: Optional[Sequence] = None,
                 sparse: bool = False, fast: Optional[F16Search] = None):
    """PassageBank.search over several banks held by one process (a corpus loaded bank by bank, an fp16 bank beside a compressed
    one of the same li_dim) as over one bank holding their passages in the order of `banks`: every bank is searched
    (search_bank_part: `plaid` for each, `filters[i]` a BankFilter of bank i or None), the lists are merged on the device
    (RerankEngine.bank_merge_topk, rr_bank_merge_topk) and the ids come from each bank's table.  Returns (passage_ids, scores,
    counts): passage_ids[q] the ids of query q best first, at its true length (at most k); scores float32 [n_queries, k] on the
    device, -inf behind the count; counts int32 [n_queries] on the device.  With the exact search this is, byte for byte, the
    search of the one bank; with `plaid` it is by definition the merge of the per-bank pruned searches (each bank keeps its own
    ndocs).  Copies the merged indices to the host (synchronises).  At most 64 banks, len(banks) * k <= 8192.  `sparse`: every
    bank's filtered exact search in its list-driven form (a filter for every bank, no `plaid`; ValueError otherwise).  `fast` (an
    F16Search; no `plaid`, filters or `sparse`): every bank by engine.bank_search_f16 or, compressed, bank_search_f16_plaid, and a fourth result, certified int32
    [n_queries] on the device: the AND of the parts' certificates (every part's list provably exact: so is the merged one)."""
    import numpy as np
    import torch
    banks = list(banks)
    if not banks:
        raise ValueError("search_banks: no bank")
    if filters is not None and len(filters) != len(banks):
        raise ValueError(f"search_banks: {len(filters)} filters for {len(banks)} banks (one each, or None)")
    _fast_check("search_banks", fast, plaid, filters, sparse)
    if sparse:
        for f in (filters if filters is not None else [None]):
            _sparse_check("search_banks", sparse, f, plaid)
    offsets = np.zeros(len(banks) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in banks], out=offsets[1:])
    more = dict(sparse=True) if sparse else dict(fast=fast) if fast is not None else {}
    parts = [search_bank_part(engine, b, query_li, k, plaid, None if filters is None else filters[i], **more) for i, b in enumerate(banks)]
    r = engine.bank_merge_topk(torch.stack([p["indices"] for p in parts]), torch.stack([p["scores"] for p in parts]),
                               torch.stack([p["counts"] for p in parts]), offsets, k, want_parts=True)
    counts = r["counts"].tolist()
    ids = [[banks[p].table.ids[g - int(offsets[p])] for g, p in zip(row[:c], prow[:c])]
           for row, prow, c in zip(r["indices"].tolist(), r["parts"].tolist(), counts)]
    if fast is not None:
        return ids, r["scores"], r["counts"], torch.stack([p["certified"] for p in parts]).min(dim=0).values
    return ids, r["scores"], r["counts"]
