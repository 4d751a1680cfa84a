"""GPU: a passage bank that lives through random sequences of add, remove, build_ivf, extend_ivf, clear and search
(tests/bank_life.py; the scripts are shown to reach the hard situations by tests/test_bank_life_cpu.py).  What a long-lived bank
carries from call to call (first / len / used_rows and the searches' cached table on the C side, the inverted file and its prefix,
BankTable, generation and padded_len in Python) is checked as a whole:

AFTER EVERY STEP the lived bank A is compared with the Shadow, a host model that calls nothing of the library: info, len, ids,
coverage, generation, every passage read back, the export and the inverted file (against its definition, ivf_numpy), what remove
returns, a refused add that changes nothing, a stale filter that is refused.  No second kernel enters these checks.
EVERY EIGHTH STEP and after the last, A is compared with a FRESH bank B filled from the Shadow (the covered prefix, build_ivf, the
rest); also after an add, remove or clear that met a current device table of the searches (the Shadow knows: the table is then cut
or dropped and the next search uploads the rest).  These are the two contracts "to the bit what a fresh bank
of the same contents would be" (rr_bank_remove, rr_bank_extend_ivf) through reads, export, file, the three searches, a filtered
search and bank_li_scores with an explicit padded_len (a bank's own padded_len is a high-water mark of its adds, not a function of
its contents).
Two lived banks searched as one (search_banks) equal one fresh bank of their passages.  At its end a compressed script is saved as
a PLAID index and loaded back with its inverted file.

THE CUT TABLE.  Every search entry and rr_bank_export_plaid begin by bringing the searches' device table up to date, so a check that
searches or exports directly behind a removal would hand the next operation a whole table again.  A removal that is directly
followed by an add or a remove is therefore a QUIET step (`_Life.quiet`): the passages are still read back and everything else is
compared with the Shadow, but the export check, the extra comparison with a fresh bank and every search of the harness wait for the
next step, so that remove, remove and search, remove, add reach the bank with the table as the removal cut it.  Two things still
stand between such operations: the comparison of every eighth step and the acceptance search behind a removal that a stale filter
was waiting for; tests/test_bank_life_cpu.py counts the two situations only where neither does.

Everything is equality of bytes; there is no tolerance anywhere.

THE CODED KIND is an fp16 bank with a centroid table (rr_bank_set_centroids): fp16 rows, one code a row, a mask byte, three arrays of
2 D / 4 / 1 bytes that a removal moves together.  It is checked as an fp16 bank (rows and mask read back, the exact and the filtered
search, bank_li_scores) AND as a bank with codes (the codes read back, the file against its definition, the pruned searches and
their covered-prefix forms).  Its scripts switch between two tables of 16 and 12 centroids: after a set_centroids the codes are
the Shadow's codes under the new table (a float64 argmax, tests/bank_life.py), the file is gone, the generation is unchanged and
a filter built before the call is still accepted.  It has no residuals: export_compressed and save_plaid_index refuse.

A saved index holds the unmasked rows alone (rr_bank_export_plaid), so the loaded bank C is compared with the Shadow's unmasked rows
and with A's export, file and searches, not with A's masked rows."""
import types

import numpy as np
import pytest
import torch

import bank_life as BL
from test_bank_life_cpu import EVERY, PAIRS, SEEDS, STEPS, WINDOWED, ops_of, step
from test_gpu_bank_li_scores import _queries
from test_gpu_bank_remove import DEFAULT_KB, _Window, _bits, _same_ivf, _same_searches
from test_gpu_bank_search_plaid import _near_queries
from test_gpu_li_scores import _engine as _bare_engine

pytestmark = pytest.mark.gpu

D = BL.D
PADDED = 136                                               # an explicit padded_len above the longest passage (130)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _padded(passages, key, dtype):
    """[n, Lc, D] rows of `key` and the [n, Lc] mask of one add / add_compress call, Lc the call's longest passage."""
    n, Lc = len(passages), max(p["length"] for p in passages)
    li, cm = torch.zeros(n, Lc, D, dtype=dtype), torch.zeros(n, Lc)
    for i, p in enumerate(passages):
        rows = _t(p[key])
        li[i, :p["length"]] = rows.view(torch.float16) if dtype == torch.float16 else rows
        cm[i, :p["length"]] = _t(p["mask"]).float()
    return li.cuda(), cm.cuda()


def _add(bank, passages, via):
    ids, lens = [p["id"] for p in passages], [p["length"] for p in passages]
    if via == "add":
        return bank.add(ids, *_padded(passages, "rows", torch.float16), lengths=lens)
    if via == "add_compress":
        return bank.add_compress(ids, *_padded(passages, "x", torch.float32), lengths=lens)
    assert via == "add_compressed"
    return bank.add_compressed(ids, _t(np.concatenate([p["codes"] for p in passages])), _t(np.concatenate([p["res"] for p in passages])),
                               lens, mask=_t(np.concatenate([p["mask"] for p in passages])))


def _create(eng, sh, rows=None, slots=None):
    """An empty bank of the Shadow's kind, for a coded kind with the table the Shadow holds."""
    return eng.create_bank(sh.capacity_rows if rows is None else rows, sh.max_passages if slots is None else slots, codec=BL.codec_of(sh.kind),
                           centroids=BL.tables()[sh.table] if sh.coded else None)


def _fresh(eng, sh):
    """A fresh bank of the Shadow's contents: the covered prefix in one call, build_ivf, the rest in one call."""
    B = _create(eng, sh)
    via = "add_compressed" if sh.nbits else "add"
    if sh.covered:
        _add(B, sh.passages[:sh.covered], via)
        assert B.build_ivf()["passages_covered"] == sh.covered
    if sh.covered < len(sh):
        _add(B, sh.passages[sh.covered:], via)
    return B


def _check_against_shadow(A, sh, what, export=True):
    """Everything the library offers to look at a bank with, against the host model: no second kernel.  `export`: False on a quiet
    step (the export brings the searches' device table up to date, as a search does)."""
    assert A.info() == sh.info() and len(A) == len(sh), f"{what}: info {A.info()} for {sh.info()}"
    assert A.table.ids == sh.ids and A.table.lengths == sh.lengths, what
    assert A.generation == sh.generation, f"{what}: generation {A.generation} for {sh.generation}"
    assert A.padded_len == sh.padded_len, f"{what}: padded_len {A.padded_len}, the high-water mark of the adds is {sh.padded_len}"
    if not sh.nbits:
        for p in sh.passages:
            rows, mask = A.read(p["id"])
            assert torch.equal(_bits(rows), _t(p["rows"])) and torch.equal(mask, _t(p["mask"])), f"{what}: passage {p['id']}"
            if sh.coded:
                assert torch.equal(A.codes(p["id"]), _t(sh.codes_of(p))), f"{what}: the codes of passage {p['id']} under table {sh.table}"
        if not sh.coded:
            return
        assert A.n_centroids == sh.n_centroids and A.format() == dict(nbits=0, n_centroids=sh.n_centroids, bytes_per_row=2 * D + 1 + 4), what
    assert A.ivf_info()["passages_covered"] == sh.covered, f"{what}: coverage {A.ivf_info()} for {sh.covered}"
    for p in sh.passages if sh.nbits else []:
        codes, res, mask = A.read_compressed(p["id"])
        assert torch.equal(codes, _t(p["codes"])) and torch.equal(res, _t(p["res"])) and torch.equal(mask, _t(p["mask"])), \
            f"{what}: passage {p['id']}"
    if len(sh) and export and sh.nbits:
        sh.search()                                        # the table is whole again
        codes, res, doclens = A.export_compressed()
        want_codes, want_res, want_doclens = sh.export()
        assert list(doclens) == want_doclens and torch.equal(codes.cpu(), _t(want_codes)) and torch.equal(res.cpu(), _t(want_res)), \
            f"{what}: the export"
    if sh.covered:
        pids, lengths = A.ivf()
        want_pids, want_lengths = sh.expected_ivf()
        assert torch.equal(lengths, _t(want_lengths)), f"{what}: list lengths {lengths.tolist()} for {want_lengths.tolist()}"
        assert torch.equal(pids, _t(want_pids)), f"{what}: postings"
        assert A.ivf_info() == dict(passages_covered=sh.covered, postings=len(want_pids), longest_list=int(want_lengths.max())), what


def _same_bank(A, B, sh, what):
    """_same_compressed of tests/test_gpu_bank_remove.py over this script's ids, and its fp16 counterpart."""
    assert A.info() == B.info() and A.table.ids == B.table.ids, what
    for pid in sh.ids:
        got, want = (A.read_compressed(pid), B.read_compressed(pid)) if sh.nbits else (A.read(pid), B.read(pid))
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want)), f"{what}: passage {pid}"
        if sh.coded:
            assert torch.equal(A.codes(pid), B.codes(pid)), f"{what}: the codes of passage {pid}"
    if sh.nbits:
        (ca, ra, da), (cb, rb, db) = A.export_compressed(), B.export_compressed()
        assert list(da) == list(db) and torch.equal(ca, cb) and torch.equal(ra, rb), f"{what}: the export"


def _queries_of(sh, seed):
    if sh.coded:                                           # near centroids of the first table: a passage's rows lie near one of each table
        return _near_queries(types.SimpleNamespace(centroids=BL.tables()[0]), 2, 9, seed=seed)
    return _near_queries(BL.codec_of(sh.kind), 2, 9, seed=seed) if sh.nbits else _queries(2, 9, D, seed=seed)


def _check_against_fresh(eng, A, sh, what, seed):
    B = _fresh(eng, sh)
    n, q = len(sh), _queries_of(sh, seed)
    sh.search()                                            # the searches below bring A's device table up to date
    _same_bank(A, B, sh, what)
    if sh.has_codes:
        if sh.covered:
            _same_ivf(A, B)
        else:
            assert A.ivf_info() == B.ivf_info() and A.ivf_info()["passages_covered"] == 0
        if 0 < sh.covered < n:
            _same_searches(eng, A, B, q, count=sh.covered)
            _same_searches(eng, A, B, q, ivf=False)
        else:
            _same_searches(eng, A, B, q, ivf=sh.covered == n)
    if not sh.nbits:
        (ia, sa), (ib, sb) = A.search(eng, q, n), B.search(eng, q, n)
        assert ia == ib and torch.equal(sa.view(torch.int32), sb.view(torch.int32)), f"{what}: the exact search"
    # the searches whose first pass runs on the fp16 matrix core read the same cached device table: with every passage rescored
    # (ndocs 1024 >= n) they must give the plain search's ids and score bytes on both banks, every query certified
    if n <= 1024 and D % 32 == 0 and (not sh.nbits or D in (32, 64, 128, 256)):
        from rmr_amd import F16Search
        for name, bank in (("the lived bank", A), ("the fresh bank", B)):
            ids, scores = bank.search(eng, q, n)
            r = bank.search(eng, q, n, fast=F16Search(1024))
            torch.cuda.synchronize()
            assert [[bank.table.ids[j] for j in row] for row in r["indices"].tolist()] == ids, f"{what}: the fp16 matrix-core search of {name}"
            assert torch.equal(r["scores"].view(torch.int32), scores.view(torch.int32)), f"{what}: the fp16 matrix-core search of {name}"
            assert r["certified"].tolist() == [1] * q.shape[0], f"{what}: every passage of {name} is rescored, the query is certified"
    # the exact search under a fresh filter that excludes every third passage
    out = sh.ids[::3]
    (ia, sa), (ib, sb) = A.search(eng, q, n, filter=A.filter(excluded=out)), B.search(eng, q, n, filter=B.filter(excluded=out))
    assert ia == ib and torch.equal(sa.view(torch.int32), sb.view(torch.int32)), f"{what}: the filtered search"
    assert all(len(row) == n - len(out) and not set(row) & set(out) for row in ia), f"{what}: the filter's passages"
    # the retriever's scores of every passage, in a shuffled order, under an explicit padded length
    order = np.random.default_rng(seed).permutation(n)
    ids, pq = [sh.ids[j] for j in order], [int(j) % 2 for j in range(n)]
    sa = eng.bank_li_scores(A, q, ids, pair_query=pq, want_scores=True, padded_len=PADDED)
    sb = eng.bank_li_scores(B, q, ids, pair_query=pq, want_scores=True, padded_len=PADDED)
    torch.cuda.synchronize()
    assert sa["scores"].shape == (n, PADDED, q.shape[1])
    assert torch.equal(sa["maxsim"].view(torch.int32), sb["maxsim"].view(torch.int32)), f"{what}: maxsim"
    assert torch.equal(sa["scores"].view(torch.int32), sb["scores"].view(torch.int32)), f"{what}: the score block"
    B.close()


class _Life:
    """One bank, its Shadow and its script; `run(i)` carries out step i on both and checks the bank against the Shadow."""

    def __init__(self, eng, kind, seed, prefix="p"):
        self.eng, self.kind, self.seed = eng, kind, seed
        self.ops = ops_of(seed, kind, prefix)
        rows, slots = BL.capacity(self.ops)
        self.sh = BL.Shadow(kind, rows, slots)
        self.A = _create(eng, self.sh)
        self.pending, self.stale = None, False             # a filter built at a stale_filter step; a remove or clear has run since
        self.watch = False                                 # a comparison with a fresh bank is due besides those of every eighth step
        self.q = _queries_of(self.sh, 5)

    def run(self, i, check=True):
        A, sh, op = self.A, self.sh, self.ops[i]
        what = op["op"]
        where = f"{self.kind} seed {self.seed} step {i} {what}"
        if what in ("add", "remove", "clear") and sh.table_current:            # the cached table is cut, dropped or grown
            self.watch = True
        if what == "add":
            assert _add(A, op["passages"], op["via"]) == step(sh, op), where
        elif what == "add_refused":
            assert isinstance(step(sh, op), MemoryError)
            with pytest.raises(MemoryError):
                _add(A, op["passages"], "add_compressed" if sh.nbits else "add")
            assert not any(p["id"] in A for p in op["passages"]), where
        elif what == "remove":
            got, want = A.remove(op["ids"]), step(sh, op)
            assert got["new_index"].dtype == np.int32 and np.array_equal(got["new_index"], want["new_index"]), where
            assert got["passages"] == want["passages"] and got["rows_freed"] == want["rows_freed"], where
        elif what == "build_ivf":
            step(sh, op)
            assert A.build_ivf()["passages_covered"] == sh.covered, where
        elif what == "extend_ivf":
            step(sh, op)
            assert A.extend_ivf()["passages_covered"] == sh.covered, where
        elif what == "clear":
            step(sh, op)
            A.clear()
        elif what == "set_centroids":
            gen, held = A.generation, A.filter(excluded=sh.ids[:1]) if len(sh) else None
            step(sh, op)
            A.set_centroids(BL.tables()[op["table"]])
            assert A.generation == gen == sh.generation and A.n_centroids == BL.TABLE_SIZES[op["table"]], where
            assert A.ivf_info() == dict(passages_covered=0, postings=0, longest_list=0), f"{where}: the file goes with the table it named"
            if held is not None:                           # the passages are as they were: a filter from before the call is accepted
                ids, _ = A.search(self.eng, self.q, len(sh), filter=held)
                assert all(sorted(row) == sorted(sh.ids[1:]) for row in ids), where
                sh.search()
            if self.pending is not None and not self.stale and self.ops[i - 1]["op"] == "stale_filter":
                A.search(self.eng, self.q, 1, filter=self.pending)             # so is the one of the stale_filter step before it
        elif what == "search":
            step(sh, op)
            ids, scores = A.search(self.eng, self.q, min(3, len(sh)))
            assert all(len(row) == min(3, len(sh)) and set(row) <= set(sh.ids) for row in ids), where
        else:
            assert what == "stale_filter"
            self.pending, self.stale = A.filter(excluded=sh.ids[:1]), False
            A.search(self.eng, self.q, 1, filter=self.pending)                 # accepted while nothing has changed
            sh.search()
        if what in ("remove", "clear") and self.pending is not None and not self.stale:
            self.stale = True
            if len(sh):        # a filter built now is accepted: that it is taken and what it lets through, nothing about the table
                ids, _ = A.search(self.eng, self.q, len(sh), filter=A.filter(excluded=sh.ids[:1]))
                assert all(sorted(row) == sorted(sh.ids[1:]) for row in ids), where
                sh.search()
        if self.stale:                                     # refused from the change on, whatever the bank has been refilled to
            with pytest.raises(ValueError, match="build it again"):
                A.search(self.eng, self.q, 1, filter=self.pending)
        if check:
            _check_against_shadow(A, sh, where, export=not self.quiet(i))
        return where

    def quiet(self, i):
        """Step i is a removal directly followed by an add or a remove: nothing of the harness touches the table it has cut."""
        return self.ops[i]["op"] == "remove" and i + 1 < len(self.ops) and self.ops[i + 1]["op"] in ("add", "remove")

    def checkpoint(self, i):
        due = i % EVERY == EVERY - 1 or i == len(self.ops) - 1 or (self.watch and not self.quiet(i))
        if due:
            self.watch = False
        return due


CASES = [(kind, seed) for kind in sorted(SEEDS) for seed in SEEDS[kind]]


@pytest.mark.parametrize("kind,seed", CASES)
def test_a_lived_bank_equals_its_shadow_after_every_step_and_a_fresh_bank_every_eighth(kind, seed, tmp_path):
    eng = _bare_engine(D)
    life = _Life(eng, kind, seed)
    A, sh = life.A, life.sh
    compared = 0
    with _Window(eng, 4 if seed == WINDOWED[kind] else DEFAULT_KB):            # bank_move_kb = 4: removals in many windows
        for i in range(STEPS):
            where = life.run(i)
            if life.checkpoint(i) and len(sh):
                _check_against_fresh(eng, A, sh, where, seed=41 + i)
                compared += 1
        if sh.nbits:
            _save_and_load(eng, life, str(tmp_path / "index"))
        elif sh.coded:                                     # no residuals: nothing to export or to save
            for call in (A.export_compressed, lambda: A.save_plaid_index(str(tmp_path / "index"))):
                with pytest.raises(NotImplementedError):
                    call()
            assert not (tmp_path / "index").exists()
    assert compared >= STEPS // EVERY - 1, f"{compared} comparisons with a fresh bank"
    A.close()


def _save_and_load(eng, life, path):
    """The end of a compressed script: the bank saved as a PLAID index with its file, and loaded into an empty bank."""
    from rmr_amd import read_plaid_index
    A, sh = life.A, life.sh
    empty = [p["id"] for p in sh.passages if not p["mask"].any()]              # an index cannot hold a passage without a row
    if empty:
        got, want = A.remove(empty), sh.remove(empty)
        assert np.array_equal(got["new_index"], want["new_index"]) and got["rows_freed"] == want["rows_freed"]
    if not len(sh):
        again = [dict(p, id=f"again/{p['id']}") for p in life.ops[0]["passages"] if p["mask"].any()]
        assert _add(A, again, "add_compressed") == sh.add(again) == 0
    _check_against_shadow(A, sh, "before the save")
    meta = A.save_plaid_index(path, ivf=True)
    sh.save_plaid_index()
    assert sh.covered == len(sh) and meta["num_embeddings"] == sum(sh.export()[2])
    _check_against_shadow(A, sh, "after the save")
    C = eng.create_bank(sh.capacity_rows, sh.max_passages, codec=read_plaid_index(path)[0])
    assert C.load_plaid_index(path, ivf=True) == len(sh) and C.table.ids == sh.ids
    _same_ivf(A, C)
    (ca, ra, da), (cc, rc, dc) = A.export_compressed(), C.export_compressed()
    assert list(da) == list(dc) == sh.export()[2] and torch.equal(ca, cc) and torch.equal(ra, rc)
    for p in sh.passages:
        live = p["mask"] != 0
        codes, res, mask = C.read_compressed(p["id"])
        assert torch.equal(codes, _t(p["codes"][live])) and torch.equal(res, _t(p["res"][live])) and bool(mask.all()), p["id"]
    _same_searches(eng, A, C, _queries_of(sh, 53))
    C.close()


@pytest.mark.parametrize("kind", sorted(PAIRS))
def test_two_lived_banks_searched_as_one_equal_one_fresh_bank(kind):
    from rmr_amd import search_banks
    eng = _bare_engine(D)
    lives = [_Life(eng, kind, seed, prefix) for seed, prefix in zip(PAIRS[kind], "pq")]
    compared = 0
    for i in range(STEPS):
        for life in lives:
            life.run(i, check=False)
            assert life.A.info() == life.sh.info() and life.A.table.ids == life.sh.ids
        held = [p for life in lives for p in life.sh.passages]
        due = [life.checkpoint(i) for life in lives]
        if any(due) and held:
            assert len(set(p["id"] for p in held)) == len(held), "the two banks hold disjoint ids"
            F = _create(eng, lives[0].sh, sum(p["length"] for p in held), len(held))
            for life in lives:
                if len(life.sh):
                    _add(F, life.sh.passages, "add_compressed" if life.sh.nbits else "add")
            q, k = _queries_of(lives[0].sh, 61 + i), min(8, len(held))
            ids, scores, counts = search_banks(eng, [life.A for life in lives], q, k)
            want_ids, want_scores = F.search(eng, q, k)
            for life in lives:
                life.sh.search()
            assert ids == want_ids and counts.tolist() == [k] * q.shape[0], f"{kind} step {i}"
            assert torch.equal(scores.view(torch.int32), want_scores.view(torch.int32)), f"{kind} step {i}"
            compared += all(len(life.sh) for life in lives)
            F.close()
    assert compared >= 2, "both banks held passages at fewer than two of the comparisons"
    for life in lives:
        life.A.close()
