"""A host model of a long-lived passage bank and a generator of scripts that live one (tests/test_bank_life_cpu.py,
tests/test_gpu_bank_life.py).  No device and no call into the library's C code: of the package only the PlaidCodec class is used, as
a host container of the codec's tables, beside helpers of tests/test_gpu_bank_search_plaid.py that are torch on the CPU.  The codes
of the one add_compress operation of a compressed script come from the host definition (PlaidCodec.compress), which the TESTS call
and hand to `materialise`; so the CPU tests of the compressed kinds need the built library, as the project's other CPU tests do.

`Shadow` holds what a bank of the same history must hold: the passages in order (id, length and per row the centroid code, the
residual bytes and the mask byte, or the fp16 row bits and the mask byte), the row and passage-slot capacity, how many passages the
inverted file covers (0: no file), the generation, and whether the searches' cached device table is current.  Its methods mirror
the mutators of PassageBank and predict what they return and leave behind (include/rerank_mi355.h: rr_bank_add* refuse with the bank
unchanged; REMOVING PASSAGES; THE INVERTED FILE, LIFETIME).  `expected_ivf` is the definition of the file (ivf_numpy of
tests/test_bank_ivf_cpu.py) over the covered prefix.

The kind `coded` is an fp16 bank with a centroid table (rr_bank_set_centroids): its passages hold fp16 row bits and, under each of the
two tables of `tables()`, the codes of their rows (`codes2` int32 [2, len]: a float64 argmax with an asserted margin, _coded_rows).
It has nbits 0 and so `info()` of an fp16 bank, but it holds codes: the file motifs apply to it, and its scripts have the operation
set_centroids, which switches to the other table (the codes switch, the file goes, the generation stays).

`script(seed, kind, steps)` draws a deterministic list of operations with numpy.random.default_rng.  The operations are drawn as
short motifs (a search, a removal, an add; an add, an extend, a removal inside the prefix; ...) so that the situations the tests
count occur within 40 steps; which of them occurred is counted by tests/test_bank_life_cpu.py, not assumed here.  The capacity is
tight: `capacity(ops)` is the largest row total and passage count the script ever holds, so an add behind a removal succeeds only on
the rows and slots that removal gave back."""
import functools

import numpy as np
import torch

from bank_remove_cases import GPU_LENGTHS
from test_bank_ivf_cpu import ivf_numpy
from test_gpu_bank_search_plaid import _codec, _topic_rows

D = 64
C_CENTROIDS = 16
KINDS = {"fp16": 0, "plaid2": 2, "plaid8": 8, "coded": 0}  # kind -> nbits (0: an fp16 bank); residual rows of 16 and 64 bytes
STREAMS = {"fp16": 0, "plaid2": 1, "plaid8": 2, "coded": 3}         # the generator's stream of a kind: fixed, so that a new kind leaves the others' scripts alone
TABLE_SIZES = (16, 12)                                     # the two centroid tables a coded bank switches between (set_centroids)
TARGET_ROWS, TARGET_SLOTS = 1200, 48                       # what the generator fills up to; capacity() is what a script reached
MAX_ADD = 12
FULLY_MASKED = 5                                           # the serial number of the passage without an unmasked row
REMOVE_SHAPES = ("leading", "trailing", "interior", "behind_prefix", "whole_prefix", "everything", "any")


@functools.lru_cache(maxsize=None)
def codec_of(kind):
    """The codec of a compressed kind: 16 unit centroids, bucket weights, and cutoffs (add_compress and a saved index need them)."""
    from rmr_amd import PlaidCodec
    nbits = KINDS[kind]
    if not nbits:
        return None
    base = _codec(D, nbits, C_CENTROIDS)
    # a residual is a difference of fp16 values, a multiple of 2^-24: cutoffs 2^-26 off the grid are never met exactly (0 would be)
    cutoffs = torch.linspace(-0.1, 0.1, (1 << nbits) - 1) + 2.0 ** -26
    return PlaidCodec(base.centroids, base.bucket_weights, nbits, bucket_cutoffs=cutoffs)


def holds_codes(kind):
    """A compressed bank, or an fp16 bank with a centroid table (a "coded" one): what the inverted file and the pruned searches need."""
    return bool(KINDS[kind]) or kind == "coded"


@functools.lru_cache(maxsize=None)
def tables():
    """The two tables of the coded kind, host fp16 [16, D] and [12, D]: unit centroids, unrelated to one another."""
    return tuple(_codec(D, 8, n, seed=40 + i).centroids.half() for i, n in enumerate(TABLE_SIZES))


def _coded_rows(n, gen):
    """fp16 rows [n, D] near one centroid of EACH table (as via="add_compress" draws x near one), and their codes under both tables,
    int32 [2, n]: the first maximum of the float64 product with the fp16 row, asserted to lead the second best by a margin (as
    _assert_exact_input), so that the code hangs on no order of a float32 sum and owes nothing to the library."""
    cens = [t.double() for t in tables()]
    picks = [torch.randint(0, len(c), (n,), generator=gen) for c in cens]
    x = sum(c[p].float() for c, p in zip(cens, picks)) + 0.5 * torch.randn(n, D, generator=gen) / D ** 0.5
    rows = torch.nn.functional.normalize(x, dim=-1).half()
    codes = []
    for c in cens:
        top =(rows.double() @ c.T).topk(2, dim=1)
        assert float((top.values[:, 0] - top.values[:, 1]).min()) > 1e-3, "two centroids nearly tie for a row"
        codes.append(top.indices[:, 0].to(torch.int32).numpy())
    return rows.view(torch.int16).numpy(), np.stack(codes)


def _mask_of(serial, length):
    """Every third passage of three rows or more has interior masked rows; one passage has no unmasked row at all."""
    m = np.ones(length, dtype=np.uint8)
    if serial == FULLY_MASKED:
        m[:] = 0
    elif serial % 3 == 1 and length >= 3:
        m[1:-1:2] = 0
    return m


def make_passages(kind, ids, lens, serial0, seed, via="add"):
    """The passages of one add as dicts: id, length, mask uint8 [len], and `codes` int32 [len] / `res` uint8 [len, bytes] (compressed,
    _topic_rows over the 16 centroids), or `rows` int16 [len, D] = fp16 bits (an fp16 bank), or for via == "add_compress" `x` float32
    [len, D]: unit rows near a centroid, whose codes and bytes `materialise` takes from the host definition."""
    codec = codec_of(kind)
    out, r0 = [], 0
    gen = torch.Generator().manual_seed(int(seed))
    if kind == "coded":
        rows, codes2 = _coded_rows(sum(lens), gen)
    elif codec is None:
        rows = torch.nn.functional.normalize(torch.randn(sum(lens), D, generator=gen), dim=-1).half().view(torch.int16).numpy()
    elif via == "add_compress":
        cen = codec.centroids.float()
        pick = torch.randint(0, C_CENTROIDS, (sum(lens),), generator=gen)
        x = torch.nn.functional.normalize(cen[pick] + 0.5 * torch.randn(sum(lens), D, generator=gen) / D ** 0.5, dim=-1)
        _assert_exact_input(codec, x)
        x = x.numpy()
    else:
        codes, res = _topic_rows(codec, lens, seed=int(seed))
        codes, res = codes.numpy(), res.numpy()
    for i, (pid, ln) in enumerate(zip(ids, lens)):
        p = dict(id=pid, length=int(ln), mask=_mask_of(serial0 + i, ln))
        if codec is None:
            p["rows"] = rows[r0:r0 + ln].copy()
            if kind == "coded":
                p["codes2"] = codes2[:, r0:r0 + ln].copy()
        elif via == "add_compress":
            p["x"] = x[r0:r0 + ln].copy()
        else:
            p["codes"], p["res"] = codes[r0:r0 + ln].copy(), res[r0:r0 + ln].copy()
        out.append(p)
        r0 += ln
    return out


def _assert_exact_input(codec, x):
    """No tie between centroids and no residual on a bucket cutoff: the compressed row does not hang on how a score is summed."""
    cen = codec.centroids.float()
    x16 = x.half().float()
    top = (x16 @ cen.T).topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) > 1e-3, "two centroids nearly tie for a row"
    resid = x16 - cen[(x16 @ cen.T).argmax(dim=1)]
    assert float((resid[:, :, None] - codec.bucket_cutoffs[None, None, :]).abs().min()) > 0.0, "a residual lies on a cutoff"


def materialise(ops, compress):
    """Give the passages of the add_compress operations their codes and residual bytes: compress(x float32 [R, D]) -> (codes,
    residuals), the host definition (PlaidCodec.compress), called by the tests: this module calls nothing of the library."""
    for op in ops:
        if op["op"] == "add" and op.get("via") == "add_compress":
            for p in op["passages"]:
                if "codes" not in p:
                    codes, res = compress(p["x"])
                    p["codes"], p["res"] = np.asarray(codes, dtype=np.int32), np.asarray(res, dtype=np.uint8)
    return ops


class Shadow:
    def __init__(self, kind, capacity_rows, max_passages):
        self.kind, self.nbits = kind, KINDS[kind]
        self.coded = kind == "coded"
        self.has_codes = holds_codes(kind)
        self.table = 0                       # which of tables() a coded bank holds
        self.capacity_rows, self.max_passages = int(capacity_rows), int(max_passages)
        self.passages = []
        self.covered = 0                     # passages the inverted file covers; 0: no file
        self.generation = 0
        self.table_current = False           # a search has run since the last change: the searches' device table is up to date
        self.padded_len = 0                  # the high-water mark PassageBank.padded_len keeps

    def __len__(self):
        return len(self.passages)

    @property
    def ids(self):
        return [p["id"] for p in self.passages]

    @property
    def lengths(self):
        return [p["length"] for p in self.passages]

    @property
    def rows_used(self):
        return sum(self.lengths)

    def info(self):
        out = dict(passages=len(self), rows_used=self.rows_used, capacity_rows=self.capacity_rows)
        if self.nbits:
            out.update(nbits=self.nbits, bytes_per_row=4 + D * self.nbits // 8 + 1)
        return out

    def fits(self, passages):
        return (len(self) + len(passages) <= self.max_passages
                and self.rows_used + sum(p["length"] for p in passages) <= self.capacity_rows)

    def add(self, passages, padded=None):
        """The first dense index of the new passages; MemoryError, with nothing changed, when rows or slots do not suffice.
        `padded`: the Lc of the padded tensors of an add / add_compress (a compressed add's is its longest passage)."""
        if not self.fits(passages):
            raise MemoryError("rows or passage slots do not suffice")
        held = set(self.ids)
        assert not any(p["id"] in held for p in passages)
        first = len(self)
        self.passages += list(passages)
        self.padded_len = max(self.padded_len, max(p["length"] for p in passages) if padded is None else padded)
        self.table_current = False
        return first

    def remove(self, ids):
        """{"new_index", "passages", "rows_freed"} as PassageBank.remove returns them.  The file follows the survivors of its
        prefix and is dropped when none survives."""
        gone = set(ids)
        assert len(gone) == len(ids) and gone <= set(self.ids)
        new_index = np.full(len(self), -1, dtype=np.int32)
        keep, freed, covered = [], 0, 0
        for i, p in enumerate(self.passages):
            if p["id"] in gone:
                freed += p["length"]
            else:
                new_index[i] = len(keep)
                keep.append(p)
                covered += i < self.covered
        self.passages, self.covered = keep, covered
        if ids:
            self.generation += 1
        self.table_current = False
        return dict(new_index=new_index, passages=len(keep), rows_freed=freed)

    @property
    def n_centroids(self):
        return TABLE_SIZES[self.table] if self.coded else C_CENTROIDS

    def codes_of(self, p):
        return p["codes2"][self.table] if self.coded else p["codes"]

    def set_centroids(self, table):
        """A coded bank takes table `table` of tables(): every row is assigned anew and the inverted file is dropped; the passages,
        the generation (a filter stays valid) and the searches' device table are as they were."""
        assert self.coded
        self.table, self.covered = int(table), 0

    def build_ivf(self):
        assert self.has_codes and len(self)
        self.covered = len(self)

    def extend_ivf(self):
        """True when there was something to do (a file over fewer passages than held, or none: then the call is the build)."""
        assert self.has_codes and len(self)
        work = self.covered < len(self)
        self.covered = len(self)
        return work

    def save_plaid_index(self):
        """save_plaid_index(ivf=True) extends a short file first: the bank is fully covered afterwards."""
        self.extend_ivf()

    def clear(self):
        self.passages, self.covered = [], 0
        self.generation += 1
        self.table_current = False

    def search(self):
        self.table_current = True

    def concat(self, first=0, count=None):
        """(codes, residuals, mask, lengths) of passages first .. first + count - 1, rows back to back."""
        ps = self.passages[first:None if count is None else first + count]
        rb = D * self.nbits // 8
        codes = np.concatenate([self.codes_of(p) for p in ps]) if ps else np.zeros(0, dtype=np.int32)
        res = np.concatenate([p["res"] for p in ps]) if ps and self.nbits else np.zeros((sum(p["length"] for p in ps), rb), dtype=np.uint8)
        mask = np.concatenate([p["mask"] for p in ps]) if ps else np.zeros(0, dtype=np.uint8)
        return codes, res, mask, [p["length"] for p in ps]

    def export(self):
        """What export_compressed gives: the unmasked rows back to back, and per passage how many it has."""
        codes, res, mask, _ = self.concat()
        live = mask != 0
        return codes[live], res[live], [int(p["mask"].sum()) for p in self.passages]

    def expected_ivf(self):
        """(pids int32 [postings], lengths int64 [C]) of the file over the covered prefix, as PassageBank.ivf returns them."""
        assert self.covered
        codes, _, mask, lens = self.concat(0, self.covered)
        offsets, pids = ivf_numpy(codes, mask, lens, self.n_centroids)
        return pids, np.diff(offsets)


def expected_ivf(shadow):
    """The inverted file a bank with the Shadow's history must hold: ivf_numpy over the covered prefix."""
    return shadow.expected_ivf()


# ---- the script generator ---------------------------------------------------------------------------------------------------------------
_MOTIFS = [                                                # (weight, operations, False: any bank / True: banks with codes / "coded")
    (20, ["add"], False), (8, ["remove"], False), (6, ["search"], False), (4, ["add_refused"], False), (1, ["clear"], False),
    (6, ["extend_ivf"], True), (3, ["build_ivf"], True),
    (4, ["remove", "remove"], False),
    (5, ["search", "remove", "add"], False),
    (5, ["add", "extend_ivf", "remove:in_prefix"], True),
    (4, ["file", "add", "remove:behind_prefix"], True),
    (3, ["file", "add", "remove:whole_prefix"], True),
    (3, ["remove:everything", "add"], False),
    (3, ["file", "clear", "add", "extend_ivf"], True),
    (3, ["file", "extend_ivf"], True),
    (7, ["fill", "remove", "add"], False),
    (3, ["stale_filter", "remove"], False),
    (2, ["stale_filter", "clear", "add", "add"], False),
    (4, ["file", "set_centroids", "search"], "coded"),
    (4, ["set_centroids", "add", "build_ivf"], "coded"),
    (4, ["file", "add", "set_centroids", "extend_ivf"], "coded"),
    (3, ["set_centroids", "remove", "set_centroids"], "coded"),
    (3, ["stale_filter", "set_centroids"], "coded"),
]
_SHAPE_WEIGHTS = dict(leading=2, trailing=2, interior=4, any=3, behind_prefix=1, whole_prefix=0.5, everything=0.3)


def _pick_removal(rng, shape, n, covered):
    """The dense indices of a removal of `shape` from n passages, `covered` of them under the file; None when the shape does not
    apply.  `in_prefix` is `any` restricted to the covered prefix."""
    few = lambda m: int(rng.integers(1, max(1, min(m, 1 + n // 4)) + 1))
    if shape == "everything":
        return list(range(n))
    if shape == "leading" and n >= 2:
        return list(range(few(n - 1)))
    if shape == "trailing" and n >= 2:
        return list(range(n - few(n - 1), n))
    if shape == "interior" and n >= 3:
        return sorted(rng.choice(np.arange(1, n - 1), size=few(n - 2), replace=False).tolist())
    if shape == "any" and n >= 2:
        return sorted(rng.choice(n, size=few(n - 1), replace=False).tolist())
    if shape == "behind_prefix" and 0 < covered < n:
        return sorted((covered + rng.choice(n - covered, size=few(n - covered), replace=False)).tolist())
    if shape == "whole_prefix" and 0 < covered < n:
        return list(range(covered))
    if shape == "in_prefix" and covered >= 2:
        return sorted(rng.choice(covered, size=few(covered - 1), replace=False).tolist())
    return None


def _coins(rows, most):
    """At most `most` lengths of GPU_LENGTHS, largest first, that sum to `rows` or to as much of it as they can."""
    out = []
    for c in sorted(GPU_LENGTHS, reverse=True):
        while rows >= c and len(out) < most:
            out.append(c)
            rows -= c
    return out


@functools.lru_cache(maxsize=None)
def script(seed, kind, steps=40, prefix="p"):
    """`steps` operations: dicts with "op" in add (passages, via: add / add_compressed / add_compress), add_refused (passages),
    remove (ids, shape), build_ivf, extend_ivf, clear, search, stale_filter, set_centroids (table; the coded kind).  Deterministic in (seed, kind, steps, prefix)."""
    rng = np.random.default_rng([int(seed), STREAMS[kind]])
    compressed, files, coded = bool(KINDS[kind]), holds_codes(kind), kind == "coded"
    sh = Shadow(kind, 1 << 40, 1 << 40)                    # ids, lengths and coverage; the targets bound the adds
    ops, queue, gone, serial = [], [], [], [0]
    motifs = [m for m in _MOTIFS if m[2] is False or (m[2] is True and files) or (m[2] == "coded" and coded)]
    weights = np.array([m[0] for m in motifs], dtype=np.float64)
    compress_left = [compressed]

    def emit_add(lens, via=None):
        ids = [f"{prefix}{serial[0] + i}" for i in range(len(lens))]
        if gone and rng.random() < 0.3:                    # a removed id may come back
            ids[0] = gone.pop(int(rng.integers(len(gone))))
        if via is None:
            via = "add_compressed" if compressed else "add"
            if compress_left[0] and len(ops) >= 2:
                via, compress_left[0] = "add_compress", False
        ps = make_passages(kind, ids, lens, serial[0], seed=int(rng.integers(1 << 30)), via=via)
        serial[0] += len(lens)
        sh.add(ps)
        ops.append(dict(op="add", passages=ps, via=via))

    def add(fill=None):
        free_rows, free_slots = TARGET_ROWS - sh.rows_used, TARGET_SLOTS - len(sh)
        most = min(MAX_ADD, free_slots)
        if most < 1 or free_rows < 1:
            return remove("any")
        if fill == "rows":
            lens = _coins(free_rows, most)
            rng.shuffle(lens)
        elif fill == "slots":
            most = min(most, free_rows)
            lens, left = [], free_rows
            for i in range(most):
                fit = [c for c in (1, 2, 3, 5) if c <= left - (most - 1 - i)]
                if not fit:
                    break
                lens.append(int(rng.choice(fit)))
                left -= lens[-1]
        else:
            lens, left = [], free_rows
            for _ in range(int(rng.integers(1, most + 1))):
                fit = [c for c in GPU_LENGTHS if c <= left]
                if not fit:
                    break
                lens.append(int(rng.choice(fit)))
                left -= lens[-1]
        emit_add(lens)

    def remove(shape=None):
        n = len(sh)
        if n == 0:
            return add()
        idx = None if shape is None else _pick_removal(rng, shape, n, sh.covered)
        while idx is None:
            names = list(_SHAPE_WEIGHTS)
            w = np.array([_SHAPE_WEIGHTS[s] for s in names])
            shape = names[int(rng.choice(len(names), p=w / w.sum()))]
            idx = _pick_removal(rng, shape, n, sh.covered)
        ids = [sh.ids[i] for i in idx]
        rng.shuffle(ids)                                   # the call takes any order
        sh.remove(ids)
        gone.extend(ids)
        ops.append(dict(op="remove", ids=ids, shape=shape))

    while len(ops) < steps:
        if not queue:
            queue = list(motifs[int(rng.choice(len(motifs), p=weights / weights.sum()))][1])
        what = queue.pop(0)
        n = len(sh)
        if what == "fill":
            how = "rows" if rng.random() < 0.5 else "slots"
            for _ in range(3):
                if len(ops) < steps and len(sh) < TARGET_SLOTS and sh.rows_used < TARGET_ROWS:
                    add(fill=how)
        elif what == "add" or n == 0:
            add()
        elif what.startswith("remove"):
            remove(what.partition(":")[2] or None)
        elif what == "file":                               # make sure a file exists; no operation when it covers the bank
            if sh.covered < n:
                ops.append(dict(op="extend_ivf" if sh.covered else "build_ivf"))
                sh.covered = n
        elif what in ("build_ivf", "extend_ivf"):
            ops.append(dict(op=what))
            sh.covered = n
        elif what == "clear":
            gone.extend(sh.ids)
            sh.clear()
            ops.append(dict(op="clear"))
        elif what == "set_centroids":
            ops.append(dict(op="set_centroids", table=1 - sh.table))
            sh.set_centroids(1 - sh.table)
        elif what == "add_refused":
            ops.append(dict(op="add_refused", how="rows" if rng.random() < 0.5 else "slots", seed=int(rng.integers(1 << 30))))
        else:
            assert what in ("search", "stale_filter"), what
            ops.append(dict(op=what))
    del ops[steps:]
    _refusals(ops, kind, prefix)
    return ops


def capacity(ops):
    """(rows, slots): the largest totals the script ever holds."""
    rows = slots = cur_rows = cur_slots = 0
    lens = {}
    for op in ops:
        if op["op"] == "add":
            for p in op["passages"]:
                lens[p["id"]] = p["length"]
        elif op["op"] == "remove":
            for pid in op["ids"]:
                del lens[pid]
        elif op["op"] == "clear":
            lens.clear()
        cur_rows, cur_slots = sum(lens.values()), len(lens)
        rows, slots = max(rows, cur_rows), max(slots, cur_slots)
    return rows, slots


def _refusals(ops, kind, prefix):
    """Give every add_refused its passages, one more than what is free under the script's capacity: 130-row passages beyond the free
    rows, or (where few slots are free) one-row passages beyond the free slots."""
    cap_rows, cap_slots = capacity(ops)
    lens, k = {}, 0
    for op in ops:
        if op["op"] == "add":
            lens.update((p["id"], p["length"]) for p in op["passages"])
        elif op["op"] == "remove":
            for pid in op["ids"]:
                del lens[pid]
        elif op["op"] == "clear":
            lens.clear()
        elif op["op"] == "add_refused":
            free_rows, free_slots = cap_rows - sum(lens.values()), cap_slots - len(lens)
            if op["how"] == "slots" and free_slots < MAX_ADD:
                new = [1] * (free_slots + 1)
            else:
                op["how"] = "rows"
                new = [130] * (free_rows // 130 + 1)
            ids = [f"{prefix}refused{k}/{i}" for i in range(len(new))]
            via = "add_compressed" if KINDS[kind] else "add"
            op["passages"] = make_passages(kind, ids, new, 1000, seed=op["seed"], via=via)      # serial 1000: interior masks, no full one
            k += 1
