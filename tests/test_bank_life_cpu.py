"""CPU: the scripts of tests/bank_life.py bite.  tests/test_gpu_bank_life.py checks a lived bank after every step of these scripts;
it can only find what the scripts reach.  Here every script the GPU test runs (SEEDS, STEPS) is replayed on the Shadow alone and the
situations a long-lived bank has to get right are COUNTED, per kind over its seeds; a situation that never occurs fails the test,
with the counts of all of them in the message.  The seeds are chosen here so that every count is at least 1.

The two situations about the searches' cached table (two removals in a row; search, remove, add) are counted only where the GPU
test lets them reach the bank unbroken: not where its comparison of every eighth step (EVERY) or the acceptance search behind a
removal that a stale filter waited for stands between the operations (tests/test_gpu_bank_life.py, THE CUT TABLE).

An fp16 bank has no inverted file: the situations about the file are asked of the kinds that hold codes (FILE_ONLY): the compressed
kinds and `coded`, an fp16 bank with a centroid table.  The situations about set_centroids are asked of `coded` alone (CODED_ONLY).

The scripts of the kinds that were here before `coded` are held to digests taken before it came (SCRIPT_DIGESTS): the generator's
stream of a kind is fixed (bank_life.STREAMS), so a new kind changes none of them and the chosen SEEDS stay valid.

The same scripts also drive BankTable, the host table of a PassageBank, which is pure Python: after every step its ids, its lengths
and what lookup returns are the Shadow's."""
import numpy as np
import pytest

import bank_life as BL
from rmr_amd import BankTable

STEPS = 40
EVERY = 8                                                  # the GPU test compares with a fresh bank, and so searches, every eighth step
SEEDS = {"fp16": (0, 1, 2), "plaid2": (0, 1, 2), "plaid8": (0, 1, 12), "coded": (0, 1, 12)}
WINDOWED = {kind: seeds[1] for kind, seeds in SEEDS.items()}             # the seed that runs with bank_move_kb = 4 on the device
PAIRS = {"plaid2": (0, 1), "plaid8": (0, 1), "coded": (0, 1)}                           # two lived banks searched as one: the seeds of A1 and A2

SITUATIONS = (
    "two removals with nothing between them",
    "a removal inside the covered prefix after an extend_ivf",
    "a removal only behind the prefix: the coverage is unchanged",
    "the whole prefix removed with passages left behind it: the file is dropped",
    "every passage removed, then an add",
    "clear with a file, then add and extend_ivf",
    "extend_ivf with nothing to do",
    "a search directly before a remove and an add directly after it",
    "an add that fits only in rows a removal freed",
    "an add that fits only in a slot a removal freed",
    "a refused add",
    "a stale filter after a remove",
    "a stale filter after a clear",
    "at least 40 passages held",
    "a list of the expected file with old and new postings",
    "set_centroids with a file in place",
    "an add directly behind a set_centroids",
    "extend_ivf behind a set_centroids: with no file left, the extend is the build",
    "a removal between two set_centroids",
    "a filter built before a set_centroids and used behind it",
)
FILE_ONLY = {SITUATIONS[i] for i in (1, 2, 3, 5, 6, 14)}
CODED_ONLY = {SITUATIONS[i] for i in (15, 16, 17, 18, 19)}


def asked_of(kind):
    """The situations asked of a kind: those about the file of the kinds that hold codes, those about set_centroids of the coded kind."""
    return [s for s in SITUATIONS if (BL.holds_codes(kind) or s not in FILE_ONLY) and (kind == "coded" or s not in CODED_ONLY)]


def compress_with(kind):
    """The host definition of the compressed row (PlaidCodec.compress, rr_util_plaid_compress_rows) as bank_life.materialise takes it."""
    import torch
    codec = BL.codec_of(kind)

    def compress(x):
        codes, res = codec.compress(torch.from_numpy(np.ascontiguousarray(x)))
        return codes.numpy(), res.numpy()
    return compress


def ops_of(seed, kind, prefix="p"):
    ops = BL.script(seed, kind, STEPS, prefix)
    return BL.materialise(ops, compress_with(kind)) if BL.KINDS[kind] else ops


def step(sh, op):
    """One operation on the Shadow; what the mutator returns (a refused add: the MemoryError)."""
    what = op["op"]
    if what == "add":
        return sh.add(op["passages"])
    if what == "add_refused":
        try:
            sh.add(op["passages"])
        except MemoryError as ex:
            return ex
        raise AssertionError("the Shadow took an add that was to be refused")
    if what == "remove":
        return sh.remove(op["ids"])
    if what in ("build_ivf", "extend_ivf", "clear", "search"):
        return getattr(sh, what)()
    if what == "set_centroids":
        return sh.set_centroids(op["table"])
    assert what == "stale_filter"
    return None


def count_situations(ops, kind):
    rows, slots = BL.capacity(ops)
    sh = BL.Shadow(kind, rows, slots)
    n = dict.fromkeys(SITUATIONS, 0)
    extended = False                         # the file in place was last made by an extend_ivf that had work to do
    pending = False                          # a filter waits for the next remove or clear
    freed_rows = freed_slots = 0             # by the removals directly before this operation
    tables_set = 0                           # set_centroids so far
    removed_since_set = no_file_since_set = False
    for i, op in enumerate(ops):
        what = op["op"]
        nxt = [o["op"] for o in ops[i + 1:i + 3]]
        held, covered, used = len(sh), sh.covered, sh.rows_used
        if what == "remove":
            idx = sorted(sh.ids.index(pid) for pid in op["ids"])
            inside = [j for j in idx if j < covered]
            unbroken = not pending and i % EVERY != EVERY - 1
            n[SITUATIONS[0]] += nxt[:1] == ["remove"] and unbroken
            n[SITUATIONS[1]] += bool(inside) and extended
            got = step(sh, op)
            if covered and not inside:
                assert sh.covered == covered
                n[SITUATIONS[2]] += 1
            if covered and len(inside) == covered and len(sh):
                assert sh.covered == 0
                n[SITUATIONS[3]] += 1
            n[SITUATIONS[4]] += len(sh) == 0 and nxt[:1] == ["add"]
            n[SITUATIONS[7]] += i > 0 and ops[i - 1]["op"] == "search" and nxt[:1] == ["add"] and unbroken
            n[SITUATIONS[11]] += pending
            pending = False
            removed_since_set = tables_set > 0
            freed_rows, freed_slots = freed_rows + got["rows_freed"], freed_slots + len(idx)
            extended = extended and sh.covered > 0
            continue
        if what == "add":
            new_rows = sum(p["length"] for p in op["passages"])
            n[SITUATIONS[8]] += freed_rows > 0 and used + freed_rows + new_rows > rows
            n[SITUATIONS[9]] += freed_slots > 0 and held + freed_slots + len(op["passages"]) > slots
            n[SITUATIONS[16]] += i > 0 and ops[i - 1]["op"] == "set_centroids"
        elif what == "add_refused":
            n[SITUATIONS[10]] += 1
        elif what == "clear":
            n[SITUATIONS[5]] += covered > 0 and nxt == ["add", "extend_ivf"]
            n[SITUATIONS[12]] += pending
            pending, extended, no_file_since_set = False, False, False
        elif what == "build_ivf":
            extended = no_file_since_set = False
        elif what == "set_centroids":
            n[SITUATIONS[15]] += covered > 0
            n[SITUATIONS[18]] += removed_since_set
            n[SITUATIONS[19]] += pending and ops[i - 1]["op"] == "stale_filter"
            tables_set, removed_since_set, no_file_since_set, extended = tables_set + 1, False, True, False
        elif what == "extend_ivf":
            n[SITUATIONS[6]] += covered == held
            n[SITUATIONS[17]] += no_file_since_set and covered == 0 and held > 0
            no_file_since_set = False
            if 0 < covered < held:
                extended = True
            elif covered == 0:
                extended = False
        elif what == "stale_filter":
            assert held >= 1, "a filter needs a passage"
            pending = True
        step(sh, op)
        if what == "extend_ivf" and 0 < covered < held:
            pids, lengths = sh.expected_ivf()
            first = np.concatenate([[0], np.cumsum(lengths)])
            lists = [pids[first[c]:first[c + 1]] for c in range(sh.n_centroids)]
            n[SITUATIONS[14]] += any((l < covered).any() and (l >= covered).any() for l in lists)
        n[SITUATIONS[13]] = max(n[SITUATIONS[13]], int(len(sh) >= 40))
        freed_rows = freed_slots = 0
    assert sh.rows_used <= rows and len(sh) <= slots
    return n


@pytest.mark.parametrize("kind", sorted(SEEDS))
def test_every_situation_occurs_for_every_kind(kind):
    total = dict.fromkeys(SITUATIONS, 0)
    for seed in SEEDS[kind]:
        ops = ops_of(seed, kind)
        assert len(ops) == STEPS
        rows, slots = BL.capacity(ops)
        assert slots <= 60 and max(p["length"] for op in ops if op["op"] == "add" for p in op["passages"]) <= 130
        for name, c in count_situations(ops, kind).items():
            total[name] += c
    asked = asked_of(kind)
    counts = "; ".join(f"{s}: {total[s]}" for s in asked)
    print(f"[{kind}] {counts}")
    missing = [s for s in asked if total[s] < 1]
    assert not missing, f"{kind}, seeds {SEEDS[kind]}: never reached: {missing}.  Counts: {counts}"


@pytest.mark.parametrize("kind", sorted(SEEDS))
def test_scripts_are_deterministic_and_hold_what_the_issue_lists(kind):
    seed = SEEDS[kind][0]
    BL.script.cache_clear()
    a = ops_of(seed, kind)
    BL.script.cache_clear()
    b = ops_of(seed, kind)
    assert [o["op"] for o in a] == [o["op"] for o in b]
    for x, y in zip(a, b):
        assert x.get("ids") == y.get("ids")
        for p, q in zip(x.get("passages", []), y.get("passages", [])):
            assert p["id"] == q["id"] and all(np.array_equal(p[k], q[k]) for k in p if k != "id" and k != "length")
    shapes, vias, masked, full = set(), set(), 0, 0
    for seed in SEEDS[kind]:
        ops = ops_of(seed, kind)
        sh = BL.Shadow(kind, *BL.capacity(ops))
        for op in ops:
            if op["op"] == "remove":                         # what the removal IS in the bank it meets, whatever it was drawn as
                idx, n, cov = sorted(sh.ids.index(pid) for pid in op["ids"]), len(sh), sh.covered
                shapes.add("everything" if len(idx) == n else "leading" if idx[0] == 0 else
                           "trailing" if idx == list(range(idx[0], n)) else "interior" if idx[-1] < n - 1 else "any")
                if 0 < cov < n:
                    shapes.update({"behind_prefix"} if idx[0] >= cov else {"whole_prefix"} if idx == list(range(cov)) else ())
            step(sh, op)
            vias.add(op.get("via"))
            for p in op.get("passages", []):
                assert 1 <= p["length"] <= 130
                masked += bool(p["mask"].any() and not p["mask"].all())
                full += not p["mask"].any()
    want = set(BL.REMOVE_SHAPES) - {"any"} - (set() if BL.holds_codes(kind) else {"behind_prefix", "whole_prefix"})
    assert want <= shapes, f"removal shapes that never occur: {want - shapes}"
    assert masked >= 3 and full == len(SEEDS[kind]), "interior masked rows, and one fully masked passage per script"
    if BL.KINDS[kind]:
        assert {"add_compressed", "add_compress"} <= vias, "one add of every compressed script goes through add_compress"


@pytest.mark.parametrize("kind", sorted(SEEDS))
def test_bank_table_follows_the_shadow(kind):
    for seed in SEEDS[kind]:
        ops = ops_of(seed, kind)
        rows, slots = BL.capacity(ops)
        sh, table = BL.Shadow(kind, rows, slots), BankTable()
        for i, op in enumerate(ops):
            what = op["op"]
            got = step(sh, op)
            if what == "add":
                ids, lens = [p["id"] for p in op["passages"]], [p["length"] for p in op["passages"]]
                table.check_new(ids)
                assert table.append(ids, lens, first_index=got) == got
            elif what == "add_refused":
                assert isinstance(got, MemoryError)
                table.check_new([p["id"] for p in op["passages"]])           # the ids are new: the refusal is one of room alone
            elif what == "remove":
                idx = table.check_remove(op["ids"])
                assert table.remove(idx) == got["new_index"].tolist(), f"seed {seed} step {i}"
                with pytest.raises(KeyError):
                    table.lookup(op["ids"][:1])
            elif what == "clear":
                table.clear()
            assert table.ids == sh.ids and table.lengths == sh.lengths and len(table) == len(sh), f"seed {seed} step {i} {what}"
            if len(sh):
                order = list(reversed(sh.ids))
                idx, lens = table.lookup(order)
                assert idx.tolist() == list(range(len(sh) - 1, -1, -1)) and lens.tolist() == list(reversed(sh.lengths))
            assert all(pid in table for pid in sh.ids) and "nobody" not in table


# sha256 (16 hex digits) over the operations of script(seed, kind, STEPS, prefix), taken before the kind `coded` was added
SCRIPT_DIGESTS = {
    ("fp16", 0, "p"): "e8cecea8093b1219", ("fp16", 1, "p"): "609b50d26d0f344e", ("fp16", 2, "p"): "08ab96ce38ce29ae",
    ("plaid2", 0, "p"): "e5988697e4a9e8bc", ("plaid2", 0, "q"): "bd28d921a6a5c64d", ("plaid2", 1, "p"): "226d690dca315d19",
    ("plaid2", 1, "q"): "fb190a831ab833e4", ("plaid2", 2, "p"): "e47862d146296ed4", ("plaid8", 0, "p"): "e8d4913e0bb2b8f0",
    ("plaid8", 0, "q"): "bab570b569063516", ("plaid8", 1, "p"): "4190b5c607bdf3c9", ("plaid8", 1, "q"): "47a82228baab7f8e",
    ("plaid8", 12, "p"): "7ae4e14ab4f2a720",
}


def script_digest(ops):
    """Every field of every operation and passage; of an add_compress passage what the generator drew (x), not what materialise added."""
    import hashlib

    from test_coded_exact_cases_cpu import feed
    h = hashlib.sha256()
    for op in ops:
        for key in sorted(op):
            if key != "passages":
                h.update(key.encode())
                feed(h, op[key])
        for p in op.get("passages", []):
            for key in sorted(p):
                if not ("x" in p and key in ("codes", "res")):
                    h.update(key.encode())
                    feed(h, p[key])
    return h.hexdigest()[:16]


def test_the_scripts_of_the_earlier_kinds_are_unchanged():
    run = {(kind, seed, "p") for kind in ("fp16", "plaid2", "plaid8") for seed in SEEDS[kind]}
    run |= {(kind, seed, "q") for kind in ("plaid2", "plaid8") for seed in PAIRS[kind]}
    assert run == set(SCRIPT_DIGESTS), "every script the GPU test runs of the earlier kinds has its digest here"
    got = {key: script_digest(BL.script(key[1], key[0], STEPS, key[2])) for key in SCRIPT_DIGESTS}
    changed = sorted(key for key in got if got[key] != SCRIPT_DIGESTS[key])
    assert not changed, f"scripts that changed: {changed}"
    assert [BL.STREAMS[k] for k in ("fp16", "plaid2", "plaid8")] == [0, 1, 2] and len(set(BL.STREAMS.values())) == len(BL.KINDS)


def test_the_coded_kind_s_codes_are_the_host_definition_under_both_tables():
    """The Shadow's codes are a float64 argmax with a margin (bank_life._coded_rows); PlaidCodec.compress on the fp16 rows agrees."""
    import torch
    from rmr_amd import PlaidCodec
    rows = checked = 0
    for t, cen in enumerate(BL.tables()):
        codec = PlaidCodec(cen, torch.linspace(-0.1, 0.1, 256), 8, bucket_cutoffs=torch.linspace(-0.1, 0.1, 255))
        assert cen.shape == (BL.TABLE_SIZES[t], BL.D) and cen.dtype == torch.float16
        for seed in SEEDS["coded"]:
            for op in ops_of(seed, "coded"):
                for p in op.get("passages", []):
                    got = codec.compress(torch.from_numpy(p["rows"]).view(torch.float16))[0].numpy()
                    assert np.array_equal(got, p["codes2"][t]), f"table {t}, seed {seed}, passage {p['id']}"
                    rows, checked = rows + p["length"], checked + 1
    used = [set(np.concatenate([p["codes2"][t] for seed in SEEDS["coded"] for op in ops_of(seed, "coded") for p in op.get("passages", [])]).tolist())
            for t in range(2)]
    assert checked > 100 and [len(u) for u in used] == list(BL.TABLE_SIZES), f"{checked} passages, {rows} rows, centroids used {used}"


def test_set_centroids_on_the_shadow_switches_codes_drops_the_file_and_keeps_the_generation():
    ops = ops_of(SEEDS["coded"][0], "coded")
    sh = BL.Shadow("coded", *BL.capacity(ops))
    seen = 0
    for op in ops:
        gen, before = sh.generation, (sh.ids, sh.lengths, sh.table_current)
        step(sh, op)
        if op["op"] == "set_centroids":
            assert sh.table == op["table"] and sh.covered == 0 and sh.generation == gen and (sh.ids, sh.lengths, sh.table_current) == before
            assert sh.n_centroids == BL.TABLE_SIZES[sh.table]
            if len(sh):
                assert np.array_equal(sh.concat()[0], np.concatenate([p["codes2"][sh.table] for p in sh.passages]))
            seen += 1
    assert seen >= 2 and "nbits" not in sh.info() and "bytes_per_row" not in sh.info(), f"{seen} set_centroids"
