"""GPU: the inverted file of a compressed bank extended over added passages on the device (rr_bank_extend_ivf, include/rerank_mi355.h,
"THE INVERTED FILE").  CONTRACT: the bytes of a fresh rr_bank_build_ivf over every passage the bank holds.  The oracle is a fresh
build on a second bank filled with the same passages in one go, with rr_util_plaid_ivf / the numpy restatement over the full codes.

1. The boundaries of the merge (old list without a tail, tail without an old list, neither; tails of 1, 2, 4096, 4097 and above;
   an old list above one copy run under a shift that is no multiple of 4 entries; the long passage under a passage-index base).
2. Growth in steps.   3. Nothing to do, nothing to start from.   4. With removal.   5. The search.   6. The Python surface.
7. Refusals.   8. Many centroids.
Exact equality everywhere; no tolerance."""
import numpy as np
import pytest
import torch

from test_bank_ivf_cpu import ivf_lib, ivf_numpy
from test_gpu_bank_ivf import _both, _outputs, _raw, _read_raw
from test_gpu_bank_li_scores import POISON
from test_gpu_bank_search import IPOISON
from test_gpu_bank_search_plaid import CONFIGS, K, LEN_CYCLE, NDOCS, THRESHOLD, _build, _case, _codec, _near_queries, _topic_rows
from test_gpu_li_scores import _engine as _bare_engine

pytestmark = pytest.mark.gpu

COPY_RUN = 512                                                    # old postings a workgroup of the copy moves (csrc/bank_ivf.hip)
SORT_SLICE = 4096                                                 # entries one LDS sort holds


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rows(first, a, b):
    return slice(int(first[a]), int(first[b]))


def _empty_bank(eng, codec, lens):
    return eng.create_bank(sum(lens) + 4, len(lens) + 1, codec=codec)


def _add(bank, lens, codes, res, mask, a, b, **kw):
    """Passages a .. b - 1 of the full arrays, under the ids _build gives them."""
    first = np.concatenate([[0], np.cumsum(lens)])
    r = _rows(first, a, b)
    return bank.add_compressed([f"p{i}" for i in range(a, b)], codes[r], res[r], lens[a:b], mask=None if mask is None else mask[r], **kw)


def _assert_same_file(bank, fresh, what=""):
    """The file of `bank` equals the one `fresh` holds, byte for byte, info included.  Returns (offsets, pids, info)."""
    off, pids, info = _read_raw(bank)
    want_off, want_pids, want_info = _read_raw(fresh)
    assert info == want_info, f"{what}: info {info} for {want_info}"
    assert np.array_equal(off, want_off), f"{what}: offsets differ from list {int(np.flatnonzero(off != want_off)[0])} on"
    bad = np.flatnonzero(pids != want_pids)
    assert bad.size == 0, f"{what}: pids differ at {bad[:5].tolist()}: {pids[bad[:5]].tolist()} for {want_pids[bad[:5]].tolist()}"
    return off, pids, info


# ---- 1. the boundaries of the merge ---------------------------------------------------------------------------------------------------
P0, NEW, C1 = 1003, 4300, 400
EVERYWHERE, UNUSED, OLD_ONLY, NEW_ONLY, TAIL1, TAIL2 = 7, 123, 50, 51, 60, 61
LONG, LONG_ROWS, ALL_MASKED = P0 + 77, 150, P0 + 3000
_B1 = {}


def _merge_case():
    """1 003 old and 4 300 new passages of 1 .. 5 rows over 400 centroids.  EVERYWHERE is the first, unmasked row of every passage
    but the fully masked new passage ALL_MASKED: an old list of 1 003 (two copy runs) with a tail above one sort slice.  OLD_ONLY
    is held by old passages alone, NEW_ONLY by new ones alone, UNUSED by none, TAIL1 by one new passage and TAIL2 by two.  The new
    passage LONG holds 150 rows of ten codes in turn; every third passage of three rows or more has an interior masked row."""
    if not _B1:
        P = P0 + NEW
        lens = (torch.arange(P) * 3 % 5 + 1).tolist()
        lens[LONG] = LONG_ROWS
        codec = _codec(64, 2, C1)
        special = (EVERYWHERE, UNUSED, OLD_ONLY, NEW_ONLY, TAIL1, TAIL2)
        codes, res = _topic_rows(codec, lens, seed=P, topics_from=[c for c in range(C1) if c not in special])
        first = np.concatenate([[0], np.cumsum(lens)])
        mask = torch.ones(len(codes), dtype=torch.uint8)
        ten = torch.tensor([0, C1 - 1, 11, 12, 13, 200, 255, 256, 257, 300], dtype=torch.int32)
        codes[first[LONG]:first[LONG + 1]] = ten[torch.arange(LONG_ROWS) % 10]
        mask[first[LONG] + 5:first[LONG + 1]:7] = 0
        for p in range(0, P, 3):
            if lens[p] >= 3:
                mask[first[p] + 1] = 0
        codes[first[:-1]] = EVERYWHERE
        mask[first[:-1]] = 1
        last = lambda p: first[p + 1] - 1                         # the last row of a passage of two rows or more: unmasked, not its first
        two_up = [p for p in range(P) if 2 <= lens[p] <= 5 and p != ALL_MASKED]
        old2, new2 = [p for p in two_up if p < P0], [p for p in two_up if p >= P0]
        for p in old2[5:40:3]:
            codes[last(p)] = OLD_ONLY
        for p in new2[9:300:7]:
            codes[last(p)] = NEW_ONLY
        codes[last(new2[1000])] = TAIL1
        codes[last(new2[20])] = TAIL2
        codes[last(new2[2500])] = TAIL2
        mask[first[ALL_MASKED]:first[ALL_MASKED + 1]] = 0
        _B1.update(eng=_bare_engine(64), codec=codec, lens=lens, codes=codes, res=res, mask=mask)
    return _B1


def test_the_boundaries_of_the_merge_equal_a_fresh_build_and_the_definition():
    b = _merge_case()
    eng, codec, lens, codes, res, mask = (b[k] for k in ("eng", "codec", "lens", "codes", "res", "mask"))
    P = P0 + NEW
    fresh = _build(eng, codec, lens, codes, res, mask)
    fresh.build_ivf()
    bank = _empty_bank(eng, codec, lens)
    _add(bank, lens, codes, res, mask, 0, P0)
    bank.build_ivf()
    old_off, old_pids, old_info = _read_raw(bank)
    old_off, old_pids = old_off.copy(), old_pids.copy()
    assert old_info["passages_covered"] == P0
    _add(bank, lens, codes, res, mask, P0, P)                     # one call
    assert bank.ivf_info() == old_info
    info = bank.extend_ivf()
    off, pids, raw_info = _assert_same_file(bank, fresh, "extend")
    want_off, want_pids = ivf_numpy(codes.numpy(), mask.numpy(), lens, C1)
    host_off, host_pids = ivf_lib(codes.numpy(), mask.numpy(), lens, C1)
    assert np.array_equal(host_off, want_off) and np.array_equal(host_pids, want_pids), "the host definition"
    assert np.array_equal(off, want_off) and np.array_equal(pids, want_pids)
    lengths, old_len = np.diff(off), np.diff(old_off)
    tail = lengths - old_len
    assert info == raw_info == dict(passages_covered=P, postings=int(off[-1]), longest_list=int(lengths.max()))
    # the fixture bites
    assert old_len[NEW_ONLY] == 0 and tail[NEW_ONLY] > 2, "an empty old list with a tail"
    assert old_len[OLD_ONLY] > 2 and tail[OLD_ONLY] == 0, "an old list without a tail"
    assert old_len[UNUSED] == 0 and tail[UNUSED] == 0, "neither"
    assert tail[TAIL1] == 1 and tail[TAIL2] == 2
    assert tail[EVERYWHERE] == NEW - 1 > SORT_SLICE and (tail[np.arange(C1) != EVERYWHERE] <= SORT_SLICE).all()
    shift = off[:-1] - old_off[:-1]
    assert old_len[EVERYWHERE] == P0 > COPY_RUN and shift[EVERYWHERE] % 4 != 0, "an old list above one copy run, moved off its alignment"
    for m in (0, 1, 2, 3):                                        # every relative alignment of the copy on lists long enough for 16-byte accesses
        assert ((shift % 4 == m) & (shift > 0) & (old_len >= 8)).any(), f"no old list of 8 entries under a shift of {m} mod 4"
    assert P0 % 4 and P0 % 32
    assert ALL_MASKED not in pids.tolist() and mask[int(np.cumsum(lens)[LONG - 1]) + 5] == 0
    for c in (0, C1 - 1, 256):
        lst = pids[off[c]:off[c + 1]].tolist()
        assert lst.count(LONG) == 1 and lst == sorted(lst)
    assert np.array_equal(pids[off[EVERYWHERE]:off[EVERYWHERE] + P0], old_pids[old_off[EVERYWHERE]:old_off[EVERYWHERE + 1]])
    # the same bytes from run to run: a second bank, grown the same way
    again = _empty_bank(eng, codec, lens)
    _add(again, lens, codes, res, mask, 0, P0)
    again.build_ivf()
    _add(again, lens, codes, res, mask, P0, P)
    again.extend_ivf()
    _assert_same_file(again, bank, "two extends")


def test_tails_of_exactly_one_sort_slice_and_one_more():
    """Ten old passages; 4 097 new ones of two rows: centroid 3 in the first 4 096 of them, centroid 5 in all."""
    eng, codec = _bare_engine(64), _codec(64, 2, 16)
    old, new = 10, SORT_SLICE + 1
    lens = [2] * (old + new)
    codes, res = _topic_rows(codec, lens, seed=4097, topics_from=[8, 9, 10, 11])
    codes[2 * old::2] = 3
    codes[2 * old + 1::2] = 5
    codes[-2] = 9
    fresh = _build(eng, codec, lens, codes, res, None)
    fresh.build_ivf()
    bank = _empty_bank(eng, codec, lens)
    _add(bank, lens, codes, res, None, 0, old)
    bank.build_ivf()
    _add(bank, lens, codes, res, None, old, old + new)
    bank.extend_ivf()
    off, pids, _ = _assert_same_file(bank, fresh)
    lengths = np.diff(off)
    assert lengths[3] == SORT_SLICE and lengths[5] == SORT_SLICE + 1
    want_off, want_pids = ivf_lib(codes.numpy(), None, lens, 16)
    assert np.array_equal(off, want_off) and np.array_equal(pids, want_pids)


# ---- 2. growth in steps --------------------------------------------------------------------------------------------------------------
def _cycle_case(P, C, seed, nbits=4):
    eng, codec = _bare_engine(64), _codec(64, nbits, C)
    lens = [LEN_CYCLE[i % len(LEN_CYCLE)] for i in range(P)]
    codes, res = _topic_rows(codec, lens, seed=seed)
    masks = [torch.ones(ln, dtype=torch.uint8) for ln in lens]
    for m in masks[::2]:
        m[2::3] = 0                                               # interior masked rows; every passage keeps an unmasked row
    return eng, codec, lens, codes, res, torch.cat(masks)


def test_growth_in_steps_equals_a_fresh_build_after_every_step():
    steps = [200, 201, 264, 964]
    eng, codec, lens, codes, res, mask = _cycle_case(steps[-1], 64, seed=21)
    bank, lazy = _empty_bank(eng, codec, lens), _empty_bank(eng, codec, lens)
    for b in (bank, lazy):
        _add(b, lens, codes, res, mask, 0, steps[0])
        assert b.build_ivf()["passages_covered"] == steps[0]
    for a, n in zip(steps[:-1], steps[1:]):
        _add(bank, lens, codes, res, mask, a, n)
        _add(lazy, lens, codes, res, mask, a, n)                  # no extend in between
        assert bank.extend_ivf()["passages_covered"] == n
        first = np.concatenate([[0], np.cumsum(lens)])
        fresh = _build(eng, codec, lens[:n], codes[:first[n]], res[:first[n]], mask[:first[n]])
        fresh.build_ivf()
        off, pids, _ = _assert_same_file(bank, fresh, f"{n} passages")
        if n == steps[-1]:
            want_off, want_pids = ivf_lib(codes.numpy(), mask.numpy(), lens, 64)
            assert np.array_equal(off, want_off) and np.array_equal(pids, want_pids)
    assert lazy.ivf_info()["passages_covered"] == steps[0]
    lazy.extend_ivf()
    _assert_same_file(lazy, bank, "one extend after three adds")


# ---- 3. nothing to do, and nothing to start from -------------------------------------------------------------------------------------
def test_a_file_that_covers_the_bank_is_left_alone_and_no_file_means_a_build():
    eng, codec, lens, codes, res, mask = _cycle_case(120, 64, seed=31)
    fresh = _build(eng, codec, lens, codes, res, mask)
    fresh.build_ivf()
    off, pids, info = _read_raw(fresh)
    off, pids = off.copy(), pids.copy()
    assert fresh.lib.rr_bank_extend_ivf(fresh.h, _stream()) == 0
    assert fresh.extend_ivf() == info
    again_off, again_pids, again_info = _read_raw(fresh)
    assert np.array_equal(again_off, off) and np.array_equal(again_pids, pids) and again_info == info
    bank = _build(eng, codec, lens, codes, res, mask)
    assert bank.ivf_info()["passages_covered"] == 0
    assert bank.extend_ivf() == info                              # no file: the build
    _assert_same_file(bank, fresh, "an extend without a file")


# ---- 4. with removal ------------------------------------------------------------------------------------------------------------------
def test_after_a_removal_the_extend_equals_a_fresh_build_over_the_survivors():
    eng, codec, lens, codes, res, mask = _cycle_case(460, 64, seed=41)
    first = np.concatenate([[0], np.cumsum(lens)])
    bank = _empty_bank(eng, codec, lens)
    _add(bank, lens, codes, res, mask, 0, 300)
    bank.build_ivf()
    _add(bank, lens, codes, res, mask, 300, 400)
    gone = list(range(3, 300, 30)) + list(range(301, 400, 10))    # ten of the covered prefix, ten behind it
    assert len(gone) == 20
    bank.remove([f"p{i}" for i in gone])
    assert bank.ivf_info()["passages_covered"] == 290 and len(bank) == 380, "the file covers the survivors of the old prefix"

    def fresh_over(keep):
        rows = torch.cat([torch.arange(first[p], first[p + 1]) for p in keep])
        f = _build(eng, codec, [lens[p] for p in keep], codes[rows], res[rows], mask[rows])
        f.build_ivf()
        return f
    keep = [p for p in range(400) if p not in set(gone)]
    assert bank.extend_ivf()["passages_covered"] == 380
    _assert_same_file(bank, fresh_over(keep), "after the removal")
    _add(bank, lens, codes, res, mask, 400, 460)
    assert bank.ivf_info()["passages_covered"] == 380
    assert bank.extend_ivf()["passages_covered"] == 440
    _assert_same_file(bank, fresh_over(keep + list(range(400, 460))), "after the second add")


# ---- 5. the search --------------------------------------------------------------------------------------------------------------------
def test_the_search_refuses_before_the_extend_and_equals_the_scan_path_after_it():
    from rmr_amd import _lib as L
    name, Lq, Lqc, ncells = CONFIGS[3]                            # A, Lq 32, 20 coarse tokens, two cells
    eng, codec, _, q, codes, mask, lens = _case(name, Lq)[:7]
    codes, mask = torch.from_numpy(codes), torch.from_numpy(mask)
    gen = torch.Generator().manual_seed(5)
    res = torch.randint(0, 256, (len(codes), codec.residual_bytes), generator=gen, dtype=torch.uint8)
    half = len(lens) // 2
    bank = _empty_bank(eng, codec, lens)
    _add(bank, lens, codes, res, mask, 0, half)
    bank.build_ivf()
    _add(bank, lens, codes, res, mask, half, len(lens))
    kw = dict(Lqc=Lqc, ncells=ncells, thr=THRESHOLD, ndocs=NDOCS)
    out = _outputs(q.shape[0], K)
    assert _raw("rr_bank_search_plaid_ivf", eng, bank, q, out, K, **kw) == L.RR_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out[0] == IPOISON).all() and (out[1] == POISON).all() and (out[2] == IPOISON).all(), "a refused call writes nothing"
    bank.extend_ivf()
    gi, gs, gc = _both(eng, bank, q, K, **kw)
    assert gc.tolist() == [K] * q.shape[0]
    _both(eng, bank, q, K, first=half - 7, n=len(lens) - half + 3, **kw)


def test_a_query_whose_best_passages_are_all_new():
    """Old passages hold centroids 0 .. 31, new ones 32 .. 63; the queries lie near centroids of the upper half."""
    eng, codec = _bare_engine(64), _codec(64, 8, 64)
    old, new, k = 90, 70, 6
    lens = [LEN_CYCLE[i % len(LEN_CYCLE)] for i in range(old + new)]
    first = np.concatenate([[0], np.cumsum(lens)])
    lo, _ = _topic_rows(codec, lens[:old], seed=51, topics_from=list(range(32)))
    hi, _ = _topic_rows(codec, lens[old:], seed=52, topics_from=list(range(32, 64)))
    codes = torch.cat([lo, hi])
    gen = torch.Generator().manual_seed(53)
    res = torch.randint(0, 256, (len(codes), codec.residual_bytes), generator=gen, dtype=torch.uint8)
    bank = _empty_bank(eng, codec, lens)
    _add(bank, lens, codes, res, None, 0, old)
    bank.build_ivf()
    _add(bank, lens, codes, res, None, old, old + new)
    bank.extend_ivf()
    pick = 32 + torch.randint(0, 32, (2, 12), generator=gen)
    q = torch.nn.functional.normalize(codec.centroids[pick].float() + 0.3 * torch.randn(2, 12, 64, generator=gen) / 8.0, dim=-1).cuda()
    gi, gs, gc = _both(eng, bank, q, k, ncells=2, thr=0.3, ndocs=32)
    assert gc.tolist() == [k, k] and int(gi.min()) >= old, f"best passages {gi.tolist()} are not all behind the first {old}"


# ---- 6. the Python surface -----------------------------------------------------------------------------------------------------------
def test_the_keyword_on_an_add_and_the_saved_index(tmp_path):
    from test_gpu_bank_export import _bank
    b = _bank()
    eng, codec, lens, codes, res, mask = (b[k] for k in ("eng", "codec", "lens", "codes", "res", "mask"))
    P, old = len(lens), 171
    bank, twin = _empty_bank(eng, codec, lens), _empty_bank(eng, codec, lens)
    for bk in (bank, twin):
        _add(bk, lens, codes, res, mask, 0, old)
        bk.build_ivf()
    _add(twin, lens, codes, res, mask, old, P)
    _add(bank, lens, codes, res, mask, old, P - 40)
    assert bank.ivf_info()["passages_covered"] == old            # the default: today's behaviour
    _add(bank, lens, codes, res, mask, P - 40, P - 20, extend_ivf=True)
    assert bank.ivf_info()["passages_covered"] == len(bank) == P - 20
    assert eng.bank_extend_ivf(bank) == bank.ivf_info()
    _add(bank, lens, codes, res, mask, P - 20, P)
    assert bank.ivf_info()["passages_covered"] == P - 20 < len(bank)             # short coverage at the save
    twin.build_ivf()
    d1, d2 = str(tmp_path / "extended"), str(tmp_path / "built")
    bank.save_plaid_index(d1, chunk_passages=64)
    twin.save_plaid_index(d2, chunk_passages=64)
    assert bank.ivf_info()["passages_covered"] == P
    with open(d1 + "/ivf.pid.pt", "rb") as f1, open(d2 + "/ivf.pid.pt", "rb") as f2:
        assert f1.read() == f2.read(), "ivf.pid.pt after an extend and after a build"
    from rmr_amd import read_plaid_index
    loaded = eng.create_bank(int(mask.sum()) + 4 + sum(lens[:5]), P + 6, codec=read_plaid_index(d1)[0])
    _add(loaded, lens, codes, res, mask, 0, 5)
    loaded.build_ivf()
    assert loaded.load_plaid_index(d1, passage_ids=[f"q{i}" for i in range(P)]) == P
    assert loaded.ivf_info()["passages_covered"] == 5            # the default
    loaded.clear()
    _add(loaded, lens, codes, res, mask, 0, 5)
    loaded.build_ivf()
    assert loaded.load_plaid_index(d1, passage_ids=[f"q{i}" for i in range(P)], extend_ivf=True) == P
    assert loaded.ivf_info()["passages_covered"] == len(loaded) == P + 5


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_in_the_order_of_the_build_leave_the_file_alone():
    from rmr_amd import _lib as L
    eng, codec, lens, codes, res, mask = _cycle_case(60, 64, seed=71)
    lib = eng.lib
    assert lib.rr_bank_extend_ivf(None, None) == L.RR_ERR_BAD_ARG
    plain = eng.create_bank(64, 4)
    plain.add(["a", "b"], torch.nn.functional.normalize(torch.randn(2, 8, 64), dim=-1), torch.ones(2, 8), lengths=[8, 3])
    assert lib.rr_bank_extend_ivf(plain.h, _stream()) == L.RR_ERR_UNSUPPORTED and b"fp16 bank" in lib.rr_bank_last_error(plain.h)
    with pytest.raises(NotImplementedError):
        plain.extend_ivf()
    empty = eng.create_bank(64, 4, codec=codec)
    assert lib.rr_bank_extend_ivf(empty.h, _stream()) == L.RR_ERR_BAD_SHAPE
    with pytest.raises(ValueError):
        empty.extend_ivf()
    bank = _empty_bank(eng, codec, lens)
    _add(bank, lens, codes, res, mask, 0, 40)
    bank.build_ivf()
    _add(bank, lens, codes, res, mask, 40, 60)                    # a file over a prefix: an extend would have work to do
    off, pids, info = _read_raw(bank)
    off, pids = off.copy(), pids.copy()
    probe = torch.zeros(1, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            probe.add_(1.0)
            rc = lib.rr_bank_extend_ivf(bank.h, _stream())
            msg = lib.rr_bank_last_error(bank.h)
        graph.replay()
        torch.cuda.synchronize()
    assert rc == L.RR_ERR_BAD_ARG and b"captured" in msg and b"rr_bank_extend_ivf" in msg and probe.item() == 1.0
    again_off, again_pids, again_info = _read_raw(bank)
    assert again_info == info and info["passages_covered"] == 40
    assert np.array_equal(again_off, off) and np.array_equal(again_pids, pids), "the refused extend left the file"
    assert bank.extend_ivf()["passages_covered"] == 60            # and what is right is taken


# ---- 8. many centroids ---------------------------------------------------------------------------------------------------------------
def test_sixty_five_thousand_centroids_and_nearly_every_list_empty():
    C, old, new = 65536, 2000, 2000
    eng, codec = _bare_engine(64), _codec(64, 2, C)
    lens = (torch.arange(old + new) * 3 % 5 + 1).tolist()
    gen = torch.Generator().manual_seed(C)
    codes = torch.randint(0, C, (sum(lens),), generator=gen, dtype=torch.int32)
    res = torch.randint(0, 256, (len(codes), codec.residual_bytes), generator=gen, dtype=torch.uint8)
    codes[0], codes[-1] = 0, C - 1                                # the first and the last list
    fresh = _build(eng, codec, lens, codes, res, None)
    fresh.build_ivf()
    bank = _empty_bank(eng, codec, lens)
    _add(bank, lens, codes, res, None, 0, old)
    bank.build_ivf()
    _add(bank, lens, codes, res, None, old, old + new)
    bank.extend_ivf()
    off, pids, info = _assert_same_file(bank, fresh)
    want_off, want_pids = ivf_lib(codes.numpy(), None, lens, C)
    assert np.array_equal(off, want_off) and np.array_equal(pids, want_pids)
    assert (np.diff(off) == 0).sum() > C * 3 // 4 and pids[0] == 0 and pids[-1] == old + new - 1
