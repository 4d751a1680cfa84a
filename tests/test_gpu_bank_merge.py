"""GPU: rr_bank_merge_topk ("THE MERGED LIST", include/rerank_mi355.h) and what is built on it.

(a) the kernel, through rr_op_bank_merge_topk and rr_bank_merge_topk, equals the host definition rr_util_bank_merge_topk byte for
    byte on the cases of tests/bank_merge_cases.py at 1, 3 and 17 queries, and from run to run;
(b) the PROPERTY: a corpus of 300 passages searched as three ranges of one bank, or as three banks of unequal size (one smaller than
    k), and merged, is the search of the one bank byte for byte: exact on fp16 and compressed banks, filtered, and both pruned forms
    with ncells = n_centroids and a large ndocs;
(c) search_banks against PassageBank.search of the one bank;
(d) the rerank where the passage lives: rerank_owned for the parts in turn, combine_owned and the head, against forward_passages on
    the one bank with the same candidate lists, bit for bit, NORMAL and MORES;
(e) the refusals that need a device: stream capture, a misaligned pointer, a full-context handle.
"""
import functools

import numpy as np
import pytest
import torch

import bank_merge_cases as MC
from test_gpu_li_scores import _engine as _bare_engine
from test_gpu_passage_bank import _int_args, _model
from test_gpu_plaid_bank import N_CENTROIDS, _codec

pytestmark = pytest.mark.gpu

IPOISON = 0x7b7b7b7b
N, LC, K = 300, 12, 8
SIZES = [100, 195, 5]                         # the third bank holds fewer than k passages
TWINS = range(93, 108)                        # identical passages on both sides of the border at 100: equal scores across parts
DARK = 50                                     # a fully masked passage


# ---- (a) the kernel against the host definition ----------------------------------------------------------------------------------
def _device_case(case):
    """The case's one block on the device and the addresses of its three arrays in it."""
    block = torch.from_numpy(case["block"].reshape(-1).copy()).cuda()
    at = lambda a: 0 if a is None else block.data_ptr() + (a.ctypes.data - case["block"].ctypes.data)
    return block, at(case["idx"]), at(case["sc"]), at(case["cnt"])


def _outputs(nq, k):
    return dict(indices=torch.full((nq, k), IPOISON, dtype=torch.int32, device="cuda"),
                scores=torch.full((nq, k), IPOISON, dtype=torch.int32, device="cuda"),
                counts=torch.full((nq,), IPOISON, dtype=torch.int32, device="cuda"),
                parts=torch.full((nq, k), IPOISON, dtype=torch.int32, device="cuda"))


def _call(fn, lead, case, ptrs, out):
    st = torch.cuda.current_stream().cuda_stream
    return fn(*lead, ptrs[0], ptrs[1], ptrs[2], case["part_stride"], case["count_stride"], case["P"], case["offsets"].ctypes.data,
              case["nq"], case["k_in"], case["k"], out["indices"].data_ptr(), out["scores"].data_ptr(), out["counts"].data_ptr(),
              out["parts"].data_ptr(), st)


def _host(lib, case):
    from test_bank_merge_cpu import run_util
    rc, want = run_util(lib, case)
    assert rc == 0
    return want


@pytest.mark.parametrize("nq", [1, 3, 17])
def test_kernel_equals_the_host_definition_byte_for_byte(nq):
    eng = _bare_engine(64)
    lib = eng.lib
    for case in MC.cases(nq):
        want = _host(lib, case)
        block, *ptrs = _device_case(case)
        runs = []
        for fn, lead in ((lib.rr_op_bank_merge_topk, ()), (lib.rr_bank_merge_topk, (eng.h,)), (lib.rr_bank_merge_topk, (eng.h,))):
            out = _outputs(nq, case["k"])
            assert _call(fn, lead, case, ptrs, out) == 0, (case["name"], lib.rr_last_error(eng.h))
            torch.cuda.synchronize()
            runs.append({n: v.cpu().numpy() for n, v in out.items()})
        for got in runs:
            for n in ("counts", "indices", "scores", "parts"):
                assert np.array_equal(got[n].view(np.int32), np.asarray(want[n]).view(np.int32)), f"{case['name']}, nq {nq}: {n}"
        assert torch.equal(block.cpu(), torch.from_numpy(case["block"].reshape(-1))), "the inputs are read only"


def test_engine_method_over_tensors_and_strided_views():
    eng = _bare_engine(64)
    case = MC.make_case("3 x 5", 3, 5, 4, 3, 21)
    want = _host(eng.lib, case)
    block = torch.from_numpy(case["block"].copy()).cuda()                # [P, stride]
    w, nq, k_in = 15, 3, 5
    idx, sc, cnt = block[:, :w].unflatten(1, (nq, k_in)), block[:, w:2 * w].view(torch.float32).unflatten(1, (nq, k_in)), block[:, 2 * w:2 * w + nq]
    viewed = eng.bank_merge_topk(idx, sc, cnt, case["offsets"], 4, part_stride=block.shape[1], count_stride=block.shape[1], want_parts=True)
    tight = eng.bank_merge_topk(idx.contiguous(), sc.contiguous(), cnt.contiguous(), case["offsets"], 4, want_parts=True)
    torch.cuda.synchronize()
    for got in (viewed, tight):
        for n in ("counts", "indices", "scores", "parts"):
            assert np.array_equal(got[n].cpu().numpy().view(np.int32), np.asarray(want[n]).view(np.int32)), n
    assert "parts" not in eng.bank_merge_topk(idx.contiguous(), sc.contiguous(), None, case["offsets"], 4)
    with pytest.raises(AssertionError):
        eng.bank_merge_topk(idx.contiguous(), sc.contiguous(), None, case["offsets"], 6)
    with pytest.raises(NotImplementedError):
        big = torch.zeros((3, 1, 2731), dtype=torch.int32, device="cuda")
        eng.bank_merge_topk(big, big.float(), None, case["offsets"], 1)


# ---- (b), (c), (d): a corpus as one bank and as three ---------------------------------------------------------------------------
TWIN_ROWS = 6


def _lengths():
    gen = torch.Generator().manual_seed(77)
    lens = torch.randint(1, LC + 1, (N,), generator=gen).tolist()
    for i in TWINS:
        lens[i] = TWIN_ROWS
    return lens


def _masks(lens):
    cm = (torch.arange(LC)[None, :] < torch.tensor(lens)[:, None]).float()
    cm[DARK] = 0.0
    return cm


def _ids(a, b):
    return [f"p{i}" for i in range(a, b)]


OFF = [0] + [int(x) for x in np.cumsum(SIZES)]


@functools.lru_cache(maxsize=None)
def _world(name):
    """(model, the one fp16 bank, the three fp16 banks, the one compressed bank, the three compressed banks) for a fixture."""
    m, g = _model(name)
    eng = m.engine
    D = int(eng.arch["li_dim"])
    lens = _lengths()
    gen = torch.Generator().manual_seed(5)
    li = torch.nn.functional.normalize(torch.randn(N, LC, D, generator=gen), dim=-1)
    q, _, qm, _ = _int_args(g)
    q3, qm3 = torch.cat([q, q[:1].flip(1)]), torch.cat([qm, qm[:1].flip(1)])
    for i in TWINS:                                                     # the first rows of query 0 themselves: its best passages, all equal
        li[i] = 0.0
        li[i, :TWIN_ROWS] = torch.nn.functional.normalize(q3[0, :TWIN_ROWS].float().cpu(), dim=-1)
    cm = _masks(lens)

    def fp16(a, b):
        bank = eng.create_bank(sum(lens[a:b]) + 4, b - a + 1)
        bank.add(_ids(a, b), li[a:b], cm[a:b])
        return bank
    codec = _codec(D, 2)
    first = [0] + [int(x) for x in np.cumsum(lens)]
    ggen = torch.Generator().manual_seed(9)
    codes = torch.randint(0, N_CENTROIDS, (first[-1],), generator=ggen, dtype=torch.int32)
    res = torch.randint(0, 256, (first[-1], codec.residual_bytes), generator=ggen, dtype=torch.uint8)
    t0 = TWINS[0]
    for i in TWINS:
        codes[first[i]:first[i + 1]] = codes[first[t0]:first[t0 + 1]]
        res[first[i]:first[i + 1]] = res[first[t0]:first[t0 + 1]]
    mask = torch.cat([cm[i, :lens[i]] for i in range(N)]).to(torch.uint8)

    def plaid(a, b):
        bank = eng.create_bank(first[b] - first[a] + 4, b - a + 1, codec=codec)
        bank.add_compressed(_ids(a, b), codes[first[a]:first[b]], res[first[a]:first[b]], lens[a:b], mask=mask[first[a]:first[b]])
        return bank
    cuts = list(zip(OFF[:-1], OFF[1:]))
    return dict(model=m, eng=eng, q=q3, qm=qm3, one=fp16(0, N), three=[fp16(a, b) for a, b in cuts], pone=plaid(0, N),
                pthree=[plaid(a, b) for a, b in cuts])


def _merge_ranges(eng, search, k):
    """Form 1: `search(first, count, k_local)` over the three ranges of the one bank, made local, padded, merged."""
    nq = None
    parts = []
    for a, b in zip(OFF[:-1], OFF[1:]):
        kl = min(k, b - a)
        r = search(a, b - a, kl)
        nq = r["indices"].shape[0]
        idx = torch.full((nq, k), -1, dtype=torch.int32, device="cuda")
        sc = torch.full((nq, k), float("-inf"), device="cuda")
        idx[:, :kl] = torch.where(r["indices"] >= 0, r["indices"] - a, r["indices"])
        sc[:, :kl] = r["scores"]
        cnt = r["counts"] if "counts" in r else torch.full((nq,), kl, dtype=torch.int32, device="cuda")
        parts.append((idx, sc, cnt))
    return eng.bank_merge_topk(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), torch.stack([p[2] for p in parts]),
                               OFF, k)


def _merge_banks(eng, banks, q, k, plaid=None):
    from rmr_amd.passage_bank import search_bank_part
    parts = [search_bank_part(eng, b, q, k, plaid) for b in banks]
    assert [int(p["counts"][0]) for p in parts] == [min(k, len(b)) for b in banks]
    return eng.bank_merge_topk(torch.stack([p["indices"] for p in parts]), torch.stack([p["scores"] for p in parts]),
                               torch.stack([p["counts"] for p in parts]), OFF, k, want_parts=True)


def _same(got, want, what, counts=None):
    torch.cuda.synchronize()
    assert torch.equal(got["indices"], want["indices"]), f"{what}: indices"
    assert torch.equal(got["scores"].view(torch.int32), want["scores"].view(torch.int32)), f"{what}: scores"
    k = want["indices"].shape[1]
    want_c = want["counts"] if "counts" in want else torch.full_like(got["counts"], k)
    assert torch.equal(got["counts"], want_c), f"{what}: counts"


@pytest.mark.parametrize("kind", ["one", "pone"])
def test_property_exact_search_ranges_and_banks(kind):
    w = _world("int_tiny")
    eng, q, one = w["eng"], w["q"], w[kind]
    three = w["three" if kind == "one" else "pthree"]
    want = eng.bank_search(one, q, K)
    top = want["indices"].cpu()
    if kind == "one":                                                   # query 0's best are the twins, on both sides of the border
        assert top[0].tolist() == list(TWINS)[:K] and OFF[1] - TWINS[0] < K
    _same(_merge_ranges(eng, lambda a, n, kl: eng.bank_search(one, q, kl, first=a, count=n), K), want, f"{kind}: ranges")
    merged = _merge_banks(eng, three, q, K)
    _same(merged, want, f"{kind}: banks")
    parts = merged["parts"].cpu()
    assert torch.equal(parts, torch.bucketize(top, torch.tensor(OFF[1:]), right=True).to(torch.int32))
    # the whole order, so that the twins on both sides of the border and the fully masked passage take part
    whole = eng.bank_search(one, q, N)
    k_all = max(SIZES)
    deep = _merge_banks(eng, three, q, k_all)
    torch.cuda.synchronize()
    assert torch.equal(deep["indices"], whole["indices"][:, :k_all]) and torch.equal(deep["scores"], whole["scores"][:, :k_all])
    row = whole["indices"][0].tolist()
    at = sorted(row.index(i) for i in TWINS)
    assert at == list(range(at[0], at[0] + len(TWINS))) and [row[j] for j in at] == list(TWINS), "equal scores: ascending global index"


def test_property_filtered_search_with_one_absolute_filter():
    w = _world("int_tiny")
    eng, q, one = w["eng"], w["q"], w["one"]
    allowed = [f"p{i}" for i in (3, 40, 97, 98, 99, 100, 101, 102, 150, 151, 152, 200, 250, 296, 299)]
    filt = one.filter(allowed=allowed)
    for k in (K, 12):
        want = eng.bank_search_filtered(one, q, k, filt)
        got = _merge_ranges(eng, lambda a, n, kl: eng.bank_search_filtered(one, q, kl, filt, first=a, count=n), k)
        _same(got, want, f"filtered, k {k}")
    assert int(want["counts"].min()) == 12


@pytest.mark.parametrize("ivf", [False, True])
def test_property_plaid_with_every_cell_and_a_large_ndocs(ivf):
    from rmr_amd import PlaidSearch
    w = _world("int_tiny")
    eng, q, one, three = w["eng"], w["q"], w["pone"], w["pthree"]
    plaid = PlaidSearch(N_CENTROIDS, -1e30, 1024, ivf=ivf)
    if ivf:
        for b in three + [one]:
            b.build_ivf()
    want = eng.bank_search(one, q, K)
    _same(_merge_banks(eng, three, q, K, plaid), want, "pruned: banks")
    entry = eng.bank_search_plaid_ivf if ivf else eng.bank_search_plaid
    kw = dict(ncells=plaid.ncells, centroid_score_threshold=plaid.centroid_score_threshold, ndocs=plaid.ndocs)
    _same(_merge_ranges(eng, lambda a, n, kl: entry(one, q, kl, first=a, count=n, **kw), K), want, "pruned: ranges")


def test_search_banks_gives_the_ids_of_the_one_bank():
    from rmr_amd import search_banks
    w = _world("int_tiny")
    eng, q = w["eng"], w["q"]
    want_ids, want_sc = w["one"].search(eng, q, K)
    ids, sc, counts = search_banks(eng, w["three"], q, K)
    assert ids == want_ids and torch.equal(sc, want_sc) and counts.tolist() == [K] * q.shape[0]
    ids, sc, counts = search_banks(eng, [w["three"][2], w["three"][0]], q, K)      # another order of banks is another corpus order
    assert all(len(row) == K for row in ids) and set(ids[0]) <= set(_ids(0, 100) + _ids(295, 300))
    mixed_ids, _, _ = search_banks(eng, [w["three"][0], w["pthree"][1], w["three"][2]], q, K)   # an fp16 bank beside a compressed one
    assert all(len(row) == K for row in mixed_ids)
    empty = eng.create_bank(8, 2)
    ids2, sc2, _ = search_banks(eng, [w["three"][0], empty, w["three"][1], w["three"][2]], q, K)
    assert ids2 == want_ids and torch.equal(sc2, want_sc)


@pytest.mark.parametrize("name", ["int_tiny", "mores_tiny"])
def test_rerank_where_the_passage_lives_equals_the_one_bank(name):
    from rmr_amd.sharding import combine_owned, head_over_merged, rerank_owned
    w = _world(name)
    m, eng, q, qm = w["model"], w["eng"], w["q"], w["qm"]
    merged = _merge_banks(eng, w["three"], q, K)
    merged["part_offsets"] = [int(x) for x in OFF]
    parts = merged["parts"].cpu()
    assert len(set(parts.reshape(-1).tolist())) >= 2, "the winners live in more than one bank"
    buffers = torch.stack([rerank_owned(m, w["three"][p], merged, p, q, qm) for p in range(3)])
    none = dict(merged, parts=torch.full_like(merged["parts"], 1))
    assert not rerank_owned(m, w["three"][2], dict(none), 2, q, qm).any(), "a part that owns nothing runs no forward"
    logits = combine_owned(buffers, merged["parts"])
    counts = merged["counts"].tolist()
    got = head_over_merged(m, logits, counts, K)
    flat = [f"p{g}" for row, c in zip(merged["indices"].tolist(), counts) for g in row[:c]]
    m.bank = w["one"]
    want = m.forward_passages(q, qm, flat, None, candidates_per_query=counts, want_order=True)
    torch.cuda.synchronize()
    d = (got.logits - want.logits).abs().max().item()
    print(f"[{name}] rerank where the passage lives vs the one bank: max |dlogit| = {d:.3e}")
    assert torch.equal(got.logits.view(torch.int32), want.logits.view(torch.int32)), f"logits differ by {d:.3e}"
    assert torch.equal(got.order, want.order) and torch.equal(got.loss, want.loss) and torch.equal(got.list_loss, want.list_loss)


# ---- (e) the refusals that need a device -----------------------------------------------------------------------------------------
def test_refusals_that_need_a_device():
    from rmr_amd import _lib as L
    eng = _bare_engine(64)
    lib = eng.lib
    case = MC.make_case("3 x 5", 3, 5, 5, 3, 31)
    block, *ptrs = _device_case(case)
    out = _outputs(3, 5)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == IPOISON).all()) for t in out.values())
    # a misaligned device pointer
    assert _call(lib.rr_bank_merge_topk, (eng.h,), case, [ptrs[0], ptrs[1] + 2, ptrs[2]], out) == L.RR_ERR_BAD_ARG and untouched()
    assert b"misaligned" in lib.rr_last_error(eng.h)
    assert _call(lib.rr_op_bank_merge_topk, (), case, [ptrs[0] + 1, ptrs[1], ptrs[2]], out) == L.RR_ERR_BAD_ARG and untouched()
    # a full-context handle, as the searches refuse it
    full = _bare_engine(64, "full_context")
    assert _call(lib.rr_bank_merge_topk, (full.h,), case, ptrs, out) == L.RR_ERR_BAD_ARG and untouched()
    assert lib.rr_last_error(full.h) == b"rr_bank_merge_topk on a full-context model"
    # 8193 entries on the device entry points too
    wide = dict(case, k_in=2731, k=1, part_stride=1 << 30)
    assert _call(lib.rr_bank_merge_topk, (eng.h,), wide, ptrs, out) == L.RR_ERR_UNSUPPORTED and untouched()
    # a capturing stream: nothing but the probe enters the graph
    probe = torch.zeros(1, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        warm = _outputs(3, 5)
        assert _call(lib.rr_bank_merge_topk, (eng.h,), case, ptrs, warm) == 0
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            probe.add_(1.0)
            got = (_call(lib.rr_bank_merge_topk, (eng.h,), case, ptrs, out), lib.rr_last_error(eng.h))
            got_op = _call(lib.rr_op_bank_merge_topk, (), case, ptrs, out)
        graph.replay()
        torch.cuda.synchronize()
    assert got[0] == L.RR_ERR_BAD_ARG and b"rr_bank_merge_topk cannot be captured into a graph" in got[1] and got_op == L.RR_ERR_BAD_ARG
    assert probe.item() == 1.0 and untouched()
    assert _call(lib.rr_bank_merge_topk, (eng.h,), case, ptrs, out) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(out[n], warm[n]) for n in out)
