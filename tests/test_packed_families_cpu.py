"""CPU: the packed forwards of the joint and interaction reranker families — ABI surface (rr_forward_joint_packed,
rr_forward_interaction_packed, rr_head_joint), host-side packing (lengths -> segments, pack / scatter, fusion-score slicing)
and the drop-in classes' `packed_rows` routing, checked with a stub engine.  No compute calls here."""
import ctypes as C

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from rmr_amd import _lib
    return _lib.load()


# ---- ABI surface -------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_exported_and_bound(lib):
    from rmr_amd import _lib
    for name in ("rr_forward_joint_packed", "rr_forward_interaction_packed", "rr_head_joint"):
        assert hasattr(lib, name) and name in _lib.EXPORTED
        assert getattr(lib, name).restype is C.c_int


def test_null_handle_is_a_bad_argument(lib):
    from rmr_amd import _lib
    one = (C.c_int32 * 1)(1)
    assert lib.rr_forward_joint_packed(None, None, None, None, None, None, 1.0, 1, one, one, 8, 2, -1, None, None,
                                       None) == _lib.RR_ERR_BAD_ARG
    assert lib.rr_forward_interaction_packed(None, None, None, None, None, None, 1.0, 1, one, one, 8, 2, None, None,
                                             None) == _lib.RR_ERR_BAD_ARG
    assert lib.rr_head_joint(None, None, None, 1, 1, None, None, None, None) == _lib.RR_ERR_BAD_ARG


def test_constructors_fail_loudly_without_a_gpu(lib):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import rmr_amd
    with pytest.raises(RuntimeError):
        rmr_amd.RerankModel(dict(loss_fn="2H_BCE", packed_rows=True))
    with pytest.raises(RuntimeError):
        rmr_amd.InteractionRerankModel(dict(loss_fn="BCE", interaction_type="MORES", packed_rows=True))
    with pytest.raises(RuntimeError):
        rmr_amd.FullContextRerankModel(dict(loss_fn="BCE", packed_rows=True))


# ---- host packing ------------------------------------------------------------------------------------------------------
def test_joint_mask_lengths_give_the_expected_segments():
    from rmr_amd.pair_inputs import group_pairs_by_length, pair_lengths
    S, ql = 64, 8
    joint_len = [64, 61, 51, 42, 58, 46, 20]
    ids = torch.zeros(len(joint_len), S, dtype=torch.int64)
    am = torch.zeros_like(ids)
    for p, n in enumerate(joint_len):
        am[p, :5] = 1                       # query part: 5 real tokens, padded to ql ...
        am[p, ql:n] = 1                     # ... then the context tokens
        ids[p] = am[p] * (p + 7)
    lens = pair_lengths(ids, am)
    assert lens.tolist() == joint_len
    floor = max(ql + 1, min(S, 32))         # every segment keeps the query part and the mapping network's window
    order, seg_n, seg_len = group_pairs_by_length(lens.numpy(), S, 16, floor)
    assert seg_len == [32, 48, 64] and seg_n == [1, 2, 4]
    assert order.tolist() == [6, 3, 5, 0, 1, 2, 4]


def test_context_mask_lengths_give_the_expected_segments():
    from rmr_amd.pair_inputs import group_pairs_by_length, pair_lengths
    cm = torch.zeros(5, 40)
    for p, n in enumerate([12, 23, 22, 40, 1]):
        cm[p, :n] = 1
    cm[1, 10] = 0                           # a hole inside a context does not shorten it
    lens = pair_lengths(cm)
    assert lens.tolist() == [12, 23, 22, 40, 1]
    order, seg_n, seg_len = group_pairs_by_length(lens.numpy(), 40, 8, 1)
    assert seg_len == [8, 16, 24, 40] and seg_n == [1, 1, 2, 1]
    assert order.tolist() == [4, 0, 1, 2, 3]
    assert pair_lengths(torch.zeros(2, 6)).tolist() == [1, 1]          # an empty row still occupies one position


def test_pack_then_scatter_is_the_identity():
    from rmr_amd.pair_inputs import group_pairs_by_length, pack_rows, scatter_packed
    N, S, D = 9, 24, 3
    gen = torch.Generator().manual_seed(0)
    lens = torch.randint(1, S + 1, (N,), generator=gen)
    order_h, seg_n, seg_len = group_pairs_by_length(lens.numpy(), S, 8)
    order = torch.from_numpy(order_h)
    assert sorted(order.tolist()) == list(range(N))
    x = torch.arange(N * S * D, dtype=torch.float32).reshape(N, S, D)
    packed = pack_rows(x, order, seg_n, seg_len)
    assert packed.shape == (sum(n * s for n, s in zip(seg_n, seg_len)), D)
    r, o = 0, 0
    for n, s in zip(seg_n, seg_len):
        for i in range(n):
            p = int(order[o + i])
            assert lens[p] <= s
            assert torch.equal(packed[r: r + s], x[p, :s])
            r += s
        o += n
    # the logits come back in packed order: the scatter inverts the permutation
    assert torch.equal(scatter_packed(order.float(), order), torch.arange(N, dtype=torch.float32))
    v = torch.randn(N, generator=gen)
    assert torch.equal(scatter_packed(v.index_select(0, order), order), v)
    ids = torch.arange(N * S).reshape(N, S)                            # int64 rows pack the same way
    assert torch.equal(pack_rows(ids, order, seg_n, seg_len)[:seg_len[0]], ids[int(order[0]), :seg_len[0]])


def test_fusion_scores_are_sliced_and_stay_padded():
    from rmr_amd.pair_inputs import pack_fusion_scores
    N, S, ql, P = 4, 20, 5, 3
    s = torch.randn(N, S, ql + P)
    order = torch.tensor([2, 0, 3, 1])
    j = pack_fusion_scores(s, order, 2, S - ql)                         # joint: the context rows, padded axis kept
    assert j.shape == (N, S - ql, ql + P) and j.is_contiguous()
    for i, p in enumerate(order.tolist()):
        assert torch.equal(j[i], s[p, 2:2 + S - ql])
    Lc, Lq = 11, 6
    t = torch.randn(N, Lc, Lq)
    it = pack_fusion_scores(t, order)                                   # interaction: [N, Lc, Lq] whole
    assert it.shape == t.shape and torch.equal(it, t.index_select(0, order))


# ---- drop-in routing with a stub engine ----------------------------------------------------------------------------------
class _StubEngine:
    def __init__(self, arch):
        self.arch, self.device, self.calls = arch, torch.device("cpu"), []

    def _rec(self, name, N):
        def f(*a, **kw):
            self.calls.append((name, a, kw))
            return dict(logits=torch.zeros(N), logits2=torch.zeros(N), loss=torch.zeros(()), scores=None, order=None)
        return f

    def bind(self, N):
        for n in ("forward_ids", "forward_ids_packed", "forward_joint", "forward_joint_packed", "forward_interaction",
                  "forward_interaction_packed"):
            setattr(self, n, self._rec(n, N))
        return self


def _drop_in(cls, engine, **attrs):
    m = cls.__new__(cls)
    torch.nn.Module.__init__(m)
    m.engine = engine
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


@pytest.mark.parametrize("packed", [False, True])
def test_rerank_model_routing(packed):
    import rmr_amd
    Bq, K, ql, S = 2, 3, 4, 16
    eng = _StubEngine(dict(max_pos=S, loss_fn="2H_BCE")).bind(Bq * K)
    m = _drop_in(rmr_amd.RerankModel, eng, image_feature_fn=None, instruction_token_id=7, packed_rows=packed)
    q_ids, q_am = torch.ones(Bq, ql, dtype=torch.int64), torch.ones(Bq, ql, dtype=torch.int64)
    c_ids, c_am = torch.ones(Bq * K, S, dtype=torch.int64), torch.ones(Bq * K, S, dtype=torch.int64)
    feats = (torch.zeros(Bq, 8), torch.zeros(Bq, 2, 8))
    m(q_ids, q_am, None, c_ids, c_am, K - 1, image_features=feats, want_order=True)
    ((name, a, kw),) = eng.calls
    assert name == ("forward_joint_packed" if packed else "forward_joint")
    assert a[2:5] == (Bq, K, ql) and a[7] == 7
    assert kw == dict(preflmr_scores=None, fusion_multiplier=1.0, want_order=True)
    if packed:                              # pair_range slices stay padded
        eng.calls.clear()
        m(q_ids, q_am, None, c_ids, c_am, K - 1, image_features=feats, pair_range=(0, 2), want_loss=False)
        assert eng.calls[0][0] == "forward_joint"


@pytest.mark.parametrize("packed", [False, True])
def test_interaction_model_routing(packed):
    import rmr_amd
    Bq, K, Lq, Lc, D = 2, 3, 5, 9, 4
    eng = _StubEngine(dict(loss_fn="BCE")).bind(Bq * K)
    m = _drop_in(rmr_amd.InteractionRerankModel, eng, packed_rows=packed)
    q, c = torch.zeros(Bq, Lq, D), torch.zeros(Bq * K, Lc, D)
    qm, cm = torch.ones(Bq, Lq), torch.ones(Bq * K, Lc)
    m(q, c, K - 1, qm, cm, labels=[1.0, 0, 0, 1, 0, 0])
    ((name, a, kw),) = eng.calls
    assert name == ("forward_interaction_packed" if packed else "forward_interaction")
    assert a[0] is q and a[1] is c and a[2] is qm and a[3] is cm and a[4:6] == (Bq, K)
    assert kw == dict(preflmr_scores=None, fusion_multiplier=1.0)


@pytest.mark.parametrize("packed", [False, True])
def test_full_context_routing_and_host_lengths(packed):
    import rmr_amd
    from rmr_amd.pair_inputs import pair_lengths
    Bq, K, S = 1, 3, 12
    eng = _StubEngine(dict(loss_fn="BCE")).bind(Bq * K)
    enc = dict(input_ids=torch.zeros(Bq * K, S, dtype=torch.int64), attention_mask=torch.zeros(Bq * K, S, dtype=torch.int64),
               token_type_ids=torch.zeros(Bq * K, S, dtype=torch.int64))
    for p, n in enumerate([5, 12, 8]):
        enc["input_ids"][p, :n] = 3
        enc["attention_mask"][p, :n] = 1

    class Tok:                              # HF-style tokenizer stand-in: the pair encoding is given
        def encode(self, text, **kw):
            return [3]

        def decode(self, ids):
            return "x"

        def batch_encode_plus(self, pairs, **kw):
            return enc

    m = _drop_in(rmr_amd.FullContextRerankModel, eng, max_query_length=4, max_context_length=4, max_decoder_source_length=S,
                 query_tokenizer=Tok(), native_tokenizer=None, image_feature_fn=None, packed_rows=packed)
    m.forward(["q"], None, ["a", "b", "c"], K - 1)
    ((name, a, kw),) = eng.calls
    assert name == ("forward_ids_packed" if packed else "forward_ids")
    assert a[3:5] == (Bq, K) and a[5] is None and a[7] is None
    if packed:                              # the tokenizer's lengths travel as host data: no device -> host copy
        assert isinstance(kw["lengths"], np.ndarray)
        assert kw["lengths"].tolist() == pair_lengths(enc["input_ids"], enc["attention_mask"]).tolist() == [5, 12, 8]
    else:
        assert kw == {}
    eng.calls.clear()
    m.forward_ids(enc["input_ids"], enc["attention_mask"], enc["token_type_ids"], K - 1, want_order=True)
    ((name, a, kw),) = eng.calls
    assert name == ("forward_ids_packed" if packed else "forward_ids") and kw == dict(want_order=True)
