"""GPU: the scoring head over lists of unequal length (rr_head_lists) against rr_head / rr_head_joint, which it must reproduce
bit for bit list by list (the same arithmetic in the same order), its gather and its refusals; the packed forwards of the three
families over a list layout against each query run alone; and rerank_dataset_pipelined(ragged=True) against the serial loop run
one query per forward, the reference executor's loop (src/executors/Reranker_base_executor.py:807-976 of the reference)."""
import json
import random
import threading

import numpy as np
import pytest
import torch

from helpers import O, golden_inputs, load_golden
from test_gpu_head import _engine, _logits

pytestmark = pytest.mark.gpu

# (loss_fn, pos_weight, explicit labels, joint): every loss kind the head computes
KINDS = [("BCE", None, False, False), ("BCE", 2.5, False, False), ("BCE", None, True, False), ("BCE", 2.5, True, False),
         ("2H_BCE", None, False, False), ("2H_BCE", 3.0, False, False), ("2H_BCE", 3.0, True, False),
         ("BCE", None, False, True), ("2H_BCE", None, False, True), ("2H_BCE", 3.0, False, True),
         ("negative_sampling", None, False, False)]
KIND_IDS = [f"{k[0]}{'-pw' if k[1] else ''}{'-labels' if k[2] else ''}{'-joint' if k[3] else ''}" for k in KINDS]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _labels(n, seed):
    return (torch.rand(n, generator=torch.Generator().manual_seed(seed)) < 0.2).float()


def _flat(sizes, seed, ties):
    """One vector of logits per list, as test_gpu_head makes them: exact ties and +-inf with `ties`."""
    return [_logits(1, k, seed + 7 * i, ties=ties).reshape(-1) for i, k in enumerate(sizes)]


def _head(eng, x, x1, labels, Bq, K, joint, **kw):
    return eng.head(x.cuda(), None if x1 is None else x1.cuda(), None if labels is None else labels.cuda(), Bq, K, joint=joint, **kw)


def _head_lists(eng, x, x1, labels, sizes, joint, **kw):
    return eng.head_lists(x.cuda(), None if x1 is None else x1.cuda(), None if labels is None else labels.cuda(), sizes,
                          joint=joint, **kw)


# ---- 5. a uniform layout gives rr_head's / rr_head_joint's bits ---------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("K", [1, 5, 100, 4096])
@pytest.mark.parametrize("Bq", [1, 3, 64])
def test_uniform_layout_equals_rr_head_bit_for_bit(kind, K, Bq):
    loss_fn, pw, with_labels, joint = kind
    eng = _engine(loss_fn, pw)
    two = loss_fn == "2H_BCE"
    for ties in (False, True):
        x = _logits(Bq, K, seed=K + Bq, ties=ties).reshape(-1)
        x1 = _logits(Bq, K, seed=K + Bq + 1000, ties=False).reshape(-1) if two else None
        labels = _labels(Bq * K, 2) if with_labels else None
        want = _head(eng, x, x1, labels, Bq, K, joint, want_scores=True)
        got = _head_lists(eng, x, x1, labels, [K] * Bq, joint, want_scores=True)
        torch.cuda.synchronize()
        assert _same_bits(got["loss"], want["loss"]), (ties, got["loss"].item(), want["loss"].item())
        assert _same_bits(got["scores"], want["scores"]), ties
        assert torch.equal(got["order"].cpu(), want["order"].cpu().reshape(-1)), ties
        assert got["list_loss"].shape == (Bq,)


# ---- 6. a ragged layout: every list is rr_head on that list alone --------------------------------------------------------

RAGGED = [1, 2, 63, 64, 65, 100, 4096, 1, 64, 2, 100]


def _weights(kind, sizes, labels):
    loss_fn, pw, with_labels, joint = kind
    if loss_fn == "negative_sampling":
        return [1.0] * len(sizes)
    if loss_fn == "2H_BCE" and not joint and pw is not None:        # sum of the class weights [1, pos_weight] of the targets
        out, o = [], 0
        for k in sizes:
            y = labels[o:o + k] if labels is not None else torch.tensor([1.0] + [0.0] * (k - 1))
            out.append(float((y != 0).sum()) * pw + float((y == 0).sum()))
            o += k
        return out
    return [float(k) for k in sizes]


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_ragged_layout_equals_rr_head_per_list(kind):
    loss_fn, pw, with_labels, joint = kind
    eng = _engine(loss_fn, pw)
    two = loss_fn == "2H_BCE"
    sizes, N = RAGGED, sum(RAGGED)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    labels = _labels(N, 5) if with_labels else None
    for ties in (True, False):
        xs = _flat(sizes, 11, ties)
        x1s = _flat(sizes, 500, False) if two else None
        x, x1 = torch.cat(xs), (torch.cat(x1s) if two else None)
        got = _head_lists(eng, x, x1, labels, sizes, joint, want_scores=True)
        torch.cuda.synchronize()
        singles = []
        for q, k in enumerate(sizes):
            lab = labels[offs[q]:offs[q + 1]] if with_labels else None
            one = _head(eng, xs[q], x1s[q] if two else None, lab, 1, k, joint, want_scores=True)
            torch.cuda.synchronize()
            sl = slice(int(offs[q]), int(offs[q + 1]))
            assert _same_bits(got["scores"][sl], one["scores"]), (q, k, ties)
            assert torch.equal(got["order"][sl].cpu(), one["order"].cpu().reshape(-1)), (q, k, ties)
            assert got["order"][sl].cpu().tolist() == O.rank_descending_stable(xs[q].tolist()), (q, k, ties)
            assert _same_bits(got["list_loss"][q], one["loss"]), (q, k, ties, got["list_loss"][q].item(), one["loss"].item())
            singles.append(float(one["loss"].double().item()))
        if ties:
            continue                                     # +-inf belongs to the rank cases: the batch loss on finite logits only
        # sum(part_loss) / sum(part_w) on the host in float64 from the single-list results and the known weights.  Between the
        # two there is only the fp32 rounding of each single-list loss (relative 2**-24 each) and of the result:
        # |difference| <= 4 * 2**-24 * sum(|loss_q| * w_q) / sum(w_q)   (absolute values: the joint loss's terms change sign)
        w = _weights(kind, sizes, labels)
        want = sum(l * wq for l, wq in zip(singles, w)) / sum(w)
        bound = 4 * 2.0 ** -24 * sum(abs(l) * wq for l, wq in zip(singles, w)) / sum(w)
        diff = abs(float(got["loss"].double().item()) - want)
        print(f"[{KIND_IDS[KINDS.index(kind)]}] batch loss {got['loss'].item():.9g}, host {want:.9g}, |diff| {diff:.3e}, bound {bound:.3e}")
        assert diff <= bound
        if loss_fn == "BCE" and not joint:              # the reference's loss function on the concatenated logits
            lab = labels.tolist() if with_labels else [1.0 if p in set(offs[:-1].tolist()) else 0.0 for p in range(N)]
            lg, lb = O.prepare_logits_labels("BCE", x.reshape(-1, 1), x.reshape(-1, 1), 1, N - 1, lab)
            ref = O.loss_value("BCE", pw, lg, lb)
            assert abs(got["loss"].item() - ref.item()) <= 2e-6 * max(1.0, abs(ref.item()))


# ---- 7. a list's outputs do not depend on its neighbours -------------------------------------------------------------------

@pytest.mark.parametrize("kind", [KINDS[1], KINDS[5], KINDS[9], KINDS[10]], ids=[KIND_IDS[i] for i in (1, 5, 9, 10)])
@pytest.mark.parametrize("k", [1, 65, 100, 4096])
def test_a_list_does_not_depend_on_its_neighbours(kind, k):
    loss_fn, pw, _, joint = kind
    eng = _engine(loss_fn, pw)
    two = loss_fn == "2H_BCE"
    mine, mine1 = _logits(1, k, 77, ties=True).reshape(-1), _logits(1, k, 78, ties=False).reshape(-1)
    results = []
    for place, (before, after) in enumerate([([], [3, 4096]), ([64], [100, 2]), ([2, 4096], [])]):   # first, in the middle, last
        sizes = before + [k] + after
        parts = [_logits(1, s, 200 + 13 * place + i, ties=True).reshape(-1) * (place + 1) for i, s in enumerate(sizes)]
        parts1 = [_logits(1, s, 300 + 13 * place + i, ties=False).reshape(-1) for i, s in enumerate(sizes)]
        parts[len(before)], parts1[len(before)] = mine, mine1
        got = _head_lists(eng, torch.cat(parts), torch.cat(parts1) if two else None, None, sizes, joint, want_scores=True)
        torch.cuda.synchronize()
        o = sum(before)
        results.append((got["scores"][o:o + k].cpu(), got["order"][o:o + k].cpu(), got["list_loss"][len(before)].cpu()))
    for r in results[1:]:
        assert _same_bits(r[0], results[0][0]) and torch.equal(r[1], results[0][1]) and _same_bits(r[2], results[0][2])


# ---- 8. gather ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [KINDS[3], KINDS[6], KINDS[8], KINDS[10]], ids=[KIND_IDS[i] for i in (3, 6, 8, 10)])
def test_gather_reads_permuted_logits(kind):
    loss_fn, pw, with_labels, joint = kind
    eng = _engine(loss_fn, pw)
    two = loss_fn == "2H_BCE"
    sizes = [5, 1, 100, 64, 4096, 2]
    N = sum(sizes)
    x, x1 = torch.cat(_flat(sizes, 21, True)), (torch.cat(_flat(sizes, 22, False)) if two else None)
    labels = _labels(N, 9) if with_labels else None
    want = _head_lists(eng, x, x1, labels, sizes, joint, want_scores=True)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(4))           # packed position i holds pair perm[i]
    inverse = torch.empty(N, dtype=torch.int32)
    inverse[perm] = torch.arange(N, dtype=torch.int32)
    got = _head_lists(eng, x[perm], x1[perm] if two else None, labels, sizes, joint, want_scores=True, gather=inverse.cuda())
    torch.cuda.synchronize()
    for k in ("loss", "list_loss", "scores"):
        assert _same_bits(got[k], want[k]), k
    assert torch.equal(got["order"], want["order"])


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------

def test_bad_offsets_are_refused_and_nothing_is_written():
    from rmr_amd import _lib as L
    eng = _engine("BCE")
    x = torch.randn(5000, generator=torch.Generator().manual_seed(1)).cuda()
    loss = torch.full((), -7.0, device="cuda")
    ll = torch.full((8,), -7.0, device="cuda")
    scores = torch.full((5000,), -7.0, device="cuda")
    order = torch.full((5000,), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(offsets):
        off = np.asarray(offsets, dtype=np.int32)
        return eng.lib.rr_head_lists(eng.h, x.data_ptr(), None, None, len(off) - 1, off.ctypes.data, None, 0, loss.data_ptr(),
                                     ll.data_ptr(), scores.data_ptr(), order.data_ptr(), stream)
    assert call([1, 4, 9]) == L.RR_ERR_BAD_SHAPE                     # offsets[0] != 0
    assert call([0, 4, 4, 9]) == L.RR_ERR_BAD_SHAPE                  # an empty list
    assert call([0, 9, 4, 12]) == L.RR_ERR_BAD_SHAPE                 # a descending pair
    assert call([0, 3, 4100]) == L.RR_ERR_UNSUPPORTED                # a list of 4097
    assert call([0]) == L.RR_ERR_BAD_SHAPE                           # no list at all
    torch.cuda.synchronize()
    for t in (loss, ll, scores):
        assert (t == -7.0).all().item()
    assert (order == -7).all().item()
    with pytest.raises(AssertionError):
        eng.head_lists(x[:9], None, None, [4, 0, 5])
    with pytest.raises(NotImplementedError):
        eng.head_lists(x[:4100], None, None, [3, 4097])
    assert call([0, 4, 9, 4105]) == 0                                # 4096 is fine, and the same buffers are written
    torch.cuda.synchronize()
    assert not (scores[:4105] == -7.0).any().item() and loss.item() != -7.0 and (scores[4105:] == -7.0).all().item()
    # what rr_head refuses is refused in the same way
    ns = _engine("negative_sampling")
    with pytest.raises(ValueError):                                  # utils.py:233: no labels with the listwise loss
        ns.head_lists(x[:9], None, torch.zeros(9).cuda(), [4, 5])
    with pytest.raises(ValueError):                                  # the first head is missing
        _engine("2H_BCE").head_lists(x[:9], None, None, [4, 5])
    with pytest.raises(NotImplementedError):                         # RerankModel with negative_sampling has no loss
        ns.head_lists(x[:9], None, None, [4, 5], joint=True)


# ---- 10. end to end: the packed forwards over a list layout ----------------------------------------------------------------

CPQ = [3, 7, 1, 5]


def _rank_check(r, sizes, ranked_key="logits"):
    o = 0
    ranked = r[ranked_key].cpu()
    for k in sizes:
        assert r["order"][o:o + k].cpu().tolist() == O.rank_descending_stable(ranked[o:o + k].tolist())
        o += k


def test_full_context_lists_equal_each_query_alone_bit_for_bit():
    import rmr_amd
    from helpers import arch_from_cfg
    g = load_golden("tiny")
    eng = rmr_amd.RerankEngine(arch_from_cfg(g["cfg"], False))
    eng.load_state_dict(O.make_weights(g["cfg"], 0, False))
    eng.set_option("resid_split", 0)
    ids, am, tt, _ = golden_inputs(g)
    pick = torch.arange(sum(CPQ)) % ids.shape[0]
    ids, am, tt = ids[pick].cuda(), am[pick].cuda(), tt[pick].cuda()
    labels = _labels(sum(CPQ), 3).cuda() if g["cfg"].loss_fn != "negative_sampling" else None
    got = eng.forward_ids_packed(ids, am, tt, None, None, labels=labels, list_sizes=CPQ, want_order=True, want_scores=True, granule=8)
    torch.cuda.synchronize()
    o = 0
    for q, k in enumerate(CPQ):
        sl = slice(o, o + k)
        one = eng.forward_ids_packed(ids[sl], am[sl], tt[sl], 1, k, labels=None if labels is None else labels[sl], want_order=True,
                                     want_scores=True, granule=8)
        torch.cuda.synchronize()
        assert _same_bits(got["logits"][sl], one["logits"]), q
        assert _same_bits(got["list_loss"][q], one["loss"]) and _same_bits(got["scores"][sl], one["scores"]), q
        assert torch.equal(got["order"][sl], one["order"].reshape(-1)), q
        o += k
    _rank_check(got, CPQ)
    # the drop-in keyword: the same call, flat logits, and a clear error without packed rows
    conf = dict(cross_encoder_num_hidden_layers=g["cfg"].ce_layers, cross_encoder_max_position_embeddings=g["cfg"].ce_max_pos,
                loss_fn=g["cfg"].loss_fn, pos_weight=g["cfg"].pos_weight, text_only=True, arch=arch_from_cfg(g["cfg"], False),
                packed_rows=True)
    m = rmr_amd.FullContextRerankModel(conf, state_dict=O.make_weights(g["cfg"], 0, False))
    m.engine.set_option("resid_split", 0)
    out = m.forward_ids(ids, am, tt, 0, labels=None if labels is None else labels.tolist(), candidates_per_query=CPQ, granule=8)
    torch.cuda.synchronize()
    assert _same_bits(out.logits.reshape(-1), got["logits"]) and torch.equal(out.order, got["order"])
    assert _same_bits(out.list_loss, got["list_loss"]) and _same_bits(out.loss, got["loss"])
    assert out.logits.shape == ((sum(CPQ),) if g["cfg"].loss_fn == "negative_sampling" else (sum(CPQ), 1))
    m.packed_rows = False
    with pytest.raises(ValueError, match="packed_rows"):
        m.forward_ids(ids, am, tt, 0, candidates_per_query=CPQ)


def test_joint_lists_equal_each_query_alone():
    from test_gpu_packed_families import GATE, _cfg, _joint_engine, _npz
    g = _npz("rm_tiny")
    eng = _joint_engine(_cfg(g, "2H_BCE"))
    Bq, K = int(g["Bq"]), int(g["K"])
    t = lambda k: torch.from_numpy(g[k]).cuda()
    ql = g["query_input_ids"].shape[1]
    qpick = torch.arange(len(CPQ)).cuda() % Bq
    owner = torch.repeat_interleave(torch.arange(len(CPQ)), torch.tensor(CPQ)).cuda()
    cpick = torch.arange(sum(CPQ)).cuda() % (Bq * K)
    q_ids, q_am = t("query_input_ids")[qpick], t("query_attention_mask")[qpick]
    ids = torch.cat([q_ids[owner], t("context_input_ids")[cpick][:, 2:2 - ql]], 1).long().contiguous()
    am = torch.cat([q_am[owner], t("context_attention_mask")[cpick][:, 2:2 - ql]], 1).long().contiguous()
    cls, pat = t("image_cls")[qpick].contiguous(), t("image_patches")[qpick].contiguous()
    instr = int(g["instruction_token_id"])
    got = eng.forward_joint_packed(ids, am, None, None, ql, cls, pat, instr, want_order=True, granule=8, list_sizes=CPQ)
    torch.cuda.synchronize()
    o, worst = 0, 0.0
    for q, k in enumerate(CPQ):
        sl = slice(o, o + k)
        one = eng.forward_joint_packed(ids[sl], am[sl], 1, k, ql, cls[q:q + 1], pat[q:q + 1], instr, want_order=True, granule=8)
        torch.cuda.synchronize()
        worst = max(worst, (got["logits"][sl] - one["logits"]).abs().max().item(), (got["logits2"][sl] - one["logits2"]).abs().max().item())
        o += k
    print(f"joint lists vs each query alone: |dlogit| {worst:.3e}")
    assert worst <= GATE
    _rank_check(got, CPQ)
    assert got["list_loss"].shape == (len(CPQ),) and torch.isfinite(got["loss"]).item()


@pytest.mark.parametrize("name", ["int_tiny", "mores_tiny"])
def test_interaction_lists_equal_each_query_alone(name):
    from test_gpu_packed_families import GATE, _int_args, _int_engine
    eng, g = _int_engine(name)
    Bq, K = int(g["Bq"]), int(g["K"])
    q_li, c_li, qm, cm = _int_args(g)
    qpick = torch.arange(len(CPQ)).cuda() % Bq
    cpick = torch.arange(sum(CPQ)).cuda() % (Bq * K)
    q_li, qm = q_li[qpick].contiguous(), qm.reshape(Bq, -1)[qpick].contiguous()
    c_li, cm = c_li[cpick].contiguous(), cm.reshape(Bq * K, -1)[cpick].contiguous()
    got = eng.forward_interaction_packed(q_li, c_li, qm, cm, None, None, want_order=True, granule=16, list_sizes=CPQ)
    torch.cuda.synchronize()
    o, worst = 0, 0.0
    for q, k in enumerate(CPQ):
        sl = slice(o, o + k)
        one = eng.forward_interaction_packed(q_li[q:q + 1], c_li[sl], qm[q:q + 1], cm[sl], 1, k, want_order=True, granule=16)
        torch.cuda.synchronize()
        worst = max(worst, (got["logits"][sl] - one["logits"]).abs().max().item())
        o += k
    print(f"{name} lists vs each query alone: |dlogit| {worst:.3e}")
    assert worst <= GATE
    _rank_check(got, CPQ)


# ---- 11. the pipelined loop over ragged lists --------------------------------------------------------------------------------

def _ragged(qs, K, seed):
    rng = random.Random(seed)
    for q in qs:
        q["retrieved_docs"] = q["retrieved_docs"][:rng.randint(1, K)]
        q["pos_item_ids"] = [d["passage_id"] for d in rng.sample(q["retrieved_docs"], min(2, len(q["retrieved_docs"])))]
    return qs


@pytest.mark.parametrize("loss_fn", ["BCE", "negative_sampling"])
def test_ragged_pipelined_loop_equals_one_query_per_forward(tmp_path, loss_fn):
    import rmr_amd
    from test_gpu_pipeline import _models, _queries, _serial
    m, cfg = _models(tmp_path, False, loss_fn)
    K, B, n = 10, 3, 17
    qs = _ragged(_queries(n, K, seed=7), K, 5)
    sizes = [len(q["retrieved_docs"]) for q in qs]
    assert len(set(sizes)) > 3
    Ks = [1, 5, 10]

    def one(batch):                                      # the existing uniform call, one query of its own K
        (q,) = batch
        return _serial(m, len(q["retrieved_docs"]))(batch)
    want = rmr_amd.rerank_dataset(qs, one, 1, Ks, docs_to_rerank=K, ragged=True)
    before = set(threading.enumerate())
    stats = {}
    got = rmr_amd.rerank_dataset_pipelined(qs, m, B, Ks, docs_to_rerank=K, out_path=str(tmp_path / "pred.json"), stats=stats,
                                           ragged=True)
    assert set(threading.enumerate()) == before
    assert stats["batches"] == 6 and [len(r["top_ranking_passages"]) for r in got["output"]] == sizes
    assert json.dumps(got["output"]) == json.dumps(want["output"])
    assert got["metrics"] == want["metrics"]
    assert json.load(open(tmp_path / "pred.json")) == {"output": want["output"]}
    # the serial loop over whole ragged batches, through the drop-in keyword, gives the same records
    def whole(batch):
        labels = None
        if loss_fn != "negative_sampling":
            labels = [1.0 if d["passage_id"] in x["pos_item_ids"] else 0.0 for x in batch for d in x["retrieved_docs"]]
        r = m([x["question"] for x in batch], None, [d["content"] for x in batch for d in x["retrieved_docs"]], 0, labels=labels,
              candidates_per_query=[len(x["retrieved_docs"]) for x in batch])
        return {"logits": r.logits.tolist(), "order": r.order.tolist(), "loss": r.loss.item(), "list_loss": r.list_loss.tolist()}
    again = rmr_amd.rerank_dataset(qs, whole, B, Ks, docs_to_rerank=K, ragged=True)
    assert json.dumps(again["output"]) == json.dumps(want["output"])


@pytest.mark.parametrize("vit,instr,K,n,B", [(True, None, 12, 7, 3), (False, 777, 6, 9, 2)])
def test_ragged_pipelined_joint_loop_equals_one_query_per_forward(tmp_path, vit, instr, K, n, B):
    import rmr_amd
    from test_gpu_joint_pipeline import _model, _queries, _serial
    from test_gpu_pipeline import _hf_tokenizer
    hf = _hf_tokenizer(tmp_path)
    m, cfg = _model(hf, packed=True, vit=vit, instr=instr)
    qs = _ragged(_queries(n, K, 16, 100 + K, cfg, instr=instr), K, 6)
    sizes = [len(q["retrieved_docs"]) for q in qs]
    assert len(set(sizes)) > 2
    Ks = sorted({1, min(5, K), K})

    def one(batch):
        (q,) = batch
        return _serial(m, hf, len(q["retrieved_docs"]))(batch)
    want = rmr_amd.rerank_dataset(qs, one, 1, Ks, docs_to_rerank=K, ragged=True)
    before = set(threading.enumerate())
    stats = {}
    got = rmr_amd.rerank_dataset_pipelined(qs, m, B, Ks, docs_to_rerank=K, stats=stats, ragged=True)
    assert set(threading.enumerate()) == before
    assert stats["batches"] == -(-n // B) and [len(r["top_ranking_passages"]) for r in got["output"]] == sizes
    worst = max(abs(a["score"] - b["score"]) for x, y in zip(got["output"], want["output"])
                for a, b in zip(sorted(x["top_ranking_passages"], key=lambda p: p["passage_id"]),
                                sorted(y["top_ranking_passages"], key=lambda p: p["passage_id"])))
    print(f"ragged joint pipeline vs one query per forward: |dscore| {worst:.3e}, "
          f"|dloss| {max(abs(x['loss'] - y['loss']) for x, y in zip(got['output'], want['output'])):.3e}")
    assert json.dumps(got["output"]) == json.dumps(want["output"])
    assert got["metrics"] == want["metrics"]
