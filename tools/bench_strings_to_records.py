"""Strings -> prediction records on one MI355X: rerank_dataset_pipelined against the serial loop and the device-bound rate.

c3 shape: bert-base text encoder, one cross-encoder layer, K = 100 candidates, 8 queries per batch, fp16 operands, packed rows
(granule 16), one vision line (81 vision tokens: 32 prefix + 49 patches from pixel values through the in-library CLIP ViT-B/32)
and one text-only line.  Contexts are synthetic WordPiece text built as tools/bench_tokenizer.py builds it, with pair lengths
spread over U[64, 512] tokens (the bench's realistic regime).  Three modes, each over the same queries after a warm-up:
  resident_inputs        padded ids and pixels already on the device; per batch the ViT, forward_ids_packed with the host
                         lengths (the same segments as the string modes), the head and non-blocking copies of logits and order
                         into pinned memory; one synchronisation at the end.  The device-bound rate.
  serial_from_strings    evaluate.rerank_dataset driving FullContextRerankModel.forward (native_tokenizer, packed_rows).
  pipelined_from_strings pipeline.rerank_dataset_pipelined.
--family joint measures the two-head RerankModel instead (the reference's monoPreFLMR-B_pointwise_softmax: loss 2H_BCE, the
same bert-base / one-layer geometry, ViT from pixels), one line "joint": the queries carry the dataset's query ids and mask
(32 entries) and the passages' joint lengths query_len + min(m + 1, 512 - query_len) spread over U[64, 512]; resident_inputs
runs forward_joint_packed on padded joint rows already on the device, serial_from_strings drives RerankModel.forward (packed
rows) with the passages tokenised and padded per batch, pipelined_from_strings is rerank_dataset_pipelined (JointStages).
--ragged LO:HI (full_context family): the lists' lengths are drawn uniformly from [LO, HI] (seeded) and the batches go through
rerank_dataset_pipelined(ragged=True); each line then holds, for the same model in the same process, the pipelined rate over
uniform lists of K candidates and over the ragged lists, both as pairs/s (LO + HI = 2 K gives the same expected pairs per batch).
Prints one JSON line.  Usage: python tools/bench_strings_to_records.py [--queries 64] [--warmup 16] [--family joint]
[--ragged 1:199]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import rmr_amd  # noqa: E402
from rmr_amd.pair_inputs import NativePairTokenizer, host_threads  # noqa: E402
from rmr_amd.ranking import rank_descending_stable  # noqa: E402


class VocabTokenizer:
    """The smallest object FullContextRerankModel's native tokenizer needs: an id-ordered vocabulary."""

    do_lower_case = True

    def __init__(self, vocab):
        self._v = {t: i for i, t in enumerate(vocab)}

    def get_vocab(self):
        return dict(self._v)


def make_corpus(n_queries, K, seed=0, joint_query_len=0):
    rng = random.Random(seed)
    syll = ["ka", "to", "mi", "ra", "ne", "so", "lu", "vi", "en", "or", "th", "st", "ing", "ed", "er", "al", "pre", "con"]
    words = sorted({"".join(rng.choice(syll) for _ in range(rng.randint(1, 3))) for _ in range(4000)})
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words + \
        ["##" + s for s in syll] + list(".,?!'-")
    text = lambda n: " ".join(rng.choice(words) + rng.choice(["", "", "", ",", "."]) for _ in range(n))
    tok = NativePairTokenizer(vocab, n_threads=1)
    sample = [text(200) for _ in range(20)]
    per_word = sum(len(tok.encode(s)) for s in sample) / (200.0 * len(sample))      # tokens per word of this generator
    queries = []
    for i in range(n_queries):
        q = text(12) + "?"
        ql = len(tok.encode(q))
        docs = []
        for k in range(K):
            target = rng.randint(64, 512)                                             # pair length, [CLS] q [SEP] c [SEP]
            overhead = joint_query_len + 1 if joint_query_len else ql + 3             # joint: q_ids (padded) t [SEP]
            docs.append({"passage_id": f"p{i}_{k}", "content": text(max(0, round((target - overhead) / per_word)))})
        queries.append({"question_id": f"q{i}", "question": q, "retrieved_docs": docs,
                        "pos_item_ids": [docs[j]["passage_id"] for j in rng.sample(range(K), 3)], "neg_item_ids": []})
        if joint_query_len:                               # the dataset's query tokens: [CLS] q [SEP], padded to max_query_length
            ids = [vocab.index("[CLS]")] + tok.encode(q)[:joint_query_len - 2] + [vocab.index("[SEP]")]
            pad = joint_query_len - len(ids)
            queries[-1]["query_input_ids"] = torch.tensor(ids + [0] * pad)
            queries[-1]["query_attention_mask"] = torch.tensor([1] * len(ids) + [0] * pad)
    return vocab, queries


def build_model(vocab, vision, dev):
    conf = dict(cross_encoder_num_hidden_layers=1, cross_encoder_max_position_embeddings=750, loss_fn="BCE", pos_weight=None,
                max_query_length=32, max_decoder_source_length=512, compute_dtype="fp16", vision_encoder=vision,
                text_only=not vision, tokenizer=VocabTokenizer(vocab), native_tokenizer=True, packed_rows=True)
    arch = rmr_amd.make_arch(conf)
    if not vision:
        arch["has_vision"] = 0
    sd = rmr_amd.synthetic_state_dict(arch, seed=0, hf_init=True)
    m = rmr_amd.FullContextRerankModel(conf, state_dict=sd, device=dev)
    m.native_tokenizer.n_threads = host_threads()      # both string modes: the CPUs this process may use, not the machine's
    return m


def labels_of(batch):
    return [1.0 if d["passage_id"] in q["pos_item_ids"] else 0.0 for q in batch for d in q["retrieved_docs"]]


def serial_forward(m, K):
    def fwd(batch):
        px = torch.stack([q["pixel_values"] for q in batch]) if "pixel_values" in batch[0] else None
        r = m([q["question"] for q in batch], px, [d["content"] for q in batch for d in q["retrieved_docs"]], K - 1,
              labels=labels_of(batch))
        logits = r.logits.view(len(batch), K).tolist()
        return {"logits": logits, "order": [rank_descending_stable(x) for x in logits], "loss": r.loss.item()}
    return fwd


def resident(m, batches, K):
    """Inputs tokenised and uploaded beforehand; the timed part only queues device work and pinned read-backs."""
    tok, eng = m.native_tokenizer, m.engine
    prepared = []
    for b in batches:
        enc = tok.prepare_full_context_inputs([q["question"] for q in b], [d["content"] for q in b for d in q["retrieved_docs"]],
                                              m.max_query_length, m.max_context_length, m.max_decoder_source_length, K)
        lengths = (((enc["input_ids"] != 0) | (enc["attention_mask"] != 0)) * torch.arange(1, enc["input_ids"].shape[1] + 1)).amax(1)
        px = torch.stack([q["pixel_values"] for q in b]).to(eng.device) if "pixel_values" in b[0] else None
        prepared.append(([enc[k].to(eng.device) for k in ("input_ids", "attention_mask", "token_type_ids")], lengths.numpy(), px,
                         torch.tensor(labels_of(b), device=eng.device), len(b)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    keep = []
    for (ids, am, tt), lengths, px, labels, n in prepared:
        cls = pat = None
        if px is not None:
            cls, pat = eng.encode_image(px)
        r = eng.forward_ids_packed(ids, am, tt, n, K, cls, pat, labels, want_order=True, lengths=lengths)
        lh = torch.empty((n, K), dtype=torch.float32, pin_memory=True).copy_(r["logits"].view(n, K), non_blocking=True)
        oh = torch.empty((n, K), dtype=torch.int32, pin_memory=True).copy_(r["order"], non_blocking=True)
        keep.append((r, lh, oh))
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run_line(vocab, queries, vision, args, dev):
    K, B = args.K, args.batch
    m = build_model(vocab, vision, dev)
    if vision:
        g = torch.Generator().manual_seed(3)
        for q in queries:
            q["pixel_values"] = 1.2 * torch.randn(3, 224, 224, generator=g)
    else:
        for q in queries:
            q.pop("pixel_values", None)
    warm, timed = queries[:args.warmup], queries[args.warmup:]
    Ks = [1, 5, 10, K]
    # warm-up of every mode (kernels, workspaces, pinned pools, tokenizer worker threads)
    rmr_amd.rerank_dataset(warm, serial_forward(m, K), B, Ks, docs_to_rerank=K)
    rmr_amd.rerank_dataset_pipelined(warm, m, B, Ks, docs_to_rerank=K)
    resident(m, [warm[i:i + B] for i in range(0, len(warm), B)], K)
    nb = -(-len(timed) // B)
    out = {}
    t = resident(m, [timed[i:i + B] for i in range(0, len(timed), B)], K)
    out["resident_inputs"] = dict(queries_per_s=round(len(timed) / t, 2), ms_per_batch=round(t * 1e3 / nb, 3))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ser = rmr_amd.rerank_dataset(timed, serial_forward(m, K), B, Ks, docs_to_rerank=K)
    t = time.perf_counter() - t0
    out["serial_from_strings"] = dict(queries_per_s=round(len(timed) / t, 2), ms_per_batch=round(t * 1e3 / nb, 3))
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pip = rmr_amd.rerank_dataset_pipelined(timed, m, B, Ks, docs_to_rerank=K, stats=stats)
    t = time.perf_counter() - t0
    out["pipelined_from_strings"] = dict(queries_per_s=round(len(timed) / t, 2), pairs_per_s=round(len(timed) * K / t, 1),
                                         ms_per_batch=round(t * 1e3 / nb, 3),
                                         host_tokenise_ms_per_batch=round(stats["tokenise_ms"] / stats["batches"], 3),
                                         host_records_ms_per_batch=round(stats["records_ms"] / stats["batches"], 3))
    out["pipelined_over_resident"] = round(out["pipelined_from_strings"]["queries_per_s"] / out["resident_inputs"]["queries_per_s"], 4)
    out["serial_over_resident"] = round(out["serial_from_strings"]["queries_per_s"] / out["resident_inputs"]["queries_per_s"], 4)
    out["records_identical"] = json.dumps(ser["output"]) == json.dumps(pip["output"])
    out["metrics_identical"] = ser["metrics"] == pip["metrics"]
    lens = [min(512, 3 + len(m.native_tokenizer.encode(q["question"])) + len(m.native_tokenizer.encode(d["content"])))
            for q in timed[:2] for d in q["retrieved_docs"]]
    out["mean_pair_tokens_sample"] = round(sum(lens) / len(lens), 1)
    return out


def run_ragged_line(vocab, queries, ragged_queries, vision, args, dev):
    """Pipelined strings -> records over uniform lists (K each) and over ragged lists, same model, alternating, twice each."""
    K, B = args.K, args.batch
    m = build_model(vocab, vision, dev)
    g = torch.Generator().manual_seed(3)
    for q, r in zip(queries, ragged_queries):
        if vision:
            q["pixel_values"] = r["pixel_values"] = 1.2 * torch.randn(3, 224, 224, generator=g)
        else:
            q.pop("pixel_values", None)
            r.pop("pixel_values", None)
    hi = max(len(q["retrieved_docs"]) for q in ragged_queries)
    Ks = [1, 5, 10]

    def timed(qs, ragged):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = {}
        if ragged:
            rmr_amd.rerank_dataset_pipelined(qs, m, B, Ks + [hi], docs_to_rerank=hi, stats=stats, ragged=True)
        else:
            rmr_amd.rerank_dataset_pipelined(qs, m, B, Ks + [K], docs_to_rerank=K, stats=stats)
        t = time.perf_counter() - t0
        pairs = sum(len(q["retrieved_docs"]) for q in qs)
        return dict(pairs=pairs, pairs_per_s=round(pairs / t, 1), queries_per_s=round(len(qs) / t, 2),
                    ms_per_batch=round(t * 1e3 / stats["batches"], 3),
                    host_tokenise_ms_per_batch=round(stats["tokenise_ms"] / stats["batches"], 3))
    w = args.warmup
    timed(queries[:w], False)
    timed(ragged_queries[:w], True)
    out = {"uniform": [], "ragged": []}
    for _ in range(2):
        out["uniform"].append(timed(queries[w:], False))
        out["ragged"].append(timed(ragged_queries[w:], True))
    out["uniform_pairs_per_s"] = max(r["pairs_per_s"] for r in out["uniform"])
    out["ragged_pairs_per_s"] = max(r["pairs_per_s"] for r in out["ragged"])
    out["ragged_over_uniform"] = round(out["ragged_pairs_per_s"] / out["uniform_pairs_per_s"], 4)
    return out


def ragged_corpus(n_queries, lo, hi, seed=0):
    """make_corpus with hi candidates per query, each list then cut to a length drawn from U[lo, hi] (its own seeded stream)."""
    vocab, queries = make_corpus(n_queries, hi, seed)
    rng = random.Random(seed + 1)
    for q in queries:
        q["retrieved_docs"] = q["retrieved_docs"][:rng.randint(lo, hi)]
        q["pos_item_ids"] = [q["retrieved_docs"][0]["passage_id"]]
    return vocab, queries


# ---- the joint family (RerankModel) ------------------------------------------------------------------------------------

def build_joint_model(vocab, dev):
    conf = dict(cross_encoder_num_hidden_layers=1, cross_encoder_max_position_embeddings=750, loss_fn="2H_BCE", pos_weight=None,
                max_decoder_source_length=512, compute_dtype="fp16", vision_encoder=True, decoder_tokenizer=VocabTokenizer(vocab),
                packed_rows=True)
    sd = rmr_amd.synthetic_state_dict(rmr_amd.make_arch(conf), seed=0, hf_init=True)
    m = rmr_amd.RerankModel(conf, state_dict=sd, device=dev)
    m.native_tokenizer.n_threads = host_threads()
    return m


def padded_contexts(m, texts):
    """tokenize_retrieved_docs' padded rows ([CLS] [unused1] t [SEP] [PAD]..., int64 [N, 512]) from the native tokenizer."""
    tok, S = m.native_tokenizer, m.max_decoder_source_length
    cls, sep, pad = tok.special_ids
    d_marker = tok.vocab.index("[unused1]")
    pool, off, ln = tok.prepare_contexts_compact(texts, S - 3, pin_memory=False)
    pool = pool.numpy()
    ids = np.full((len(texts), S), pad, dtype=np.int64)
    am = np.zeros((len(texts), S), dtype=np.int64)
    for i, (o, n) in enumerate(zip(off.tolist(), ln.tolist())):
        ids[i, 0], ids[i, 1], ids[i, 2:2 + n], ids[i, 2 + n] = cls, d_marker, pool[o:o + n], sep
        am[i, :n + 3] = 1
    return torch.from_numpy(ids), torch.from_numpy(am)


def joint_serial_forward(m, K):
    def fwd(batch):
        c_ids, c_am = padded_contexts(m, [d["content"] for q in batch for d in q["retrieved_docs"]])
        r = m(torch.stack([q["query_input_ids"] for q in batch]), torch.stack([q["query_attention_mask"] for q in batch]),
              torch.stack([q["pixel_values"] for q in batch]), c_ids, c_am, K - 1)
        logits = r.logits.view(len(batch), K).tolist()
        return {"logits": logits, "order": [rank_descending_stable(x) for x in logits], "loss": r.loss.item()}
    return fwd


def joint_resident(m, batches, K):
    """Padded joint rows, their host lengths and the pixels on the device beforehand; the timed part queues the ViT,
    forward_joint_packed, the head and the pinned read-backs."""
    eng, dev = m.engine, m.engine.device
    prepared = []
    for b in batches:
        q_ids = torch.stack([q["query_input_ids"] for q in b])
        q_am = torch.stack([q["query_attention_mask"] for q in b])
        ql = q_ids.shape[1]
        c_ids, c_am = padded_contexts(m, [d["content"] for q in b for d in q["retrieved_docs"]])
        ids = torch.cat([q_ids.repeat_interleave(K, 0), c_ids[:, 2:2 - ql]], 1)
        am = torch.cat([q_am.repeat_interleave(K, 0), c_am[:, 2:2 - ql]], 1)
        lengths = (((ids != 0) | (am != 0)) * torch.arange(1, ids.shape[1] + 1)).amax(1)
        prepared.append((ids.to(dev), am.to(dev), lengths.numpy(), torch.stack([q["pixel_values"] for q in b]).to(dev), ql, len(b)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    keep = []
    for ids, am, lengths, px, ql, n in prepared:
        cls, pat = eng.encode_image(px)
        r = eng.forward_joint_packed(ids, am, n, K, ql, cls, pat, None, want_order=True, lengths=lengths)
        lh = torch.empty((n, K), dtype=torch.float32, pin_memory=True).copy_(r["logits"].view(n, K), non_blocking=True)
        oh = torch.empty((n, K), dtype=torch.int32, pin_memory=True).copy_(r["order"], non_blocking=True)
        keep.append((r, lh, oh))
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run_joint_line(vocab, queries, args, dev):
    K, B = args.K, args.batch
    m = build_joint_model(vocab, dev)
    g = torch.Generator().manual_seed(3)
    for q in queries:
        q["pixel_values"] = 1.2 * torch.randn(3, 224, 224, generator=g)
    warm, timed = queries[:args.warmup], queries[args.warmup:]
    Ks = [1, 5, 10, K]
    rmr_amd.rerank_dataset(warm, joint_serial_forward(m, K), B, Ks, docs_to_rerank=K)
    rmr_amd.rerank_dataset_pipelined(warm, m, B, Ks, docs_to_rerank=K)
    joint_resident(m, [warm[i:i + B] for i in range(0, len(warm), B)], K)
    nb = -(-len(timed) // B)
    out = {}
    t = joint_resident(m, [timed[i:i + B] for i in range(0, len(timed), B)], K)
    out["resident_inputs"] = dict(queries_per_s=round(len(timed) / t, 2), ms_per_batch=round(t * 1e3 / nb, 3))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ser = rmr_amd.rerank_dataset(timed, joint_serial_forward(m, K), B, Ks, docs_to_rerank=K)
    t = time.perf_counter() - t0
    out["serial_from_strings"] = dict(queries_per_s=round(len(timed) / t, 2), ms_per_batch=round(t * 1e3 / nb, 3))
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pip = rmr_amd.rerank_dataset_pipelined(timed, m, B, Ks, docs_to_rerank=K, stats=stats)
    t = time.perf_counter() - t0
    out["pipelined_from_strings"] = dict(queries_per_s=round(len(timed) / t, 2), ms_per_batch=round(t * 1e3 / nb, 3),
                                         host_tokenise_ms_per_batch=round(stats["tokenise_ms"] / stats["batches"], 3),
                                         host_records_ms_per_batch=round(stats["records_ms"] / stats["batches"], 3))
    out["pipelined_over_resident"] = round(out["pipelined_from_strings"]["queries_per_s"] / out["resident_inputs"]["queries_per_s"], 4)
    out["serial_over_resident"] = round(out["serial_from_strings"]["queries_per_s"] / out["resident_inputs"]["queries_per_s"], 4)
    out["records_identical"] = json.dumps(ser["output"]) == json.dumps(pip["output"])
    out["metrics_identical"] = ser["metrics"] == pip["metrics"]
    ql = int(timed[0]["query_input_ids"].numel())
    lens = [ql + min(len(m.native_tokenizer.encode(d["content"])) + 1, 512 - ql) for q in timed[:2] for d in q["retrieved_docs"]]
    out["mean_pair_tokens_sample"] = round(sum(lens) / len(lens), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=64, help="timed queries per mode (after the warm-up)")
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--lines", default="vision,text_only")
    ap.add_argument("--family", choices=["full_context", "joint"], default="full_context",
                    help="full_context: FullContextRerankModel (--lines); joint: the two-head RerankModel, one line")
    ap.add_argument("--ragged", default=None, metavar="LO:HI",
                    help="list lengths drawn uniformly from [LO, HI]: pipelined pairs/s over ragged lists beside uniform lists of K")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if args.family == "joint":
        vocab, queries = make_corpus(args.warmup + args.queries, args.K, joint_query_len=32)
        res = {"tool": "bench_strings_to_records", "family": "joint", "shape": f"c3 bert-base, RerankModel 2H_BCE, K={args.K}, "
               f"{args.batch} queries/batch, fp16, packed joint rows granule 16, query_len 32, joint lengths U[64, 512], ViT from "
               "pixels", "queries_timed": args.queries, "host_threads": host_threads(), "gpu": torch.cuda.get_device_name(dev),
               "joint": run_joint_line(vocab, queries, args, dev)}
        print(json.dumps(res))
        return
    if args.ragged:
        lo, hi = (int(x) for x in args.ragged.split(":"))
        assert 1 <= lo <= hi
        vocab, queries = make_corpus(args.warmup + args.queries, args.K)           # the same vocabulary: same seed, same words
        _, ragged_queries = ragged_corpus(args.warmup + args.queries, lo, hi)
        res = {"tool": "bench_strings_to_records", "mode": "ragged", "shape": f"c3 bert-base, {args.batch} queries/batch, fp16, "
               f"packed rows granule 16, pair lengths U[64, 512]; uniform lists K={args.K} against list lengths U[{lo}, {hi}]",
               "queries_timed": args.queries, "host_threads": host_threads(), "gpu": torch.cuda.get_device_name(dev)}
        for line in args.lines.split(","):
            res[line] = run_ragged_line(vocab, queries, ragged_queries, line == "vision", args, dev)
        print(json.dumps(res))
        return
    vocab, queries = make_corpus(args.warmup + args.queries, args.K)
    res = {"tool": "bench_strings_to_records", "shape": f"c3 bert-base, K={args.K}, {args.batch} queries/batch, fp16, packed rows "
           "granule 16, pair lengths U[64, 512]", "queries_timed": args.queries, "host_threads": host_threads(),
           "gpu": torch.cuda.get_device_name(dev)}
    for line in args.lines.split(","):
        res[line] = run_line(vocab, queries, line == "vision", args, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
