"""The PLAID pruned-search fixture, produced by EXECUTING THE REFERENCE'S OWN CODE (build container only; never on the GPU box).

Two functions of the reference are read AS TEXT at run time from /root/reference, cut out of their files with `ast` and executed;
nothing of them is copied into this repository:
  get_cells             third_party/ColBERT/colbert/search/candidate_generation.py (CandidateGeneration.get_cells): the centroid
                        scores of a query and the cells of its tokens;
  colbert_score_reduce  third_party/ColBERT/colbert/modeling/colbert.py: the masked column maximum and its sum, which
                        IndexScorer.score_pids (search/index_storage.py:104-147) applies to every candidate's padded block of
                        centroid scores, once over the codes that pass the threshold and once over all of them.
The rest of score_pids' two pruning passes (the threshold mask `idx`, the padding, torch.topk at ndocs and ndocs // 4) is three
lines each and is restated here in torch, with the same calls.  The candidate set is what the reference's IVF lists: per cell the
passages holding a token with that code (indexing/utils.py:8-48).

Index: 64 centroids of dim 64 (rounded to fp16, as the index stores them), 60 passages of 1 .. 70 tokens whose codes come from a
few "topic" centroids per passage, one query of 32 tokens drawn near a handful of centroids.  Per configuration (ncells,
threshold, ndocs) the fixture records the reference's cells, the candidates, both approximate scores of every candidate and the
survivors of both cuts.  Thresholds: a query token here lies near its centroid with a score around 0.7 and scores the others
within +-0.3, so thresholds of 0.25 .. 0.35 keep some centroids and drop others, as 0.45 does on a trained index.
The reference's `.sum` may add in another order than the contract's chain, so a consumer compares the scores within 1e-4 and the
sets exactly; that is only meaningful if no cut is decided inside that tolerance, which is ASSERTED here on the reference's
numbers alone: at both cuts the last kept and the first dropped score lie more than 1e-3 apart, and in no
column do the centroid scores on the two sides of the ncells cut lie within 1e-5.  Data only.

Usage:  python tests/golden/make_plaid_search_fixture.py      -> tests/golden/plaid_search_ref.npz
"""
from __future__ import annotations

import ast
import os
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
COLBERT = "third_party/ColBERT/colbert"
C, DIM, P, LQ, SEED = 64, 64, 60, 32, 4      # the seed: the first for which every assertion below holds
CONFIGS = ((1, 0.35, 16), (2, 0.3, 24), (3, 0.25, 10))         # (ncells, centroid_score_threshold, ndocs); 10 // 4 = 2


def reference_function(rel, name, ns):
    """The function `name` of the reference file `rel` (top level or a method), compiled from its own source text into `ns`."""
    path = os.path.join(REF, COLBERT, rel)
    tree = ast.parse(open(path).read(), path)
    found = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(found) == 1, (rel, name, len(found))
    mod = ast.Module(body=[found[0]], type_ignores=[])
    exec(compile(mod, path, "exec"), ns)
    return ns[name]


def build_index(seed):
    g = torch.Generator().manual_seed(seed)
    cen = torch.nn.functional.normalize(torch.randn(C, DIM, generator=g), dim=-1).half()
    lens = torch.randint(1, 71, (P,), generator=g).tolist()
    lens[0], lens[1] = 1, 70
    codes = []
    for ln in lens:
        topics = torch.randperm(C, generator=g)[:4]
        codes.append(topics[torch.randint(0, 4, (ln,), generator=g)])
    near = torch.randperm(C, generator=g)[:6]
    pick = near[torch.randint(0, 6, (LQ,), generator=g)]
    Q = torch.nn.functional.normalize(cen[pick].float() + 0.9 * torch.randn(LQ, DIM, generator=g) / DIM ** 0.5, dim=-1)
    return cen, torch.cat(codes).to(torch.int32), lens, Q


def padded_blocks(S, codes, lens, pids, idx):
    """score_pids' padded tensors for `pids`: per passage the rows S[code] of its codes with idx[code], zero-padded, and the mask."""
    first = np.concatenate([[0], np.cumsum(lens)])
    rows = []
    for p in pids:
        c = codes[first[p]:first[p + 1]].long()
        rows.append(S[c[idx[c]]])
    width = max(1, max(r.shape[0] for r in rows))
    pad = torch.zeros(len(rows), width, S.shape[1])
    mask = torch.zeros(len(rows), width)
    for i, r in enumerate(rows):
        pad[i, :r.shape[0]], mask[i, :r.shape[0]] = r, 1.0
    return pad, mask


def cut(scores, pids, keep, what):
    """torch.topk as score_pids applies it; the gap at the cut is asserted."""
    if keep >= len(pids):
        return pids
    top = torch.topk(scores, k=keep + 1).values
    gap = float(top[keep - 1] - top[keep])
    assert gap > 1e-3, f"{what}: the last kept and the first dropped score lie {gap:.2e} apart"
    return pids[torch.topk(scores, k=keep).indices]


def main():
    ns = {"torch": torch}
    get_cells = reference_function("search/candidate_generation.py", "get_cells", ns)
    reduce_ = reference_function("modeling/colbert.py", "colbert_score_reduce", dict(ns, ColBERTConfig=object))
    config = types.SimpleNamespace(interaction="colbert", query_maxlen=LQ)
    cen, codes, lens, Q = build_index(SEED)
    first = np.concatenate([[0], np.cumsum(lens)])
    blob = dict(Q=Q.numpy(), centroids=cen.numpy(), codes=codes.numpy(), doclens=np.asarray(lens, dtype=np.int32),
                configs=np.asarray(CONFIGS, dtype=np.float64))
    me = types.SimpleNamespace(codec=types.SimpleNamespace(centroids=cen.float()))
    for ci, (ncells, thr, ndocs) in enumerate(CONFIGS):
        cells, St = get_cells(me, Q, ncells)                           # St [C, Lq] = centroids @ Q.T
        S = St.float()
        srt = S.sort(dim=0, descending=True).values
        margin = float((srt[ncells - 1] - srt[ncells]).min())
        assert margin > 1e-5, f"config {ci}: a column's scores straddle the ncells cut within {margin:.2e}"
        cellset = set(cells.tolist())
        pids = torch.tensor([p for p in range(P) if cellset & set(codes[first[p]:first[p + 1]].tolist())])
        assert 0 < len(pids) < P, f"config {ci}: {len(pids)} candidates of {P}"
        idx = S.max(-1).values >= thr                                  # index_storage.py:107
        assert bool(idx.any()) and not bool(idx.all())
        a1 = reduce_(*padded_blocks(S, codes, lens, pids.tolist(), idx), config).float()
        s1 = cut(a1, pids, ndocs, f"config {ci}, first cut")
        everything = torch.ones(C, dtype=torch.bool)
        a2_all = reduce_(*padded_blocks(S, codes, lens, pids.tolist(), everything), config).float()
        a2 = reduce_(*padded_blocks(S, codes, lens, s1.tolist(), everything), config).float()
        s2 = cut(a2, s1, ndocs // 4, f"config {ci}, second cut")
        assert len(s1) < len(pids) and len(s2) < len(s1), f"config {ci}: a cut drops nothing"
        blob.update({f"c{ci}/S": S.numpy(), f"c{ci}/cells": np.sort(cells.numpy()), f"c{ci}/candidates": pids.numpy(),
                     f"c{ci}/a1": a1.numpy(), f"c{ci}/a2": a2_all.numpy(), f"c{ci}/survivors1": np.sort(s1.numpy()),
                     f"c{ci}/survivors2": np.sort(s2.numpy())})
        print(f"config {ci} (ncells {ncells}, threshold {thr}, ndocs {ndocs}): {len(cellset)} cells, {int(idx.sum())} centroids kept, "
              f"{len(pids)} candidates -> {len(s1)} -> {len(s2)}; column margin {margin:.2e}; "
              f"{int((a1 == LQ * -9999.0).sum())} candidates without a kept code")
    out = os.path.join(HERE, "plaid_search_ref.npz")
    np.savez_compressed(out, **blob)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
