"""The late-interaction score formula the GPU tests compare rr_li_scores with (include/rerank_mi355.h): the reference's
colbert_score (flmr_utils.py:22-48) restated in plain torch.  tests/test_li_scores_cpu.py pins it, in float32, to the arrays
the reference's own function returned (tests/golden/li_scores_ref.npz); the GPU tests evaluate it in float64."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MASKED = -9999.0


def li_scores_formula(query_li, context_li, context_mask, K, dtype=torch.float32):
    """(maxsim [N], scores [N, Lc, Lq]) of query_li [Bq, Lq, D], context_li [N, Lc, D], context_mask [N, Lc]."""
    q = query_li.to(dtype).repeat_interleave(K, dim=0)
    scores = context_li.to(dtype) @ q.permute(0, 2, 1)
    scores[~context_mask.bool()] = MASKED
    return scores.max(1).values.sum(-1), scores


def load_li_scores_ref():
    z = np.load(os.path.join(GOLDEN, "li_scores_ref.npz"), allow_pickle=False)
    g = {k: (int(z[k]) if z[k].ndim == 0 else torch.from_numpy(z[k])) for k in z.files}
    return g


def retriever_inputs(Bq, K, Lq, Lc, D, seed, holes=True, full_mask_pair=None):
    """Unit-norm retriever embeddings as O.make_interaction_inputs makes them (no rows zeroed: the mask alone must decide),
    ragged context lengths, optionally holes inside the passages and one fully masked pair."""
    g = torch.Generator().manual_seed(seed)
    N = Bq * K
    q = torch.nn.functional.normalize(torch.randn(Bq, Lq, D, generator=g), dim=-1)
    c = torch.nn.functional.normalize(torch.randn(N, Lc, D, generator=g), dim=-1)
    cm = torch.zeros(N, Lc)
    for n in range(N):
        L = int(torch.randint(max(1, Lc // 4), Lc + 1, (1,), generator=g))
        cm[n, :L] = 1
        if holes and L > 4:
            cm[n, torch.randperm(L, generator=g)[: L // 5]] = 0
    if full_mask_pair is not None:
        cm[full_mask_pair] = 0
    return q, c, cm


def aligned_context(query_li, context_li, query_mask, context_mask, K, noise=0.3, seed=3):
    """Contexts that answer their query: every second unmasked context token becomes a unit-norm copy of an unmasked query
    token of its own query plus noise of relative size `noise` (scores up to ~1 where a passage matches, as a retriever's
    top candidates have them; random unit vectors alone stay near 0 and the fusion bias near uniform)."""
    gen = torch.Generator().manual_seed(seed)
    c = context_li.clone()
    for n in range(c.shape[0]):
        qi = n // K
        valid_q = query_mask[qi].nonzero().flatten()
        for i, t in enumerate(context_mask[n].nonzero().flatten()[::2].tolist()):
            v = query_li[qi, valid_q[i % len(valid_q)]]
            v = v + noise * torch.randn(v.shape, generator=gen) / v.numel() ** 0.5
            c[n, t] = torch.nn.functional.normalize(v, dim=-1)
    return c
