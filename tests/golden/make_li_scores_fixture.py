"""tests/golden/li_scores_ref.npz: the retriever's late-interaction scores as the reference's OWN function computes them.

In the manner of make_reference_fixtures.py: the reference module cannot be imported (torch.distributed plumbing, package
layout), so this script reads src/models/flmr/models/flmr/flmr_utils.py AS TEXT at run time, takes the two function
definitions `colbert_score` / `colbert_score_reduce` (flmr_utils.py:22-48) out of its AST and executes them with only
`torch` in scope.  Nothing of the reference is copied into this repository; the .npz holds the inputs this script draws
and the two arrays the function returns (`maxsim` [N], `scores` [N, Lc, Lq] = the executor's `scores_raw`).

The case: the int_tiny geometry (Bq 2, K 3, Lq 9, Lc 40, D 64), unit-norm token embeddings, a context mask with holes
(the retriever's skiplist masks punctuation in the middle of a passage) and one fully masked pair, whose MaxSim is
-9999 * Lq exactly.  tests/test_li_scores_cpu.py checks that the plain formula restated in the header
(include/rerank_mi355.h, rr_li_scores) reproduces both arrays bit for bit; the GPU tests compare the kernel with them.

Usage:  python tests/golden/make_li_scores_fixture.py [--check]     (--check: compare with the committed file, write nothing)
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RR_REFERENCE", "/root/reference")
REL = "src/models/flmr/models/flmr/flmr_utils.py"
OUT = os.path.join(HERE, "li_scores_ref.npz")

Bq, K, Lq, Lc, D, SEED = 2, 3, 9, 40, 64, 2024


def reference_functions():
    with open(os.path.join(REF, REL)) as f:
        tree = ast.parse(f.read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("colbert_score", "colbert_score_reduce")]
    assert len(keep) == 2, "flmr_utils.py no longer defines colbert_score / colbert_score_reduce"
    ns = {"torch": torch}
    exec(compile(ast.fix_missing_locations(ast.Module(body=keep, type_ignores=[])), "reference:" + REL, "exec"), ns)
    return ns["colbert_score"]


def inputs():
    g = torch.Generator().manual_seed(SEED)
    N = Bq * K
    q = F.normalize(torch.randn(Bq, Lq, D, generator=g), dim=-1)
    c = F.normalize(torch.randn(N, Lc, D, generator=g), dim=-1)
    cm = torch.zeros(N, Lc)
    for n in range(N):
        L = int(torch.randint(Lc // 4, Lc + 1, (1,), generator=g))
        cm[n, :L] = 1
        holes = torch.randperm(L, generator=g)[: max(1, L // 5)]        # skiplist tokens inside the passage
        cm[n, holes] = 0
    cm[4] = 0                                                           # one pair without a single valid context token
    return q, c, cm


def main():
    colbert_score = reference_functions()
    q, c, cm = inputs()
    with torch.no_grad():
        # FLMRModelForRetrieval.score (modeling_flmr.py:932-936,1601-1602): Q repeated per candidate, D_mask = the context mask
        maxsim, scores = colbert_score(q.repeat_interleave(K, dim=0), c.clone(), cm.clone())
    rec = dict(Bq=np.int64(Bq), K=np.int64(K), Lq=np.int64(Lq), Lc=np.int64(Lc), D=np.int64(D),
               query_li=q.numpy(), context_li=c.numpy(), context_mask=cm.numpy(),
               maxsim=maxsim.numpy(), scores=scores.numpy())
    assert rec["scores"].shape == (Bq * K, Lc, Lq) and rec["scores"].dtype == np.float32
    assert float(rec["maxsim"][4]) == -9999.0 * Lq
    if "--check" in sys.argv:
        z = np.load(OUT, allow_pickle=False)
        bad = [k for k in rec if not np.array_equal(np.asarray(rec[k]), z[k])]
        print("li_scores_ref.npz:", "reproduced bit for bit" if not bad else f"DIFFERS in {bad}")
        sys.exit(1 if bad else 0)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT}: {len(rec)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
