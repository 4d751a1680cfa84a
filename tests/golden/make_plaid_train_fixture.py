"""The PLAID codec-training fixture, produced by EXECUTING THE REFERENCE'S OWN CODE (build container only; never on the GPU box).

`CollectionIndexer._compute_avg_residual` (third_party/ColBERT/colbert/indexing/collection_indexer.py:295-319 of the reference) is
read AS TEXT at run time: the module cannot be imported here (faiss, ujson, ...), so the one function is cut out of the parsed
source by name and compiled on its own, with `ResidualCodec` bound to the reference's class as make_plaid_fixture.py executes it
(its `reference_codec_class`) and `torch` to torch; nothing of it is copied into this repository.  It runs its CPU branch
(use_gpu False): codes by argmax of centroids @ heldout.T.float(), residual = heldout (half) - centroid (float32), the mean
absolute residual, and the two torch.quantile calls that give the bucket cutoffs and weights.

One case, data only: 256 held-out fp16 rows of D 16 around 8 centroids given as fp16 values (unit vectors rounded to fp16), nbits 2.
Stored: rows, centroids, the reference's codes, cutoffs, weights, avg_residual (float32) and the smallest top-2 score margin.

The maker asserts that every row's best centroid score exceeds its second best by more than 1e-3 in float64 and walks seeds until
that holds: a float32 dot product at D 16 of unit vectors carries far less than that of rounding error whatever the order of
summation, so the reference's matmul and the library's fmaf chain choose the same code and the residuals are the same float32
subtractions.

Usage:  python tests/golden/make_plaid_train_fixture.py      -> tests/golden/plaid_train_ref.npz
"""
from __future__ import annotations

import ast
import importlib.util
import os
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REL = "third_party/ColBERT/colbert/indexing/collection_indexer.py"
DIM, NBITS, N_CENTROIDS, N_ROWS = 16, 2, 8, 256
MIN_MARGIN = 1e-3


def _plaid_fixture_module():
    spec = importlib.util.spec_from_file_location("make_plaid_fixture", os.path.join(HERE, "make_plaid_fixture.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def reference_compute_avg_residual():
    """The reference's _compute_avg_residual as a plain function (self, centroids, heldout), compiled from its source text."""
    base = _plaid_fixture_module()
    path = os.path.join(base.REF, REL)
    tree = ast.parse(open(path).read(), path)
    found = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "_compute_avg_residual"]
    assert len(found) == 1, f"{path}: {len(found)} definitions of _compute_avg_residual"
    mod = ast.Module(body=[found[0]], type_ignores=[])
    ns = {"torch": torch, "ResidualCodec": base.reference_codec_class(), "print": lambda *a, **k: None}
    exec(compile(mod, path, "exec"), ns)
    return ns["_compute_avg_residual"]


def make_case(fn, seed):
    g = torch.Generator().manual_seed(seed)
    centroids = torch.nn.functional.normalize(torch.randn(N_CENTROIDS, DIM, generator=g), dim=-1).half()
    pick = torch.randint(0, N_CENTROIDS, (N_ROWS,), generator=g)
    rows = torch.nn.functional.normalize(centroids[pick].float() + 0.6 * torch.randn(N_ROWS, DIM, generator=g) / DIM ** 0.5, dim=-1).half()
    scores = centroids.double() @ rows.double().T                       # [C, R]
    top2 = scores.topk(2, dim=0).values
    margin = float((top2[0] - top2[1]).min())
    if not margin > MIN_MARGIN:
        return None
    cfg = types.SimpleNamespace(total_visible_gpus=0, dim=DIM, nbits=NBITS, rank=0)
    me = types.SimpleNamespace(config=cfg, use_gpu=False)
    cutoffs, weights, avg = fn(me, centroids.float(), rows)
    codes = scores.argmax(dim=0).to(torch.int32)
    assert cutoffs.shape == (3,) and weights.shape == (4,) and cutoffs.dtype == torch.float32 and avg.dtype == torch.float32
    return dict(rows=rows.numpy(), centroids=centroids.numpy(), nbits=np.int32(NBITS), codes=codes.numpy(), cutoffs=cutoffs.numpy(),
                weights=weights.numpy(), avg_residual=np.float32(avg.item()), min_margin=np.float64(margin))


def main():
    fn = reference_compute_avg_residual()
    for attempt in range(1000):
        case = make_case(fn, 4099 + 7919 * attempt)
        if case is not None:
            break
    else:
        raise SystemExit(f"no seed with a top-2 margin above {MIN_MARGIN}")
    print(f"attempt {attempt}: margin {float(case['min_margin']):.2e}, {len(set(case['codes'].tolist()))} distinct codes, "
          f"cutoffs {case['cutoffs'].tolist()}, avg_residual {float(case['avg_residual']):.6f}")
    out = os.path.join(HERE, "plaid_train_ref.npz")
    np.savez_compressed(out, **case)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
