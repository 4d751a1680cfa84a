"""The PLAID compression fixture, produced by EXECUTING THE REFERENCE'S OWN CODE (build container only; never on the GPU box).

`ResidualCodec` (third_party/ColBERT/colbert/indexing/codecs/residual.py of the reference) is read as text at run time and executed
exactly as make_plaid_fixture.py does it (its `reference_codec_class`, imported from that file); nothing of it is copied into this
repository.  The codec runs its CPU branch: `compress` = argmax of centroids.float() @ emb.float(), residual = emb (half) -
centroid (float), torch.bucketize, np.packbits (residual.py:169-221).

Cases: dim in {64, 128} x nbits in {1, 2, 4, 8}; 80 centroids (unit vectors rounded to fp16, as an index stores them); 64 fp16 rows:
row 0 all zero, rows 1 .. 31 clustered around centroids, rows 32 .. 63 random unit vectors.  Cutoffs / weights: the quantiles of the
sample's residuals, as the reference's indexer takes them (collection_indexer.py, _compute_avg_residual).  Stored per case: rows
(fp16), centroids (fp16), cutoffs, weights, and the reference's `compress` output (codes int32, packed residuals uint8).  Data only.

The maker asserts that every row's top-2 margin in float64 is at least 1e-4 and walks seeds until that holds: a float32 dot product
of unit vectors at D <= 512 carries at most ~3e-5 of rounding error whatever the order of summation, so two orders cannot pick
different centroids above 6e-5.  The one row without a margin is the zero row: every score is an exact 0 in any order, the
reference's argmax returns index 0 there (asserted), and that is the lowest-index rule of the compressed row.

Usage:  python tests/golden/make_plaid_compress_fixture.py      -> tests/golden/plaid_compress_ref.npz
"""
from __future__ import annotations

import importlib.util
import os
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DIMS, NBITS, N_CENTROIDS, N_ROWS = (64, 128), (1, 2, 4, 8), 80, 64
MIN_MARGIN = 1e-4


def _codec_class():
    spec = importlib.util.spec_from_file_location("make_plaid_fixture", os.path.join(HERE, "make_plaid_fixture.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.reference_codec_class()


def make_case(Codec, dim, nbits, seed):
    g = torch.Generator().manual_seed(seed)
    centroids = torch.nn.functional.normalize(torch.randn(N_CENTROIDS, dim, generator=g), dim=-1).half()
    half = N_ROWS // 2
    pick = torch.randint(0, N_CENTROIDS, (half,), generator=g)
    near = torch.nn.functional.normalize(centroids[pick].float() + 0.35 * torch.randn(half, dim, generator=g) / dim ** 0.5, dim=-1)
    far = torch.nn.functional.normalize(torch.randn(N_ROWS - half, dim, generator=g), dim=-1)
    embs = torch.cat([near, far])
    embs[0] = 0.0
    embs = embs.half()
    scores = centroids.double() @ embs.double().T                      # [C, R]
    top2 = scores.topk(2, dim=0).values
    margin = (top2[0] - top2[1])[1:]                                   # the zero row has none
    if float(margin.min()) < MIN_MARGIN:
        return None
    cfg = types.SimpleNamespace(total_visible_gpus=0, dim=dim, nbits=nbits, rank=0)
    plain = Codec(config=cfg, centroids=centroids.float())
    codes = plain.compress_into_codes(embs, out_device="cpu")
    assert torch.equal(codes[1:], scores.argmax(dim=0)[1:]), "the reference's float32 argmax differs from the float64 one"
    resid = (embs - plain.lookup_centroids(codes, out_device="cpu")).float().flatten()
    nb = 1 << nbits
    cutoffs = resid.quantile(torch.arange(1, nb) / nb)
    weights = resid.quantile((torch.arange(0, nb) + 0.5) / nb)
    codec = Codec(config=cfg, centroids=centroids.float(), avg_residual=resid.abs().mean(), bucket_cutoffs=cutoffs, bucket_weights=weights)
    comp = codec.compress(embs)
    assert int(comp.codes[0]) == 0, "the reference's argmax over equal scores must return the first index"
    assert torch.equal(comp.codes, codes) and comp.residuals.shape == (N_ROWS, dim // 8 * nbits)
    return dict(rows=embs.numpy(), centroids=centroids.numpy(), cutoffs=cutoffs.float().numpy(), weights=weights.float().numpy(),
                codes=comp.codes.to(torch.int32).numpy(), residuals=comp.residuals.to(torch.uint8).numpy(),
                min_margin=np.float64(margin.min()), near_min_margin=np.float64(margin[:half - 1].min()))


def main():
    Codec = _codec_class()
    blob = {}
    for dim in DIMS:
        for nbits in NBITS:
            for attempt in range(100):
                seed = 1000 * dim + 10 * nbits + 7919 * attempt
                case = make_case(Codec, dim, nbits, seed)
                if case is not None:
                    break
            else:
                raise SystemExit(f"dim {dim} nbits {nbits}: no seed with a top-2 margin of {MIN_MARGIN}")
            for k, v in case.items():
                blob[f"d{dim}_n{nbits}/{k}"] = v
            print(f"dim {dim} nbits {nbits}: seed {seed}, margin {float(case['min_margin']):.2e} (clustered rows {float(case['near_min_margin']):.2f}), "
                  f"{len(set(case['codes'].tolist()))} distinct codes")
    out = os.path.join(HERE, "plaid_compress_ref.npz")
    np.savez_compressed(out, **blob)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
