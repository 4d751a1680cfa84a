"""The PLAID residual codec fixture, produced by EXECUTING THE REFERENCE'S OWN CODE (build container only; never on the GPU box).

`ResidualCodec` (third_party/ColBERT/colbert/indexing/codecs/residual.py of the reference) is read AS TEXT at run time from
/root/reference and executed; nothing of it is copied into this repository.  Its three `colbert` imports cannot be resolved here
(the package needs faiss / ujson / git at import time) and are stubbed: `ColBERTConfig` (only named in `load`, which is not run),
`print_message` (print) and `ResidualEmbeddings`, of which `compress` / `decompress` use the constructor and the two attributes
`codes` / `residuals` alone.  The codec runs its CPU branch (config.total_visible_gpus = 0): np.packbits in `binarize`, and in
`decompress` reversed_bit_map -> decompression_lookup_table -> bucket_weights, centroid add, F.normalize (residual.py:264-275).

Cases: dim in {64, 128} x nbits in {1, 2, 4, 8}; 16 centroids (rounded to fp16, as the index stores them, residual.py:161), row 0 of
them all zero; 40 embedding rows, row 0 all zero.  Cutoffs / weights: the quantiles of the sample's residuals (rows 1..) the reference's
indexer takes (collection_indexer.py, _compute_avg_residual), then the weight of the bucket a zero residual falls into is set to
an exact 0 — so the zero embedding (code 0: every dot product is 0 and argmax takes the first; residual 0) decodes to a row of
norm zero.  Stored per case: centroids (fp16), cutoffs, weights, the `compress` output (codes int32, packed residuals uint8) and
the float32 `decompress` output.  Data only.

Usage:  python tests/golden/make_plaid_fixture.py      -> tests/golden/plaid_codec_ref.npz
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REL = "third_party/ColBERT/colbert/indexing/codecs/residual.py"
DIMS, NBITS, N_CENTROIDS, N_ROWS = (64, 128), (1, 2, 4, 8), 16, 40


def reference_codec_class():
    class ResidualEmbeddings:
        def __init__(self, codes, residuals):
            self.codes, self.residuals = codes, residuals

    stubs = {"colbert": {}, "colbert.infra": {}, "colbert.infra.config": dict(ColBERTConfig=type("ColBERTConfig", (), {})),
             "colbert.indexing": {}, "colbert.indexing.codecs": {},
             "colbert.indexing.codecs.residual_embeddings": dict(ResidualEmbeddings=ResidualEmbeddings),
             "colbert.utils": {}, "colbert.utils.utils": dict(print_message=print)}
    saved = {k: sys.modules.get(k) for k in stubs}
    try:
        for name, attrs in stubs.items():
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            m.__path__ = []
            sys.modules[name] = m
        ns = {"__name__": "reference_residual"}
        path = os.path.join(REF, REL)
        exec(compile(open(path).read(), path, "exec"), ns)
        return ns["ResidualCodec"]
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def make_case(Codec, dim, nbits, seed):
    g = torch.Generator().manual_seed(seed)
    centroids = torch.nn.functional.normalize(torch.randn(N_CENTROIDS, dim, generator=g), dim=-1)
    centroids[0] = 0.0
    centroids = centroids.half()
    pick = torch.randint(1, N_CENTROIDS, (N_ROWS,), generator=g)
    embs = torch.nn.functional.normalize(centroids[pick].float() + 0.35 * torch.randn(N_ROWS, dim, generator=g) / dim ** 0.5, dim=-1)
    embs[0] = 0.0
    cfg = types.SimpleNamespace(total_visible_gpus=0, dim=dim, nbits=nbits, rank=0)
    plain = Codec(config=cfg, centroids=centroids.float())
    codes = plain.compress_into_codes(embs, out_device="cpu")
    resid = (embs - plain.lookup_centroids(codes, out_device="cpu"))[1:].flatten()      # without the zero row's zeros
    nb = 1 << nbits
    cutoffs = resid.quantile(torch.arange(1, nb) / nb)
    weights = resid.quantile((torch.arange(0, nb) + 0.5) / nb)
    weights[int(torch.bucketize(torch.zeros(1), cutoffs))] = 0.0
    codec = Codec(config=cfg, centroids=centroids.float(), avg_residual=resid.abs().mean(), bucket_cutoffs=cutoffs, bucket_weights=weights)
    comp = codec.compress(embs)
    out = codec.decompress(comp)
    assert int((weights == 0).sum()) == 1
    assert int(comp.codes[0]) == 0 and not bool(out[0].any()), "the zero embedding must give a zero-norm row"
    assert comp.residuals.shape == (N_ROWS, dim // 8 * nbits) and out.dtype == torch.float32
    return dict(centroids=centroids.numpy(), cutoffs=cutoffs.numpy(), weights=weights.float().numpy(),
                codes=comp.codes.to(torch.int32).numpy(), residuals=comp.residuals.to(torch.uint8).numpy(), decompressed=out.numpy())


def main():
    Codec = reference_codec_class()
    blob = {}
    for dim in DIMS:
        for nbits in NBITS:
            case = make_case(Codec, dim, nbits, seed=1000 * dim + nbits)
            for k, v in case.items():
                blob[f"d{dim}_n{nbits}/{k}"] = v
            print(f"dim {dim} nbits {nbits}: codes {sorted(set(case['codes'].tolist()))}, |weights| max {abs(case['weights']).max():.4f}")
    out = os.path.join(HERE, "plaid_codec_ref.npz")
    np.savez_compressed(out, **blob)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
