"""The fixtures of the fp16-matrix-core search over COMPRESSED banks (rr_bank_search_f16_plaid, include/rerank_mi355.h), on top of
tests/bank_f16_cases.py: a codec made from a fixture's own rows, and the fixture with its rows compressed and decoded by the host
definitions (rr_util_plaid_compress_rows / rr_util_plaid_decode_rows through PlaidCodec).  No device.
"""
import numpy as np
import torch

N_CENTROIDS = 64


def fixture_codec(fx, nbits):
    """A PlaidCodec for the rows of `fx`: N_CENTROIDS of its own rows (a seeded choice among the unmasked ones, as fp16) as the
    centroid table, and cutoffs and weights from the quantiles of the fixture's own residuals against the best centroid of every
    row (PlaidCodec.bucket_statistics: what the reference's indexer computes on its held-out block)."""
    from rmr_amd import PlaidCodec
    rows = fx["rows"].astype(np.float32)
    rng = np.random.default_rng(1000 * fx["D"] + nbits)
    pick = rng.choice(np.flatnonzero(fx["mask"]), N_CENTROIDS, replace=False)
    cen = rows[np.sort(pick)].astype(np.float16)
    code = np.argmax(rows @ cen.astype(np.float32).T, axis=1)
    resid = torch.from_numpy(rows - cen.astype(np.float32)[code])
    cutoffs, weights, _ = PlaidCodec.bucket_statistics(resid, nbits)
    return PlaidCodec(torch.from_numpy(cen), weights, nbits, bucket_cutoffs=cutoffs)


def decoded_fixture(fx, codec):
    """(`fx` with its rows replaced by what the codec decodes them to, codes int32 [R], residual bytes uint8 [R, .]): the host
    definitions alone.  The decoded rows are fp16 values, as every fixture's rows are."""
    codes, res = codec.compress(torch.from_numpy(fx["rows"].astype(np.float32)))
    rows = codec.decode(codes, res).float().numpy()
    return dict(fx, rows=rows), codes, res
