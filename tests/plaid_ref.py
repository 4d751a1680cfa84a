"""A float64 numpy restatement of the decoded row of a compressed passage bank (include/rerank_mi355.h, rr_bank_create_plaid),
written from the header's text alone: bit layout, centroid + bucket weight, L2 normalisation with the 1e-12 floor.  No fp16
rounding and no float32 arithmetic: what the reference's `ResidualCodec.decompress` computes, up to its own float32 error."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plaid_codec_ref.npz")
CASES = [(d, n) for d in (64, 128) for n in (1, 2, 4, 8)]


def load_case(dim, nbits):
    """The fixture's case as a dict: centroids (fp16), cutoffs, weights, codes, residuals, decompressed."""
    z = np.load(GOLDEN)
    pre = f"d{dim}_n{nbits}/"
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def buckets_of(residuals, nbits, dim):
    """[R, dim] bucket indices from the packed bytes [R, dim * nbits / 8]."""
    per = 8 // nbits
    res = np.asarray(residuals, dtype=np.uint8).astype(np.int64)
    out = np.empty((res.shape[0], dim), dtype=np.int64)
    for e in range(dim):
        j, g = divmod(e, per)
        x = (res[:, j] >> (8 - nbits * (g + 1))) & ((1 << nbits) - 1)
        b = np.zeros_like(x)
        for k in range(nbits):                       # the nbits bits reversed
            b |= ((x >> k) & 1) << (nbits - 1 - k)
        out[:, e] = b
    return out


def pack_buckets(buckets, nbits):
    """The inverse: [R, dim] bucket indices -> packed bytes, bit 0 of a bucket first, bytes filled from the most significant end."""
    b = np.asarray(buckets, dtype=np.int64)
    bits = ((b[:, :, None] >> np.arange(nbits)[None, None, :]) & 1).astype(np.uint8)
    return np.packbits(bits.reshape(b.shape[0], -1), axis=1)


def decode(centroids, weights, nbits, codes, residuals):
    """The decoded rows in float64, before any rounding."""
    c = np.asarray(centroids).astype(np.float64)
    w = np.asarray(weights).astype(np.float64)
    s = c[np.asarray(codes, dtype=np.int64)] + w[buckets_of(residuals, nbits, c.shape[1])]
    n = np.sqrt((s * s).sum(axis=1, keepdims=True))
    return s / np.maximum(n, 1e-12)
