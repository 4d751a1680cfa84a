"""CPU: the PLAID residual codec of the compressed passage bank — rr_util_plaid_decode_rows (pure host code: the bit-level
definition the device kernels are held to), rmr_amd.PlaidCodec and rmr_amd.read_plaid_index.  No device.

Reference: tests/golden/plaid_codec_ref.npz, written by tests/golden/make_plaid_fixture.py from the reference's own
`ResidualCodec.compress` / `.decompress` (CPU branch).  Bound on every decoded element, |float(y) - reference| <= 2^-12 +
(D + 4) * 2^-24: the first term is the fp16 half-ulp below 1 (a unit row has no element above 1), the second the float32 add,
sum of D squares, square root and divide.  tests/plaid_ref.py restates the decode in float64."""
import json
import os

import numpy as np
import pytest
import torch

import plaid_ref as PR


def _decode(cen, w, nbits, codes, res):
    from rmr_amd import PlaidCodec
    return PlaidCodec(torch.from_numpy(np.asarray(cen)), torch.from_numpy(np.asarray(w, dtype=np.float32)), nbits).decode(codes, res)


@pytest.mark.parametrize("dim,nbits", PR.CASES)
def test_host_decoder_matches_the_reference_decompress(dim, nbits):
    c = PR.load_case(dim, nbits)
    assert c["centroids"].dtype == np.float16 and c["codes"].dtype == np.int32 and c["residuals"].shape == (40, dim * nbits // 8)
    assert not c["centroids"][0].any() and (c["weights"] == 0).sum() == 1
    y = _decode(c["centroids"], c["weights"], nbits, c["codes"], c["residuals"]).float().numpy()
    bound = 2.0 ** -12 + (dim + 4) * 2.0 ** -24
    err = np.abs(y.astype(np.float64) - c["decompressed"].astype(np.float64)).max()
    restated = np.abs(PR.decode(c["centroids"], c["weights"], nbits, c["codes"], c["residuals"]) - c["decompressed"]).max()
    print(f"[dim {dim} nbits {nbits}] host decoder vs reference {err:.3e} (bound {bound:.3e}); float64 restatement vs reference {restated:.3e}")
    assert restated <= 5e-8, "the restated bit layout is the reference's"
    assert err <= bound


@pytest.mark.parametrize("dim,nbits", PR.CASES)
def test_host_decoder_is_the_float32_definition_bit_for_bit(dim, nbits):
    """The order of the header, restated with numpy float32 scalars: per 8 elements an fma chain (computed in float64 and rounded
    once: a product of two float32 values is exact in float64, and the float64 sum of it and a float32 value rounds to float32 as
    the fused operation does unless it lies within 2^-29 relative of a float32 tie — none of the fixture's 20 480 steps does, or
    this test would differ), then the pairwise tree, sqrt, max, divide, fp16."""
    c = PR.load_case(dim, nbits)
    cen, w = c["centroids"].astype(np.float32), c["weights"].astype(np.float32)
    s = (cen[c["codes"]] + w[PR.buckets_of(c["residuals"], nbits, dim)]).astype(np.float32)
    want = np.empty((s.shape[0], dim), dtype=np.float16)
    for r in range(s.shape[0]):
        q = []
        for c8 in range(dim // 8):
            acc = np.float32(0.0)
            for k in range(8):
                v = np.float64(s[r, 8 * c8 + k])
                acc = np.float32(v * v + np.float64(acc))
            q.append(acc)
        while len(q) > 1:
            q = [np.float32(q[2 * i] + q[2 * i + 1]) for i in range(len(q) // 2)]
        d = np.maximum(np.sqrt(q[0], dtype=np.float32), np.float32(1e-12))
        want[r] = (s[r] / d).astype(np.float32).astype(np.float16)
    got = _decode(c["centroids"], c["weights"], nbits, c["codes"], c["residuals"]).numpy()
    assert np.array_equal(got.view(np.int16), want.view(np.int16))


@pytest.mark.parametrize("nbits", [1, 2, 4, 8])
def test_bit_layout_buckets_in_element_order(nbits):
    """A row whose buckets are 0, 1, 2, ... in element order decodes to the weights in that order (zero centroid; the weights
    scaled so that the row has unit norm and fp16 represents every value: the normalisation then changes nothing)."""
    dim, nb = 256, 1 << nbits                                           # every bucket of nbits 8 appears
    buckets = (np.arange(dim) % nb)[None, :]
    res = PR.pack_buckets(buckets, nbits)
    assert res.shape == (1, dim * nbits // 8)
    if nbits == 2:
        assert res[0, 0] == 0b00100111                                  # buckets 0, 1, 2, 3: bit 0 first, MSB-first bytes
    assert np.array_equal(PR.buckets_of(res, nbits, dim), buckets)
    # weight (k + 1) / 256 for bucket k
    w = (np.arange(nb, dtype=np.float32) + 1.0) / 256.0
    got = _decode(np.zeros((2, dim), np.float16), w, nbits, np.zeros(1, np.int32), res).float().numpy()[0]
    s = w[buckets[0]]
    ratio = got / s
    assert np.all(np.diff(got[:nb]) > 0), "distinct weights stay in bucket order"
    assert np.allclose(ratio, ratio[0], rtol=2e-3), "one common scale: element e got the weight of bucket e % 2^nbits"
    want = PR.decode(np.zeros((2, dim), np.float16), w, nbits, np.zeros(1, np.int32), res)[0]
    assert np.abs(got - want).max() <= 2.0 ** -12 + (dim + 4) * 2.0 ** -24
    # a permuted table moves the values with it: element e reads w[bucket e], nothing else
    perm = np.random.RandomState(nbits).permutation(nb)
    got_p = _decode(np.zeros((2, dim), np.float16), w[perm], nbits, np.zeros(1, np.int32), res).float().numpy()[0]
    want_p = PR.decode(np.zeros((2, dim), np.float16), w[perm], nbits, np.zeros(1, np.int32), res)[0]
    assert np.abs(got_p - want_p).max() <= 2.0 ** -12 + (dim + 4) * 2.0 ** -24
    assert np.array_equal(np.argsort(got_p[:nb], kind="stable"), np.argsort(w[perm], kind="stable"))


@pytest.mark.parametrize("dim,nbits", PR.CASES)
def test_zero_norm_row_decodes_to_zeros(dim, nbits):
    c = PR.load_case(dim, nbits)
    assert c["codes"][0] == 0 and not c["decompressed"][0].any()
    y = _decode(c["centroids"], c["weights"], nbits, c["codes"][:1], c["residuals"][:1])
    assert y.shape == (1, dim) and not bool(y.view(torch.int16).any()), "zeros, and +0 at that"


def test_codec_refusals():
    from rmr_amd import PlaidCodec
    ok = PlaidCodec(torch.randn(16, 64), torch.randn(4), 2)
    assert ok.centroids.dtype == torch.float16 and ok.bucket_weights.dtype == torch.float32 and ok.residual_bytes == 16
    with pytest.raises(ValueError):
        PlaidCodec(torch.randn(16, 64), torch.randn(8), 3)              # nbits 3
    with pytest.raises(ValueError):
        PlaidCodec(torch.randn(16, 96), torch.randn(4), 2)              # D 96: no power of two
    with pytest.raises(ValueError):
        PlaidCodec(torch.randn(16, 64), torch.randn(5), 2)              # a weight table of the wrong length
    with pytest.raises(ValueError):
        PlaidCodec(torch.randn(16, 8), torch.randn(4), 2)               # 8 is no multiple of 8 * nbits
    with pytest.raises(ValueError):
        PlaidCodec(torch.randint(0, 9, (16, 64)), torch.randn(4), 2)    # integer centroids
    with pytest.raises(ValueError):
        ok.decode([16], np.zeros((1, 16), np.uint8))                    # a code equal to C


def test_library_refuses_what_the_bank_does_not_take():
    from rmr_amd import _lib as L
    lib = L.load()
    cen, w = np.zeros((4, 96), np.float16), np.zeros(256, np.float32)
    codes, res, out = np.zeros(1, np.int32), np.zeros((1, 96), np.uint8), np.zeros((1, 96), np.float16)

    def call(nbits, D, n_cent=4):
        return lib.rr_util_plaid_decode_rows(cen.ctypes.data, n_cent, w.ctypes.data, nbits, D, codes.ctypes.data, res.ctypes.data, 1,
                                             out.ctypes.data)
    assert call(3, 64) == L.RR_ERR_UNSUPPORTED and call(2, 96) == L.RR_ERR_UNSUPPORTED and call(8, 32) == L.RR_ERR_UNSUPPORTED
    assert call(2, 1024) == L.RR_ERR_UNSUPPORTED and call(1, 8) == L.RR_OK and call(8, 64) == L.RR_OK
    codes[0] = 4
    assert call(8, 64) == L.RR_ERR_BAD_SHAPE


def test_reader_on_a_synthetic_index(tmp_path):
    """An index directory of two chunks as the reference's indexer lays it out, written with torch.save / json."""
    import sys

    from rmr_amd import PlaidCodec, read_plaid_index
    c = PR.load_case(128, 8)
    cutoffs, weights = torch.from_numpy(c["cutoffs"]), torch.from_numpy(c["weights"])
    torch.save(torch.from_numpy(c["centroids"]), tmp_path / "centroids.pt")
    torch.save((cutoffs, weights), tmp_path / "buckets.pt")
    torch.save(torch.tensor([0.01]), tmp_path / "avg_residual.pt")
    doclens = [[7, 1, 12], [15, 5]]
    rows = [sum(d) for d in doclens]
    assert sum(rows) == 40
    o = 0
    for i, (d, n) in enumerate(zip(doclens, rows)):
        torch.save(torch.from_numpy(c["codes"][o:o + n].astype(np.int32)), tmp_path / f"{i}.codes.pt")
        torch.save(torch.from_numpy(c["residuals"][o:o + n]), tmp_path / f"{i}.residuals.pt")
        (tmp_path / f"doclens.{i}.json").write_text(json.dumps(d))
        (tmp_path / f"{i}.metadata.json").write_text(json.dumps(dict(passage_offset=sum(len(x) for x in doclens[:i]), num_passages=len(d),
                                                                      num_embeddings=n)))
        o += n
    (tmp_path / "metadata.json").write_text(json.dumps(dict(config=dict(nbits=8, dim=128, index_name="synthetic"), num_chunks=2,
                                                             num_partitions=16, num_embeddings=40)))
    codec, chunks = read_plaid_index(str(tmp_path))
    assert isinstance(codec, PlaidCodec) and (codec.nbits, codec.dim, codec.n_centroids) == (8, 128, 16)
    assert torch.equal(codec.centroids, torch.from_numpy(c["centroids"])) and torch.equal(codec.bucket_weights, weights)
    got = list(chunks)
    assert [g[0] for g in got] == [0, 3] and [g[3] for g in got] == doclens
    assert all(g[1].dtype == torch.int32 and g[2].dtype == torch.uint8 and g[2].shape == (n, 128) for g, n in zip(got, rows))
    assert np.array_equal(torch.cat([g[1] for g in got]).numpy(), c["codes"])
    assert np.array_equal(torch.cat([g[2] for g in got]).numpy(), c["residuals"])
    y = codec.decode(torch.cat([g[1] for g in got]), torch.cat([g[2] for g in got])).float().numpy()
    assert np.abs(y - c["decompressed"]).max() <= 2.0 ** -12 + 132 * 2.0 ** -24
    assert not [m for m in sys.modules if m == "colbert" or m.startswith("colbert.")], "the reader imports nothing of colbert"
    (tmp_path / "doclens.1.json").write_text(json.dumps([15, 4]))
    with pytest.raises(ValueError):
        list(read_plaid_index(str(tmp_path))[1])
