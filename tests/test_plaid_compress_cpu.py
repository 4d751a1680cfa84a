"""CPU: compressing embeddings into PLAID residual codes (rr_util_plaid_compress_rows, PlaidCodec.compress): the host definition of
the compressed row (include/rerank_mi355.h, rr_bank_add_compress) against what the reference's ResidualCodec.compress gave
(tests/golden/plaid_compress_ref.npz, made by tests/golden/make_plaid_compress_fixture.py) — every row, codes and bytes equal — and
against a restatement of the header's text (tests/plaid_compress_ref.py) on the cases the definition settles by rule: ties, the
zero row, NaN scores, a residual on a cutoff.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

import plaid_compress_ref as P
import plaid_ref


def _codec(case, nbits, cutoffs=True):
    import rmr_amd
    return rmr_amd.PlaidCodec(torch.from_numpy(case["centroids"]), torch.from_numpy(case["weights"]), nbits,
                              bucket_cutoffs=torch.from_numpy(case["cutoffs"]) if cutoffs else None)


@pytest.mark.parametrize("dim,nbits", P.CASES)
def test_host_compress_equals_the_reference_on_every_row(dim, nbits):
    case = P.load_case(dim, nbits)
    assert case["rows"].dtype == np.float16 and case["rows"].shape == (64, dim) and case["centroids"].shape == (80, dim)
    assert not case["rows"][0].any() and float(case["min_margin"]) >= 1e-4
    codec = _codec(case, nbits)
    for rows in (torch.from_numpy(case["rows"]), torch.from_numpy(case["rows"]).float()):
        codes, res = codec.compress(rows)
        assert codes.dtype == torch.int32 and res.dtype == torch.uint8 and tuple(res.shape) == (64, dim // 8 * nbits)
        assert np.array_equal(codes.numpy(), case["codes"])
        assert np.array_equal(res.numpy(), case["residuals"])


@pytest.mark.parametrize("dim,nbits", P.CASES)
def test_the_c_entry_point_equals_the_reference(dim, nbits):
    from rmr_amd import _lib as L
    lib = L.load()
    case = P.load_case(dim, nbits)
    rows, cen, cut = (np.ascontiguousarray(case[k]) for k in ("rows", "centroids", "cutoffs"))
    codes = np.full(64, -1, dtype=np.int32)
    res = np.full((64, dim // 8 * nbits), 0xAA, dtype=np.uint8)
    rc = lib.rr_util_plaid_compress_rows(rows.ctypes.data, L.RR_F16, 64, dim, cen.ctypes.data, 80, cut.ctypes.data, nbits,
                                         codes.ctypes.data, res.ctypes.data)
    assert rc == L.RR_OK
    assert np.array_equal(codes, case["codes"]) and np.array_equal(res, case["residuals"])
    # the packing named by tests/plaid_ref.py (the inverse of the decoded row) gives the same bytes from the buckets
    assert np.array_equal(plaid_ref.pack_buckets(plaid_ref.buckets_of(res, nbits, dim), nbits), res)


@pytest.mark.parametrize("dim,nbits", P.CASES)
def test_decode_of_compress_equals_decode_of_the_reference_arrays(dim, nbits):
    case = P.load_case(dim, nbits)
    codec = _codec(case, nbits)
    got = codec.decode(*codec.compress(torch.from_numpy(case["rows"])))
    want = codec.decode(case["codes"], case["residuals"])
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_the_restatement_agrees_with_the_host_code_on_a_fixture_case():
    case = P.load_case(64, 2)
    codes, res, _ = P.compress(case["rows"][:12], case["centroids"], case["cutoffs"], 2)
    assert np.array_equal(codes, case["codes"][:12]) and np.array_equal(res, case["residuals"][:12])


def _host(rows, centroids, cutoffs, nbits):
    import rmr_amd
    w = torch.zeros(1 << nbits)
    codec = rmr_amd.PlaidCodec(torch.as_tensor(centroids), w, nbits, bucket_cutoffs=torch.as_tensor(cutoffs, dtype=torch.float32))
    codes, res = codec.compress(torch.as_tensor(rows))
    return codes.numpy(), res.numpy()


def test_definition_ties_zero_row_and_nan():
    g = np.random.default_rng(5)
    D, nbits = 32, 2
    cen = g.standard_normal((6, D)).astype(np.float16)
    cen[4] = cen[1]                                    # a duplicate: the lower index wins
    cen[5, 3] = 0.0                                    # inf * 0: the first NaN score of row 3 below
    cut = np.array([-0.5, 0.0, 0.5], dtype=np.float32)
    rows = g.standard_normal((5, D)).astype(np.float32)
    rows[0] = 10.0 * cen[1].astype(np.float32)          # nearest to centroid 1 == centroid 4
    rows[1] = 0.0                                      # the zero row: every score 0, code 0
    rows[2, 7] = np.nan                                # every score NaN: the first centroid
    rows[3] = 0.0
    rows[3, 3] = np.inf                                # scores +-inf but for centroid 5, whose score is NaN: a NaN wins
    want_codes, want_res, S = P.compress(rows, cen, cut, nbits)
    assert want_codes[0] == 1 and S[0, 1] == S[0, 4]
    assert want_codes[1] == 0 and not S[1].any()
    assert want_codes[2] == 0 and np.isnan(S[2]).all()
    assert want_codes[3] == 5 and np.isnan(S[3, 5]) and not np.isnan(S[3, :5]).any() and np.isinf(S[3, :5]).all()
    codes, res = _host(rows, cen, cut, nbits)
    assert np.array_equal(codes, want_codes) and np.array_equal(res, want_res)
    # a NaN residual has bucket 0: row 2, element 7 (two bits per element, four elements per byte)
    assert plaid_ref.buckets_of(res, nbits, D)[2, 7] == 0


def test_definition_plus_and_minus_zero_scores_tie_by_index():
    D = 16
    cen = np.zeros((3, D), dtype=np.float16)
    cen[0, 0], cen[1, 0], cen[2, 0] = -1.0, -0.0, 0.0   # scores against x = (0, ..): -0 * .. chains: all zero of either sign
    rows = np.zeros((2, D), dtype=np.float32)
    rows[1, 0] = -0.0
    cut = np.array([0.0], dtype=np.float32)
    want_codes, want_res, S = P.compress(rows, cen, cut, 1)
    assert not S.any() and want_codes.tolist() == [0, 0]
    codes, res = _host(rows, cen, cut, 1)
    assert np.array_equal(codes, want_codes) and np.array_equal(res, want_res)


def test_definition_a_residual_on_a_cutoff_takes_the_lower_bucket():
    D, nbits = 16, 2
    cen = np.zeros((1, D), dtype=np.float16)
    cen[0] = 0.25
    cut = np.array([-0.25, 0.25, 0.5], dtype=np.float32)
    rows = np.full((1, D), 0.25, dtype=np.float32)
    rows[0, :6] = [0.5, 0.5 + 2 ** -10, 0.0, -2 ** -12, 0.75, 0.75 + 2 ** -9]   # residuals 0.25, just above, -0.25, just below, 0.5, above
    codes, res = _host(rows, cen, cut, nbits)
    b = plaid_ref.buckets_of(res, nbits, D)[0]
    assert codes.tolist() == [0] and b[:6].tolist() == [1, 2, 0, 0, 2, 3] and (b[6:] == 1).all()    # residual 0: cutoffs below it: one
    assert np.array_equal(res, P.compress(rows, cen, cut, nbits)[1])


def test_float32_input_is_rounded_to_fp16_first():
    case = P.load_case(64, 4)
    codec = _codec(case, 4)
    rows = torch.from_numpy(case["rows"]).float()
    bumped = rows + rows.abs() * 2.0 ** -13              # below half an fp16 ulp: rounds back to the same fp16 value
    assert not torch.equal(bumped, rows) and torch.equal(bumped.half(), rows.half())
    a, b = codec.compress(bumped), codec.compress(rows)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_cutoff_validation():
    import rmr_amd
    from rmr_amd import _lib as L
    cen, w = torch.zeros(4, 16), torch.zeros(4)
    rmr_amd.PlaidCodec(cen, w, 2)                                          # positional, as before: no cutoffs
    assert rmr_amd.PlaidCodec(cen, w, 2).bucket_cutoffs is None
    ok = rmr_amd.PlaidCodec(cen, w, 2, bucket_cutoffs=[-1.0, 0.0, 0.0])      # equal neighbours are fine
    assert ok.bucket_cutoffs.dtype == torch.float32 and ok.bucket_cutoffs.tolist() == [-1.0, 0.0, 0.0]
    for bad in ([0.0, 1.0], [0.0, 1.0, 2.0, 3.0], [0.0, float("nan"), 1.0], [0.0, 1.0, 0.5], torch.tensor([0, 1, 2])):
        with pytest.raises(ValueError):
            rmr_amd.PlaidCodec(cen, w, 2, bucket_cutoffs=bad)
    with pytest.raises(ValueError):
        rmr_amd.PlaidCodec(cen, w, 2).compress(torch.zeros(1, 16))           # no cutoffs
    with pytest.raises(ValueError):
        ok.compress(torch.zeros(1, 32))                                    # another width
    lib = L.load()
    z = np.zeros(64, dtype=np.float32)
    out = np.zeros(64, dtype=np.int32)
    rb = np.zeros(64, dtype=np.uint8)
    args = lambda D, nbits, dt=L.RR_F32: (z.ctypes.data, dt, 1, D, z.ctypes.data, 1, z.ctypes.data, nbits, out.ctypes.data, rb.ctypes.data)
    assert lib.rr_util_plaid_compress_rows(*args(16, 2)) == L.RR_OK
    assert lib.rr_util_plaid_compress_rows(*args(8, 1)) == L.RR_ERR_UNSUPPORTED       # no matrix-core step
    assert lib.rr_util_plaid_compress_rows(*args(16, 4)) == L.RR_ERR_UNSUPPORTED      # D % (8 nbits)
    assert lib.rr_util_plaid_compress_rows(*args(16, 3)) == L.RR_ERR_UNSUPPORTED
    assert lib.rr_util_plaid_compress_rows(*args(16, 2, L.RR_BF16)) == L.RR_ERR_BAD_DTYPE
    assert lib.rr_set_tuning(b"compress_chunk", 48) == L.RR_OK and lib.rr_set_tuning(b"compress_chunk", 0) == L.RR_OK
    assert lib.rr_set_tuning(b"compress_chunk", 40) == L.RR_ERR_BAD_ARG and lib.rr_set_tuning(b"compress_chunk", -16) == L.RR_ERR_BAD_ARG


def test_read_plaid_index_keeps_the_cutoffs(tmp_path):
    import rmr_amd
    case = P.load_case(64, 2)
    d = str(tmp_path)
    with open(os.path.join(d, "metadata.json"), "w") as f:
        json.dump({"config": {"nbits": 2, "dim": 64}, "num_chunks": 1}, f)
    torch.save(torch.from_numpy(case["centroids"]), os.path.join(d, "centroids.pt"))
    torch.save((torch.from_numpy(case["cutoffs"]), torch.from_numpy(case["weights"])), os.path.join(d, "buckets.pt"))
    torch.save(torch.from_numpy(case["codes"]), os.path.join(d, "0.codes.pt"))
    torch.save(torch.from_numpy(case["residuals"]), os.path.join(d, "0.residuals.pt"))
    with open(os.path.join(d, "doclens.0.json"), "w") as f:
        json.dump([40, 24], f)
    codec, chunks = rmr_amd.read_plaid_index(d)
    assert torch.equal(codec.bucket_cutoffs, torch.from_numpy(case["cutoffs"])) and codec.nbits == 2
    (first, codes, res, doclens), = list(chunks)
    assert first == 0 and doclens == [40, 24]
    got = codec.compress(torch.from_numpy(case["rows"]))                   # the index's own codec reproduces the index's arrays
    assert torch.equal(got[0], codes) and torch.equal(got[1], res)
