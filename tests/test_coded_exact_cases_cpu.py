"""CPU: the coded exact cases of tests/coded_exact_cases.py (what tests/test_gpu_bank_coded_scale.py runs on the device) BITE, shown
on the float64 / numpy oracle alone and COUNTED, the counts in the assertion messages:

1. every case has rows whose maximum is shared by a centroid below index 256 and one from 256 on (the device meets such a tie in
   the key_max over the splits of compress_codes_kernel, not inside one split), the copies of the repeated centroid rows never
   appear as a code (the lowest index wins), the float64 codes differ from the compressed case's codes, every query keeps a
   survivor, some query has fewer candidates than passages, and the final lists differ from the compressed oracle's: a coded bank
   that behaved like the compressed bank of the same case would be seen;
2. the host definition of the code (PlaidCodec.compress, rr_util_plaid_compress_rows) equals the float64 codes: here it is the host
   code that is checked against float64, not the other way round;
3. the stage-3 widths the cases were chosen for: all four of li_pick_jt, and the second column block;
4. the six cases of tests/plaid_exact_cases.py come out of the split builder byte for byte as before (digests taken before the split).
No device."""
import hashlib

import numpy as np
import pytest

import coded_exact_cases as K
import plaid_exact_cases as X

# sha256 (16 hex digits) over every entry of plaid_exact_cases.build(name), taken before build_from was split off
DIGESTS = {"c257": "9d86e84e34e7c9ef", "c300": "132345dd00ea01f6", "c1000": "a8fd61500f8731c8", "c16384": "4ce508ec67b9f9a2",
           "c16384w": "9418c02d4e8193e4", "c262144": "192ebf5de69c5e31"}


def feed(h, v):
    if isinstance(v, np.ndarray):
        h.update(f"{v.dtype}{v.shape}".encode() + np.ascontiguousarray(v).tobytes())
    else:
        h.update(repr(v).encode())


def case_digest(case):
    h = hashlib.sha256()
    for key in sorted(case):
        h.update(key.encode())
        feed(h, case[key])
    return h.hexdigest()[:16]


@pytest.mark.parametrize("name", list(X.CASES))
def test_the_six_existing_cases_are_unchanged(name):
    case, _ = X.get(name)
    assert case_digest(case) == DIGESTS[name], f"{name}: plaid_exact_cases.build gives other bytes than before"


@pytest.mark.parametrize("name", K.CASES)
def test_the_coded_case_bites_on_the_oracle_alone(name):
    case, want, _ = K.get(name)
    P, codes64, shared = len(case["lens"]), case["codes64"], case["shared"]
    compressed = X.oracle(dict(case, codes=case["codes_compressed"]))
    tied = int((shared.sum(axis=1) > 1).sum())
    spans = int(((shared[:, 0] > 0) & (shared[:, 1] > 0)).sum())
    copies = sorted({d for _, d in case["repeats"]} & set(codes64.tolist()))
    differ = int((codes64 != case["codes_compressed"]).sum())
    cand = [int((w["a1"] != -np.inf).sum()) for w in want]
    survivors = [len(w["list2"]) for w in want]
    finals = sum(w["final"] != c["final"] for w, c in zip(want, compressed))
    counts = (f"{name}: {len(codes64)} rows, {tied} with a tie, {spans} whose tie spans index 256, copies that are a code: {copies}, "
              f"{differ} codes differ from the compressed case's, candidates {cand} of {P} passages, survivors {survivors}, "
              f"{finals} of {len(want)} final lists differ from the compressed oracle's")
    print(counts)
    assert spans >= 1 and not copies and differ >= 1, counts
    assert {256, 200, case["C"] - 1} >= {d for _, d in case["repeats"]}, counts
    assert min(survivors) >= 1 and min(cand) < P and finals >= 1, counts
    assert all(len(w["final"]) == min(case["k"], len(w["list2"])) for w in want), counts
    assert case["rows"].dtype == np.float16 and np.array_equal(case["codes"], codes64)


@pytest.mark.parametrize("name", K.CASES)
def test_the_filtered_oracle_drops_every_third_passage_and_keeps_a_survivor(name):
    case, want, filtered = K.get(name)
    for w, f in zip(want, filtered):
        assert len(f["list2"]) >= 1 and all(p % 3 != 2 for p in f["list1"])
    assert any(w["final"] != f["final"] for w, f in zip(want, filtered)), f"{name}: the filter changes no final list"


@pytest.mark.parametrize("name", K.CASES)
def test_the_host_definition_of_the_code_equals_float64(name):
    import torch
    from rmr_amd import PlaidCodec
    case, _, _ = K.get(name)
    nbits = case["nbits"]
    codec = PlaidCodec(case["centroids"], case["weights"], nbits, bucket_cutoffs=torch.linspace(-0.1, 0.1, (1 << nbits) - 1))
    # the host code is one scalar loop over rows x centroids: every DISTINCT row once (a case draws its rows from a few hundred),
    # and above 16 384 centroids 64 of them, those whose tie spans index 256 first
    _, first = np.unique(case["rows"].view(np.uint16), axis=0, return_index=True)
    spans = (case["shared"][first] > 0).all(axis=1)
    first = first[np.argsort(~spans, kind="stable")]
    if case["C"] > 16384:
        first = first[:64]
    assert spans.sum() >= 1 and len(first) >= 48, f"{name}: {len(first)} distinct rows, {int(spans.sum())} with a tie across index 256"
    got = codec.compress(torch.from_numpy(case["rows"][first]))[0].numpy()
    want = case["codes64"][first]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{name}: {bad.size} of {len(first)} codes differ, first rows {first[bad[:5]].tolist()}: {got[bad[:5]].tolist()} for {want[bad[:5]].tolist()}"


def test_every_width_of_stage_3_and_the_second_column_block():
    seen = {}
    for name in K.CASES:
        p = K.params(name)
        seen.setdefault(K.li_pick_jt(p["Lq"]), []).append((name, p["D"], p["Lq"]))
    assert sorted(seen) == [1, 2, 4, 8], seen
    assert any(D <= 128 and Lq > 128 for _, D, Lq in seen[8]) and any(D == 128 and 64 < Lq <= 128 for _, D, Lq in seen[8]), seen
    assert all(K.JT[n] == K.li_pick_jt(K.params(n)["Lq"]) for n in K.CASES)
