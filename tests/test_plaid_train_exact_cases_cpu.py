"""CPU: the exact cases of tests/plaid_train_exact_cases.py (what tests/test_gpu_plaid_train_scale.py runs on the device).

1. Every case BITES, on the numpy oracle alone: the exactness bound holds in every iteration, equal initial rows tie at every listed
   centroid-index distance and the lower index takes the rows, the upper cluster is re-seeded, codes still change in later
   iterations, cluster sizes are no powers of two, winners lie in every quarter of the index range (in cp262144 beyond index
   65 535), residuals lie ON cutoffs.  The builder asserts the same while it builds.
2. rr_util_plaid_kmeans (the library's host code) equals the oracle bit for bit — table, counts, statistics — on km512d, km256d,
   km32d and a 2-iteration cut of km64d: dimensions and centroid counts the slow restatement cannot reach.
3. rr_util_plaid_compress_rows equals the oracle's codes and packed bytes on cp65536.
4. The fast oracle equals the slow restatement (tests/plaid_train_ref.py, which loops over every (row, centroid) pair) on the tiny
   exact case: the new oracle is anchored to the one already trusted.
No device."""
import numpy as np
import pytest

import plaid_train_exact_cases as X
import plaid_train_ref as T
from test_plaid_train_cpu import _bits, _host


@pytest.mark.parametrize("name", list(X.KM))
def test_the_kmeans_case_bites_on_the_oracle_alone(name):
    p = X.get(name)
    f = X.km_facts(p)
    print(name, {k: f[k] for k in ("reseeds", "changed", "odd_sizes", "max_size", "bounds")})
    C, R, niters = p["C"], p["R"], p["niters"]
    assert f["changed"][0] == R and sum(0 < ch < R for ch in f["changed"]) >= 2
    assert f["reseeds"][0] >= len(p["pairs"]) >= 1
    assert any(s & (s - 1) for s in f["odd_sizes"])
    assert all(bound < limit for bound, limit in f["bounds"]) and len(f["bounds"]) == niters
    if name != "tiny":
        assert all(q == [0, 1, 2, 3] for q in f["quarters"])
    dist = {d for d, _, _ in f["ties"]}
    assert dist >= {d for d in (16, 64, 256, 1024, 4096, C // 2) if d < C}
    for (s, t, a, b), (d, code_a, code_b) in zip(p["pairs"], f["ties"]):
        assert code_a == s and code_b == s and t == s + d     # both rows at the lower index: the upper cluster is empty
    w = p["want"]
    assert int(w["counts"].sum()) == R and w["centroids"].dtype == np.float16 and w["centroids"].shape == (C, p["D"])
    # both sources hold the same fp16 rows, and the float32 one holds no fp16 value
    assert np.array_equal(p["rows32"].astype(np.float16).view(np.uint16), p["rows16"].view(np.uint16))
    assert (p["rows32"] != p["rows16"].astype(np.float32)).all()
    assert np.signbit(p["rows16"][p["rows16"] == 0]).any() and not np.signbit(p["rows16"][p["rows16"] == 0]).all()


def test_the_planned_splits_of_the_scale_cases():
    """The automatic plan's arithmetic (csrc/bank_compress.hip, rr_plaid_compress_plan) restated: 16 splits at km4096, 64 at the cp
    cases, and the tie distances cross a split boundary in each."""
    def splits(R, C, jt):
        row_blocks = -(-R // (16 * jt))
        want = max(1, min(64, 1024 // row_blocks))
        chunk = -(-max(256, -(-C // want)) // 16) * 16
        return -(-C // chunk), chunk
    assert splits(8192, 4096, 8) == (16, 256)
    assert splits(300, 65536, 8) == (64, 1024)
    assert splits(130, 262144, 8) == (64, 4096)
    for name, chunk in (("km4096", 256), ("cp65536", 1024), ("cp262144", 4096)):
        p = X.get(name)
        pairs = [(q[0], q[1]) for q in p["pairs"]]
        assert any(s // chunk != t // chunk for s, t in pairs) and any(s // 16 % 4 == t // 16 % 4 for s, t in pairs)


@pytest.mark.parametrize("name", list(X.CP))
def test_the_compression_case_bites_on_the_oracle_alone(name):
    p = X.get(name)
    C, code, pick = p["C"], p["codes"], p["pick"]
    print(name, p["bound"], "winners beyond 65535:", int((code > 65535).sum()))
    assert p["bound"][0] < p["bound"][1]
    assert sorted(set((code.astype(np.int64) * 4 // C).tolist())) == [0, 1, 2, 3]
    assert {t - s for s, t in p["pairs"]} == {16, 64, 256, 1024, 4096, C // 2}
    for s, t in p["pairs"]:
        assert (code[pick == t] == s).all() and (pick == t).sum() >= 2
    assert ((code > 65535).sum() >= 16) == (C > 65536)
    assert (p["rows32"] != p["rows16"].astype(np.float32)).all()
    for nbits, q in p["packed"].items():
        assert np.isin(p["residuals"], q["cutoffs"]).any()
        assert q["bytes"].shape == (p["R"], p["D"] // 8 * nbits)


def _hold_host_kmeans(p, rows, niters, want):
    rc, cen, cnt, stats = _host(rows, p["init_rows"], niters, p["seed"])
    assert rc == 0
    assert np.array_equal(_bits(cen), _bits(want["centroids"])), "centroids"
    assert np.array_equal(cnt, want["counts"]), "counts"
    assert np.array_equal(stats, want["stats"]), (stats.tolist(), want["stats"].tolist())


@pytest.mark.parametrize("name,src", [("km512d", "rows32"), ("km256d", "rows32"), ("km256d", "rows16"), ("km32d", "rows32"),
                                      ("km32d", "rows16")])
def test_host_kmeans_equals_the_oracle(name, src):
    p = X.get(name)
    _hold_host_kmeans(p, p[src], p["niters"], p["want"])


def test_host_kmeans_equals_the_oracle_on_a_cut_of_km64d():
    p = X.get("km64d")
    want = X.kmeans(p["rows16"], p["init_rows"], 2, p["seed"])
    assert np.array_equal(want["stats"], p["want"]["stats"][:2]) and not np.array_equal(_bits(want["centroids"]), _bits(p["want"]["centroids"]))
    _hold_host_kmeans(p, p["rows16"], 2, want)


@pytest.mark.parametrize("nbits,src,R", [(8, "rows32", None), (2, "rows16", 60)])      # rows are independent: the first 60 of them
def test_host_compress_equals_the_oracle_on_cp65536(nbits, src, R):
    from rmr_amd import _lib as L
    lib = L.load()
    p = X.get("cp65536")
    R = p["R"] if R is None else R
    q = p["packed"][nbits]
    rows = np.ascontiguousarray(p[src][:R])
    cen = np.ascontiguousarray(p["centroids"])
    codes = np.full(R, -7, dtype=np.int32)
    res = np.full((R, q["bytes"].shape[1]), 0xA5, dtype=np.uint8)
    rc = lib.rr_util_plaid_compress_rows(rows.ctypes.data, L.RR_F16 if rows.dtype == np.float16 else L.RR_F32, R, p["D"],
                                         cen.ctypes.data, p["C"], q["cutoffs"].ctypes.data, nbits, codes.ctypes.data, res.ctypes.data)
    assert rc == L.RR_OK
    assert np.array_equal(codes, p["codes"][:R]) and np.array_equal(res, q["bytes"][:R])


def test_the_fast_oracle_equals_the_slow_restatement_on_the_tiny_case():
    p = X.get("tiny")
    for rows in (p["rows16"], p["rows32"]):
        for niters in (0, 1, p["niters"]):
            fast = X.kmeans(rows, p["init_rows"], niters, p["seed"])
            cen, counts, stats, codes = T.kmeans(rows, p["init_rows"], niters, p["seed"])
            assert np.array_equal(_bits(fast["centroids"]), _bits(cen))
            assert np.array_equal(fast["counts"], counts) and np.array_equal(fast["stats"], stats)
            if niters:
                assert np.array_equal(fast["codes"][-1], codes)
            _hold_host_kmeans(p, rows, niters, fast)
    # the residual oracle against the slow compressed row, on the tiny case's last table
    import plaid_compress_ref as P
    table = p["want"]["tables"][-1]
    cut = X.cutoffs_of(2)
    codes, res, _ = P.compress(p["rows32"], table, cut, 2)
    fc, fr = X.residuals(p["rows32"], table)
    assert np.array_equal(fc, codes) and np.array_equal(X.pack(fr, cut, 2)[1], res)
