"""The exact cases of tests/plaid_exact_cases.py as CODED fp16 banks (rr_bank_set_centroids, include/rerank_mi355.h), with an oracle in
float64 numpy that calls nothing of the library.  Helper of tests/test_coded_exact_cases_cpu.py and tests/test_gpu_bank_coded_scale.py.

A coded bank holds fp16 rows and, per row, the code the device assigns: the centroid of the largest row . centroid, the lowest index
among equals.  Here the rows are a case's `decoded` rows (multiples of 1/8) and the table is its centroid table (multiples of 1/4):
every product is a multiple of 2^-5 and a row's sum of |products| stays far below 2^19, so any float32 order of the sum gives the
float64 value, the maxima TIE exactly (thousands of rows a case, many of them between a centroid below index 256 and one at or above
it: the repeated centroid rows), and "the first maximum of the float64 product" (`codes64`) predicts every code.  The rows are no
longer the centroid plus a residual of their original code: `codes64` differs from the case's `codes` on thousands of rows, so the
pruning oracle over `codes64` (plaid_exact_cases.oracle) cannot be met by a bank that behaves like the compressed one.  S, the exact
scores (MaxSim over exactly these rows) and the queries are the case's own; the inverted file is ivf_numpy over `codes64`.

Beside the six cases of plaid_exact_cases.CASES there are two derived ones, so that stage 3 on fp16 rows runs at every width of
li_pick_jt: `c300q48` (Lq 48: JT 4) and `c1000w100` (D 128, Lq 100: JT 8 in one column block); Lq 4 (JT 1), 32 (JT 2) and 130 at
D 64 (JT 8, two blocks, the second of 2 columns) come with the six.  The coded form of c262144 has 27 base passages (30 passages,
1 422 rows: the assignment oracle is a [rows, 262144] float64 product, and the table alone takes seconds to draw).

Measured on 16 CPU threads: get() (the build, codes64, the pruning oracle with and without the filter) takes 5.0 s for c262144, of
which the compressed case's builder is 3 s, 3.0 s for c16384, 2.8 s for c16384w, 1.0 - 1.6 s for each of the others: 17 s for all eight."""
import numpy as np

import plaid_exact_cases as X
from test_bank_ivf_cpu import ivf_numpy

DERIVED = {
    "c300q48":   dict(C=300, D=64, nbits=4, Lq=48, Lqc=30, ncells=4, ndocs=16, k=4, nq=2, n_base=270, seed=5),
    "c1000w100": dict(C=1000, D=128, nbits=2, Lq=100, Lqc=40, ncells=4, ndocs=32, k=8, nq=2, n_base=90, seed=6),
}
OVERRIDE = {"c262144": dict(n_base=27)}
CASES = list(X.CASES) + list(DERIVED)
JT = {"c257": 2, "c300": 8, "c1000": 2, "c16384": 2, "c16384w": 2, "c262144": 1, "c300q48": 4, "c1000w100": 8}
CHUNK = 8192                                             # centroids a block of the float64 product


def li_pick_jt(Lq):
    """The column tile of stage 3 (li_pick_jt, csrc/li_scores_core.h), restated: what the cases are chosen to cover."""
    return 1 if Lq <= 16 else 2 if Lq <= 32 else 4 if Lq <= 64 else 8


def params(name):
    return dict(X.CASES[name], **OVERRIDE.get(name, {})) if name in X.CASES else dict(DERIVED[name])


def assert_exact(rows, cen):
    """rows [n, D] . cen [C, D] in the style of plaid_exact_cases._assert_exact, without the [n, C] matrix: every product a multiple
    of 2^-5 (rows: of 1/8, centroids: of 1/4), every sum of |products| at most max |row entry| * max sum |centroid row| < 2^19."""
    assert (rows * 8 == np.round(rows * 8)).all() and (cen * 4 == np.round(cen * 4)).all(), "a product is no multiple of 2^-5"
    bound = np.abs(rows).max() * np.abs(cen).sum(axis=1).max()
    assert bound < 2.0 ** 19, f"a row's sum of |products| may reach {bound}"


def codes64_of(rows, cen):
    """int32 [n]: per row the LOWEST index among the maxima of the float64 product rows @ cen.T, and how many centroids share that
    maximum below index 256 and from 256 on (int32 [n, 2])."""
    rows, cen = np.asarray(rows, dtype=np.float64), np.asarray(cen, dtype=np.float64)
    assert_exact(rows, cen)
    best = np.full(len(rows), -np.inf)
    code = np.zeros(len(rows), dtype=np.int64)
    shared = np.zeros((len(rows), 2), dtype=np.int32)
    for c0 in range(0, len(cen), CHUNK):
        s = rows @ cen[c0:c0 + CHUNK].T
        at = s.argmax(axis=1)                             # numpy: the first maximum of the block
        top = s[np.arange(len(rows)), at]
        hit = s == top[:, None]
        cut = max(0, min(CHUNK, 256 - c0))
        here = np.stack([hit[:, :cut].sum(axis=1), hit[:, cut:].sum(axis=1)], axis=1).astype(np.int32)
        better, equal = top > best, top == best           # strictly: an equal maximum of a later block does not take the code
        best[better], code[better] = top[better], c0 + at[better]
        shared[better] = here[better]
        shared[equal] += here[equal]
    assert (shared.sum(axis=1) >= 1).all() and np.isfinite(best).all()
    return code.astype(np.int32), shared


def build(name):
    """The coded case: the compressed case's dict with `rows` (= decoded, fp16), `codes64`, `shared`, and `codes` REPLACED by codes64
    (so that plaid_exact_cases.oracle prunes over them); the compressed case's own codes stay as `codes_compressed`."""
    case = X.build_from(params(name), name)
    assert li_pick_jt(case["Lq"]) == JT[name]
    codes64, shared = codes64_of(case["decoded"], case["centroids"])
    return dict(case, rows=case["decoded"], codes64=codes64, shared=shared, codes=codes64, codes_compressed=case["codes"])


def masked_for(case, gone):
    """The case with the passages `gone` (bool [P]) fully masked: what a filter that clears them makes of the search."""
    return dict(case, mask=np.where(np.repeat(gone, case["lens"]), 0, case["mask"]).astype(np.uint8))


def every_third(case):
    return np.arange(len(case["lens"])) % 3 == 2


def ivf_of(case):
    """(pids int32, lengths int64 [C]) of the inverted file over codes64, as PassageBank.ivf returns them.  ivf_numpy is the
    definition one list at a time; above 16 384 lists only the lists some row names are asked of it (the others are empty)."""
    C = case["C"]
    if C <= 16384:
        off, pids = ivf_numpy(case["codes64"], case["mask"], case["lens"], C)
        return pids, np.diff(off)
    used = np.unique(case["codes64"])
    off, pids = ivf_numpy(np.searchsorted(used, case["codes64"]), case["mask"], case["lens"], len(used))
    lengths = np.zeros(C, dtype=np.int64)
    lengths[used] = np.diff(off)
    return pids, lengths


_BUILT = {}


def get(name):
    """(case, oracle, oracle under the every-third filter), built once a process and left unchanged by whoever takes it."""
    if name not in _BUILT:
        case = build(name)
        _BUILT[name] = (case, X.oracle(case), X.oracle(masked_for(case, every_third(case))))
    return _BUILT[name]
