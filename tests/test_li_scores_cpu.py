"""The formula the GPU tests of rr_li_scores use, pinned to the reference's own function: tests/golden/li_scores_ref.npz
holds what colbert_score (flmr_utils.py:22-48), executed from the reference's source text by
tests/golden/make_li_scores_fixture.py, returned on the int_tiny geometry.  Reads only the committed file."""
import torch

from li_scores_ref import MASKED, li_scores_formula, load_li_scores_ref


def test_formula_reproduces_the_references_arrays_bit_for_bit():
    g = load_li_scores_ref()
    assert (g["Bq"], g["K"], g["Lq"], g["Lc"], g["D"]) == (2, 3, 9, 40, 64)
    maxsim, scores = li_scores_formula(g["query_li"], g["context_li"], g["context_mask"], g["K"])
    assert scores.dtype == torch.float32 and torch.equal(scores, g["scores"])
    assert torch.equal(maxsim, g["maxsim"])


def test_fixture_has_the_shape_the_retriever_produces():
    g = load_li_scores_ref()
    cm, sc = g["context_mask"].bool(), g["scores"]
    assert (sc[~cm] == MASKED).all() and sc[cm].abs().max() <= 1.0 + 1e-6          # unit-norm rows: cosines
    lengths = [int(r.nonzero().max()) + 1 if r.any() else 0 for r in cm]
    assert any((~cm[n, :lengths[n]]).any() for n in range(cm.shape[0])), "no hole inside a passage"
    full = [n for n in range(cm.shape[0]) if not cm[n].any()]
    assert full == [4] and float(g["maxsim"][4]) == MASKED * g["Lq"]              # integers below 2^24: exact
    assert (g["query_li"].norm(dim=-1) - 1).abs().max() < 1e-6


def test_float64_formula_is_within_the_dot_product_bound_of_the_fixture():
    """The bound the GPU test applies to the kernel, applied to torch's own fp32 matmul: D * 2^-23 per entry."""
    g = load_li_scores_ref()
    m64, s64 = li_scores_formula(g["query_li"], g["context_li"], g["context_mask"], g["K"], torch.float64)
    cm = g["context_mask"].bool()
    assert (g["scores"].double() - s64)[cm].abs().max() <= g["D"] * 2.0 ** -23
    assert (g["maxsim"].double() - m64).abs().max() <= g["Lq"] * g["D"] * 2.0 ** -23 + g["Lq"] ** 2 * 2.0 ** -24
