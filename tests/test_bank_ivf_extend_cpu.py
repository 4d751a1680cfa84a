"""CPU: rr_bank_extend_ivf (include/rerank_mi355.h, "THE INVERTED FILE") where no device is needed: the entry is exported and bound,
a NULL bank is refused before anything touches a device, and the Python surface (PassageBank.extend_ivf, RerankEngine.bank_extend_ivf,
the `extend_ivf=` keyword of the three calls that add passages) is there with the defaults that keep the earlier behaviour."""
import inspect
import os
import re

from rmr_amd import PassageBank, RerankEngine
from rmr_amd import _lib as L

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "rerank_mi355.h")


def test_the_entry_is_declared_exported_and_bound():
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"^int rr_bank_extend_ivf\(rr_bank_handle b, void\* hip_stream\);", text, re.M)
    lib = L.load()
    fn = lib.rr_bank_extend_ivf                                   # AttributeError: not exported
    assert fn.argtypes is not None and len(fn.argtypes) == 2 and fn.argtypes == lib.rr_bank_build_ivf.argtypes
    assert fn.restype is lib.rr_bank_build_ivf.restype


def test_a_null_bank_is_refused_without_a_device():
    lib = L.load()
    assert lib.rr_bank_extend_ivf(None, None) == L.RR_ERR_BAD_ARG
    assert lib.rr_bank_build_ivf(None, None) == L.RR_ERR_BAD_ARG  # the refusal it shares


def test_the_python_surface_and_its_defaults():
    sig = inspect.signature(PassageBank.extend_ivf)
    assert list(sig.parameters) == ["self"] and "rr_bank_extend_ivf" in PassageBank.extend_ivf.__doc__
    assert list(inspect.signature(RerankEngine.bank_extend_ivf).parameters) == ["self", "bank"]
    for name in ("add_compress", "add_compressed", "load_plaid_index"):
        p = inspect.signature(getattr(PassageBank, name)).parameters
        assert "extend_ivf" in p and p["extend_ivf"].default is False, name
        assert list(p)[-1] == "extend_ivf", f"{name}: the new keyword comes last, so positional callers see no change"
