"""rqsid_quant_error's host side: declared, bound and exported, and every refusal returns before any launch
(no GPU needed: the pointers below are never dereferenced)."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest

from generative_ranking_recommender_amd import _lib

REPO = Path(__file__).resolve().parent.parent
NAMES = ("rqsid_quant_error_workspace_bytes", "rqsid_quant_error")


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_declared_bound_and_exported(lib):
    header = (REPO / "include" / "rqsid.h").read_text()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (rqsid_\w+)", out))
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        assert name in exported, name
    assert len(_lib.SIGNATURES["rqsid_quant_error"][1]) == 22
    assert "quant_error.hip" in {p.name for p in _lib.SRCS}
    assert "quant_error.hip" in (REPO / "tools" / "ab_build.sh").read_text()


def test_workspace_query(lib):
    sizes = [lib.rqsid_quant_error_workspace_bytes(n) for n in (0, 1, 1000, 10_000_000, 2**31 - 1)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert lib.rqsid_quant_error_workspace_bytes(-1) == -1


# n = 0: every check comes before the empty-input return, and a call the checks let through launches nothing
def _call(lib, *, x=0x1000, x_format=0, n=0, dim=64, n_levels=1, err=0x2000, ws=0x3000, ws_bytes=None,
          c0=0x4000, id0=0x5000):
    if ws_bytes is None:
        ws_bytes = lib.rqsid_quant_error_workspace_bytes(n)
    return lib.rqsid_quant_error(x, x_format, n, dim, None, n_levels, 1, c0, 4, id0, None, 0, None, None, 0, None,
                                 err, None, None, ws, ws_bytes, None)


@pytest.mark.parametrize("kwargs, code", [
    (dict(x_format=3), -1),
    (dict(n_levels=0), -1),
    (dict(n_levels=4), -1),
    (dict(dim=48), -1),
    (dict(err=None), -1),
    (dict(x=None), -1),
    (dict(c0=None), -1),
    (dict(id0=None), -1),
    (dict(n=-1), -1),
    (dict(n_levels=2), -1),   # level 1 used but its pointers are NULL
    (dict(ws_bytes="short"), -3),
])
def test_refusals_before_any_launch(lib, kwargs, code):
    kwargs = dict(kwargs)
    if kwargs.get("ws_bytes") == "short":
        kwargs["ws_bytes"] = lib.rqsid_quant_error_workspace_bytes(8) - 1
    # clear the thread's error text with a call that sets another one
    lib.rqsid_prepare_centers(None, 4, 48, None, None, None)
    assert _call(lib, **kwargs) == code
    assert "quant_error" in lib.rqsid_last_error().decode()


def test_argument_error_maps_to_value_error(lib):
    with pytest.raises(ValueError):
        _lib.check(_call(lib, dim=48), "rqsid_quant_error")
    with pytest.raises(RuntimeError):
        _lib.check(_call(lib, ws_bytes=0), "rqsid_quant_error")
    assert isinstance(ctypes.c_int64(lib.rqsid_quant_error_workspace_bytes(1)).value, int)
