"""rqsid_assign_topk's host side: declared, bound and exported, and every refusal returns before any launch
(no GPU needed: the pointers below are never dereferenced)."""
import re
import subprocess
from pathlib import Path

import pytest

from generative_ranking_recommender_amd import _lib

REPO = Path(__file__).resolve().parent.parent
NAMES = ("rqsid_assign_topk_workspace_bytes", "rqsid_assign_topk")


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
    assert re.search(r"#define\s+RQSID_TOPK_MAX\s+8\b", header)
    assert len(_lib.SIGNATURES["rqsid_assign_topk"][1]) == 33
    assert "assign_topk.hip" in {p.name for p in _lib.SRCS}


def test_workspace_query_is_monotone(lib):
    q = lib.rqsid_assign_topk_workspace_bytes
    assert q(0, 1) >= 16  # the error word and the three counters
    for k in (1, 2, 8):
        sizes = [q(n, k) for n in (0, 1, 1000, 10_000_000, 2**31 - 1)]
        assert sizes == sorted(sizes)
    for n in (1, 1000, 10_000_000):
        sizes = [q(n, k) for k in range(1, 9)]
        assert sizes == sorted(sizes)


P = dict(x=0x1000, sro=0x2000, sto=0x3000, centers=0x4000, meta=0x5000, base=0x6000, count=0x7000, ol=0x8000,
         og=0x9000, od=0xA000, ws=0xB000)


def _call(lib, *, x_format=0, n=256, dim=64, k=2, ws_bytes=None, **over):
    p = dict(P, **over)
    if ws_bytes is None:
        ws_bytes = lib.rqsid_assign_topk_workspace_bytes(max(n, 0), max(k, 1))
    return lib.rqsid_assign_topk(p["x"], x_format, n, dim, None, 1, p["sro"], p["sto"], 2, p["centers"], p["meta"], 16,
                                 p["base"], p["count"], 16, None, None, None, 0, 0, None, None, None, None, None, None,
                                 k, p["ol"], p["og"], p["od"], p["ws"], ws_bytes, None)


@pytest.mark.parametrize("kwargs, code", [
    (dict(k=0), -1),
    (dict(k=9), -1),
    (dict(dim=48), -1),
    (dict(dim=1056), -1),
    (dict(x_format=7), -1),
    (dict(od=None), -1),
    (dict(x=None), -1),
    (dict(centers=None), -1),
    (dict(ws_bytes="short"), -3),
    (dict(ws=None), -3),
])
def test_refusals_before_any_launch(lib, kwargs, code):
    kwargs = dict(kwargs)
    if kwargs.get("ws_bytes") == "short":
        kwargs["ws_bytes"] = lib.rqsid_assign_topk_workspace_bytes(256, 2) - 1
    lib.rqsid_prepare_centers(None, 4, 48, None, None, None)  # another error text first
    assert _call(lib, **kwargs) == code
    assert "assign_topk" in lib.rqsid_last_error().decode()


def test_no_rows_succeeds_with_null_data_pointers(lib):
    none = {k: None for k in P}
    assert _call(lib, n=0, ws_bytes=0, **none) == 0
    assert _call(lib, n=0, k=9, ws_bytes=0, **none) == -1  # the limits are checked first


def test_argument_error_maps_to_value_error(lib):
    with pytest.raises(ValueError):
        _lib.check(_call(lib, k=0), "rqsid_assign_topk")
    with pytest.raises(RuntimeError):
        _lib.check(_call(lib, ws_bytes=0), "rqsid_assign_topk")
