"""rqsid_id_cells's host side: declared, bound and exported, and every refusal returns before any HIP call
(no GPU needed: the pointers below are never dereferenced)."""
import re
import subprocess
from pathlib import Path

import pytest

from generative_ranking_recommender_amd import _lib

REPO = Path(__file__).resolve().parent.parent
NAMES = ("rqsid_id_cells_lds_rows", "rqsid_id_cells_workspace_bytes", "rqsid_id_cells")
FINE_MAX = 8192


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
    assert re.search(r"#define\s+RQSID_CELLS_FINE_MAX\s+%d\b" % FINE_MAX, header)
    assert re.search(r"#define\s+RQSID_CELLS_GROUP_SKIP\s+1u\b", header)
    assert len(_lib.SIGNATURES["rqsid_id_cells"][1]) == 18
    assert len(_lib.SIGNATURES["rqsid_id_cells_workspace_bytes"][1]) == 3
    assert "id_cells.hip" in {p.name for p in _lib.SRCS}
    c = lib.rqsid_id_cells_lds_rows()
    assert c >= 64 and c & (c - 1) == 0  # the sort's width


def test_workspace_query(lib):
    q = lib.rqsid_id_cells_workspace_bytes
    assert q(0, 0, 1) >= 4 + 37 * 4  # the error word and the counters
    sizes = [q(n, 100, 256) for n in (0, 1, 1000, 10_000_000, 2**31 - 1)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    sizes = [q(100_000, g, 256) for g in (0, 1, 2, 16385, 2**24 + 1)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    sizes = [q(100_000, 100, f) for f in (1, 2, 255, 256, 257, FINE_MAX)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    for bad in ((-1, 10, 16), (2**31, 10, 16), (1000, 10, 0), (1000, 10, FINE_MAX + 1), (1000, -1, 16)):
        lib.rqsid_prepare_centers(None, 4, 48, None, None, None)  # another error text first
        assert q(*bad) == -1, bad
        assert "id_cells" in lib.rqsid_last_error().decode()


P = dict(idx=0x1000, sro=0x2000, flags=0x3000, fine=0x4000, key=0x5000, order=0x6000, rank=0x7000, size=0x8000,
         cell=0x9000, off=0xA000, grp=0xB000, cfine=0xC000, ws=0xD000)


def _call(lib, *, n=1000, n_groups=8, n_fine=16, ws_bytes=None, **over):
    p = dict(P, **over)
    if ws_bytes is None:
        ws_bytes = max(lib.rqsid_id_cells_workspace_bytes(max(min(n, 2**31 - 1), 0), max(n_groups, 0),
                                                          min(max(n_fine, 1), FINE_MAX)), 0)
    return lib.rqsid_id_cells(n, p["idx"], n_groups, p["sro"], p["flags"], p["fine"], n_fine, p["key"], p["order"],
                              p["rank"], p["size"], p["cell"], p["off"], p["grp"], p["cfine"], p["ws"], ws_bytes, None)


@pytest.mark.parametrize("kwargs, code", [
    (dict(n=-1), -1),
    (dict(n=2**31), -1),
    (dict(n_fine=0), -1),
    (dict(n_fine=FINE_MAX + 1), -1),
    (dict(n_groups=0), -1),
    (dict(n_groups=-3), -1),
    (dict(sro=None), -1),
    (dict(fine=None, n_fine=2), -1),      # NULL fine_id means one cell per group
    (dict(order=None), -1),
    (dict(rank=None), -1),
    (dict(size=None), -1),
    (dict(cell=None), -1),
    (dict(off=None), -1),
    (dict(grp=None), -1),
    (dict(cfine=None), -1),
    (dict(ws_bytes="short"), -3),
    (dict(ws=None), -3),
])
def test_refusals_before_any_hip_call(lib, kwargs, code):
    kwargs = dict(kwargs)
    if kwargs.get("ws_bytes") == "short":
        kwargs["ws_bytes"] = lib.rqsid_id_cells_workspace_bytes(1000, 8, 16) - 1
    lib.rqsid_prepare_centers(None, 4, 48, None, None, None)  # another error text first
    assert _call(lib, **kwargs) == code
    assert "id_cells" in lib.rqsid_last_error().decode()


def test_zero_rows_succeed_with_null_pointers(lib):
    none = {k: None for k in P}
    assert _call(lib, n=0, ws_bytes=0, **none) == 0
    assert _call(lib, n=0, n_groups=0, ws_bytes=0, **none) == 0
    assert _call(lib, n=0, n_fine=0, ws_bytes=0, **none) == -1  # the limits are checked first


def test_error_codes_map_to_exceptions(lib):
    with pytest.raises(ValueError):
        _lib.check(_call(lib, n_fine=0), "rqsid_id_cells")
    with pytest.raises(RuntimeError):
        _lib.check(_call(lib, ws_bytes=0), "rqsid_id_cells")
