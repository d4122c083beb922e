"""rqsid_probe_knn's host side: declared, bound and exported, and every refusal returns before any HIP call
(no GPU needed: the pointers below are never dereferenced)."""
import re
import subprocess
from pathlib import Path

import pytest

from generative_ranking_recommender_amd import _lib

REPO = Path(__file__).resolve().parent.parent
NAMES = ("rqsid_probe_knn_workspace_bytes", "rqsid_probe_knn")


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
    assert re.search(r"#define\s+RQSID_PROBE_MAX\s+32\b", header)
    assert len(_lib.SIGNATURES["rqsid_probe_knn"][1]) == 19
    assert len(_lib.SIGNATURES["rqsid_probe_knn_workspace_bytes"][1]) == 4
    assert "probe_knn.hip" in {p.name for p in _lib.SRCS}
    assert "knn_core.h" in {p.name for p in _lib.DEPS}


def test_workspace_query_is_monotone(lib):
    q = lib.rqsid_probe_knn_workspace_bytes
    assert q(0, 0, 1, 1) >= 20  # the error word and the four counters
    # (the sizes around 2^23 rows are where the item sort's key count reaches its cap)
    sizes = [q(n, 1000, 4, 10) for n in (0, 1, 127, 128, 129, 1000, 2_000_000, 8_388_000, 8_388_608, 8_388_736,
                                          10_000_000, 2**31 - 1)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    sizes = [q(100_000, m, 4, 10) for m in (0, 1, 31, 32, 33, 128, 129, 50_000)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    sizes = [q(100_000, 1000, p, 10) for p in range(1, 33)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    sizes = [q(100_000, 1000, 4, k) for k in range(1, 17)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    # per item (padded to 128): one 16-byte record, k + 8 (value, row) pairs, four int32 tables; and two column
    # tables: with so few items a block holds one item, so 128 columns per item; from 128 items per block on, one
    assert q(100_000, 128, 2, 10) - q(100_000, 128, 1, 10) == 128 * (16 + 18 * 8 + 4 * 4) + 128 * 128 * 2 * 4
    assert q(100_000, 2**19, 2, 10) - q(100_000, 2**19, 1, 10) == 2**19 * (16 + 18 * 8 + 6 * 4)
    sizes = [q(100_000, m, 1, 10) for m in (1000, 1023, 1024, 2047, 2048, 2049, 4095, 4096, 131_071, 131_072, 200_000)]
    assert sizes == sorted(sizes)  # (the sizes at which the items per block change)
    for bad in ((-1, 10, 4, 10), (2**31, 10, 4, 10), (1000, -1, 4, 10), (1000, 10, 0, 10), (1000, 10, 33, 10),
                (1000, 10, 4, 0), (1000, 10, 4, 17), (1000, 2**30, 2, 10)):
        lib.rqsid_prepare_centers(None, 4, 48, None, None, None)  # another error text first
        assert q(*bad) == -1, bad
        assert "probe_knn" in lib.rqsid_last_error().decode()
    assert q(1000, 2**30 - 1, 2, 10) > 0  # 2^31 - 2 items


P = dict(x=0x1000, q=0x3000, qself=0x4000, lo=0x5000, hi=0x5800, rows=0x6000, val=0x7000, scanned=0x8000, ws=0xA000)


def _call(lib, *, x_format=0, n=1000, dim=64, m=100, probes=4, metric=0, k=10, ws_bytes=None, **over):
    p = dict(P, **over)
    if ws_bytes is None:
        ws_bytes = max(lib.rqsid_probe_knn_workspace_bytes(max(n, 0), min(max(m, 0), 1000), min(max(probes, 1), 32),
                                                           min(max(k, 1), 16)), 0)
    return lib.rqsid_probe_knn(p["x"], x_format, n, dim, None, p["q"], m, p["qself"], probes, p["lo"], p["hi"],
                               metric, k, p["rows"], p["val"], p["scanned"], p["ws"], ws_bytes, None)


@pytest.mark.parametrize("kwargs, code", [
    (dict(x_format=7), -1),
    (dict(dim=0), -1),
    (dict(dim=48), -1),
    (dict(dim=1056), -1),
    (dict(k=0), -1),
    (dict(k=17), -1),
    (dict(probes=0), -1),
    (dict(probes=33), -1),
    (dict(metric=2), -1),
    (dict(metric=-1), -1),
    (dict(n=2**31), -1),
    (dict(m=-1), -1),
    (dict(m=2**30, probes=2), -1),       # 2^31 items
    (dict(x=None), -1),
    (dict(q=None), -1),
    (dict(x=0x1008), -1),
    (dict(q=0x3004), -1),
    (dict(lo=None), -1),
    (dict(hi=None), -1),
    (dict(rows=None), -1),
    (dict(val=None), -1),
    (dict(ws_bytes="short"), -3),
    (dict(ws=None), -3),
])
def test_refusals_before_any_hip_call(lib, kwargs, code):
    kwargs = dict(kwargs)
    if kwargs.get("ws_bytes") == "short":
        kwargs["ws_bytes"] = lib.rqsid_probe_knn_workspace_bytes(1000, 100, 4, 10) - 1
    lib.rqsid_prepare_centers(None, 4, 48, None, None, None)  # another error text first
    assert _call(lib, **kwargs) == code
    assert "probe_knn" in lib.rqsid_last_error().decode()


def test_zero_sizes_succeed_with_null_pointers(lib):
    none = {k: None for k in P}
    assert _call(lib, n=0, ws_bytes=0, **none) == 0
    assert _call(lib, m=0, ws_bytes=0, **none) == 0
    assert _call(lib, n=0, dim=48, ws_bytes=0, **none) == -1  # the limits are checked first
    assert _call(lib, m=0, probes=33, ws_bytes=0, **none) == -1


def test_error_codes_map_to_exceptions(lib):
    with pytest.raises(ValueError):
        _lib.check(_call(lib, probes=33), "rqsid_probe_knn")
    with pytest.raises(RuntimeError):
        _lib.check(_call(lib, ws_bytes=0), "rqsid_probe_knn")
