"""Host side of rqsid_id_trie, rqsid_trie_mask and rqsid_trie_beam_step: declared, bound and exported, and every
refusal returns before any HIP call (no GPU needed: the device pointers below are never dereferenced)."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest

from generative_ranking_recommender_amd import _lib

REPO = Path(__file__).resolve().parent.parent
NAMES = ("rqsid_id_trie_workspace_bytes", "rqsid_id_trie", "rqsid_trie_mask_workspace_bytes", "rqsid_trie_mask",
         "rqsid_trie_beam_step")
LEVELS_MAX, VOCAB_MAX, BEAM_MAX, FINE_MAX = 8, 1 << 20, 64, 8192


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _sizes(*s):
    return (ctypes.c_int32 * len(s))(*s)


def test_declared_bound_and_exported(lib):
    header = (REPO / "include" / "rqsid.h").read_text()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (rqsid_\w+)", out))
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        assert name in exported, name
    assert re.search(r"#define\s+RQSID_TRIE_LEVELS_MAX\s+%d\b" % LEVELS_MAX, header)
    assert re.search(r"#define\s+RQSID_TRIE_VOCAB_MAX\s+%d\b" % VOCAB_MAX, header)
    assert re.search(r"#define\s+RQSID_TRIE_BEAM_MAX\s+%d\b" % BEAM_MAX, header)
    assert len(_lib.SIGNATURES["rqsid_id_trie"][1]) == 13
    assert len(_lib.SIGNATURES["rqsid_trie_mask"][1]) == 24
    assert len(_lib.SIGNATURES["rqsid_trie_beam_step"][1]) == 23
    assert "id_trie.hip" in {p.name for p in _lib.SRCS}


def test_workspace_queries_are_monotone(lib):
    q = lib.rqsid_id_trie_workspace_bytes
    sizes = [q(n, 3) for n in (0, 1, 2047, 2048, 2049, 5_280_000, 2**31 - 1)]
    assert sizes == sorted(sizes) and sizes[0] >= 256
    assert q(100_000, 1) <= q(100_000, 8)
    for bad in ((-1, 3), (2**31, 3), (100, 0), (100, LEVELS_MAX + 1)):
        lib.rqsid_prepare_centers(None, 4, 48, None, None, None)  # another error text first
        assert q(*bad) == -1, bad
        assert "rqsid_id_trie" in lib.rqsid_last_error().decode()
    m = lib.rqsid_trie_mask_workspace_bytes
    sizes = [m(b) for b in (0, 1, 64, 2048, 2**31 - 1)]
    assert sizes == sorted(sizes) and sizes[0] >= 16
    for bad in (-1, 2**31):
        lib.rqsid_prepare_centers(None, 4, 48, None, None, None)
        assert m(bad) == -1
        assert "rqsid_trie_mask" in lib.rqsid_last_error().decode()


T = dict(grp=0x1000, fine=0x2000, keep=0x3000, count=0x4000, value=0x5000, child=0x6000, leaf=0x7000, ws=0x8000)


def _trie(lib, *, n=1000, levels=3, sizes=(5, 4, 7), ws_bytes=None, **over):
    p = dict(T, **over)
    if ws_bytes is None:
        ws_bytes = max(lib.rqsid_id_trie_workspace_bytes(max(min(n, 2**31 - 1), 0), min(max(levels, 1), 8)), 0)
    return lib.rqsid_id_trie(n, p["grp"], p["fine"], levels, None if sizes is None else _sizes(*sizes), p["keep"],
                             p["count"], p["value"], p["child"], p["leaf"], p["ws"], ws_bytes, None)


@pytest.mark.parametrize("kwargs, code", [
    (dict(n=-1), -1),
    (dict(n=2**31), -1),
    (dict(levels=0, sizes=(4,)), -1),
    (dict(levels=9, sizes=(2,) * 9), -1),
    (dict(sizes=None), -1),
    (dict(sizes=(5, 0, 7)), -1),
    (dict(sizes=(5, 4, FINE_MAX + 1)), -1),           # the last level's limit
    (dict(sizes=(4097, 4096, 7)), -1),                # the other levels multiply to more than 2^24
    (dict(levels=1, sizes=(2**24 + 1,)), -1),
    (dict(grp=None), -1),
    (dict(fine=None), -1),
    (dict(count=None), -1),
    (dict(value=None), -1),
    (dict(child=None), -1),
    (dict(leaf=None), -1),
    (dict(ws_bytes="short"), -3),
    (dict(ws=None), -3),
])
def test_id_trie_refusals_before_any_hip_call(lib, kwargs, code):
    kwargs = dict(kwargs)
    if kwargs.get("ws_bytes") == "short":
        kwargs["ws_bytes"] = lib.rqsid_id_trie_workspace_bytes(1000, 3) - 1
    lib.rqsid_prepare_centers(None, 4, 48, None, None, None)  # another error text first
    assert _trie(lib, **kwargs) == code
    assert "rqsid_id_trie" in lib.rqsid_last_error().decode()


def test_id_trie_zero_cells_succeed_with_null_pointers(lib):
    none = {k: None for k in T}
    assert _trie(lib, n=0, ws_bytes=0, **none) == 0
    assert _trie(lib, n=0, levels=1, sizes=(9,), ws_bytes=0, **none) == 0
    assert _trie(lib, n=0, levels=0, sizes=(9,), ws_bytes=0, **none) == -1  # the limits are checked first


M = dict(count=0x1000, value=0x2000, child=0x3000, ids=0x4000, scores=0x5000, code=0x6000, ltok=0x7000, kind=0x8000,
         node=0x9000, cnt=0xA000, ws=0xB000)


def _mask(lib, *, cap=100, levels=3, sizes=(5, 4, 7), ids_format=1, B=8, T_len=6, ids_ld=None, x_format=0, V=1003,
          ld=None, eos=1, ws_bytes=None, **over):
    p = dict(M, **over)
    if ws_bytes is None:
        ws_bytes = max(lib.rqsid_trie_mask_workspace_bytes(max(min(B, 2**31 - 1), 0)), 0)
    return lib.rqsid_trie_mask(cap, levels, None if sizes is None else _sizes(*sizes), p["count"], p["value"],
                               p["child"], p["ids"], ids_format, B, T_len, T_len if ids_ld is None else ids_ld,
                               p["scores"], x_format, V, V if ld is None else ld, p["code"], p["ltok"], eos,
                               p["kind"], p["node"], p["cnt"], p["ws"], ws_bytes, None)


@pytest.mark.parametrize("kwargs, code", [
    (dict(cap=-1), -1),
    (dict(levels=0), -1),
    (dict(levels=9, sizes=(2,) * 9), -1),
    (dict(sizes=None), -1),
    (dict(sizes=(5, 4, FINE_MAX + 1)), -1),
    (dict(ids_format=2), -1),
    (dict(x_format=3), -1),
    (dict(x_format=-1), -1),
    (dict(B=-1), -1),
    (dict(B=2**31), -1),
    (dict(T_len=-1), -1),
    (dict(V=-1), -1),
    (dict(V=VOCAB_MAX + 1), -1),
    (dict(ld=1002), -1),                 # ld < vocab
    (dict(ids_ld=5), -1),                # ids_ld < n_tokens
    (dict(eos=-1), -1),
    (dict(eos=1003), -1),
    (dict(B=2**24, V=VOCAB_MAX), -1),    # rows x slices beyond a grid
    (dict(count=None), -1),
    (dict(value=None), -1),
    (dict(child=None), -1),
    (dict(ids=None), -1),
    (dict(scores=None), -1),
    (dict(scores=0x5001, x_format=1), -1),  # not aligned to the element
    (dict(code=None), -1),
    (dict(ltok=None), -1),
    (dict(ws_bytes="short"), -3),
    (dict(ws=None), -3),
])
def test_trie_mask_refusals_before_any_hip_call(lib, kwargs, code):
    kwargs = dict(kwargs)
    if kwargs.get("ws_bytes") == "short":
        kwargs["ws_bytes"] = lib.rqsid_trie_mask_workspace_bytes(8) - 1
    lib.rqsid_prepare_centers(None, 4, 48, None, None, None)
    assert _mask(lib, **kwargs) == code
    assert "rqsid_trie_mask" in lib.rqsid_last_error().decode()


def test_trie_mask_zero_sizes_succeed_with_null_pointers(lib):
    none = {k: None for k in M}
    assert _mask(lib, B=0, ws_bytes=0, **none) == 0
    assert _mask(lib, V=0, eos=0, ws_bytes=0, **none) == 0
    assert _mask(lib, B=0, V=0, T_len=0, ws_bytes=0, **none) == 0
    assert _mask(lib, B=0, levels=0, ws_bytes=0, **none) == -1  # the limits are checked first


S = dict(count=0x1000, value=0x2000, child=0x3000, node_in=0x4000, score_in=0x5000, logp=0x6000, ltok=0x7000,
         node=0x8000, score=0x9000, parent=0xA000, val=0xB000, tok=0xC000)


def _step(lib, *, cap=100, levels=3, sizes=(5, 4, 7), depth=1, B=3, beam_in=4, beam_out=5, x_format=0, V=17, ld=None,
          **over):
    p = dict(S, **over)
    return lib.rqsid_trie_beam_step(cap, levels, None if sizes is None else _sizes(*sizes), p["count"], p["value"],
                                    p["child"], depth, B, beam_in, beam_out, p["node_in"], p["score_in"], p["logp"],
                                    x_format, V, V if ld is None else ld, p["ltok"], p["node"], p["score"],
                                    p["parent"], p["val"], p["tok"], None)


@pytest.mark.parametrize("kwargs", [
    dict(cap=-1), dict(levels=0), dict(sizes=None), dict(sizes=(5, 4, 0)), dict(depth=-1), dict(depth=3),
    dict(beam_in=0), dict(beam_in=BEAM_MAX + 1), dict(beam_out=0), dict(beam_out=BEAM_MAX + 1), dict(B=-1),
    dict(x_format=3), dict(V=0), dict(V=VOCAB_MAX + 1), dict(ld=16), dict(count=None), dict(value=None),
    dict(child=None), dict(node_in=None), dict(logp=None), dict(ltok=None), dict(node=None), dict(score=None),
])
def test_trie_beam_step_refusals_before_any_hip_call(lib, kwargs):
    lib.rqsid_prepare_centers(None, 4, 48, None, None, None)
    assert _step(lib, **kwargs) == -1
    assert "rqsid_trie_beam_step" in lib.rqsid_last_error().decode()


def test_trie_beam_step_zero_rows_succeed_with_null_pointers(lib):
    none = {k: None for k in S}
    assert _step(lib, B=0, **none) == 0
    assert _step(lib, B=0, beam_out=0, **none) == -1  # the limits are checked first


def test_error_codes_map_to_exceptions(lib):
    with pytest.raises(ValueError):
        _lib.check(_trie(lib, levels=0), "rqsid_id_trie")
    with pytest.raises(RuntimeError):
        _lib.check(_mask(lib, ws_bytes=0), "rqsid_trie_mask")
