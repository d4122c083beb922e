"""rqsid_assign_x (16-bit row formats): declared, bound, exported, and an unknown format is refused on the host."""
import re
import subprocess

import pytest

from generative_ranking_recommender_amd import _lib


def test_assign_x_is_bound_and_exported():
    assert "rqsid_assign_x" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["rqsid_assign_x"]
    r0, a0 = _lib.SIGNATURES["rqsid_assign"]
    # the row pointer, the format, then every argument of rqsid_assign in its order
    assert res == r0 and args == [a0[0], _lib.c_i32] + a0[1:]
    _lib.build()
    assert hasattr(_lib.load(), "rqsid_assign_x")
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    assert "rqsid_assign_x" in set(re.findall(r"\bT (rqsid_\w+)", out))


def test_header_names_the_row_formats():
    text = _lib.HEADER.read_text()
    got = {m[0]: int(m[1]) for m in re.findall(r"^#define (RQSID_X_\w+) (\d+)", text, re.M)}
    assert got == {"RQSID_X_F32": 0, "RQSID_X_F16": 1, "RQSID_X_BF16": 2}


@pytest.mark.parametrize("x_format", [3, -1])
def test_unknown_row_format_is_an_argument_error(x_format):
    """The format check runs before any other work: no GPU, no launch."""
    lib = _lib.load()
    nargs = len(_lib.SIGNATURES["rqsid_assign_x"][1])
    args = [None, x_format] + [0 if t in (_lib.c_i32, _lib.c_i64) else None
                               for t in _lib.SIGNATURES["rqsid_assign_x"][1][2:]]
    assert len(args) == nargs
    rc = lib.rqsid_assign_x(*args)
    assert rc == -1
    msg = lib.rqsid_last_error().decode()
    assert "assign" in msg and "x_format" in msg
    with pytest.raises(ValueError):
        _lib.check(rc, "rqsid_assign_x")
