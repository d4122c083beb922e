"""Where rqsid_assign_pair runs the 2-term pairwise screen (csrc/assign_plan.h, AssignPlan::pair), asked of the
library's own host-only query rqsid_assign_plan_pair: no GPU.  The form is the per-tile single-pass 3-term screen
of fp32 rows with a pair table present; everything else keeps what tests/test_assign_plan.py pins."""
import pytest

from generative_ranking_recommender_amd import _lib

BASE = dict(x_format=0, n_rows=1_000_000, dim=512, n_segments=128, cand_count_max=128, res_levels=1, norm=1,
            screen_terms=0, has_cand_lid=0, has_den_out=1, has_pair=1)
ORDER = ["x_format", "n_rows", "dim", "n_segments", "cand_count_max", "res_levels", "norm", "screen_terms",
         "has_cand_lid", "has_den_out", "has_pair"]

# (changes to BASE / environment, runs the 2-term pairwise form)
TABLE = [
    ({}, 1),                                   # PROD level 1: auto picks it where it picked 3 terms
    ({"screen_terms": 2}, 1),
    ({"screen_terms": 3}, 0),
    ({"screen_terms": 1}, 0),
    ({"has_pair": 0}, 0),
    ({"RQSID_NO_PAIR": 1}, 0),
    ({"RQSID_NO_PAIR": 1, "screen_terms": 2}, 0),
    ({"res_levels": 2, "cand_count_max": 100}, 1),
    ({"res_levels": 0}, 0),                    # auto: 1 term at level 0
    ({"res_levels": 0, "screen_terms": 2}, 1),
    ({"cand_count_max": 256}, 0),              # the candidate split keeps 3 terms
    ({"cand_count_max": 256, "screen_terms": 2}, 0),
    ({"x_format": 1}, 0),                      # 16-bit rows keep 3 terms
    ({"x_format": 2, "screen_terms": 2}, 0),
    ({"RQSID_PC": 2}, 0),                      # the producer/consumer screen has no such form
    ({"RQSID_SCREEN_VARIANT": 2}, 0),          # the multi-sweep list epilogue neither
    ({"RQSID_SCREEN_VARIANT": 1}, 1),
    ({"dim": 32, "has_cand_lid": 1}, 1),
]


@pytest.mark.parametrize("changes,want", TABLE)
def test_plan_pair(changes, want, monkeypatch):
    lib = _lib.load()
    for k in ("RQSID_NO_PAIR", "RQSID_PC", "RQSID_SCREEN_VARIANT", "RQSID_PCW"):
        monkeypatch.delenv(k, raising=False)
    shape = dict(BASE)
    for k, v in changes.items():
        if k.startswith("RQSID_"):
            monkeypatch.setenv(k, str(v))
        else:
            shape[k] = v
    assert lib.rqsid_assign_plan_pair(*[shape[k] for k in ORDER]) == want


def test_pair_table_bytes_and_argument_errors():
    lib = _lib.load()
    assert lib.rqsid_pair_table_bytes(128) == 128 * 128 * 128 * 2
    assert lib.rqsid_pair_table_bytes(0) == 0
    # more than 128 candidates per segment, and a null table: refused before any launch
    assert lib.rqsid_pair_table(1, 512, 1, 4, 1, 1, 1, 129, None, 16, None) == -1
    assert "pair_table" in lib.rqsid_last_error().decode()
    assert lib.rqsid_pair_table(1, 512, 1, 4, 1, 1, 1, 128, None, None, None) == -1
