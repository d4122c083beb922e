"""bench.py's roofline traffic lookup: every kernel name LEVEL_KERNELS lists for a preset must be a
kernel of the committed PMC traffic file that preset reads, or the bench line silently loses its
traffic (the names carry template arguments that change with the kernels)."""
import ast
import json
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def _level_kernels():
    tree = ast.parse((REPO / "bench.py").read_text())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "LEVEL_KERNELS" for t in node.targets):
            return ast.literal_eval(node.value)
    raise AssertionError("LEVEL_KERNELS not found in bench.py")


def test_level_kernels_match_committed_traffic():
    lk = _level_kernels()
    for preset, path in (("prod", "bench_data/traffic.json"), ("xl", "bench_data/traffic_xl.json")):
        names = set(json.loads((REPO / path).read_text())["kernels"])
        for lvl, ks in lk[preset].items():
            missing = [k for k in ks if k not in names]
            assert not missing, f"{preset} level {lvl}: {missing} not in {path}"


def test_side_watchdog_prints_the_encode_line_and_exits_nonzero(capsys):
    """a hang in the side measurements after the timed region ends with the encode line
    printed (marked stopped) and a NON-ZERO exit status, so the driver sees the failure."""
    import sys
    import time
    sys.path.insert(0, str(REPO))
    import bench
    codes = []
    line = {"metric": "vectors quantized/sec (3-level RQ, 512-d)", "value": 1.0}
    dog = bench.SideWatchdog(line, 0.05, rank=0, exit_fn=codes.append).start()
    dog.thread.join(5)
    assert codes == [bench.SideWatchdog.EXIT_CODE] and codes[0] != 0
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1
    got = json.loads(out[0])
    assert got["value"] == 1.0 and got["side_measurements"].startswith("stopped")
    assert dog.done() is False  # the main thread's late print is suppressed: one line only
    assert capsys.readouterr().out == ""


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    import sys
    sys.path.insert(0, str(REPO))
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: every row of a small output; of a larger one the same sorted sample in every run,
    float32 IDs beside their float64 row numbers."""
    import sys
    import numpy as np
    import torch
    sys.path.insert(0, str(REPO))
    import bench
    out = (torch.arange(3000, dtype=torch.int32).reshape(1000, 3) * 7) % 256
    bench.dump_outputs(tmp_path / "all", out, rank=0, world=1)
    ids, rows = np.load(tmp_path / "all" / "ids.npy"), np.load(tmp_path / "all" / "ids_rows.npy")
    assert ids.dtype == np.float32 and rows.dtype == np.float64
    assert np.array_equal(ids, out.numpy()) and np.array_equal(rows, np.arange(1000))
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 100)
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, out, rank=1, world=2)
    ids, rows = np.load(tmp_path / "a" / "ids_rank1.npy"), np.load(tmp_path / "a" / "ids_rows_rank1.npy")
    assert ids.shape == (100, 3) and len(np.unique(rows)) == 100 and (np.diff(rows) > 0).all()
    assert np.array_equal(ids, out.numpy()[rows.astype(np.int64)])
    assert np.array_equal(rows, np.load(tmp_path / "b" / "ids_rows_rank1.npy"))
    assert np.array_equal(ids, np.load(tmp_path / "b" / "ids_rank1.npy"))


def test_side_watchdog_quiet_when_done_in_time(capsys):
    import sys
    sys.path.insert(0, str(REPO))
    import bench
    codes = []
    dog = bench.SideWatchdog({"value": 2.0}, 30.0, rank=0, exit_fn=codes.append).start()
    assert dog.done() is True
    dog.thread.join(5)
    assert codes == [] and json.loads(capsys.readouterr().out)["value"] == 2.0
